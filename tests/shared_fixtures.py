"""The fixtures that many test files share, defined once.  A plain module: a test file imports the ones it uses by name
(pytest collects an imported fixture like one defined in the file, so each importing module gets its own instance)."""
import pytest

import trainer_helpers
from __graft_entry__ import load_package


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.lib()
    return p


@pytest.fixture(scope="module")
def stub_trainer(tmp_path_factory):
    return trainer_helpers.build_stub_trainer(tmp_path_factory)


@pytest.fixture(scope="module")
def trainer():
    return trainer_helpers.build_device_trainer()
