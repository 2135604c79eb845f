"""CPU: the episode recorders' part of the drop-in boundary (include/aleppo.h: aleppo_rec_config, aleppo_rec_step,
aleppo_rec_counts and the four aleppo_rec_* entry points): the ctypes structures and the numpy row type of the Python
mirror have the sizes and offsets the header states, the constants are the header's, and libaleppo.so exports the calls."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from __graft_entry__ import build


@pytest.fixture(scope="module")
def pkg():
    return build()


def test_struct_sizes_and_offsets(pkg):
    assert C.sizeof(pkg.RecConfig) == 32
    assert [getattr(pkg.RecConfig, f).offset for f in ("source", "index", "content", "capacity", "reserved")] == [0, 4, 8, 12, 16]
    want = dict(ordinal=0, action=8, reward=12, value=16, start=20, terminated=21, truncated=22, game_over=23, lives=24,
                reserved=28)
    assert C.sizeof(pkg.RecStep) == 32 and {f: getattr(pkg.RecStep, f).offset for f in want} == want
    dt = pkg.REC_STEP_DTYPE
    assert dt.itemsize == 32 and {f: dt.fields[f][1] for f in want} == want
    assert [n for n, _ in pkg.RecStep._fields_] == list(dt.names)
    assert C.sizeof(pkg.RecCounts) == 40
    assert [getattr(pkg.RecCounts, f).offset for f in ("rows", "dropped", "next_ordinal", "capacity", "frame_bytes",
                                                        "observation_bytes", "actions")] == [0, 8, 16, 24, 28, 32, 36]


def test_constants_match_the_header(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aleppo.h")).read(), flags=re.S)
    for name, val in (("ALEPPO_REC_ROLLOUT", pkg.REC_ROLLOUT), ("ALEPPO_REC_EVAL", pkg.REC_EVAL),
                      ("ALEPPO_REC_FRAMES", pkg.REC_FRAMES), ("ALEPPO_REC_OBSERVATION", pkg.REC_OBSERVATION),
                      ("ALEPPO_REC_F_STEPS", pkg.REC_FIELDS["steps"]), ("ALEPPO_REC_F_LOGITS", pkg.REC_FIELDS["logits"]),
                      ("ALEPPO_REC_F_FRAMES", pkg.REC_FIELDS["frames"]),
                      ("ALEPPO_REC_F_OBSERVATIONS", pkg.REC_FIELDS["observations"])):
        m = re.search(rf"\b{name}\s*=\s*(\d+)", txt)
        assert m and int(m.group(1)) == val, name
    assert pkg.REC_SOURCES == dict(rollout=0, eval=1)


def test_entry_points_are_exported(pkg):
    lib = pkg.lib()
    for n in ("aleppo_rec_open", "aleppo_rec_count", "aleppo_rec_read", "aleppo_rec_clear"):
        assert n in pkg.EXPORTS and hasattr(lib, n), n
