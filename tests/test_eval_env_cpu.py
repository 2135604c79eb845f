"""CPU: the device-resident evaluation environments without a GPU - the library builds and exports the entry points, the
package's names and constants are the header's, and the trainer's `device_evaluation: true` against host-only stand-ins
(tests/stub/aleppo_stub_eval_env.cc: trainer/emulator.hpp itself behind aleppo_eval_env_open / aleppo_eval_env_run, and
actions that are a fixed hash of the evaluation counter) logs the eval/* scalars of the same binary's host evaluation bit
for bit, whatever the chunk."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_eval_lanes import scalars

BASE = "total_environments: 8\nhidden_size: 32\nhorizon: 8\nnum_mini_batches: 4\nnum_rollouts: 4\ndeterministic: true\n" \
       "num_workers: 2\nmax_steps: 60\n"
EVAL = "eval_interval: 1\neval_environments: 3\neval_episodes: 4\neval_rule: epsilon\neval_epsilon: 0.05\n"
SYMBOLS = ("aleppo_eval_env_open", "aleppo_eval_env_run", "aleppo_eval_env_export_state", "aleppo_eval_env_import_state",
           "aleppo_eval_env_read")


def _make(target):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), target])
    return os.path.join(ROOT, "trainer", target)


@pytest.fixture(scope="module")
def stub():
    return _make("train_eval_stub")


def _run(exe, tmp_path, name, extra):
    d = tmp_path / name
    os.makedirs(d, exist_ok=True)
    cfg = d / "c.yaml"
    cfg.write_text(BASE + extra)
    return d, subprocess.run([exe, "rom.bin", str(d / "x.log"), str(d), "g", str(cfg)], capture_output=True, text=True,
                             timeout=300)


def _scalars(d):
    files = [f for f in os.listdir(d) if ".tfevents." in f]
    assert len(files) == 1, files
    sc = scalars(os.path.join(d, files[0]))
    return [s for s in sc if not s[0].startswith("eval/")], [s for s in sc if s[0].startswith("eval/")]


def test_library_exports_the_entry_points_and_the_package_matches_the_header():
    from __graft_entry__ import build
    pkg = build()
    lib = pkg.lib()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aleppo.h")).read(), flags=re.S)
    for name in SYMBOLS + ("aleppo_eval_set_counter",):
        assert name in pkg.EXPORTS and getattr(lib, name) is not None, name
        assert re.search(rf"\bint {name}\s*\(", txt), name
    for name in ("FRAMES", "EPISODE_RETURNS", "EPISODE_LENGTHS", "GAME_RETURNS", "GAME_LENGTHS"):
        m = re.search(rf"\bALEPPO_EEF_{name}\s*=\s*(\d+)", txt)
        assert m and int(m.group(1)) == getattr(pkg, f"EEF_{name}") == pkg.EVAL_ENV_FIELDS[name.lower()], name
    for method in ("eval_env_open", "eval_env_run", "eval_env_state", "load_eval_env_state", "eval_env_read",
                   "eval_env_episodes"):
        assert callable(getattr(pkg.Engine, method)), method


@pytest.mark.parametrize("extra", ["", "device_preprocess: true\nslot_ahead: false\n", "device_environments: true\n"],
                         ids=["84", "raw-pairs", "device-environments"])
def test_device_evaluation_logs_what_host_evaluation_logs(stub, tmp_path, extra):
    d, r = _run(stub, tmp_path, "plain", extra)
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
    plain_train, plain_eval = _scalars(d)
    d, r = _run(stub, tmp_path, "host", extra + EVAL)
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
    host_train, host_eval = _scalars(d)
    assert not plain_eval and len(host_eval) == 4 * 4 and host_train == plain_train
    assert len({s[2] for s in host_eval if s[0] == "eval/episode_return_mean"}) > 1  # (every evaluation has its own seeds)
    for S in (1, 4, 32):
        d, r = _run(stub, tmp_path, f"dev{S}", extra + EVAL + f"device_evaluation: true\ndevice_evaluation_steps: {S}\n")
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        dev_train, dev_eval = _scalars(d)
        assert dev_eval == host_eval, S
        assert dev_train == plain_train, S


@pytest.mark.parametrize("extra,message", [
    ("device_evaluation: true\n", "device_evaluation needs eval_interval > 0"),
    ("eval_interval: 0\ndevice_evaluation: true\n", "device_evaluation needs eval_interval > 0"),
    ("eval_interval: 1\ndevice_evaluation_steps: 8\n", "device_evaluation_steps needs device_evaluation: true"),
    ("eval_interval: 1\ndevice_evaluation: false\ndevice_evaluation_steps: 8\n",
     "device_evaluation_steps needs device_evaluation: true"),
    ("eval_interval: 1\ndevice_evaluation: true\ndevice_evaluation_steps: 0\n", "device_evaluation_steps must be in [1, 1024]"),
    ("eval_interval: 1\ndevice_evaluation: true\ndevice_evaluation_steps: 1025\n", "device_evaluation_steps must be in [1, 1024]"),
])
def test_invalid_keys_are_refused_when_the_config_is_loaded(stub, tmp_path, extra, message):
    _, r = _run(stub, tmp_path, "bad", extra)
    assert r.returncode == 1 and message in r.stderr and "Rollout" not in r.stdout, r.stderr


def test_library_without_the_entry_points_refuses_the_key(tmp_path):
    for target in ("train_tsan", "train_ckpt_stub"):
        _, r = _run(_make(target), tmp_path, target, EVAL + "device_evaluation: true\n")
        assert r.returncode == 1 and "Rollout" not in r.stdout, r.stderr
        assert "aleppo_eval_env_open is missing" in r.stderr or "aleppo_eval_open is missing" in r.stderr, r.stderr
