"""trainer/train.cc built against the host-only library stand-in (tests/stub/aleppo_stub.cc), and the helpers that the
tests of the trainer's config keys share: a debug.yaml variant and the event file a run leaves."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_built = []  # the one binary of this test session


def build_stub_trainer(tmp_path_factory):
    """compiles train.cc plus the stand-in out of tree (once per session); returns the binary's path"""
    if not _built:
        out = tmp_path_factory.mktemp("stub") / "train_stub"
        cxx = os.environ.get("CXX", "g++")
        subprocess.check_call([cxx, "-O1", "-std=c++17", "-pthread", os.path.join(ROOT, "trainer", "train.cc"),
                               os.path.join(ROOT, "tests", "stub", "aleppo_stub.cc"), "-o", str(out)])
        _built.append(str(out))
    return _built[0]


def debug_cfg(tmp_path, extra, rollouts=2):
    """trainer/configs/debug.yaml with num_rollouts replaced and `extra` appended, written to tmp_path / d.yaml"""
    txt = open(os.path.join(ROOT, "trainer", "configs", "debug.yaml")).read()
    txt = re.sub(r"(?m)^num_rollouts: .*$", f"num_rollouts: {rollouts}", txt) + extra
    cfg = tmp_path / "d.yaml"
    cfg.write_text(txt)
    return cfg


def events(d):
    """the bytes of the one event file in directory d"""
    files = [f for f in os.listdir(d) if ".tfevents." in f]
    assert len(files) == 1, files
    return open(os.path.join(d, files[0]), "rb").read()
