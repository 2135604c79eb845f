"""trainer/train.cc built against the host-only library stand-in (tests/stub/aleppo_stub.cc) or the device library, and
the helpers that the tests of the trainer's config keys share: a debug.yaml variant, a run of the stand-in build, the
event file a run leaves and its scalars, and the constants of include/aleppo.h."""
import os
import re
import struct
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


def event_scalars(blob, tag):
    """every value of scalar `tag` (Summary.Value{1: tag, 2: simple_value}) in the event file's bytes, in order"""
    t = tag.encode() if isinstance(tag, str) else tag
    key = b"\x0a" + bytes([len(t)]) + t + b"\x15"
    return [struct.unpack("<f", blob[m.end():m.end() + 4])[0] for m in re.finditer(re.escape(key), blob)]


def run_stub(binary, tmp_path, cfg, timeout=600):
    """one run of the stand-in trainer on config `cfg`, logging into tmp_path; the completed process"""
    return subprocess.run([binary, "rom.bin", str(tmp_path / "run.log"), str(tmp_path), "g", str(cfg)],
                          capture_output=True, text=True, timeout=timeout)


def build_device_trainer():
    """builds the package and trainer/train against it; returns the binary's path"""
    from __graft_entry__ import build
    build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer")])
    return os.path.join(ROOT, "trainer", "train")


def header_const(name, stripped=False):
    """the integer that include/aleppo.h gives `name`: an enumerator at the start of a line; stripped: anywhere in the
    header with its comments removed, as an enumerator or a #define"""
    hdr = open(os.path.join(ROOT, "include", "aleppo.h")).read()
    if stripped:
        m = re.search(rf"\b{name}\s*=?\s*(\d+)", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    else:
        m = re.search(rf"(?m)^\s*{name}\s*=\s*(\d+)", hdr)
    assert m, name
    return int(m.group(1))
