"""CPU-only checks of the drop-in boundary: libaleppo.so builds, loads without a GPU, exports every
symbol include/aleppo.h declares, and refuses to run without a device (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from __graft_entry__ import build, load_package


@pytest.fixture(scope="module")
def pkg():
    return build()


def header_functions():
    txt = open(os.path.join(ROOT, "include", "aleppo.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(aleppo_[a-z0-9_]+)\s*\(", txt)))


def test_every_declared_symbol_is_exported(pkg):
    names = header_functions()
    assert len(names) >= 30
    lib = pkg.lib()
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/aleppo.h but not exported by libaleppo.so"
    assert sorted(pkg.EXPORTS) == names
    assert lib.aleppo_abi_version() == pkg.ABI_VERSION


def test_config_struct_layout_matches_header(pkg):
    # 13 x int32, 9 x float, uint64 (include/aleppo.h aleppo_config)
    assert C.sizeof(pkg.Config) == 96 and pkg.Config.seed.offset == 88
    assert C.sizeof(pkg.MinibatchMetrics) == 28


def test_fails_loudly_without_a_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.AleppoError, match="no CPU fallback"):
        pkg.Engine(8, 8)
    import numpy as np
    with pytest.raises(pkg.AleppoError, match="no CPU fallback"):
        pkg.gae.gae(np.zeros((1, 3), np.float32), np.ones((1, 3)), np.ones((1, 3)), np.ones(1), np.zeros((1, 3)),
                    np.zeros((1, 3)), np.zeros((1, 3)), 0.99, 0.95)


def test_argument_validation_happens_before_the_device(pkg):
    import numpy as np
    with pytest.raises(pkg.AleppoInvalidArgument, match="Horizon must be greater than 0"):
        pkg.Engine(8, 0)
    with pytest.raises(pkg.AleppoInvalidArgument, match="Total environments must be greater than 0"):
        pkg.Engine(0, 8)
    with pytest.raises(pkg.AleppoInvalidArgument, match="2D except next_values"):
        pkg.gae.gae(np.zeros(3, np.float32), np.ones(3), np.ones(3), np.ones(1), np.zeros(3), np.zeros(3),
                    np.zeros(3), 0.99, 0.95)


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "ale-libtorch-ppo_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f)).read()
                assert "liboracle" not in txt and "oracle_lib" not in txt and "oracle/" not in txt.replace(
                    "``oracle/``", ""), f


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    """bench.py --gpus N under a launcher with a different WORLD_SIZE exits before touching torch or a GPU;
    without a launcher and N > 1 it would spawn torch.distributed.run itself (not exercised here: no GPUs)."""
    import subprocess
    import sys
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=3" in (r.stderr + r.stdout)


def test_bench_spawns_one_rank_per_gpu_with_the_launcher_environment():
    """`python bench.py --gpus 2` outside a launcher starts torch.distributed.run itself (as a child, before it touches a
    device): each of the two ranks reports the RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* it was handed and - this
    container has no GPU - stops at aleppo_device_check with ALEPPO_ERR_NO_DEVICE (no CPU fallback, no silent skip).
    SURVEY 8e; the reference is single-device (src/bin/train.cc:336-345)."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the ranks would run the bench")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--master-port", "29531"], capture_output=True, text=True, env=env, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode != 0
    assert "spawning:" in out and "--nproc-per-node=2" in out
    for rank in (0, 1):
        assert f"rank {rank} local_rank {rank} world_size 2 master 127.0.0.1:29531" in out, out[-3000:]
    # (the launcher terminates the other rank as soon as the first one has failed: at least one of them gets to say it)
    assert out.count("no CPU fallback") >= 1, out[-3000:]


def test_option_and_location_constants_match_the_header(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aleppo.h")).read(), flags=re.S)
    for name, val in (("ALEPPO_OPT_GENERIC_CONV", pkg.OPT_GENERIC_CONV), ("ALEPPO_OPT_FC_PIPE", pkg.OPT_FC_PIPE),
                      ("ALEPPO_OPT_FUSED_ACT", pkg.OPT_FUSED_ACT), ("ALEPPO_OPT_GATE_TIMEOUT_MS", pkg.OPT_GATE_TIMEOUT_MS),
                      ("ALEPPO_OPT_UPDATE_GRAPH", pkg.OPT_UPDATE_GRAPH), ("ALEPPO_OPT_FUSED_FWD", pkg.OPT_FUSED_FWD), ("ALEPPO_OPT_FUSED_BWD", pkg.OPT_FUSED_BWD),
                      ("ALEPPO_OPT_SERIAL_UPDATE", pkg.OPT_SERIAL_UPDATE), ("ALEPPO_OPT_FORCE_COMM", pkg.OPT_FORCE_COMM),
                      ("ALEPPO_OPT_ACT_STORE", pkg.OPT_ACT_STORE), ("ALEPPO_FC_SPLITS", pkg.FC_SPLITS),
                      ("ALEPPO_HOST_MAPPED", pkg.HOST_MAPPED), ("ALEPPO_ROLLOUT_FP16", pkg.ROLLOUT_FP16),
                      ("ALEPPO_ABI_VERSION", pkg.ABI_VERSION)):
        m = re.search(rf"\b{name}\s*=?\s*(\d+)", txt)
        assert m and int(m.group(1)) == val, name
    kc = re.search(r"ALEPPO_K_COUNT = (\d+)", txt)
    assert int(kc.group(1)) == len(pkg.KERNEL_CLASSES)


@pytest.mark.gpu
def test_bench_line_keeps_the_contract():
    """`python bench.py --full` (short: 2 steps, no CPU baseline / host legs / v1 leg) prints ONE JSON line with the keys the
    driver reads, the dominant kernel's roofline block (achieved / peak = frac, algorithmic bytes, the kernel-source stamp) and
    - on a 1-GPU bf16 run with the legs on - the fused-backward option leg."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-host-legs", "--no-v1"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "env-steps/s" and d["value"] > 0
    assert d["dtype"] == "bf16" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "kernel_source_sha16"):
        assert k in rf, k
    assert rf["bound"] in ("hbm", "mfma") and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert rf["kernel"] in rf["update_kernels"] and rf["update_kernels"][rf["kernel"]]["ms"] > 0


@pytest.mark.gpu
def test_plain_bench_run_measures_only_the_headline(tmp_path):
    """`python bench.py` without --full stops after the timed steps: the line carries the headline keys and the last timed
    step's loss, --dump-outputs still writes what that step computed, and everything --full measures in runs of its own
    (roofline passes, fused-backward / host-frames / v1-shape legs, CPU baseline, reference ratio) is null."""
    import json
    import subprocess
    import sys
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--dump-outputs",
                        str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "env-steps/s" and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["higher_is_better"] is True and d["dtype"] == "bf16"
    for k in ("roofline", "cpu_baseline", "frames_84_hbm", "host_frames", "vs_reference_published_v1_26289", "v1_shape",
              "fused_bwd_option"):
        assert d[k] is None, k
    assert "frame leg" not in r.stderr and "cpu baseline" not in r.stderr
    assert (tmp_path / "params.npy").exists()
    assert float(np.load(tmp_path / "train_loss.npy")[-1, -1]) == d["last_loss"]


# every environment variable the library reads: the per-context switches' mirrors (tuning_from_env), the replay-gate
# reference route and the gate timeout.  An A/B of anything else is two builds (tests/tools/ab.sh).
DOCUMENTED_ENV = {"ALEPPO_GENERIC_CONV", "ALEPPO_FC_PIPE", "ALEPPO_FWD_FUSED", "ALEPPO_BWD_FUSED", "ALEPPO_FUSED_ACT",
                  "ALEPPO_REPLAY_GATED", "ALEPPO_GATE_TIMEOUT_MS"}
ABLATION_ENV = {"ALEPPO_FF_ABLATE", "ALEPPO_CB_ABLATE"}  # read only by a `make ABLATIONS=1` build


def _env_names(src):
    """ALEPPO_* names passed to getenv, directly or through a helper that forwards its `name` argument to getenv"""
    names = set(re.findall(r"getenv\(\s*\"(ALEPPO_[A-Z0-9_]+)\"", src))
    for helper in re.findall(r"(\w+)\s*(?:=\s*\[[^\]]*\]\s*)?\(const char \*name[^)]*\)\s*\{[^{}]*getenv\(name\)", src):
        names |= set(re.findall(rf"\b{helper}\(\s*\"(ALEPPO_[A-Z0-9_]+)\"", src))
    return names


def test_library_reads_only_the_documented_environment():
    import glob
    default, ablation = set(), set()
    paths = sorted(glob.glob(os.path.join(ROOT, "ale-libtorch-ppo_amd", "csrc", "*.h*")))  # *.hip, *.hpp
    assert len(paths) > 30
    for path in paths:
        src = open(path).read()
        unguarded = re.sub(r"#ifdef ALEPPO_ABLATIONS\n.*?#endif", "", src, flags=re.S)  # what the default build compiles
        default |= _env_names(unguarded)
        ablation |= _env_names(src) - _env_names(unguarded)
    assert default == DOCUMENTED_ENV, sorted(default ^ DOCUMENTED_ENV)
    assert ablation == ABLATION_ENV, sorted(ablation ^ ABLATION_ENV)


# Who may allocate or free: a context's memory goes through the ownership helpers of api_core.hip (which register every
# pointer for aleppo_destroy) and nothing else in the library frees - hipFree / hipHostFree wait for every stream of the
# device.  api_core.hip also holds aleppo_host_alloc / aleppo_host_free, the caller's memory; the other two
# are process-wide allocations no context owns.  A feature that allocates behind the registry's back fails here.
MEMORY_CALLS = {
    "api_core.hip": {"hipMalloc(": 1, "hipHostMalloc(": 2, "hipFree(": 1, "hipHostFree(": 2},
    "api_ops.hip": {"hipMalloc(": 1},           # the stateless operators' arena
    "conv_patch_launch.hip": {"hipMalloc(": 1},  # the per-device 16 KB scratch
}


def test_only_the_ownership_helpers_allocate_or_free():
    import glob
    csrc = os.path.join(ROOT, "ale-libtorch-ppo_amd", "csrc")
    paths = sorted(p for ext in ("*.hip", "*.hpp", "*.inc") for p in glob.glob(os.path.join(csrc, ext)))
    assert len(paths) > 30
    found = {}
    for path in paths:
        src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        counts = {tok: len(re.findall(r"\b" + re.escape(tok), src))
                  for tok in ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(")}
        counts = {tok: n for tok, n in counts.items() if n}
        if counts:
            found[os.path.basename(path)] = counts
        assert not re.search(r"\bretire(_host)?\(", src), path  # outgrown buffers just stay in the registry
    assert found == MEMORY_CALLS, found
