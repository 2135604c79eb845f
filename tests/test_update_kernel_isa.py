"""Build-time guard of the two fused update kernels: their loops are inline-assembly software pipelines with
hand-counted `s_waitcnt` immediates and a no-spill register budget that hipcc's own passes know nothing about.  A compiler
or source change that spills, or an indexed (ALEPPO_OPT_MINIBATCH_SHUFFLE) instantiation whose memory operations differ
from the contiguous one, would only degrade at run time; here it fails on a CPU box, from the gfx950 code object of
libaleppo.so (ROCm's LLVM tools)."""
import collections
import glob
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
# fwd_fused_kernel<ABL = 0, IDX> / conv_bwd_fused_kernel<ABL = 0, IDX> (Itanium mangling)
KERNELS = {"fwd": r"^_ZN6aleppo16fwd_fused_kernelILi0ELb([01])EEEvNS_14FwdFusedParamsE$",
           "bwd": r"^_ZN6aleppo21conv_bwd_fused_kernelILi0ELb([01])EEEvNS_13ConvBwdParamsE$"}
# one wave per SIMD, the whole 512-entry register file, no scratch.  Architectural VGPRs + AGPRs as the
# code-object metadata counts them (vgpr_count = the unified total: AGPRs start at the 4-aligned accumulation offset)
MAX_AGPR = {"fwd": 252, "bwd": 252}
MAX_TOTAL = 512


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("ROCm LLVM tools not installed")
    pkg = ge.build()
    so = os.path.join(os.path.dirname(pkg.__file__), "libaleppo.so")
    d = tmp_path_factory.mktemp("co")
    shutil.copy(so, d / "lib.so")  # (llvm-objdump --offloading writes the bundles next to its input)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True,
                   capture_output=True)
    cos = sorted(glob.glob(str(d / "lib.so.*gfx950")))
    assert cos, "no gfx950 code object in libaleppo.so"
    return cos


def _kernels(cos):
    """name -> (code object, metadata dict) for the fused kernels"""
    out = {}
    for co in cos:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in re.split(r"\n  - \.", notes):  # (one block per kernel: its args list is indented deeper)
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m:
                continue
            for tag, pat in KERNELS.items():
                km = re.match(pat, m.group(1))
                if km:
                    meta = {k: int(v) for k, v in re.findall(
                        r"\.?(private_segment_fixed_size|vgpr_count|agpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)",
                        "." + blk)}
                    out[(tag, int(km.group(1)))] = (co, m.group(1), meta)
    return out


def _disasm(co, sym):
    t = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f"--disassemble-symbols={sym}", co], check=True,
                       capture_output=True, text=True).stdout
    return [ln.split("//")[0].strip() for ln in t.splitlines() if ln.startswith(("\t", "  "))]


def _profile(ins):
    ops = collections.Counter(i.split()[0] for i in ins if i)
    # the prefetch loads: 16-byte loads into accumulation registers (the inline-assembly `global_load_dwordx4 a[..]`).
    # (Not every global_load_dwordx4: hipcc may merge the prologue's bias loads differently once the index fetch is
    # there - e.g. dwordx3 + dword instead of one dwordx4 - which is outside the counted pipeline.)
    pre = sum(1 for i in ins if re.match(r"global_load_dwordx4 a\[", i))
    stores = {k: v for k, v in ops.items() if k.startswith("global_store")}
    waits = sorted({i for i in ins if i.startswith("s_waitcnt")})
    return pre, stores, waits, ops


@pytest.mark.parametrize("tag", ["fwd", "bwd"])
def test_fused_kernel_budget_and_indexed_variant(code_objects, tag):
    ks = _kernels(code_objects)
    assert (tag, 0) in ks and (tag, 1) in ks, f"contiguous / indexed {tag} instantiations missing: {sorted(ks)}"
    prof = {}
    for idx in (0, 1):
        co, name, meta = ks[(tag, idx)]
        assert meta.get("private_segment_fixed_size", 0) == 0, f"{name}: scratch {meta}"
        assert meta.get("vgpr_spill_count", 0) == 0 and meta.get("sgpr_spill_count", 0) == 0, f"{name}: spills {meta}"
        assert meta["agpr_count"] <= MAX_AGPR[tag], f"{name}: {meta}"
        assert meta["vgpr_count"] <= MAX_TOTAL, f"{name}: {meta}"
        prof[idx] = _profile(_disasm(co, name))
    (pre0, st0, w0, ops0), (pre1, st1, w1, ops1) = prof[0], prof[1]
    assert pre0 > 0
    assert pre1 == pre0, "the indexed variant issues a different number of prefetch loads"
    assert st1 == st0, "the indexed variant issues different global stores"
    assert w1 == w0, f"the indexed variant waits differently: {sorted(set(w0) ^ set(w1))}"


@pytest.mark.parametrize("kernel", ["fwd_fused_kernel", "conv_bwd_fused_kernel"])
def test_default_build_ships_no_ablation_variant(code_objects, kernel):
    """The timing-only ablations (ABL != 0: a phase left out, wrong results) exist only in a `make ABLATIONS=1` build: the
    default library holds exactly the contiguous and the indexed instantiation of ABL = 0."""
    syms = set()
    for co in code_objects:
        t = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                           text=True).stdout
        syms |= set(re.findall(rf"\.name:\s+(_ZN6aleppo\d+{kernel}I\S+)", t))
    assert syms and all(re.match(rf"_ZN6aleppo\d+{kernel}ILi0ELb[01]E", s) for s in syms), sorted(syms)
    assert sorted(re.match(rf"_ZN6aleppo\d+{kernel}ILi0ELb([01])E", s).group(1) for s in syms) == ["0", "1"], sorted(syms)
