"""Build-time guard of the head kernel's ALEPPO_OPT_KL_PENALTY entry point: every head_train_kl_kernel instantiation -
bf16 / fp32 dh, fp32 / fp16 rollout planes, the four action-set widths, value clipping off and on - runs without scratch
within the head kernel's register budget.  Checked on a CPU box from the gfx950 code object of libaleppo.so."""
import os
import re
import subprocess

from test_update_kernel_isa import LLVM, code_objects  # noqa: F401  (the module fixture: the unbundled code objects)

# head_train_kl_kernel <T, AMAX, RT, VCLIP> (Itanium mangling: ILi<AMAX>E ... ELb<VCLIP>E)
KERNEL = re.compile(r"^_ZN6aleppo20head_train_kl_kernelI(\w+?)Li(\d+)E(\w+?)Lb([01])EEEv")


def _kl_kernels(cos):
    """{name: (AMAX, VCLIP, dh type, plane type, metadata)}"""
    out = {}
    for co in cos:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in re.split(r"\n  - \.", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m:
                continue
            km = KERNEL.match(m.group(1))
            if km:
                meta = {k: int(v) for k, v in re.findall(
                    r"\.?(private_segment_fixed_size|vgpr_count|vgpr_spill_count):\s+(\d+)", "." + blk)}
                out[m.group(1)] = (int(km.group(2)), int(km.group(4)), km.group(1), km.group(3), meta)
    return out


def test_kl_head_kernels_exist_and_have_no_scratch(code_objects):  # noqa: F811
    ks = _kl_kernels(code_objects)
    # 2 dh types x 2 plane types x 4 widths x 2 value-clip states (advantage normalisation is a run-time switch)
    assert len(ks) == 32, sorted(ks)
    assert {(amax, vclip, t, rt) for amax, vclip, t, rt, _ in ks.values()} == {
        (a, v, t, rt) for a in (4, 6, 10, 18) for v in (0, 1) for t in ("f", "DF16b") for rt in ("f", "DF16_")}
    for name, (amax, _, _, _, meta) in sorted(ks.items()):
        assert meta.get("private_segment_fixed_size", 0) == 0, f"{name}: scratch {meta}"
        assert meta.get("vgpr_spill_count", 0) == 0, f"{name}: spills {meta}"
        # 8 waves per workgroup (AMAX <= 6) may use 256 registers per lane, 4 waves (AMAX = 10 and 18: the penalty's
        # extra registers did not fit 256 at AMAX = 10) the whole 512
        assert meta["vgpr_count"] <= (512 if amax >= 10 else 256), f"{name}: {meta}"
