"""Build-time guard of head_train_kernel (ALEPPO_OPT_VALUE_CLIP): every instantiation - bf16 / fp32 dh, fp32 / fp16
rollout planes, the four action-set widths, value clipping off and on - runs without scratch.  The AMAX = 18 variants
hold 19 x 8 weight-gradient accumulators per lane with one wave per SIMD; a spill there only shows as a slow update at
run time (150 us vs 22, kernels.hip), so it is checked here, on a CPU box, from the gfx950 code object of libaleppo.so."""
import os
import re
import subprocess

import pytest

from test_update_kernel_isa import LLVM, code_objects  # noqa: F401  (the module fixture: the unbundled code objects)

# head_train_kernel<T, AMAX, RT, VCLIP> (Itanium mangling: ILi<AMAX>E ... ELb<VCLIP>E)
HEAD = re.compile(r"^_ZN6aleppo17head_train_kernelI(\w+?)Li(\d+)E(\w+?)Lb([01])EEEv")


def _head_kernels(cos):
    out = {}
    for co in cos:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in re.split(r"\n  - \.", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m:
                continue
            km = HEAD.match(m.group(1))
            if km:
                meta = {k: int(v) for k, v in re.findall(
                    r"\.?(private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", "." + blk)}
                out[m.group(1)] = (int(km.group(2)), int(km.group(4)), meta)
    return out


def test_head_kernel_has_no_scratch_with_and_without_value_clipping(code_objects):  # noqa: F811
    ks = _head_kernels(code_objects)
    # 2 dh types x 2 plane types x 4 widths x 2 flag states
    assert len(ks) == 32, sorted(ks)
    assert {(amax, vclip) for amax, vclip, _ in ks.values()} == {(a, v) for a in (4, 6, 10, 18) for v in (0, 1)}
    for name, (amax, vclip, meta) in sorted(ks.items()):
        assert meta.get("private_segment_fixed_size", 0) == 0, f"{name}: scratch {meta}"
        # (SGPR spills are kept in VGPR lanes - v_writelane / v_readlane, no memory - and every instantiation has had
        # them; a spill to memory is a VGPR spill and needs a private segment)
        assert meta.get("vgpr_spill_count", 0) == 0, f"{name}: spills {meta}"
        # 8 waves per workgroup (AMAX <= 10) may use 256 registers per lane, 4 waves (AMAX = 18) the whole 512
        assert meta["vgpr_count"] <= (512 if amax > 10 else 256), f"{name}: {meta}"
