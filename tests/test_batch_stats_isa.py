"""Build-time guard of the ALEPPO_F_BATCH_STATS kernels: the first stage exists for fp32 and fp16 planes, the second stage
and the finalise kernel exist, and none of them uses scratch or spills.  Checked on a CPU box from the gfx950 code object
of libaleppo.so."""
import os
import re
import subprocess

from test_update_kernel_isa import LLVM, code_objects  # noqa: F401  (the module fixture: the unbundled code objects)

# bstat_partial_kernel<RT>, bstat_reduce_kernel, bstat_finalise_kernel (Itanium mangling, namespace aleppo)
KERNEL = re.compile(r"^_ZN6aleppo\d+(bstat_[a-z]+_kernel)(?:I(\w+?)E)?E")


def _bstat_kernels(cos):
    """{(kernel, plane type or None): metadata}"""
    out = {}
    for co in cos:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in re.split(r"\n  - \.", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m or "bstat_" not in m.group(1):
                continue
            km = KERNEL.match(m.group(1))
            assert km, m.group(1)  # (a bstat_ kernel this guard does not know)
            meta = {k: int(v) for k, v in re.findall(
                r"\.?(private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", "." + blk)}
            out[(km.group(1), km.group(2))] = meta
    return out


def test_batch_stats_kernels_exist_and_have_no_scratch(code_objects):  # noqa: F811
    ks = _bstat_kernels(code_objects)
    assert set(ks) == {("bstat_partial_kernel", "f"), ("bstat_partial_kernel", "DF16_"), ("bstat_reduce_kernel", None),
                       ("bstat_finalise_kernel", None)}, sorted(ks, key=str)
    for name, meta in ks.items():
        assert meta.get("private_segment_fixed_size", 0) == 0, f"{name}: scratch {meta}"
        assert meta.get("vgpr_spill_count", 0) == 0 and meta.get("sgpr_spill_count", 0) == 0, f"{name}: spills {meta}"
        assert meta["vgpr_count"] <= 128, f"{name}: {meta}"  # (nine double accumulators and their loads: no pressure)
