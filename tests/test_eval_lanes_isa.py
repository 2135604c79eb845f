"""Build-time guard of the evaluation lanes' head kernel: eval_head_kernel exists in the gfx950 code object of
libaleppo.so, uses no scratch, spills nothing and stays within 128 VGPRs (one wave per lane, a few dozen vector-memory
instructions: no pressure), and the acting head it was modelled on, infer_head_kernel, is still there for both rollout
plane types.  Checked on a CPU box."""
import os
import re
import subprocess

from test_update_kernel_isa import LLVM, code_objects  # noqa: F401  (the module fixture: the unbundled code objects)

# eval_head_kernel<NSPLIT> / infer_head_kernel<NSPLIT, RT> (Itanium mangling, namespace aleppo)
KERNEL = re.compile(r"^_ZN6aleppo\d+((?:eval|infer)_head_kernel)ILi(\d+)E(\w*?)EEv")


def _head_kernels(cos):
    """{(kernel, plane type or ""): metadata}"""
    out = {}
    for co in cos:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in re.split(r"\n  - \.", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m or "_head_kernel" not in m.group(1):
                continue
            km = KERNEL.match(m.group(1))
            assert km, m.group(1)  # (a head kernel this guard does not know)
            meta = {k: int(v) for k, v in re.findall(
                r"\.?(private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", "." + blk)}
            out[(km.group(1), km.group(3))] = meta
    return out


def test_eval_head_kernel_exists_without_scratch_next_to_the_acting_head(code_objects):  # noqa: F811
    ks = _head_kernels(code_objects)
    assert set(ks) == {("eval_head_kernel", ""), ("infer_head_kernel", "f"), ("infer_head_kernel", "DF16_")}, sorted(ks)
    meta = ks[("eval_head_kernel", "")]
    assert meta.get("private_segment_fixed_size", 0) == 0, f"scratch {meta}"
    assert meta.get("vgpr_spill_count", 0) == 0 and meta.get("sgpr_spill_count", 0) == 0, f"spills {meta}"
    assert meta["vgpr_count"] <= 128, meta
