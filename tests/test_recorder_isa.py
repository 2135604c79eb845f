"""Build-time guard of the episode recorders' capture kernel: both rec_capture_kernel instantiations (84x84 frames, raw
pairs) exist in the gfx950 code object of libaleppo.so, use no scratch, no LDS and spill nothing - the kernel is two copy
loops of 16-byte words and one thread's worth of game logic.  Read from the code object's metadata (llvm-readelf --notes)
on a CPU box."""
import os
import re
import subprocess

from test_update_kernel_isa import LLVM, code_objects  # noqa: F401  (the module fixture: the unbundled code objects)

# rec_capture_kernel<RAW>(RecCaptureArgs) (Itanium mangling, namespace aleppo)
KERNEL = re.compile(r"^_ZN6aleppo18rec_capture_kernelILb([01])EEEvNS_14RecCaptureArgsE$")


def _kernels(cos):
    """{RAW: metadata}"""
    out = {}
    for co in cos:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in re.split(r"\n  - \.", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            km = KERNEL.match(m.group(1)) if m else None
            if km:
                out[int(km.group(1))] = {k: int(v) for k, v in re.findall(
                    r"\.?(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):"
                    r"\s+(\d+)", "." + blk)}
    return out


def test_both_capture_kernels_exist_without_scratch_lds_or_spills(code_objects):  # noqa: F811
    ks = _kernels(code_objects)
    assert set(ks) == {0, 1}, sorted(ks)
    for raw, meta in ks.items():
        assert meta.get("private_segment_fixed_size", 0) == 0, f"scratch {raw} {meta}"
        assert meta.get("group_segment_fixed_size", 0) == 0, f"LDS {raw} {meta}"
        assert meta.get("vgpr_spill_count", 0) == 0 and meta.get("sgpr_spill_count", 0) == 0, f"spills {raw} {meta}"
