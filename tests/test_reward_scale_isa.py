"""Build-time guard of the ALEPPO_OPT_REWARD_SCALE kernels: the forward scan, the second stage and the finalise kernel
exist, the scaled GAE entry exists for fp32 and fp16 planes, none of them uses scratch or spills, and gae_kernel<float> /
gae_kernel<f16> are still there under their old names.  Checked on a CPU box from the gfx950 code object of
libaleppo.so."""
import os
import re
import subprocess

from test_update_kernel_isa import LLVM, code_objects  # noqa: F401  (the module fixture: the unbundled code objects)

# rs_scan_kernel, rs_reduce_kernel, rs_finalise_kernel, gae_scaled_kernel<RT>, gae_kernel<RT> (Itanium mangling,
# namespace aleppo); the last with its full old signature: a changed argument list would be another kernel
KERNEL = re.compile(r"^_ZN6aleppo\d+(rs_[a-z]+_kernel|gae_scaled_kernel|gae_kernel)(?:I(\w+?)E)?E")
OLD_GAE = {"f": "_ZN6aleppo10gae_kernelIfEEvPhmPKT_PS2_S5_S1_Piiiffi",
           "DF16_": "_ZN6aleppo10gae_kernelIDF16_EEvPhmPKT_PS2_S5_S1_Piiiffi"}
# rs_scan_kernel keeps two chunks of 16 slots in registers - a reward and three flag bytes per slot, one register each:
# 128 - plus four doubles (G, n, S, Q: 8) and the addresses: 168 in the build this ceiling was taken from
SCAN_VGPR_CEILING = 192


def _kernels(cos):
    """{(kernel, plane type or None): (mangled name, metadata)}"""
    out = {}
    for co in cos:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in re.split(r"\n  - \.", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            km = KERNEL.match(m.group(1)) if m else None
            if not km:
                continue
            meta = {k: int(v) for k, v in re.findall(
                r"\.?(private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", "." + blk)}
            out[(km.group(1), km.group(2))] = (m.group(1), meta)
    return out


def test_reward_scale_kernels_exist_and_have_no_scratch(code_objects):  # noqa: F811
    ks = _kernels(code_objects)
    new = {k: v for k, v in ks.items() if k[0] != "gae_kernel"}
    assert set(new) == {("rs_scan_kernel", None), ("rs_reduce_kernel", None), ("rs_finalise_kernel", None),
                        ("gae_scaled_kernel", "f"), ("gae_scaled_kernel", "DF16_")}, sorted(ks, key=str)
    for key, (name, meta) in new.items():
        assert meta.get("private_segment_fixed_size", 0) == 0, f"{name}: scratch {meta}"
        assert meta.get("vgpr_spill_count", 0) == 0 and meta.get("sgpr_spill_count", 0) == 0, f"{name}: spills {meta}"
        assert meta["vgpr_count"] <= 256, f"{name}: {meta}"
    print({k: v[1] for k, v in new.items()})
    assert new[("rs_scan_kernel", None)][1]["vgpr_count"] <= SCAN_VGPR_CEILING, new[("rs_scan_kernel", None)]
    for key in (("rs_reduce_kernel", None), ("rs_finalise_kernel", None)):
        assert new[key][1]["vgpr_count"] <= 64, new[key]


def test_the_clamping_gae_kernels_keep_their_names(code_objects):  # noqa: F811
    ks = _kernels(code_objects)
    for rt, name in OLD_GAE.items():
        assert ("gae_kernel", rt) in ks and ks[("gae_kernel", rt)][0] == name, sorted(ks, key=str)
        meta = ks[("gae_kernel", rt)][1]
        assert meta.get("private_segment_fixed_size", 0) == 0 and meta.get("vgpr_spill_count", 0) == 0, meta


def test_no_scalar_memory_writes_in_the_new_kernels(code_objects):  # noqa: F811
    """plain C++ and vector instructions only: every store and atomic of the new kernels is a vector (global_ / flat_ /
    ds_) instruction"""
    ks = _kernels(code_objects)
    for key, (name, _) in ks.items():
        if key[0] == "gae_kernel":
            continue
        for co in code_objects:
            t = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f"--disassemble-symbols={name}", co],
                               check=True, capture_output=True, text=True).stdout
            ops = {ln.split()[0] for ln in t.splitlines() if ln.startswith(("\t", "  ")) and ln.split()}
            writes = {o for o in ops if "store" in o or "atomic" in o}
            assert all(o.startswith(("global_", "flat_", "ds_")) for o in writes), (name, writes)
            if key[0] == "gae_scaled_kernel" and ops:
                assert any(o.startswith("global_atomic_add") for o in ops), (name, sorted(writes))
