"""Build-time guard of the entry points that read the clip range, the loss coefficients and the gradient-norm limit
from a device block (ALEPPO_OPT_CLIP_PARAM and its kin): head_train_dev_kernel, head_train_advn_dev_kernel and
head_train_kl_dev_kernel exist in the same 32 instantiations each as the entry points they mirror - bf16 / fp32 dh,
fp32 / fp16 rollout planes, the four action-set widths, value clipping off and on - run without scratch or spills
within their launch bounds, adam_dev_kernel exists for both precisions, and the kernel-argument entry points are all
still there.  Checked on a CPU box from the gfx950 code objects of libaleppo.so."""
import os
import re
import subprocess

from test_update_kernel_isa import LLVM, code_objects  # noqa: F401  (the module fixture: the unbundled code objects)

# <entry point><T, AMAX, RT, VCLIP> (Itanium mangling: <len><name>I<T>Li<AMAX>E<RT>Lb<VCLIP>EEEv)
HEAD = re.compile(r"^_ZN6aleppo\d+(head_train(?:_advn|_kl)?(?:_dev)?_kernel)I(\w+?)Li(\d+)E(\w+?)Lb([01])EEEv")
ADAM = re.compile(r"^_ZN6aleppo\d+(adam(?:_dev)?_kernel)I(\w+?)EEv")
ALL = {(a, v, t, rt) for a in (4, 6, 10, 18) for v in (0, 1) for t in ("f", "DF16b") for rt in ("f", "DF16_")}


def _kernels(cos):
    """({entry point: {(AMAX, VCLIP, dh type, plane type): metadata}}, {adam entry point: {T: metadata}})"""
    head, adam = {}, {}
    for co in cos:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in re.split(r"\n  - \.", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m:
                continue
            meta = {k: int(v) for k, v in re.findall(
                r"\.?(private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count|max_flat_workgroup_size):"
                r"\s+(\d+)", "." + blk)}
            km = HEAD.match(m.group(1))
            if km:
                head.setdefault(km.group(1), {})[(int(km.group(3)), int(km.group(5)), km.group(2), km.group(4))] = meta
            km = ADAM.match(m.group(1))
            if km:
                adam.setdefault(km.group(1), {})[km.group(2)] = meta
    return head, adam


def test_device_block_head_kernels_exist_without_scratch(code_objects):  # noqa: F811
    head, _ = _kernels(code_objects)
    for name in ("head_train_dev_kernel", "head_train_advn_dev_kernel", "head_train_kl_dev_kernel"):
        ks = head.get(name, {})
        assert len(ks) == 32 and set(ks) == ALL, (name, sorted(ks))
        for (amax, vclip, t, rt), meta in sorted(ks.items()):
            tag = f"{name}<{t}, {amax}, {rt}, {vclip}>: {meta}"
            assert meta.get("private_segment_fixed_size", 0) == 0, "scratch " + tag
            assert meta.get("vgpr_spill_count", 0) == 0, "spills " + tag
            # the launch bounds of the entry point it mirrors: 4 waves (one per SIMD, the whole 512-entry register file)
            # for the wide action sets and, with the KL penalty, from AMAX = 10 on; 8 waves (256 registers) otherwise
            four = amax > 10 or ("_kl_" in name and amax > 6)
            assert meta["max_flat_workgroup_size"] == (256 if four else 512), tag
            assert meta["vgpr_count"] <= (512 if four else 256), tag


def test_kernel_argument_entry_points_are_all_still_there(code_objects):  # noqa: F811
    head, adam = _kernels(code_objects)
    for name in ("head_train_kernel", "head_train_advn_kernel", "head_train_kl_kernel"):
        assert set(head.get(name, {})) == ALL, (name, sorted(head.get(name, {})))
    assert set(head) == {n + s for n in ("head_train", "head_train_advn", "head_train_kl") for s in ("_kernel", "_dev_kernel")}
    assert set(adam.get("adam_kernel", {})) == {"f", "DF16b"}
    assert set(adam.get("adam_dev_kernel", {})) == {"f", "DF16b"}
    for meta in adam["adam_dev_kernel"].values():
        assert meta.get("private_segment_fixed_size", 0) == 0 and meta.get("vgpr_spill_count", 0) == 0, meta
