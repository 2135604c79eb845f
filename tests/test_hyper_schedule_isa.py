"""Build-time guard of the update kernels that read the clip range, the loss coefficients and the gradient-norm limit
from a device block (ALEPPO_OPT_CLIP_PARAM and its kin): the head training kernel has exactly three entry points,
head_train_kernel, head_train_advn_kernel and head_train_kl_kernel, each in 32 instantiations - bf16 / fp32 dh,
fp32 / fp16 rollout planes, the four action-set widths, value clipping off and on - that run without scratch or spills
within their launch bounds; adam_kernel exists for both precisions; and no *_dev_kernel twin of either is left.
Checked on a CPU box from the gfx950 code objects of libaleppo.so."""
import os
import re
import subprocess

from test_update_kernel_isa import LLVM, code_objects  # noqa: F401  (the module fixture: the unbundled code objects)

# <entry point><T, AMAX, RT, VCLIP> (Itanium mangling: <len><name>I<T>Li<AMAX>E<RT>Lb<VCLIP>EEEv)
HEAD = re.compile(r"^_ZN6aleppo\d+(head_train\w*_kernel)I(\w+?)Li(\d+)E(\w+?)Lb([01])EEEv")
ADAM = re.compile(r"^_ZN6aleppo\d+(adam\w*_kernel)I(\w+?)EEv")
NAMES = ("head_train_kernel", "head_train_advn_kernel", "head_train_kl_kernel")
ALL = {(a, v, t, rt) for a in (4, 6, 10, 18) for v in (0, 1) for t in ("f", "DF16b") for rt in ("f", "DF16_")}


def _kernels(cos):
    """({entry point: {(AMAX, VCLIP, dh type, plane type): metadata}}, {adam entry point: {T: metadata}}, every name)"""
    head, adam, names = {}, {}, []
    for co in cos:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in re.split(r"\n  - \.", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m:
                continue
            names.append(m.group(1))
            meta = {k: int(v) for k, v in re.findall(
                r"\.?(private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count|max_flat_workgroup_size):"
                r"\s+(\d+)", "." + blk)}
            km = HEAD.match(m.group(1))
            if km:
                head.setdefault(km.group(1), {})[(int(km.group(3)), int(km.group(5)), km.group(2), km.group(4))] = meta
            km = ADAM.match(m.group(1))
            if km:
                adam.setdefault(km.group(1), {})[km.group(2)] = meta
    return head, adam, names


def test_device_block_head_kernels_exist_without_scratch(code_objects):  # noqa: F811
    head, _, _ = _kernels(code_objects)
    assert set(head) == set(NAMES), sorted(head)
    for name in NAMES:
        ks = head[name]
        assert len(ks) == 32 and set(ks) == ALL, (name, sorted(ks))
        for (amax, vclip, t, rt), meta in sorted(ks.items()):
            tag = f"{name}<{t}, {amax}, {rt}, {vclip}>: {meta}"
            assert meta.get("private_segment_fixed_size", 0) == 0, "scratch " + tag
            assert meta.get("vgpr_spill_count", 0) == 0, "spills " + tag
            # 4 waves (one per SIMD, the whole 512-entry register file) for the wide action sets and, with the KL
            # penalty, from AMAX = 10 on; 8 waves (256 registers) otherwise
            four = amax > 10 or ("_kl_" in name and amax > 6)
            assert meta["max_flat_workgroup_size"] == (256 if four else 512), tag
            assert meta["vgpr_count"] <= (512 if four else 256), tag


def test_one_adam_kernel_and_no_dev_twins(code_objects):  # noqa: F811
    _, adam, names = _kernels(code_objects)
    assert set(adam) == {"adam_kernel"}, sorted(adam)
    assert set(adam["adam_kernel"]) == {"f", "DF16b"}
    for meta in adam["adam_kernel"].values():
        assert meta.get("private_segment_fixed_size", 0) == 0 and meta.get("vgpr_spill_count", 0) == 0, meta
    assert names and not [n for n in names if "_dev_kernel" in n]
