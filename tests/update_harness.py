"""The engine-side harness that the tests of aleppo_train's opt-in update features share (test_value_clip.py,
test_kl_penalty.py, test_adv_norm_minibatch.py, test_hyper_schedule.py, test_minibatch_shuffle.py): the hashed caller
batch, one context driven through set_batch and aleppo_train, what is read back from it, and the two comparisons - bit
for bit against another run, and against the composed reference (update_ref.py) at a tolerance.  A plain helper module
(no fixtures), everything through the C ABI."""
import numpy as np

import hashfill as hf
import oracle_lib as orc

DIAG_PLANES = ("approx_kl", "clip_fraction")
PER_SAMPLE = ("total_losses", "clipped_losses", "value_losses", "entropies", "ratio") + DIAG_PLANES
# the engine's name of a per-sample plane -> the reference's
REF_PLANE = dict(total_losses="total_losses", clipped_losses="clipped", value_losses="value_losses",
                 entropies="entropies", ratio="ratio", approx_kl="approx_kl", clip_fraction="clip_fraction", kl="kl")
LAST = ("params", "grads", "exp_avg", "exp_avg_sq", "step")  # of read_update's results: the state after the call


def hashed_batch(seed, N, A, *, mask_p, with_ret=True, distinct=None):
    """(obs, actions, old_lp, adv, [ret,] masks) from hashfill seeds seed .. seed + 5; a share mask_p of the samples is
    masked, never the first"""
    if distinct:  # (large batches: byte-permuted copies of a smaller block are cheap to generate)
        base = hf.hf_bytes(seed, (N // distinct, 4, 84, 84))
        obs = np.concatenate([base ^ np.uint8(29 * k) for k in range(distinct)])
    else:
        obs = hf.hf_bytes(seed, (N, 4, 84, 84))
    actions = (hf.hf_u32(seed + 1, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(seed + 2, (N, A), -1, 1))
    adv = hf.hf_range(seed + 3, (N,), -1, 1)
    masks = (hf.hf_unit(seed + 5, N) >= np.float32(mask_p)).astype(np.uint8)
    masks[0] = 1
    if not with_ret:
        return obs, actions, old_lp, adv, masks
    return obs, actions, old_lp, adv, hf.hf_range(seed + 4, (N,), -1, 1), masks


def make_engine(pkg, E, T, A, H, prec=None, options=(), comm=False, **kw):
    """a context (fp32 unless prec says otherwise), on the 1-rank communicator with comm, its options set in order"""
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32 if prec is None else prec, **kw)
    if comm:
        eng.comm_init(pkg.Engine.comm_unique_id())
    for k, v in options:
        eng.set_option(k, v)
    return eng


def read_update(eng, m, epochs, M, *, diag=True, kl=False, adv_stats=False, state=False):
    """what one aleppo_train call (metrics m) left: the parameters and gradients, the per-sample planes, and
    diag: the approx-KL / clip-fraction planes and their means; kl: the exact-KL plane and mean; adv_stats: the
    per-minibatch advantage statistics; state: parameters, Adam moments and step from the state dict"""
    B = eng._batch_n // M
    out = dict(m=m, grads=eng.export_grads())
    if state:
        sd = eng.state_dict()
        out.update({k: sd[k] for k in ("params", "exp_avg", "exp_avg_sq", "step")})
    else:
        out["params"] = eng.export_params()
    if diag:
        out["diag"] = eng.train_diagnostics(epochs, M)
    out.update({k: eng.read_train_metric(k, epochs, M, B) for k in PER_SAMPLE if diag or k not in DIAG_PLANES})
    if kl:
        out["kl"] = eng.read_train_metric("kl", epochs, M, B)
        out["mean_kl"] = eng.kl_divergence(epochs, M)
    if adv_stats:
        out["adv_mean"], out["adv_std"] = eng.advantage_stats(epochs, M)
    return out


def run_update(pkg, E, T, A, H, params, batch, epochs, M, lr, calls=1, vold=None, configure=None, read=None, **kw):
    """one context (make_engine(**kw), then configure(eng)), the parameters, set_batch (+ values), `calls` aleppo_train
    calls; the last call's read_update(**read)"""
    eng = make_engine(pkg, E, T, A, H, **kw)
    if configure:
        configure(eng)
    eng.load_params(params)
    eng.set_batch(*batch, values=vold)
    for _ in range(calls):
        m = eng.train(lr, epochs, M)
    out = read_update(eng, m, epochs, M, **(read or {}))
    eng.close()
    return out


def concat_updates(parts):
    """the read_update results of consecutive calls as those of one call over all their epochs"""
    out = {}
    for k, v in parts[0].items():
        if k in LAST:
            out[k] = parts[-1][k]
        elif isinstance(v, dict):
            out[k] = {j: np.concatenate([q[k][j] for q in parts]) for j in v}
        else:
            out[k] = np.concatenate([q[k] for q in parts])
    return out


def assert_identical(a, b, skip=()):
    """two read_update results are the same bit for bit, in everything either holds but `skip`"""
    assert set(a) - set(skip) == set(b) - set(skip)
    for k in set(a) - set(skip):
        if isinstance(a[k], dict):
            for j in a[k]:
                np.testing.assert_array_equal(a[k][j], b[k][j], err_msg=j)
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def check_against(out, ref, tol, planes, extra=()):
    """a read_update result vs the composed reference: losses, pre-clip norms, the per-sample `planes` (the engine's
    names), the exported gradients and the parameters at tol; extra: (engine array, reference key) pairs at tol too"""
    m = out["m"]
    np.testing.assert_allclose(m["loss"], ref["loss"], atol=tol, rtol=tol)
    np.testing.assert_allclose(m["grad_norm"], ref["grad_norm"], rtol=tol)
    for k in planes:
        np.testing.assert_allclose(out[k], ref[REF_PLANE[k]], atol=tol, rtol=tol, err_msg=k)
    for got, key in extra:
        np.testing.assert_allclose(got, ref[key], atol=tol, rtol=tol, err_msg=key)
    np.testing.assert_allclose(out["grads"], ref["last_grads"], atol=tol)
    np.testing.assert_allclose(out["params"], ref["params"], atol=tol)
