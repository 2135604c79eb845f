"""The PPO head kernel (head_train_body.inc and its three entry points) in every variant, action count and policy regime,
against the float64 reference of tests/head_ref.py with its derived bounds (pytest -m gpu).

The operator.  pkg.losses.compute runs head_train_kernel<float> on an identity head, so the logits are the caller's
exactly (E = 0) and dh IS (dlogits, dvalues).  A = 1 .. 18 at B = 203 - ragged against the 16 rows per workgroup and
against 4 and 8 waves; the masked rows are r % 17 == 0, which is every wave position - in three regimes of the inputs:
"uniform" (today's: logits in [-2, 2]), "peaked" (per-row logit spread 20 .. 45, old log-probs = log-softmax of the same
logits plus a hashed drift so that rho spans both clip edges and reaches 1e-2 and 1e1, actions drawn from the old policy
with every fifth row forced to its least probable action) and "underflow" (spread 90 .. 120: some p below the smallest
fp32 normal, where only the reference's underflow term is honest).  |log rho| <= 40 everywhere.  Every returned plane,
dlogits, dvalues and the loss against their bounds; masked rows exactly zero.

The engine.  n = 37, H = 32, lr = 0 and a norm limit of 1e30 (both asserted, as tests/test_gpu_backward.py does), the
action head's weights scaled so that the CPU oracle's forward has a largest per-row logit spread of SPREAD (the peaked
regime).  A in {1, 4, 5, 6, 7, 10, 11, 18} (both sides of every dispatch boundary) x (plain, advantage normalisation, KL
at beta = 0.2, both) x value clipping off / on x (fp32 context and planes, bf16 context and f16 planes) = 128 rows, one
batch per (n, H, A); the two mixed precision pairs at A = 5 and 11; H = 96 and 512 at A = 7 and 18 with every option on;
n = 1; n = 520 in two minibatches (the export is minibatch 1: a non-zero sample-map offset, waves with more than one
row).  On the engine's own exported h: backward_ref.check_backward's head check with the extended reference (dh inside
its interval or bound, dWh and dbh under (c)), every per-sample plane, the four means against the masked mean of the
engine's own planes, the advantage statistics against update_ref.stats, the clip fraction bit for bit from the engine's
own ratio plane, and the share of ambiguous rows against head_ref.AMBIGUOUS_CAP.
Bit equalities: the KL option at beta = 0, value clipping at a range of 1e30 and normalisation on a minibatch whose
statistics are exactly (0, 1) each leave every plane and gradient of the option-off update.

The inputs are built on the CPU (operator_case, engine_case) and shared with tests/test_head_ref_cpu.py, which shows the
reference's room and teeth on them.

Measured on the MI355X, worst |d| / bound:
    operator          total  clipped  value  entropy  ratio  dlogits/dvalues  loss
      near-uniform    0.09   0.08     0.24   0.02     0.07   0.21             0.06
      peaked          0.06   0.11     0.08   0.03     0.06   0.12             0.08
      underflow       0.04   0.09     0.08   0.02     0.05   0.12             0.16
    engine            total  clipped  value  entropy  ratio  approx-KL  KL    dh    dWh   dbh   means: loss  approx-KL  cf    KL
      fp32, f32       0.06   0.06     0.24   0.02     0.06   0.05       0.04  0.06  0.17  0.17         0.08  0.12       0.02  0.05
      bf16, f16       0.04   0.04     0.17   0.01     0.05   0.04       0.03  (a)   0.15  0.13         0.08  0.09       0.03  0.07
    (a) every dh element of the bf16 contexts inside its interval; the interval is a single value on 39 - 97 % of the
    elements (median 57 %: through head weights scaled 4 to 21 times the allowance is often wider than a bf16 ulp of
    dh), and on none at n = 1 under normalisation (one sample: std = 0, inv_f = 1e8, and one ulp of mean_f is an
    advantage of 6).  The clip fraction equalled the reference's on every row and the engine's own ratio plane bit for
    bit; no ambiguous row was met (0 of 10 962 operator rows, 0 in 176 engine variants).  The underflow rows: all 1486
    gradients of a subnormal p whose exact value is representable came back non-zero - the device's expf underflows
    gradually.  The whole file takes two seconds."""
import functools

import numpy as np
import pytest

import backward_ref as br
import hashfill as hf
import head_ref as hr
import oracle_lib as orc
import update_ref as ur
from shared_fixtures import pkg  # noqa: F401
from test_gpu_layers import row_inputs

pytestmark = pytest.mark.gpu

HYPER = dict(clip=0.1, c_v=0.5, c_e=0.01)  # the Engine's defaults; the value-clip range follows the clip range
MAX_NORM = 1e30
BETA = 0.2
SPREAD = 44.0  # the largest per-row logit spread of an engine row on the CPU oracle's forward
# entry point: (name, advantage normalisation, beta or None)
ENTRIES = (("plain", False, None), ("advn", True, None), ("kl", False, BETA), ("kl+advn", True, BETA))
ENGINE_A = (1, 4, 5, 6, 7, 10, 11, 18)
PRECISIONS = (("fp32", False), ("bf16", True))  # (the context's precision, f16 planes)
MIXED = (("fp32", True), ("bf16", False))
# (n, M, H, A, context, f16 planes, [(entry, value clipping)])
EVERY = tuple((e, v) for e in ENTRIES for v in (False, True))
ALL_ON = ((ENTRIES[3], True),)
ENGINE_ROWS = [(37, 1, 32, A, prec, f16, EVERY) for A in ENGINE_A for prec, f16 in PRECISIONS]
ENGINE_ROWS += [(37, 1, 32, A, prec, f16, EVERY) for A in (5, 11) for prec, f16 in MIXED]
ENGINE_ROWS += [(37, 1, H, A, prec, f16, ALL_ON) for H in (96, 512) for A in (7, 18) for prec, f16 in PRECISIONS]
ENGINE_ROWS += [(1, 1, 32, 6, prec, f16, ALL_ON + ((ENTRIES[0], False),)) for prec, f16 in PRECISIONS]
ENGINE_ROWS += [(520, 2, 32, 7, prec, f16, ALL_ON + ((ENTRIES[0], False),)) for prec, f16 in PRECISIONS]
OPERATOR_B = 203
REGIMES = ("uniform", "peaked", "underflow")
OPERATOR_ROWS = [(A, regime) for regime in REGIMES for A in range(1, 19)]


def engine_id(r):
    return "n%d-M%d-H%d-A%d-%s-%s" % (r[0], r[1], r[2], r[3], r[4], "f16" if r[5] else "f32")


# ------------------------------------------------------------------ inputs (CPU only)
def _freeze(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def peaked_batch(seed, logits, values, masks):
    """the batch of a peaked row from its float32 logits [B, A] and values [B]: old log-probs = log_softmax(logits + drift),
    drift = 4.6 x^3 with x hashed in [-1, 1] (most rows near rho = 1, the tails at 1e-2 and 1e1); actions by the inverse
    CDF of the old policy at a hashed uniform, every fifth row its least probable action; advantages of both signs;
    returns; old values within 0.3 of the values (both sides of the value-clip range 0.1)"""
    B, A = logits.shape
    x = hf.hf_range(seed, (B, A), -1, 1).astype(np.float64)
    old_lp = orc.log_softmax((logits.astype(np.float64) + 4.6 * x ** 3).astype(np.float32))
    cdf = np.cumsum(np.exp(old_lp.astype(np.float64)), axis=1)
    u = hf.hf_unit(seed + 1, B).astype(np.float64) * cdf[:, -1]
    actions = np.minimum((cdf < u[:, None]).sum(axis=1), A - 1).astype(np.int64)
    forced = np.arange(B) % 5 == 4
    actions[forced] = np.argmin(old_lp, axis=1)[forced]
    return _freeze(dict(actions=actions, old_lp=old_lp, adv=hf.hf_range(seed + 2, (B,), -1, 1),
                        ret=hf.hf_range(seed + 3, (B,), -1, 1),
                        vold=(values + hf.hf_range(seed + 4, (B,), -0.3, 0.3)).astype(np.float32),
                        masks=np.ascontiguousarray(masks, dtype=np.uint8)))


@functools.lru_cache(maxsize=None)
def operator_case(A, regime):
    """(logits [B, A], values [B], batch) of an operator row"""
    B, seed = OPERATOR_B, 7100 + 40 * REGIMES.index(regime) + A
    masks = (np.arange(B) % 17 != 0).astype(np.uint8)
    values = hf.hf_range(seed + 5, (B,), -1, 1)
    if regime == "uniform":  # tests/test_gpu_parity.py's
        logits = hf.hf_range(seed, (B, A), -2, 2)
        batch = _freeze(dict(actions=(hf.hf_u32(seed + 1, B) % np.uint32(A)).astype(np.int64),
                             old_lp=orc.log_softmax(hf.hf_range(seed + 2, (B, A), -2, 2)),
                             adv=hf.hf_range(seed + 3, (B,), -2, 2), ret=hf.hf_range(seed + 4, (B,), -1.5, 1.5),
                             masks=masks))
    else:  # every row's logits stretched to a hashed spread
        lo, hi = (20.0, 45.0) if regime == "peaked" else (90.0, 120.0)
        raw = hf.hf_range(seed, (B, A), 0, 1).astype(np.float64)
        span = np.maximum(raw.max(axis=1) - raw.min(axis=1), 1e-30)[:, None]
        spread = hf.hf_range(seed + 6, (B,), lo, hi).astype(np.float64)[:, None]
        offset = hf.hf_range(seed + 7, (B,), -3, 3).astype(np.float64)[:, None]
        logits = ((raw - raw.min(axis=1)[:, None]) / span * spread - spread / 2 + offset).astype(np.float32)
        batch = peaked_batch(seed + 10, logits, values, masks)
    logits.setflags(write=False)
    values.setflags(write=False)
    return logits, values, batch


def operator_reference(A, regime):
    """backward_ref.head on the identity head of aleppo_ppo_loss: h = (logits, values, 0 ...) of width 32, E = 0"""
    logits, values, batch = operator_case(A, regime)
    B = logits.shape[0]
    h = np.zeros((B, 32), np.float32)
    h[:, :A], h[:, A] = logits, values
    wh = np.eye(A + 1, 32, dtype=np.float32)
    return br.head(h, wh, np.zeros(A + 1, np.float32), batch, HYPER, int(batch["masks"].sum()), exact_logits=True), (h, wh)


# (n, H, A): which hashed parameter set of the row's, the first one on which the row is not trivial (tests/test_head_ref_cpu.py
# asserts it: among 37 rows of 10 or 18 actions few sets have one with an entropy below 1e-3 at a spread of at most 45)
PARAM_SET = {(37, 32, 10): 1, (37, 32, 18): 4, (37, 96, 18): 4, (37, 512, 18): 1}


@functools.lru_cache(maxsize=None)
def engine_case(n, H, A, param_set=None):
    """(parameters, observations, batch) of an engine row: test_gpu_layers.row_inputs' observations, hashed parameters with
    the action head's weights and biases scaled so that the largest per-row logit spread of the CPU oracle's fp32 forward
    is SPREAD, and peaked_batch on that forward's logits and values; every seventh sample masked"""
    k = PARAM_SET.get((n, H, A), 0) if param_set is None else param_set
    obs = row_inputs(n, H, A, False)[1]
    params0 = hf.fill_params(9800 + n + H + A + 1000 * k, H, A)
    offs = orc.param_offsets(H, A)
    logits0, values = orc.net_forward(params0, H, A, obs)
    spread0 = float((logits0.max(axis=1) - logits0.min(axis=1)).max())
    params = np.array(params0)
    if spread0 > 0:
        params[offs[8]:offs[10]] *= np.float32(SPREAD / spread0)
    params.setflags(write=False)
    logits, values2 = orc.net_forward(params, H, A, obs)
    assert np.array_equal(values, values2)
    masks = (np.arange(n) % 7 != 6).astype(np.uint8)
    return params, obs, peaked_batch(9950 + n + H + A, logits, values, masks)


def stored_batch(batch, f16):
    """the batch as a context with these planes stores it"""
    out = dict(batch)
    for k in ("old_lp", "adv", "ret", "vold"):
        out[k] = hr.as_stored(batch[k], f16)
    return out


def head_options(batch, advn, beta, vclip):
    """backward_ref.head's options of a variant on one minibatch's (stored) samples"""
    opts = dict(beta=beta)
    if advn:
        opts["advs"] = ur.stats(batch["adv"], batch["masks"])[3:]
    if vclip:
        opts["vold"] = batch["vold"]
    return opts


def take(batch, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in batch.items()}


# ------------------------------------------------------------------ the operator
def _ratio(worst):
    return " ".join("%s %.3g" % (k.split("_")[0], v) for k, v in worst.items())


@pytest.mark.parametrize("A,regime", OPERATOR_ROWS, ids=["A%d-%s" % r for r in OPERATOR_ROWS])
def test_operator_every_plane_and_gradient(pkg, A, regime):
    logits, values, batch = operator_case(A, regime)
    hd, _ = operator_reference(A, regime)
    assert np.abs(hd.logr).max() <= 40
    o = pkg.losses.compute(logits, batch["old_lp"], batch["actions"], batch["adv"], values, batch["ret"], batch["masks"],
                           HYPER["clip"], HYPER["c_v"], HYPER["c_e"])
    got = {k: getattr(o, k) for k in ("total_losses", "clipped_losses", "value_losses", "entropies", "ratio")}
    failures, worst = hr.check_planes(hd, got)
    bad, worst["g"] = hr.check_g(hd, np.concatenate([o.dlogits, o.dvalues[:, None]], axis=1))
    failures += bad
    mean, bound = hr.mean_bound(o.total_losses, batch["masks"])
    worst["loss"] = abs(float(o.loss[0]) - mean) / bound
    amb = hr.ambiguous_rows(hd)
    small = hd.T != 0
    print("HEADSTAT operator A%d %s: worst |d| / bound: %s; ambiguous rows %d of %d; underflow rows %d" % (
        A, regime, _ratio(worst), int(amb.sum()), len(amb), int(small.sum())))
    if regime == "underflow" and A > 1:
        # what the device's expf does below the smallest normal (a report, no assertion): where p_a is subnormal and the
        # exact gradient m gs p_a is still a subnormal fp32 value, a flushed p_a leaves dlogits exactly 0
        sub = (hd.p < hr.TINY) & (np.abs(hd.g[:, :A]) >= 2.0 ** -140) & (hd.m != 0)[:, None]
        print("HEADSTAT operator A%d underflow: %d gradients of subnormal p, %d of them non-zero on the device" % (
            A, int(sub.sum()), int(((o.dlogits != 0) & sub).sum())))
    assert not failures, failures
    assert worst["loss"] <= 1
    assert amb.mean() <= hr.AMBIGUOUS_CAP



# ------------------------------------------------------------------ the engine
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _engine(pkg, n, H, A, prec, f16):
    eng = pkg.Engine(n, 1, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32,
                     rollout_precision=pkg.ROLLOUT_FP16 if f16 else pkg.ROLLOUT_FP32)
    eng.set_hyper(max_grad_norm=MAX_NORM)
    return eng


def _set_variant(pkg, eng, advn, beta, vclip):
    eng.set_option(pkg.OPT_VALUE_CLIP, int(vclip))
    eng.set_option(pkg.OPT_ADV_NORM_MINIBATCH, int(advn))
    eng.set_option(pkg.OPT_KL_PENALTY, int(beta is not None))
    eng.set_kl_coef(0.0 if beta is None else beta)


def _update(pkg, eng, params, M, kl):
    """train(lr = 0, 1 epoch, M minibatches): the parameters stay bit-identical and the clip factor is exactly 1.  Returns
    what the update left: metrics, the export (fc, dfc) of the last minibatch, the gradient, planes [M, B], means [M]"""
    m = eng.train(0.0, 1, M)
    assert np.array_equal(_bits(eng.export_params()), _bits(params))
    norm = np.float32(m["grad_norm"][0, M - 1])
    assert np.isfinite(norm) and np.float32(MAX_NORM) / (norm + np.float32(1e-6)) >= 1
    exp, B, stored = eng.export_backward(("fc", "dfc"))
    names = [k for k in hr.PLANES if kl or k != "kl"]
    planes = {k: eng.read_train_metric(k, 1, M, B)[0] for k in names}
    diag = eng.train_diagnostics(1, M)
    means = dict(total_losses=m["loss"][0], approx_kl=diag["approx_kl"][0], clip_fraction=diag["clip_fraction"][0])
    if kl:
        means["kl"] = eng.kl_divergence(1, M)[0]
    return dict(m=m, exp=exp, B=B, grads=eng.export_grads(), planes=planes, means=means)


def _check_variant(title, out, params, H, A, bf16, obs, batch, M, advn, beta, vclip, stats=None):
    """every check of one variant's update on the last minibatch (and the means of every minibatch).  batch: the stored
    batch of all N samples.  Returns (failures, figures)"""
    B = out["B"]
    failures, fig = [], {}
    # the means, on the engine's own planes
    for k in range(M):
        mk = batch["masks"][k * B:(k + 1) * B]
        for name, got in out["means"].items():
            mean, bound = hr.mean_bound(out["planes"][name][k], mk)
            r = abs(float(got[k]) - mean) / bound if bound > 0 else float(float(got[k]) != mean)
            fig["mean " + name] = max(fig.get("mean " + name, 0.0), r)
            if not r <= 1:
                failures.append("mean %s of minibatch %d: got %r, want %r, bound %r" % (name, k, float(got[k]), mean, bound))
        if stats is not None:  # the advantage statistics: mean_f exactly or one ulp, std to one ulp
            _, mean, std, mean_f, _ = ur.stats(batch["adv"][k * B:(k + 1) * B], mk)
            for what, got, want in (("mean", stats[0][0, k], mean_f), ("std", stats[1][0, k], np.float32(std))):
                if abs(float(got) - float(want)) > float(np.spacing(np.abs(want))):
                    failures.append("advantage %s of minibatch %d: got %r, want %r" % (what, k, float(got), float(want)))
    idx = np.arange((M - 1) * B, M * B)
    mb = take(batch, idx)
    opts = head_options(mb, advn, beta, vclip)
    bad, report, results = br.check_backward(params, H, A, bf16, obs[idx], mb, HYPER, int(mb["masks"].sum()), out["exp"],
                                             out["grads"], None, ("head",), head_opts=opts)
    failures += bad
    hd = results["head"]["head"]
    fig["dh single"] = results["dfc"]["single"] if bf16 else float("nan")
    if not bf16:
        fig["dh"] = results["dfc"]["c"]["worst"]
    fig["dWh"], fig["dbh"] = results["heads.w"]["c"]["worst"], results["heads.b"]["c"]["worst"]
    bad, worst = hr.check_planes(hd, {k: v[M - 1] for k, v in out["planes"].items()})
    failures += bad
    fig.update(worst)
    # the clip fraction from the engine's OWN ratio plane: the same register, so bit for bit (float32 arithmetic)
    rho = out["planes"]["ratio"][M - 1]
    own = (np.abs(rho - np.float32(1)) > np.float32(HYPER["clip"])).astype(np.float32)
    if not np.array_equal(own, out["planes"]["clip_fraction"][M - 1]):
        failures.append("clip_fraction: not |ratio - 1| > clip of the engine's own ratio plane")
    amb = hr.ambiguous_rows(hd)
    fig["ambiguous"] = int(amb.sum())
    if amb.mean() > hr.AMBIGUOUS_CAP and len(amb) >= 16:
        failures.append("ambiguous rows: %d of %d, over the cap" % (amb.sum(), len(amb)))
    return ["%s: %s" % (title, f) for f in failures], fig


def _figures(fig):
    return " ".join("%s %.3g" % kv for kv in fig.items())


@pytest.mark.parametrize("row", ENGINE_ROWS, ids=[engine_id(r) for r in ENGINE_ROWS])
def test_engine_every_variant_on_its_own_exported_h(pkg, row):
    n, M, H, A, prec, f16, variants = row
    params, obs, raw = engine_case(n, H, A)
    batch = stored_batch(raw, f16)
    bf16 = prec == "bf16"
    eng = _engine(pkg, n, H, A, prec, f16)
    eng.load_params(params)
    eng.set_batch(obs, raw["actions"], raw["old_lp"], raw["adv"], raw["ret"], raw["masks"], values=raw["vold"])
    failures = []
    for (entry, advn, beta), vclip in variants:
        _set_variant(pkg, eng, advn, beta, vclip)
        out = _update(pkg, eng, params, M, beta is not None)
        assert out["B"] == n // M
        stats = eng.advantage_stats(1, M) if advn else None
        title = "%s %s%s" % (engine_id(row), entry, " vclip" if vclip else "")
        bad, fig = _check_variant(title, out, params, H, A, bf16, obs, batch, M, advn, beta, vclip, stats)
        print("HEADSTAT engine %s: %s" % (title, _figures(fig)))
        failures += bad
    eng.close()
    assert not failures, failures


# ------------------------------------------------------------------ bit equalities
def _run(pkg, n, H, A, prec, f16, params, obs, batch, advn, beta, vclip, vrange=None):
    eng = _engine(pkg, n, H, A, prec, f16)
    if vrange is not None:
        eng.set_hyper(value_clip_range=vrange)
    eng.load_params(params)
    eng.set_batch(obs, batch["actions"], batch["old_lp"], batch["adv"], batch["ret"], batch["masks"], values=batch["vold"])
    _set_variant(pkg, eng, advn, beta, vclip)
    out = _update(pkg, eng, params, 1, beta is not None)
    eng.close()
    return out


def _assert_same_bits(a, b, what):
    for k in hr.PLANES[:7]:
        assert np.array_equal(_bits(a["planes"][k]), _bits(b["planes"][k])), (what, k)
    assert np.array_equal(_bits(a["exp"]["dfc"]), _bits(b["exp"]["dfc"])), what
    assert np.array_equal(_bits(a["grads"]), _bits(b["grads"])), what
    assert np.array_equal(_bits(a["m"]["loss"]), _bits(b["m"]["loss"])), what
    assert a["exp"]["dfc"].any()


@pytest.mark.parametrize("prec,f16", PRECISIONS)
@pytest.mark.parametrize("A", [7, 10, 11])
def test_kl_option_at_beta_zero_is_the_option_off(pkg, A, prec, f16):
    n, H = 37, 32
    params, obs, batch = engine_case(n, H, A)
    off = _run(pkg, n, H, A, prec, f16, params, obs, batch, True, None, True)
    on = _run(pkg, n, H, A, prec, f16, params, obs, batch, True, 0.0, True)
    _assert_same_bits(on, off, "beta = 0")
    assert on["planes"]["kl"].any()


@pytest.mark.parametrize("prec,f16", PRECISIONS)
def test_value_clipping_at_a_range_of_1e30_is_the_option_off(pkg, prec, f16):
    n, H, A = 37, 32, 6
    params, obs, batch = engine_case(n, H, A)
    off = _run(pkg, n, H, A, prec, f16, params, obs, batch, False, BETA, False)
    on = _run(pkg, n, H, A, prec, f16, params, obs, batch, False, BETA, True, vrange=1e30)
    _assert_same_bits(on, off, "value clip range 1e30")
    clipped = _run(pkg, n, H, A, prec, f16, params, obs, batch, False, BETA, True)  # (and the option does something)
    assert not np.array_equal(_bits(clipped["planes"]["value_losses"]), _bits(off["planes"]["value_losses"]))


def unit_stats_batch(batch):
    """the batch with advantages whose statistics over the unmasked samples are exactly (0, 1): an even number of +-1 and
    a single 0 (sum 0, sum of squares n - 1, so the variance over n - 1 is exactly 1 and fp32(1 / (1 + 1e-8)) is 1)"""
    out = dict(batch)
    masks = np.array(batch["masks"])
    live = np.flatnonzero(masks)
    if len(live) % 2 == 0:
        masks[live[-1]] = 0
        live = live[:-1]
    adv = np.array(batch["adv"])
    adv[live] = np.where(np.arange(len(live)) % 2 == 0, 1.0, -1.0)
    adv[live[-1]] = 0.0
    out.update(adv=adv.astype(np.float32), masks=masks)
    assert ur.stats(out["adv"], out["masks"])[3:] == (np.float32(0), np.float32(1))
    return out


@pytest.mark.parametrize("prec,f16", PRECISIONS)
def test_normalisation_with_statistics_0_and_1_is_the_option_off(pkg, prec, f16):
    n, H, A = 37, 32, 6
    params, obs, batch = engine_case(n, H, A)
    batch = unit_stats_batch(batch)
    for beta in (None, BETA):  # head_train_advn_kernel, and head_train_kl_kernel with and without its statistics
        off = _run(pkg, n, H, A, prec, f16, params, obs, batch, False, beta, True)
        on = _run(pkg, n, H, A, prec, f16, params, obs, batch, True, beta, True)
        _assert_same_bits(on, off, "statistics (0, 1), beta %r" % beta)
