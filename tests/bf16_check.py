"""The bf16 checker: an engine's bf16 update / forward against the bf16-emulating oracle (oracle.h, ORACLE_BF16).

A plain helper module (no fixtures): tests/test_oracle_bf16.py measures on the CPU what the bounds leave room for and
that they catch a single wrong conv3 tap; the GPU tests (test_gpu_bf16_emulated.py, test_gpu_at_size.py,
test_gpu_parity.py) apply them to the kernels.

Bounds.  The emulated oracle rounds at the device's rounding points, so a correct kernel differs from it only by the
order of its fp32 sums and by the bf16 roundings that order flips (one bf16 ulp, 2^-8 relative, each).  How far that
moves a result depends on the batch: the same emulation with sequential fp32 sums instead of double sums (the floor)
differs from it by 7e-5 .. 1.9e-3 relative L2 on the worst gradient tensor and 6e-4 .. 9e-3 on the worst output
channel over the sweep's batches (tests/test_gpu_bf16_emulated.py), and by 2.4e-3 absolute on a logit at N = 512.
So every check is bounded by
    max(base bound, FLOOR_FACTOR x the same measurement of the floor run against the emulation, on the SAME batch)
with FLOOR_FACTOR = 4 (the floor at a quarter of the bound).  emulated_train / emulated_forward return the floor run
with the emulation, and Checker measures it before it checks the engine.  The base bounds are the first estimates:"""
import numpy as np

import oracle_lib as orc

NAMES = ["conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc.w", "fc.b", "action.w", "action.b",
         "value.w", "value.b"]
# engine metric plane -> oracle plane
PLANES = (("total_losses", "total_losses"), ("ratio", "ratio"), ("entropies", "entropies"),
          ("value_losses", "value_losses"), ("clipped_losses", "clipped"))
BOUNDS = dict(
    loss=1e-3,          # |dloss| <= 1e-3 (1 + |loss|)
    grad_norm=1e-3,     # pre-clip norm, relative
    grad=2e-3,          # every gradient tensor, relative L2 (action head included)
    channel=1e-2,       # conv1-3 / fc weight gradients per output channel / row, relative L2
    plane_abs=2e-3,     # per-sample planes: |d| <= 2e-3 + 1e-3 |ref| on every sample
    plane_rel=1e-3,
    out_abs=1e-3,       # logits / values: |d| <= 1e-3 + 1e-3 |ref|
    out_rel=1e-3,
    update=1e-2,        # one step's parameter update as a vector, relative L2
)
FLOOR_FACTOR = 4


def emulated_train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, **kw):
    """orc.train with emulate_bf16=True; result["floor_run"] = the same update with fp32 sums (the floor)"""
    ref = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, emulate_bf16=True, **kw)
    ref["floor_run"] = orc.train(params, H, A, obs, actions, old_lp, adv, ret, masks, epochs, M, emulate_bf16=True,
                                 sums="float32", **kw)
    return ref


def emulated_forward(params, H, A, obs):
    """(logits, values, (floor-run logits, floor-run values)) of the emulated forward"""
    logits, values = orc.net_forward(params, H, A, obs, emulate_bf16=True)
    return logits, values, orc.net_forward(params, H, A, obs, emulate_bf16=True, sums="float32")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def channel_rel(a, b, rows):
    """max over output channels / rows of the relative L2 error; rows whose reference gradient is tiny (dead
    channels) are measured against 10 % of the tensor's rms row norm instead"""
    a = np.asarray(a, np.float64).reshape(rows, -1)
    b = np.asarray(b, np.float64).reshape(rows, -1)
    nb = np.linalg.norm(b, axis=1)
    floor = 1e-1 * np.sqrt(np.mean(nb * nb)) + 1e-30
    return float(np.max(np.linalg.norm(a - b, axis=1) / np.maximum(nb, floor)))


def _clip_coef(norm):
    return min(1.0, 0.5 / (float(norm) + 1e-6))


class Checker:
    """collects named measurements against their bounds; `failures` lists (name, value, bound).  When the reference
    carries a floor run, each bound is max(base, FLOOR_FACTOR x the floor run's own measurement)."""

    def __init__(self, bounds=None):
        self.bounds = dict(BOUNDS, **(bounds or {}))
        self.report, self.limits, self.failures = {}, {}, []
        self.floor = {}

    def check(self, name, value, base):
        bound = max(base, FLOOR_FACTOR * self.floor.get(name, 0.0))
        self.report[name] = float(value)
        self.limits[name] = float(bound)
        if not value <= bound:
            self.failures.append((name, float(value), bound))

    def _measure_floor(self, run):
        f = Checker(self.bounds)
        run(f)
        self.floor.update(f.report)

    def forward(self, logits, values, ref, tag=""):
        """ref: emulated_forward(...) (or a (logits, values) pair: base bounds only)"""
        if len(ref) == 3:
            self._measure_floor(lambda f: f.forward(ref[2][0], ref[2][1], ref[:2], tag))
        b = self.bounds
        for nm, got, r in (("logits", logits, ref[0]), ("values", values, ref[1])):
            got, r = np.asarray(got, np.float64).ravel(), np.asarray(r, np.float64).ravel()
            self.check(f"{tag}{nm}_excess", np.max(np.abs(got - r) - b["out_rel"] * np.abs(r)), b["out_abs"])

    def grads(self, g, gnorm, wg, wnorm, H, A, tag=""):
        """exported (clip-scaled) gradients of the last minibatch, each side unscaled by its own clip coefficient"""
        b = self.bounds
        g = np.asarray(g, np.float64) / _clip_coef(gnorm)
        wg = np.asarray(wg, np.float64) / _clip_coef(wnorm)
        offs = orc.param_offsets(H, A)
        rows = {0: 32, 2: 64, 4: 64, 6: H}
        for k, nm in enumerate(NAMES):
            a, r = g[offs[k]:offs[k + 1]], wg[offs[k]:offs[k + 1]]
            self.check(f"{tag}grad_{nm}", rel(a, r), b["grad"])
            if k in rows:
                self.check(f"{tag}chan_{nm}", channel_rel(a, r, rows[k]), b["channel"])

    def train(self, H, A, m, planes, g, ref, tag="", params0=None, params=None, ref_params0=None):
        """m: engine.train() metrics, planes: {engine plane name: [epochs, M, B]}, g: export_grads() or None, ref:
        emulated_train(...) on the same batch.  The gradients are compared for the LAST minibatch (export_grads), so
        they are on identical parameters only when that is the first step of both sides.  params0 / params: the
        engine's parameters before / after, for the update check (ref_params0: the oracle's start, default params0)."""
        r0 = params0 if ref_params0 is None else ref_params0
        alt = ref.get("floor_run")
        if alt is not None:
            self._measure_floor(lambda f: f.train(
                H, A, alt, {ours: alt[theirs] for ours, theirs in PLANES if ours in planes},
                None if g is None else alt["last_grads"], {k: v for k, v in ref.items() if k != "floor_run"}, tag,
                params0=None if params0 is None else r0,
                params=alt.get("params"), ref_params0=r0))
        b = self.bounds
        loss, wl = np.asarray(m["loss"], np.float64), np.asarray(ref["loss"], np.float64)
        self.check(f"{tag}loss_excess", np.max(np.abs(loss - wl) / (1 + np.abs(wl))), b["loss"])
        self.check(f"{tag}grad_norm_rel", np.max(np.abs(np.asarray(m["grad_norm"], np.float64) / ref["grad_norm"] - 1)),
                   b["grad_norm"])
        for ours, theirs in PLANES:
            if ours in planes:
                got, w = np.asarray(planes[ours], np.float64), np.asarray(ref[theirs], np.float64)
                self.check(f"{tag}{ours}_excess", np.max(np.abs(got - w) - b["plane_rel"] * np.abs(w)), b["plane_abs"])
        if g is not None:
            self.grads(g, m["grad_norm"][-1, -1], ref["last_grads"], ref["grad_norm"][-1, -1], H, A, tag)
        if params0 is not None:
            self.check(f"{tag}update_rel", rel(np.asarray(params, np.float64) - params0,
                                               np.asarray(ref["params"], np.float64) - r0), b["update"])

    def summary(self, title):
        return "%s %s" % (title, {k: "%.3g/%.3g" % (v, self.limits[k]) for k, v in self.report.items()})
