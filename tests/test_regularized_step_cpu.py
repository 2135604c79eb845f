"""The regularised optimizer step and shrink and perturb without a GPU: the bound of tests/reg_ref.py holds with room for
plain fp32 arithmetic and rejects the planted mistakes; the numpy restatement of aleppo_shrink_perturb draws recycle_ref's
values; the header, the Python mirror and the host-only stand-in agree on the option numbers, the symbols and ABI version
2; and the trainer's weight_decay / l2_init_coef / shrink_perturb_* keys on the stand-in (tests/stub/aleppo_stub_reg.cc):
the recorded calls, the anchor taken once before update 1, the checkpoint's optional section 8 written, required and
restored, and the files of runs without the keys unchanged byte for byte."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import adam_ref as ar
import recycle_ref as rr
import reg_ref as rg
import trainer_helpers
from conftest import ROOT

# the coefficients the GPU tests use (tests/test_regularized_step.py): the regime where the terms dominate - f_wd = 1e-2,
# f_an = 2e-2 at lr = 1e-3 - and one realistic row, torch.optim.AdamW's default decay at the benched rate
DOMINANT = dict(lr=1e-3, wd=10.0, la=20.0)
REALISTIC = dict(lr=2.5e-4, wd=1e-2, la=0.0)
T_STEPS = (1, 2, 10, 1000, 10 ** 6)
H, A = 32, 4
N_PARAMS = 32 * 256 + 32 + 64 * 512 + 64 + 64 * 576 + 64 + H * 3136 + H + A * H + A + H + 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the bound
def test_factors_are_one_rounding_of_the_double_product():
    f_wd, f_an = rg.factors(**DOMINANT)
    assert f_wd == np.float32(1e-2) and f_an == np.float32(2e-2)
    f_wd, f_an = rg.factors(**REALISTIC)
    assert f_wd == np.float32(2.5e-4 * float(np.float32(1e-2))) and f_an == 0 and _bits(f_an) == 0


@pytest.mark.parametrize("coef", [DOMINANT, REALISTIC, dict(lr=1e-3, wd=10.0, la=0.0), dict(lr=1e-3, wd=0.0, la=20.0)],
                         ids=["dominant", "realistic", "decay alone", "anchor alone"])
def test_fp32_restatement_within_half_of_every_bound(coef):
    """adam_element and reg_element in plain numpy float32 sit within 0.5 of every bound on adam_ref's hashed step inputs
    with a hashed anchor: the bounds are twice the plain operation count"""
    n = 1 << 18
    worst = {q: 0.0 for q in rg.QUANTITIES}
    for k, t in enumerate(T_STEPS):
        p0, m0, v0, g = ar.hashed_step_inputs(8000 + 100 * k, n)
        anchor = rg.hashed_anchor(8050 + 100 * k, n) if coef["la"] else None
        after = rg.reg_element_f32(p0, m0, v0, g, t, anchor=anchor, **coef)
        r = rg.ratios((p0, m0, v0), after, g, t, anchor=anchor, **coef)
        for q in rg.QUANTITIES:
            worst[q] = max(worst[q], float(r[q].max()))
    print("fp32 restatement, worst ratio to bound:", {q: "%.3g" % x for q, x in worst.items()})
    for q in rg.QUANTITIES:
        assert 0.1 < worst[q] <= 0.5, (q, worst[q])


def test_zero_coefficients_are_adam_ref_and_exact_zeros_stay_exact():
    """with both coefficients zero the reference and the bound of the moments are adam_ref's and p's bound is adam_ref's
    plus 2u |p|; where a bound is exactly 0 any difference fails"""
    n = 1 << 14
    p0, m0, v0, g = ar.hashed_step_inputs(8300, n)
    a, b = ar.reference_step(p0, m0, v0, g, 3, 1e-3), rg.reference_step(p0, m0, v0, g, 3, 1e-3)
    for k in ("p", "m", "v", "tol_m", "tol_v"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(b["tol_p"], a["tol_p"] + 2 * rg.U * np.abs(a["p"]))
    anchor = rg.hashed_anchor(8301, n)
    anchor[:64] = 0
    p0[:64], m0[:64], v0[:64], g[:64] = 0, 0, 0, 0  # (alignment pads: everything zero, and it stays zero)
    p, m, v = rg.reg_element_f32(p0, m0, v0, g, 3, anchor=anchor, **DOMINANT)
    ref = rg.reference_step(p0, m0, v0, g, 3, anchor=anchor, **DOMINANT)
    assert not ref["tol_p"][:64].any() and not _bits(p[:64]).any()
    offs = np.linspace(0, n, 13).astype(np.int64)
    assert not rg.check_step((p0, m0, v0), (p, m, v), g, 3, DOMINANT["lr"], offs, DOMINANT["wd"], DOMINANT["la"],
                             anchor).failures
    bad = p.copy()
    bad[5] = np.float32(1e-45)
    res = rg.check_step((p0, m0, v0), (bad, m, v), g, 3, DOMINANT["lr"], offs, DOMINANT["wd"], DOMINANT["la"], anchor)
    assert [(f[1], f[2], f[3]) for f in res.failures] == [("p", np.inf, 5)]


def _mutations(lr, wd, la):
    """name -> function(p0, m0, v0, g, t, anchor) -> (p, m, v) in float64: the regularised step with one planted mistake"""
    wd32, la32 = float(rg.f32_option(wd)), float(rg.f32_option(la))

    def step(p0, m0, v0, g, t, anchor, f_wd=None, f_an=None, decay_of="p0", sign=-1.0, read_anchor=True):
        s, c = ar.step_scalars(t, lr)
        q, m, v, _ = ar.adam_f64(p0, m0, v0, g, s, c)
        fw, fa = rg.factors(lr, wd, la)
        fw = float(fw) if f_wd is None else f_wd(float(s))
        fa = float(fa) if f_an is None else f_an(float(s))
        p0 = np.asarray(p0, np.float64)
        a = np.asarray(anchor, np.float64) if read_anchor else 0.0
        t1 = fw * (q if decay_of == "q" else p0)
        t2 = fa * (p0 + sign * a)
        return q - (t1 + t2), m, v

    return {
        "decay missing": lambda *x: step(*x, f_wd=lambda s: 0.0),
        "decay of q instead of p0": lambda *x: step(*x, decay_of="q"),
        "wd without the factor lr": lambda *x: step(*x, f_wd=lambda s: wd32),
        "the step size s in place of lr": lambda *x: step(*x, f_wd=lambda s: s * wd32, f_an=lambda s: s * la32),
        "anchor sign flipped": lambda *x: step(*x, sign=+1.0),
        "anchor read as zero": lambda *x: step(*x, read_anchor=False),
    }


# The share of elements on which a mistake must be rejected, from the size of what it changes against the bound, which is
# about 4u |p| = 2.4e-7 |p| (Adam's own term adds at most 20u s <= 7e-9), |p0|, |a| uniform below 0.1:
#   DOMINANT (f_wd = 1e-2, f_an = 2e-2, s = 5.3e-3 at t = 2)
#     decay missing, wd without lr, s in place of lr: the change is >= 1e-2 |p0|, 4e4 bounds - all but p0 = 0         >= 0.99
#     anchor sign flipped, anchor read as zero: >= 2e-2 |a| - all but a = 0                                            >= 0.99
#     decay of q: f_wd |q - p0| = 1e-2 s |m / d|; nothing where g = m0 = 0 (adam_ref's inputs: a third of g is zero and a
#       fifth of the moments, the rest of m0 is log-uniform down to 1e-12 against d >= 1e-5) - as in adam_ref's own
#       mutation test                                                                                                  >= 0.2
#   REALISTIC (f_wd = 2.5e-6, no anchor): the three mistakes that change the factor itself move p by >= 2.5e-6 |p0|, ten
#     bounds of an element whose step is small against p0.  adam_ref's hashed moments are not reachable states: |m0| up to 1
#     over sqrt(v0) down to 1e-12 gives steps far above |p0| on a few per cent of the elements, whose bound 2u |q| grows
#     with the step and hides a change of 2.5e-6 |p0|                                                                  >= 0.9
#     decay of q changes p by 2.5e-6 s |m / d| <= 3e-9, below the bound of most elements, and the two anchor mistakes
#     change nothing at la = 0: no share is demanded of them there
SHARES = {
    "dominant": (DOMINANT, {"decay missing": 0.99, "decay of q instead of p0": 0.2, "wd without the factor lr": 0.99,
                            "the step size s in place of lr": 0.99, "anchor sign flipped": 0.99,
                            "anchor read as zero": 0.99}),
    "realistic": (REALISTIC, {"decay missing": 0.9, "wd without the factor lr": 0.9,
                              "the step size s in place of lr": 0.9}),
}


@pytest.mark.parametrize("regime", sorted(SHARES))
def test_checker_rejects_each_planted_mistake(regime):
    coef, want = SHARES[regime]
    n, t = 1 << 18, 2
    p0, m0, v0, g = ar.hashed_step_inputs(8400, n)
    anchor = rg.hashed_anchor(8401, n)
    offs = np.linspace(0, n, 13).astype(np.int64)

    def rejected(after):
        r = rg.ratios((p0, m0, v0), tuple(np.asarray(a, np.float64).astype(np.float32) for a in after), g, t,
                      anchor=anchor, **coef)
        return float(np.mean(np.maximum(np.maximum(r["m"], r["v"]), r["p"]) > 1.0))

    ref = rg.reference_step(p0, m0, v0, g, t, anchor=anchor, **coef)
    assert rejected((ref["p"], ref["m"], ref["v"])) == 0.0
    shares = {}
    for name, step in _mutations(**coef).items():
        if name not in want:
            continue
        after = tuple(a.astype(np.float32) for a in step(p0, m0, v0, g, t, anchor))
        shares[name] = rejected(after)
        assert rg.check_step((p0, m0, v0), after, g, t, coef["lr"], offs, coef["wd"], coef["la"], anchor).failures, name
    print(f"{regime}: share of elements rejected:", {k: "%.3g" % v for k, v in shares.items()})
    assert set(shares) == set(want)
    for name, share in shares.items():
        assert share >= want[name], (name, share)


# ------------------------------------------------------------------ shrink and perturb
def test_shrink_perturb_restatement_draws_recycle_refs_values():
    key = 0x1234ABCD5678
    offs = ar.param_offsets(H, A)
    xi = rg.perturbation(key, H, A)
    assert xi.size == N_PARAMS == int(offs[-1])
    for k, layer in zip((0, 2, 4, 6), rr.LAYERS):  # the trunk weights: recycle_ref's re-initialisation at the same index
        idx = np.arange(int(offs[k]), int(offs[k + 1]))
        assert np.array_equal(_bits(xi[idx]), _bits(rr.reinit_values(key, idx, layer))), layer
        assert np.abs(xi[idx]).max() <= rr.bound(layer) and np.abs(xi[idx]).max() > 0.9 * rr.bound(layer)
    a_h = np.float32(np.sqrt(6.0 / H))
    for k in (8, 10):  # the head weight rows: fan_in = H
        sl = slice(int(offs[k]), int(offs[k + 1]))
        assert np.abs(xi[sl]).max() <= a_h and xi[sl].std() > 0.4 * a_h
    for k in (1, 3, 5, 7, 9, 11):  # biases only shrink
        assert not _bits(xi[int(offs[k]):int(offs[k + 1])]).any()
    p = ar.hashed_step_inputs(8500, N_PARAMS)[0]
    out = rg.shrink_perturb(p, 0.8, 0.1, key, H, A)
    want = (np.float32(0.8) * p).astype(np.float32) + (np.float32(0.1) * xi).astype(np.float32)
    assert np.array_equal(_bits(out), _bits(want))
    assert np.array_equal(_bits(rg.shrink_perturb(p, 1.0, 0.0, key, H, A)), _bits(p))  # changes no bit
    assert not np.array_equal(rg.perturbation(key + 1, H, A), xi)
    b = slice(int(offs[7]), int(offs[8]))
    assert np.array_equal(_bits(out[b]), _bits(np.float32(0.8) * p[b]))


# ------------------------------------------------------------------ header, mirror, stand-in
def test_header_mirror_and_stub_agree():
    from __graft_entry__ import load_package
    pkg = load_package()
    hdr = open(os.path.join(ROOT, "include", "aleppo.h")).read()
    assert trainer_helpers.header_const("ALEPPO_OPT_WEIGHT_DECAY") == pkg.OPT_WEIGHT_DECAY == 26
    assert trainer_helpers.header_const("ALEPPO_OPT_ANCHOR_COEF") == pkg.OPT_ANCHOR_COEF == 27
    assert trainer_helpers.header_const("ALEPPO_SP_RESET_MOMENTS", stripped=True) == pkg.SP_RESET_MOMENTS == 1
    assert trainer_helpers.header_const("ALEPPO_ABI_VERSION", stripped=True) == 2
    assert not re.search(r"(?m)^\s*ALEPPO_OPT_\w+\s*=\s*22\b", hdr)  # 22 stays unassigned
    assert pkg.REG_OPTIONS == dict(weight_decay=26, anchor_coef=27)
    stub = open(os.path.join(ROOT, "tests", "stub", "aleppo_stub_reg.cc")).read()
    for sym in ("aleppo_anchor_take", "aleppo_anchor_import", "aleppo_anchor_export", "aleppo_shrink_perturb"):
        assert re.search(rf"(?m)^int {sym}\(aleppo_ctx \*ctx", hdr), sym
        assert sym in pkg.EXPORTS and re.search(rf"(?m)^int {sym}\(aleppo_ctx \*c", stub), sym
        assert hasattr(pkg.Engine, dict(aleppo_anchor_take="anchor_take", aleppo_anchor_import="load_anchor",
                                        aleppo_anchor_export="anchor_params",
                                        aleppo_shrink_perturb="shrink_perturb")[sym])
    assert hasattr(pkg.Engine, "set_regularization") and hasattr(pkg.Engine, "regularization")
    ck = open(os.path.join(ROOT, "trainer", "checkpoint.hpp")).read()
    assert re.search(r"CK_EMA = 7,", ck) and re.search(r"CK_ANCHOR = 8 \}", ck)


# ------------------------------------------------------------------ the trainer's keys on the stand-in
@pytest.fixture(scope="module")
def reg_trainer():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_reg_stub"])
    return os.path.join(ROOT, "trainer", "train_reg_stub")


def _run_trainer(binary, d, extra, rollouts=4, env=None):
    os.makedirs(d / "tb", exist_ok=True)
    cfg = trainer_helpers.debug_cfg(d, extra, rollouts)
    return subprocess.run([binary, "breakout.bin", str(d / "tb" / "run.log"), str(d), "g", str(cfg)], capture_output=True,
                          text=True, timeout=300, env=dict(os.environ, **(env or {})))


def _sections(blob):
    """{id: bytes} of a checkpoint file (little-endian: magic, version, the 40-byte shape, sections, the end mark)"""
    assert blob[:8] == b"ALEPPOCK" and blob[-8:] == b"ALEPPOEN" and struct.unpack("<I", blob[8:12])[0] == 1
    pos, out = 12 + 40, {}
    while pos < len(blob) - 8:
        sid, n = struct.unpack("<IQ", blob[pos:pos + 12])
        out[sid] = blob[pos + 12:pos + 12 + n]
        pos += 12 + n
    assert pos == len(blob) - 8
    return out


def _counts(r):
    m = re.search(r"stub: aleppo_anchor_take calls: (\d+)\nstub: aleppo_shrink_perturb calls: (\d+)", r.stderr)
    assert m, r.stderr[-2000:]
    return int(m.group(1)), int(m.group(2))


def _splitmix64(x):
    return rr.splitmix64(x)


SP = re.compile(r"stub: aleppo_shrink_perturb shrink=(\S+) sigma=(\S+) key=(\S+) flags=(\d+) trains=(\d+)")


def test_keys_reach_the_library_and_absent_keys_change_nothing(reg_trainer, tmp_path):
    runs = {"absent": "", "decay": "weight_decay: 0.01\n", "all": "weight_decay: 0.01\nl2_init_coef: 0.02\n"
            "shrink_perturb_interval: 2\nshrink_perturb_shrink: 0.8\nshrink_perturb_sigma: 0.1\n"}
    out, ck, blobs = {}, {}, {}
    for name, extra in runs.items():
        d = tmp_path / name
        d.mkdir()
        r = out[name] = _run_trainer(reg_trainer, d, extra + f"checkpoint_path: {d / 'run.ckpt'}\n", 4)
        assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
        ck[name] = (d / "run.ckpt").read_bytes()
        blobs[name] = trainer_helpers.events(d / "tb")
    # absent: no call at all, no option, no section, nothing in the hparams
    assert _counts(out["absent"]) == (0, 0) and "ALEPPO_OPT_" not in out["absent"].stderr
    assert "aleppo_anchor" not in out["absent"].stderr.replace("aleppo_anchor_take calls", "")
    assert sorted(_sections(ck["absent"])) == [1, 2, 3, 4, 5, 6]
    for key in (b"weight_decay", b"l2_init_coef", b"shrink_perturb"):
        assert key not in blobs["absent"]
    # weight decay alone: the option with float32(0.01)'s bits, no anchor, and a file that is the absent run's byte for byte
    # (the stand-in's update does not decay)
    assert "stub: aleppo_set_option ALEPPO_OPT_WEIGHT_DECAY bits=3c23d70a" in out["decay"].stderr
    assert _counts(out["decay"]) == (0, 0) and "ALEPPO_OPT_ANCHOR_COEF" not in out["decay"].stderr
    assert ck["decay"] == ck["absent"] and b"weight_decay" in blobs["decay"]
    # all: both options, the anchor taken ONCE, from the live set, before update 1 and before the coefficient is set
    err = out["all"].stderr
    assert _counts(out["all"]) == (1, 2)
    assert err.count("stub: aleppo_anchor_take source=0 trains=0") == 1
    assert "stub: aleppo_set_option ALEPPO_OPT_ANCHOR_COEF bits=3ca3d70a" in err
    assert err.index("stub: aleppo_anchor_take source=0") < err.index("ALEPPO_OPT_ANCHOR_COEF")
    # shrink and perturb after the update of rollouts 2 and 4, keyed like the recycle: splitmix64(seed ^ rollout index)
    seed = int(re.search(r"(?m)^seed:\s*(\d+)", open(tmp_path / "all" / "d.yaml").read() + "\nseed: 42").group(1))
    calls = SP.findall(err)
    assert [(c[0], c[1], c[3], c[4]) for c in calls] == [("%.17g" % 0.8, "%.17g" % 0.1, "0", "2"),
                                                         ("%.17g" % 0.8, "%.17g" % 0.1, "0", "4")]
    assert [int(c[2], 16) for c in calls] == [_splitmix64(seed ^ 1), _splitmix64(seed ^ 3)]
    for key in (b"weight_decay", b"l2_init_coef", b"shrink_perturb_interval", b"shrink_perturb_shrink",
                b"shrink_perturb_sigma"):
        assert key in blobs["all"]
    # section 8: the anchor - the parameters the run started from, not the ones it ended with
    sec = _sections(ck["all"])
    assert sorted(sec) == [1, 2, 3, 4, 5, 6, 8] and len(sec[8]) == N_PARAMS * 4
    init = tmp_path / "init.bin"
    r = _run_trainer(reg_trainer, tmp_path / "all", runs["all"], 4, env=dict(ALEPPO_TRAINER_DUMP_INIT=str(init)))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sec[8] == init.read_bytes() and sec[8] != sec[1]


def test_resume_requires_restores_and_ignores_the_section(reg_trainer, tmp_path):
    keys = "l2_init_coef: 0.5\nweight_decay: 0.01\n"
    full, part, off = tmp_path / "full", tmp_path / "part", tmp_path / "off"
    for d in (full, part, off):
        d.mkdir()
    r = _run_trainer(reg_trainer, full, keys + f"checkpoint_path: {full / 'run.ckpt'}\ncheckpoint_interval: 2\n", 4)
    assert r.returncode == 0 and "Success" in r.stdout, r.stderr[-2000:]
    ck = part / "run.ckpt"
    ckeys = keys + f"checkpoint_path: {ck}\ncheckpoint_interval: 2\n"
    p = _run_trainer(reg_trainer, part, ckeys, 4, env=dict(ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT="2"))
    assert p.returncode == 0 and "stopped after the checkpoint of rollout 2" in p.stdout, p.stderr[-2000:]
    anchor2 = _sections(ck.read_bytes())[8]
    # restored: imported before the first update, proved by exporting it again, never taken from the resumed parameters -
    # and the run ends in the uninterrupted run's file, whose parameters the stand-in pulled toward the anchor
    res = _run_trainer(reg_trainer, part, ckeys + f"resume: {ck}\n", 4)
    assert res.returncode == 0 and "Success" in res.stdout, res.stderr[-2000:]
    assert "resumed the anchor, verified" in res.stdout and _counts(res)[0] == 0
    assert "stub: aleppo_anchor_import trains=0" in res.stderr
    assert ck.read_bytes() == (full / "run.ckpt").read_bytes() and _sections(ck.read_bytes())[8] == anchor2
    # the anchor matters to that comparison: a run without it ends elsewhere
    base = f"checkpoint_path: {off / 'run.ckpt'}\ncheckpoint_interval: 2\n"
    p = _run_trainer(reg_trainer, off, base, 4, env=dict(ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT="2"))
    assert p.returncode == 0 and sorted(_sections((off / "run.ckpt").read_bytes())) == [1, 2, 3, 4, 5, 6]
    assert _sections((off / "run.ckpt").read_bytes())[1] != _sections((full / "run.ckpt").read_bytes())[1]
    # required: with the key, a file without the section is refused before anything runs
    res = _run_trainer(reg_trainer, off, base + keys + f"resume: {off / 'run.ckpt'}\n", 4)
    assert res.returncode == 1 and "has no anchor (section 8)" in res.stderr and "Rollout" not in res.stdout
    # ignored: without the key, a file with the section resumes, never touches the anchor, and writes a file without it
    p = _run_trainer(reg_trainer, part, keys + f"checkpoint_path: {part / 'two.ckpt'}\n", 2)
    assert p.returncode == 0 and 8 in _sections((part / "two.ckpt").read_bytes())
    res = _run_trainer(reg_trainer, part, f"checkpoint_path: {part / 'plain.ckpt'}\nresume: {part / 'two.ckpt'}\n", 4)
    assert res.returncode == 0 and "Success" in res.stdout, res.stderr[-2000:]
    assert "aleppo_anchor_import" not in res.stderr and "anchor" not in res.stdout
    assert sorted(_sections((part / "plain.ckpt").read_bytes())) == [1, 2, 3, 4, 5, 6]
    # a section of the wrong size is refused
    blob = (part / "two.ckpt").read_bytes()
    at = blob.rindex(struct.pack("<IQ", 8, N_PARAMS * 4))
    bad = blob[:at] + struct.pack("<IQ", 8, N_PARAMS * 4 - 4) + blob[at + 12:-12] + blob[-8:]
    (part / "bad.ckpt").write_bytes(bad)
    res = _run_trainer(reg_trainer, part, keys + f"resume: {part / 'bad.ckpt'}\n", 4)
    assert res.returncode == 1 and "section 8" in res.stderr and "corrupt" in res.stderr, res.stderr[-2000:]


@pytest.mark.parametrize("extra,message", [
    ("weight_decay: -0.1\n", "weight_decay must be finite and non-negative"),
    ("weight_decay: 1e39\n", "weight_decay must be finite and non-negative"),
    ("l2_init_coef: -1\n", "l2_init_coef must be finite and non-negative"),
    ("l2_init_coef: often\n", "bad value for l2_init_coef"),
    ("shrink_perturb_interval: 0\n", "shrink_perturb_interval must be positive"),
    ("shrink_perturb_shrink: 0.5\n", "shrink_perturb_shrink needs shrink_perturb_interval"),
    ("shrink_perturb_sigma: 0.5\n", "shrink_perturb_sigma needs shrink_perturb_interval"),
    ("shrink_perturb_interval: 2\nshrink_perturb_shrink: 1.5\n", "shrink_perturb_shrink must be in [0, 1]"),
    ("shrink_perturb_interval: 2\nshrink_perturb_sigma: -1\n", "shrink_perturb_sigma must be finite and non-negative"),
])
def test_trainer_refuses_bad_keys(reg_trainer, tmp_path, extra, message):
    r = _run_trainer(reg_trainer, tmp_path, extra)
    assert r.returncode == 1 and message in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    assert _counts(r) == (0, 0)


def test_library_without_the_entry_points_refuses_the_keys(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "trainer"), "train_tsan"])
    plain = os.path.join(ROOT, "trainer", "train_tsan")  # (the stand-in without the anchor and shrink and perturb)
    for k, (extra, message) in enumerate((("l2_init_coef: 0.1\n", "aleppo_anchor_take is missing"),
                                          ("shrink_perturb_interval: 2\n", "aleppo_shrink_perturb is missing"))):
        d = tmp_path / str(k)
        d.mkdir()
        r = _run_trainer(plain, d, extra, 2)
        assert r.returncode == 1 and message in r.stderr and "Rollout" not in r.stdout, r.stderr[-2000:]
    (tmp_path / "off").mkdir()
    assert _run_trainer(plain, tmp_path / "off", "", 2).returncode == 0
