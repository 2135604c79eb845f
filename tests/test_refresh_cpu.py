"""aleppo_refresh_advantages on the CPU: the reference (tests/refresh_ref.py) against the oracle's finish planes, every planted
error failing its own check on the inputs of the GPU rows, the device-order restatement of the statistics inside the derived
bounds, and the header against the Python mirror.  No GPU."""
import os
import re

import numpy as np
import pytest

import hashfill as hf
import oracle_lib as orc
import refresh_ref as rf
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = np.float32(0.9)  # the reward_scale row's stored rewards: r * 0.9, |r| <= 2, so rewards beyond 1 are present


def _inputs(name):
    """the row's flags and rewards (the GPU test's), and synthetic collected / fresh values: env-major planes as stored"""
    E, T, A, H, prec, rt16, mb, scaled, norm = rf.ROWS[name]
    seed = 9100 + 10 * list(rf.ROWS).index(name)
    te, tr, st = (x.T.copy() for x in rf.row_flags(seed, E, T))
    r = rf.row_rewards(seed + 1, E, T).T.copy()
    rew = (r * SCALE).astype(np.float32) if scaled else np.clip(r, -1, 1)  # as aleppo_finish_rollout left them
    v = rf.stored(hf.hf_range(seed + 2, (E, T), -1, 1), rt16)
    nv = rf.stored(hf.hf_range(seed + 3, (E,), -1, 1), rt16)
    step = hf.hf_range(seed + 4, (E, T), 0.01, 0.06) * np.where(hf.hf_unit(seed + 5, E * T).reshape(E, T) < 0.5, -1, 1)
    fresh = (v + step).astype(np.float32)
    fresh_next = (nv + hf.hf_range(seed + 6, (E,), 0.01, 0.06)).astype(np.float32)
    o = orc.buffer_get(rew, v, nv, te, tr, st)  # the planes at entry (what the last epoch trained on)
    adv0, ret0 = rf.stored(o["advantages"], rt16), rf.stored(o["returns"], rt16)
    return dict(E=E, T=T, rt16=rt16, norm=norm, scaled=scaled, rew=rew, v=v, nv=nv, fresh=fresh, fresh_next=fresh_next,
                te=te, tr=tr, st=st, adv0=adv0, ret0=ret0)


def _ref(d, **over):
    a = dict(d, **over)
    return rf.refresh(a["rew"], a["fresh"], a["fresh_next"], a["v"], a["te"], a["tr"], a["st"], a["ret0"], a["adv0"],
                      rt16=a["rt16"], adv_norm=a["norm"])


@pytest.mark.parametrize("name", list(rf.ROWS))
def test_rows_have_what_the_checks_need(name):
    d = _inputs(name)
    T = d["T"]
    assert d["te"].sum() >= 1 and d["tr"].sum() >= 1 and (d["te"][:, T - 1].any() or d["tr"][:, T - 1].any())
    assert d["st"][:, 0].all() and d["st"][:, T - 1].any()
    assert np.abs(rf.stored(d["fresh"], d["rt16"]) - d["v"]).max() > 1e-3
    assert (np.abs(d["rew"]) > 1).any() == d["scaled"]


@pytest.mark.parametrize("rt16", [False, True])
@pytest.mark.parametrize("name", ["fp32", "bf16", "fp16_planes"])
def test_identity_reproduces_the_finish_planes(name, rt16):
    """fresh values equal to the collected ones: the oracle's finish planes bit for bit, in both plane types"""
    d = _inputs(name)
    v, nv = rf.stored(d["v"], rt16), rf.stored(d["nv"], rt16)
    o = orc.buffer_get(d["rew"], v, nv, d["te"], d["tr"], d["st"])
    got = rf.refresh(d["rew"], v, nv, v, d["te"], d["tr"], d["st"], o["returns"], o["advantages"], rt16=rt16)
    np.testing.assert_array_equal(got["advantages"], rf.stored(o["advantages"], rt16))
    np.testing.assert_array_equal(got["returns"], rf.stored(o["returns"], rt16))
    np.testing.assert_array_equal(got["masks"], o["masks"])
    np.testing.assert_array_equal(o["rewards"], d["rew"])  # (already clamped: the finish's clamp is the identity)
    s = got["stats"]
    assert s["value_change_mean"] == s["value_change_std"] == s["value_change_maxabs"] == 0.0


def _differs(a, b):
    return a.tobytes() != b.tobytes()


PLANTED = ("collected_bootstrap", "clamped_again", "scaled_again", "env_major_plane", "start_ignored",
           "return_from_collected", "not_rounded_to_half", "sign_of_change")


@pytest.mark.parametrize("error", PLANTED)
def test_planted_errors_fail_their_check(error):
    """each wrong implementation, stated on the reference's inputs, changes the plane or statistic its GPU check compares"""
    if error == "collected_bootstrap":  # bootstrap taken from the collected next_values
        for name in ("fp32", "bf16", "fp16_planes"):
            d = _inputs(name)
            good, bad = _ref(d), _ref(d, fresh_next=d["nv"])
            env = int(np.argmax(d["tr"][:, d["T"] - 1]))  # truncated at T - 1: the bootstrap enters its last advantage
            assert good["advantages"][env, -1] != bad["advantages"][env, -1], name
            assert _differs(good["returns"], bad["returns"])
    elif error in ("clamped_again", "scaled_again"):  # (the rewards beyond 1 of the reward-scale row)
        d = _inputs("reward_scale")
        rew = np.clip(d["rew"], -1, 1) if error == "clamped_again" else (d["rew"] * SCALE).astype(np.float32)
        good, bad = _ref(d), _ref(d, rew=rew)
        assert _differs(good["advantages"], bad["advantages"]) and _differs(good["returns"], bad["returns"])
    elif error == "env_major_plane":  # fresh plane written env-major where the scan reads time-major (E != T)
        for name in ("fp32", "bf16", "fp16_planes"):
            d = _inputs(name)
            E, T = d["E"], d["T"]
            assert E != T
            wrong = d["fresh"].ravel().reshape(T, E).T.copy()  # what a [T][E] reader sees of an [E][T] write
            good, bad = _ref(d), _ref(d, fresh=wrong)
            assert _differs(good["values"], bad["values"]) and _differs(good["advantages"], bad["advantages"]), name
    elif error == "start_ignored":
        for name in ("fp32", "bf16", "fp16_planes"):
            d = _inputs(name)
            st = d["st"].copy()
            st[1, d["T"] - 1] = 0  # (environment 1 starts an episode in the last slot)
            good, bad = _ref(d), _ref(d, st=st)
            assert _differs(good["advantages"], bad["advantages"]) and _differs(good["masks"], bad["masks"]), name
    elif error == "return_from_collected":  # ret = a + v_collected
        for name in ("fp32", "bf16", "fp16_planes"):
            d = _inputs(name)
            good = _ref(d)
            raw = orc.gae(d["rew"], good["values"], good["next_values"], d["te"], d["tr"], d["st"])
            assert _differs(good["returns"], rf.stored(raw + d["v"], d["rt16"])), name
            np.testing.assert_array_equal(good["returns"], rf.stored(raw + good["values"], d["rt16"]))
    elif error == "not_rounded_to_half":  # values not rounded to half on an fp16 plane
        d = _inputs("fp16_planes")
        assert _differs(d["fresh"], rf.half(d["fresh"]))
        good, bad = _ref(d), _ref(d, rt16=False)
        assert _differs(good["values"], bad["values"])
        assert _differs(good["returns"], rf.half(bad["returns"])) or _differs(good["advantages"], rf.half(bad["advantages"]))
    else:  # d' with the wrong sign
        for name in rf.ROWS:
            d = _inputs(name)
            good = _ref(d)
            s, b = good["stats"], good["bounds"]
            assert b["value_change_mean"] <= rf.MAX_BOUND
            assert 2 * abs(s["value_change_mean"]) > 1e-5 > b["value_change_mean"], name  # -mean is outside the bound
            wrong, _ = rf.stats(d["v"], good["values"], d["ret0"], d["adv0"], good["masks"])
            assert wrong["value_change_mean"] == -s["value_change_mean"]


@pytest.mark.parametrize("name", list(rf.ROWS))
def test_device_order_statistics_stay_inside_the_bounds(name):
    d = _inputs(name)
    good = _ref(d)
    got = rf.one_pass_in_device_order(good["values"], d["v"], d["ret0"], d["adv0"], good["masks"])
    rf.assert_stats(got, good["stats"], good["bounds"], name)
    assert good["stats"]["count"] == good["masks"].sum() < d["E"] * d["T"]
    assert good["stats"]["value_change_maxabs"] > 1e-3


def test_statistics_at_a_size_with_several_chunks():
    """(the rows fit one chunk of 4096: the chunk loop and the index-order sum of the partials at 3 chunks, the last ragged)"""
    N = 2 * rf.CHUNK + 77
    v = hf.hf_range(9300, (N,), -1, 2)
    f = (v + hf.hf_range(9301, (N,), -0.1, 0.2)).astype(np.float32)
    r, a = hf.hf_range(9302, (N,), -2, 3), hf.hf_range(9303, (N,), -1, 1)
    m = (hf.hf_unit(9304, N) >= np.float32(0.1)).astype(np.uint8)
    want, bounds = rf.stats(f, v, r, a, m)
    rf.assert_stats(rf.one_pass_in_device_order(f, v, r, a, m), want, bounds, "3 chunks")


def test_header_constants_and_python_mirror():
    pkg = load_package()
    raw = open(os.path.join(ROOT, "include", "aleppo.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)

    def const(name):
        m = re.search(rf"\b{name}\s*=?\s*(\d+)", hdr)
        assert m, name
        return int(m.group(1))

    assert const("ALEPPO_REFRESH_STATS_COUNT") == pkg.REFRESH_STATS_COUNT == len(rf.NAMES) == len(pkg.REFRESH_STATS) == 13
    for i, name in enumerate(rf.NAMES):
        assert pkg.REFRESH_STATS[name] == i
    for name in rf.EXTRA:
        assert const("ALEPPO_REFRESH_" + name.upper()) == pkg.REFRESH_STATS[name]
    # (no profiling class of its own: the value and statistics launches are bracketed as ALEPPO_K_ACT_STATS)
    assert const("ALEPPO_K_ACT_STATS") == pkg.KERNEL_CLASSES["act_stats"] and const("ALEPPO_K_COUNT") == len(pkg.KERNEL_CLASSES)
    flat = re.sub(r"\s+", " ", hdr)
    for proto in ("int aleppo_refresh_advantages(aleppo_ctx *ctx, int set, double *stats, size_t stat_count);",
                  "int aleppo_refresh_read(aleppo_ctx *ctx, float *values, size_t value_count, float *next_values, "
                  "size_t next_count);"):
        assert proto in flat, proto
    for name in ("aleppo_refresh_advantages", "aleppo_refresh_read"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
    for name in ("refresh_advantages", "refresh_values"):
        assert hasattr(pkg.Engine, name)
