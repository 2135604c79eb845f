"""aleppo_refresh_advantages / aleppo_refresh_read on the device (include/aleppo.h) against tests/refresh_ref.py: per row of
refresh_ref.ROWS finish, train, refresh, check, train, refresh, check - the fresh values bit for bit against aleppo_forward in
the same chunks, advantages and returns bit for bit against the reference, everything else untouched, the statistics inside
their derived bounds, and the update that follows held to the composed reference.  Then the captured update, the parameter
sets, the one-rank communicator path, every refusal, the next rollout of a context that refreshed, and the trainer's
recompute_advantages key on the device."""
import ctypes
import struct

import numpy as np
import pytest

import bf16_check as bc
import hashfill as hf
import refresh_ref as rf
import update_harness as uh
import update_ref as ur
from shared_fixtures import pkg, trainer  # noqa: F401
from test_gpu_at_size import DeviceBytes

LR = 1e-3  # (large enough that one epoch moves the values by more than 1e-3: asserted per row)
KEEP = ("masks", "values", "next_values", "log_probs", "actions", "logits", "rewards", "observations", "terminals",
        "truncations", "current_obs")
M_OF = dict(fp32=5, bf16=3, fp16_planes=2, reward_scale=5, adv_norm=5)  # minibatches of 7 / 33 / 130 samples


def _engine(pkg, name, seed, finish=True, **kw):
    """the row's context holding a finished rollout of hashed frames, rewards in [-2, 2] and the row's flags"""
    E, T, A, H, prec, rt16, mb, scaled, norm = rf.ROWS[name]
    eng = pkg.Engine(E, T, A, H, precision=pkg.BF16 if prec == "bf16" else pkg.FP32, seed=3, max_minibatch=mb,
                     advantage_norm=norm, rollout_precision=pkg.ROLLOUT_FP16 if rt16 else pkg.ROLLOUT_FP32, **kw)
    eng.load_params(hf.fill_params(seed, H, A))
    if scaled:
        eng.set_reward_scaling(True)
    if finish:
        _collect(pkg, eng, seed)
    return eng


def _collect(pkg, eng, seed):
    E, T = eng.E, eng.T
    dev = DeviceBytes(hf.hf_bytes(seed + 1, (T, E, 84, 84)))
    te, tr, st = rf.row_flags(seed + 2, E, T)
    eng.replay_rollout(dev.addr, pkg.FRAMES_84, E * 7056, rf.row_rewards(seed + 3, E, T), te, tr, st)
    eng.finish_rollout()
    dev.free()


def _forward_in_chunks(eng, obs, chunk):
    return np.concatenate([eng.forward(obs[i:i + chunk])[1] for i in range(0, len(obs), chunk)])


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), f"{what}: {k} differs"


def _planes(eng, names=("advantages", "returns", "masks")):
    return {k: eng.read_batch(k) for k in names}


def _bits(stats):
    return struct.pack("<13d", *[stats[k] for k in rf.NAMES])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rf.ROWS))
def test_row(pkg, name):
    E, T, A, H, prec, rt16, mb, scaled, norm = rf.ROWS[name]
    N, M, maxB = E * T, M_OF[name], max(E, mb)
    bf16 = prec == "bf16"
    eng = _engine(pkg, name, 9500 + 10 * list(rf.ROWS).index(name))
    te, tr = eng.read_batch("terminals"), eng.read_batch("truncations")
    assert te.sum() >= 1 and tr[:, T - 1].any() and not eng.read_batch("masks")[:, T - 1].all()
    update = None  # the state the next aleppo_train starts from, and the planes it trains on
    for rnd in (1, 2):
        m = eng.train(LR, 1, M)
        if update:  # aleppo_train after a refresh vs the composed reference on the read-back planes
            out = uh.read_update(eng, m, 1, M, diag=False)
            ref = ur.composed_train(update["params"], H, A, update["obs"], update["actions"], update["log_probs"],
                                    update["advantages"], update["returns"], update["masks"], 1, M, lr=LR,
                                    adam=update["adam"], emulate_bf16=bf16, floor=bf16)
            if bf16:
                c = bc.Checker()
                c.train(H, A, m, {ours: out[ours] for ours, _ in bc.PLANES}, None, ref, params0=update["params"],
                        params=out["params"])
                print(c.summary(f"{name}: update after a refresh vs emulated composed reference"))
                assert not c.failures, c.failures
            else:
                uh.check_against(out, ref, 1e-4, [k for k in uh.PER_SAMPLE if k not in uh.DIAG_PLANES])
        before = _planes(eng, KEEP + ("advantages", "returns"))
        digest = eng.state_digest()
        rs_before = eng.read_batch("reward_scale")
        stats = eng.refresh_advantages()
        after = _planes(eng, KEEP + ("advantages", "returns"))
        # everything but the two planes is what it was
        _same({k: before[k] for k in KEEP}, {k: after[k] for k in KEEP}, f"{name} round {rnd}")
        assert eng.state_digest() == digest and eng.read_batch("reward_scale").tobytes() == rs_before.tobytes()
        # the fresh plane: aleppo_forward on the same observations in the same chunks, rounded to the plane type
        fv, fnv = eng.refresh_values()
        obs = before["observations"].reshape(N, 4, 84, 84)
        wv = _forward_in_chunks(eng, obs, maxB).reshape(E, T)
        wnv = _forward_in_chunks(eng, before["current_obs"], maxB)
        np.testing.assert_array_equal(fv, rf.stored(wv, rt16))
        np.testing.assert_array_equal(fnv, rf.stored(wnv, rt16))
        change = np.abs(fv - before["values"]).max()
        print(f"{name} round {rnd}: max |v_fresh - v| = {change:.4g}")
        assert change > 1e-3  # (the precondition: a refresh that reused the collected values would pass otherwise)
        if scaled:
            assert (np.abs(before["rewards"]) > 1).any()  # (a second clamp would show)
        ref = rf.refresh(before["rewards"], wv, wnv, before["values"], before["terminals"], before["truncations"],
                         1 - before["masks"], before["returns"], before["advantages"], rt16=rt16, adv_norm=norm)
        np.testing.assert_array_equal(after["returns"], ref["returns"])
        if norm:
            np.testing.assert_allclose(after["advantages"], ref["advantages"], rtol=2e-4, atol=2e-5)
        else:
            np.testing.assert_array_equal(after["advantages"], ref["advantages"])
        rf.assert_stats(stats, ref["stats"], ref["bounds"], f"{name} round {rnd}")
        # a second refresh in a row: the same planes (its statistics see the refreshed targets: the value change is the same)
        again = eng.refresh_advantages()
        _same(after, _planes(eng, KEEP + ("advantages", "returns")), f"{name} second refresh")
        np.testing.assert_array_equal(eng.refresh_values()[0], fv)
        assert all(again[k] == stats[k] for k in ("count", "value_mean", "value_std") + rf.EXTRA)
        sd = eng.state_dict()
        update = dict(params=sd["params"], adam=dict(m=sd["exp_avg"], v=sd["exp_avg_sq"], step=int(sd["step"])), obs=obs,
                      actions=after["actions"].ravel(), log_probs=after["log_probs"].reshape(N, A),
                      advantages=after["advantages"].ravel(), returns=after["returns"].ravel(),
                      masks=after["masks"].ravel())
    eng.close()


@pytest.mark.gpu
def test_statistics_and_planes_over_two_chunks(pkg):
    """130 x 33 = 4290 samples: the statistics' second workgroup (partly filled) and the index-order sum of two partials,
    three GAE workgroups, one forward chunk of the whole batch"""
    E, T, A, H = 130, 33, 4, 32
    eng = pkg.Engine(E, T, A, H, precision=pkg.FP32, seed=3)
    eng.load_params(hf.fill_params(9450, H, A))
    _collect(pkg, eng, 9450)
    eng.train(LR, 1, 1)
    before = _planes(eng, ("values", "returns", "advantages", "rewards", "terminals", "truncations", "masks"))
    stats = eng.refresh_advantages()
    fv, fnv = eng.refresh_values()
    assert np.abs(fv - before["values"]).max() > 1e-3
    ref = rf.refresh(before["rewards"], fv, fnv, before["values"], before["terminals"], before["truncations"],
                     1 - before["masks"], before["returns"], before["advantages"])
    np.testing.assert_array_equal(eng.read_batch("advantages"), ref["advantages"])
    np.testing.assert_array_equal(eng.read_batch("returns"), ref["returns"])
    rf.assert_stats(stats, ref["stats"], ref["bounds"], "two chunks")
    assert E * T > rf.CHUNK and 0 < stats["count"] < E * T
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_captured_update_reads_the_refreshed_planes(pkg, name):
    """train / refresh / train / refresh / train with ALEPPO_OPT_UPDATE_GRAPH (the first call of a shape runs eagerly, the
    later ones capture and replay): the eager run's parameters and metrics bit for bit"""
    runs = []
    for graph in (0, 1):
        eng = _engine(pkg, name, 9600)
        eng.set_option(pkg.OPT_UPDATE_GRAPH, graph)
        ms = []
        for k in range(3):
            if k:
                eng.refresh_advantages(stats=False)
            ms.append(eng.train(LR, 1, M_OF[name]))
        runs.append(dict(params=eng.export_params(), **{f"{k}{i}": v for i, m in enumerate(ms) for k, v in m.items()},
                         **_planes(eng)))
        eng.close()
    _same(runs[0], runs[1], "captured vs eager")


@pytest.mark.gpu
def test_parameter_sets(pkg):
    eng = _engine(pkg, "bf16", 9700)
    M = M_OF["bf16"]
    eng.train(LR, 1, M)
    with pytest.raises(pkg.AleppoError, match="aleppo_ema_open"):
        eng.refresh_advantages(source="averaged")
    with pytest.raises(pkg.AleppoError, match="no snapshot"):
        eng.refresh_advantages(source="snapshot")
    with pytest.raises(pkg.AleppoInvalidArgument):
        eng.refresh_advantages(source=7)
    eng.snapshot_take("live")
    assert eng.export_backward(("fc",))[0]["fc"].shape[1] == eng.H  # (the update's last minibatch is there to be read ...)
    eng.refresh_advantages(source="snapshot")
    with pytest.raises(pkg.AleppoError, match="something else has run the network"):  # ... until the refresh forwards
        eng.export_backward(("fc",))
    snap = dict(_planes(eng), values=eng.refresh_values()[0], next_values=eng.refresh_values()[1])
    eng.refresh_advantages(source="live")
    live = dict(_planes(eng), values=eng.refresh_values()[0], next_values=eng.refresh_values()[1])
    _same(snap, live, "snapshot of live vs live")
    eng.train(LR, 1, M)  # the live parameters move on, the snapshot stays
    eng.refresh_advantages(source="snapshot")
    _same(snap, dict(_planes(eng), values=eng.refresh_values()[0], next_values=eng.refresh_values()[1]), "snapshot later")
    eng.refresh_advantages(source="live")
    moved = dict(_planes(eng), values=eng.refresh_values()[0], next_values=eng.refresh_values()[1])
    assert moved["values"].tobytes() != snap["values"].tobytes()
    assert moved["advantages"].tobytes() != snap["advantages"].tobytes()
    eng.ema_open()  # (the averaged set starts at the live parameters)
    eng.refresh_advantages(source="averaged")
    _same(moved, dict(_planes(eng), values=eng.refresh_values()[0], next_values=eng.refresh_values()[1]), "averaged")
    eng.close()


@pytest.mark.gpu
def test_one_rank_communicator_path_is_bit_identical(pkg):
    """advantage_norm's all-reduce on a 1-rank RCCL communicator with ALEPPO_OPT_FORCE_COMM against the plain path"""
    got = []
    for comm in (False, True):
        eng = _engine(pkg, "adv_norm", 9800)
        if comm:
            eng.comm_init(pkg.Engine.comm_unique_id())
            eng.set_option(pkg.OPT_FORCE_COMM, 1)
        eng.train(LR, 1, M_OF["adv_norm"])
        stats = eng.refresh_advantages()
        got.append(dict(_planes(eng), values=eng.refresh_values()[0], stats=np.frombuffer(_bits(stats), np.float64)))
        eng.close()
    _same(got[0], got[1], "forced communicator vs plain")


@pytest.mark.gpu
def test_refusals_change_nothing(pkg):
    name = "fp32"
    E, T, A, H = rf.ROWS[name][:4]
    eng = _engine(pkg, name, 9900, finish=False)
    with pytest.raises(pkg.AleppoError, match="no rollout batch"):  # before any rollout
        eng.refresh_advantages()
    with pytest.raises(pkg.AleppoError, match="not been refreshed"):
        eng.refresh_values()
    _collect(pkg, eng, 9900)
    eng.train(LR, 1, M_OF[name])
    with pytest.raises(pkg.AleppoError, match="not been refreshed"):  # read before the refresh
        eng.refresh_values()
    kept = _planes(eng)
    st = np.zeros(13, np.float64)

    def call(ptr, count):
        return pkg.lib().aleppo_refresh_advantages(eng._ctx, ctypes.c_int(pkg.SET_LIVE), ptr, ctypes.c_size_t(count))

    for ptr, count in ((st.ctypes.data_as(ctypes.c_void_p), 10), (st.ctypes.data_as(ctypes.c_void_p), 0),
                       (st.ctypes.data_as(ctypes.c_void_p), 14), (None, 13)):  # wrong counts
        assert call(ptr, count) == pkg.ERR_INVALID_ARGUMENT
    assert not st.any()
    v, nv = np.zeros((E, T), np.float32), np.zeros(E, np.float32)
    _same(kept, _planes(eng), "after wrong counts")
    assert call(None, 0) == pkg.OK  # (NULL with 0 is the form without statistics)
    fresh = _planes(eng)
    assert fresh["advantages"].tobytes() != kept["advantages"].tobytes()
    read = pkg.lib().aleppo_refresh_read
    vp, nvp = v.ctypes.data_as(ctypes.c_void_p), nv.ctypes.data_as(ctypes.c_void_p)
    for args in ((vp, v.size - 1, nvp, nv.size), (vp, v.size, nvp, nv.size + 1), (None, 0, None, 0), (None, v.size, nvp, E)):
        assert read(eng._ctx, args[0], ctypes.c_size_t(args[1]), args[2], ctypes.c_size_t(args[3])) == \
            pkg.ERR_INVALID_ARGUMENT
    assert read(eng._ctx, None, ctypes.c_size_t(0), nvp, ctypes.c_size_t(E)) == pkg.OK
    assert nv.tobytes() == eng.refresh_values()[1].tobytes()
    # the next rollout has begun: its first act carries the post-rollout observation into slot 0
    eng.act()
    with pytest.raises(pkg.AleppoError, match="next rollout has begun"):
        eng.refresh_advantages()
    _same(fresh, _planes(eng), "after the mid-rollout refusal")
    # while a step is armed
    fbuf, sbuf = eng.host_alloc(E * 7056), eng.host_alloc(E)
    eng.arm_step(fbuf, sbuf)
    with pytest.raises(pkg.AleppoError, match="armed"):
        eng.refresh_advantages()
    with pytest.raises(pkg.AleppoError, match="armed"):
        eng.refresh_values()
    ctypes.memset(fbuf, 0, E * 7056)
    ctypes.memset(sbuf, 0, E)
    zeros = np.zeros(E, np.uint8)
    eng.release_step(np.zeros(E, np.float32), zeros, zeros)
    with pytest.raises(pkg.AleppoError, match="next rollout has begun"):
        eng.refresh_advantages()
    eng.host_free(fbuf)
    eng.host_free(sbuf)
    eng.close()
    # a caller batch has no time axis
    eng = _engine(pkg, name, 9900)
    N = E * T
    obs, actions, old_lp, adv, ret, masks = uh.hashed_batch(9910, N, A, mask_p=0.1)
    eng.set_batch(obs, actions, old_lp, adv, ret, masks, values=ret)
    with pytest.raises(pkg.AleppoError, match="no time axis"):
        eng.refresh_advantages()
    np.testing.assert_array_equal(eng.read_batch("advantages").ravel(), adv)
    eng.close()


@pytest.mark.gpu
def test_the_next_rollout_is_the_same_with_and_without_a_refresh(pkg):
    got = []
    for refresh in (False, True):
        eng = _engine(pkg, "fp16_planes", 9950)
        eng.train(LR, 1, M_OF["fp16_planes"])
        if refresh:
            eng.refresh_advantages()
            eng.refresh_advantages(stats=False)
        _collect(pkg, eng, 9960)
        got.append({k: eng.read_batch(k) for k in pkg.FIELDS if k != "batch_stats"})
        got[-1]["digest"] = np.array(list(eng.state_digest().values()), np.uint64)
        with pytest.raises(pkg.AleppoError, match="not been refreshed"):  # (the plane belonged to the batch before)
            eng.refresh_values()
        eng.close()
    _same(got[0], got[1], "next rollout")


@pytest.mark.gpu
def test_trainer_on_the_device(trainer, tmp_path):
    """recompute_advantages: true through the real library: every update refreshes once (debug.yaml has two epochs) and
    logs rank 0's statistics; the values did move"""
    import os
    import subprocess
    import trainer_helpers
    os.makedirs(tmp_path / "tb")
    cfg = trainer_helpers.debug_cfg(tmp_path, "recompute_advantages: true\n", 3)
    r = subprocess.run([trainer, "breakout.bin", str(tmp_path / "tb" / "run.log"), str(tmp_path), "g", str(cfg)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    blob = trainer_helpers.events(tmp_path / "tb")
    got = {t: trainer_helpers.event_scalars(blob, "refresh/" + t)
           for t in ("explained_variance", "value_change_std", "value_change_maxabs")}
    print(got)
    assert all(len(v) == 3 for v in got.values()) and len(trainer_helpers.event_scalars(blob, "mean_loss")) == 3
    assert all(np.isfinite(x) and x > 0 for x in got["value_change_std"] + got["value_change_maxabs"])
    assert all(a >= s for a, s in zip(got["value_change_maxabs"], got["value_change_std"]))
    assert all(np.isnan(x) or x <= 1.0 for x in got["explained_variance"])
