"""The bf16 update on every route against the bf16-emulating oracle (pytest -m gpu, on the MI355X).

oracle.h's ORACLE_BF16 rounds where the device stores bf16 and sums in double everywhere else, so a correct kernel
differs from it only by its fp32 summation order: bf16_check.py's bounds (2e-3 relative L2 per gradient tensor, 1e-2 per
output channel, ..., or four times the summation-order floor of the same batch where that is larger) are tight enough
to see one wrong channel, tap or gate.  The route switches are swept pairwise (an L8 orthogonal array over the five
binary options, OPT_FUSED_BWD in {0, 2}: every pair of settings of every two options occurs), the minibatch sizes
straddle the kernels' thresholds and tails:
  8, 24        fewer samples than workgroups
  100          the acting-size kernel variants
  264          just past the pipelined-fc threshold (256)
  520, 1032,   ragged training sizes
  1400
  2048, 2056   the fused backward tail forced on (OPT_FUSED_BWD = 2) / off (0)
  4104         the benched size with a ragged last round
  2040, 2048   OPT_FUSED_BWD = 1 (the default): just below and at the 2048-sample threshold where it fuses
and the head over H in {256, 320, 512}, A in {1, 4, 18}.  Under OPT_MINIBATCH_SHUFFLE the oracle runs on the
host-permuted batch (Engine.sample_order)."""
import numpy as np
import pytest

import bf16_check as bc
import hashfill as hf
import oracle_lib as orc
from shared_fixtures import pkg  # noqa: F401

pytestmark = pytest.mark.gpu


# (OPT_FUSED_FWD, OPT_FUSED_BWD / 2, OPT_FC_PIPE, OPT_GENERIC_CONV, OPT_MINIBATCH_SHUFFLE): an L8 array - columns A, B,
# A^B, D, A^D - covers every pair of settings of every two options; rows 9-10 repeat rows 1 and 4; then two rows at
# the default OPT_FUSED_BWD = 1 on either side of its threshold
L8 = [(0, 0, 0, 0, 0), (0, 0, 0, 1, 1), (0, 1, 1, 0, 0), (0, 1, 1, 1, 1), (1, 0, 1, 0, 1), (1, 0, 1, 1, 0),
      (1, 1, 0, 0, 1), (1, 1, 0, 1, 0), (0, 0, 0, 0, 0), (0, 1, 1, 1, 1)]
SIZES = [8, 24, 100, 264, 520, 1032, 1400, 2048, 2056, 4104]
HEADS = [(256, 1), (320, 4), (512, 18), (512, 4), (256, 18), (320, 1), (512, 1), (256, 4), (320, 18), (512, 4)]
ROWS = [(N, H, A, fwd, 2 * bwd, pipe, gen, shuf) for N, (H, A), (fwd, bwd, pipe, gen, shuf) in zip(SIZES, HEADS, L8)]
ROWS += [(2040, 512, 6, 1, 1, 1, 0, 0), (2048, 512, 6, 1, 1, 1, 0, 1)]


def _id(r):
    N, H, A, fwd, bwd, pipe, gen, shuf = r
    return "N%d-H%d-A%d-fwd%d-bwd%d-pipe%d-gen%d-shuf%d" % (N, H, A, fwd, bwd, pipe, gen, shuf)


def sweep_batch(N, H, A):
    """(params, obs, actions, old_lp, adv, ret, masks) of the sweep row of size N (also used by test_oracle_bf16.py)"""
    seed = 2600 + N + (7 if N == 2048 and A == 6 else 0)
    params = hf.fill_params(seed, H, A)
    obs = hf.hf_bytes(seed + 1, (N, 4, 84, 84))
    actions = (hf.hf_u32(seed + 2, N) % np.uint32(A)).astype(np.int64)
    old_lp = orc.log_softmax(hf.hf_range(seed + 3, (N, A), -1, 1))
    adv, ret = hf.hf_range(seed + 4, (N,), -1, 1), hf.hf_range(seed + 5, (N,), -1, 1)
    masks = (hf.hf_unit(seed + 6, N) >= np.float32(0.1)).astype(np.uint8)
    masks[0] = 1
    return params, obs, actions, old_lp, adv, ret, masks


@pytest.mark.parametrize("row", ROWS, ids=[_id(r) for r in ROWS])
def test_bf16_update_on_every_route_vs_emulated_oracle(pkg, row):
    N, H, A, fwd, bwd, pipe, generic, shuffle = row
    params, obs, actions, old_lp, adv, ret, masks = sweep_batch(N, H, A)
    T = 8 if N % 8 == 0 else 4
    eng = pkg.Engine(N // T, T, A, H, precision=pkg.BF16)
    for opt, val in ((pkg.OPT_FUSED_FWD, fwd), (pkg.OPT_FUSED_BWD, bwd), (pkg.OPT_FC_PIPE, pipe),
                     (pkg.OPT_GENERIC_CONV, generic), (pkg.OPT_MINIBATCH_SHUFFLE, shuffle)):
        eng.set_option(opt, val)
        assert eng.get_option(opt) == val
    eng.load_params(params)
    c = bc.Checker()
    nf = min(N, 333)
    logits, values = eng.forward(obs[:nf])
    c.forward(logits, values, bc.emulated_forward(params, H, A, obs[:nf]), "fwd_")
    eng.set_batch(obs, actions, old_lp, adv, ret, masks)
    m = eng.train(2.5e-4, 1, 1)
    order = eng.sample_order(1)[0]
    if not shuffle:
        np.testing.assert_array_equal(order, np.arange(N))
    assert np.array_equal(np.sort(order), np.arange(N))
    w = bc.emulated_train(params, H, A, obs[order], actions[order], old_lp[order], adv[order], ret[order],
                          masks[order], 1, 1)
    planes = {ours: eng.read_train_metric(ours, 1, 1, N) for ours, _ in bc.PLANES}
    c.train(H, A, m, planes, eng.export_grads(), w, params0=params, params=eng.export_params())
    np.testing.assert_array_equal(m["mask_count"], np.full_like(m["mask_count"], masks.sum()))
    eng.close()
    # (report only) samples whose PPO clip state differs between the engine's ratio plane and the emulation's
    def active(rho):
        return np.where(adv[order] >= 0, rho <= 1.1, rho >= 0.9)
    flips = int(((active(planes["ratio"].ravel()) != active(w["ratio"].ravel())) & (masks[order] == 1)).sum())
    print(c.summary("bf16 vs emulated oracle " + _id(row)), "clip-state flips:", flips)
    assert not c.failures, c.failures
