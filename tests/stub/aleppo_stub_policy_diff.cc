// TEST INFRASTRUCTURE - aleppo_stub_ema.cc plus host-only aleppo_snapshot_take / aleppo_policy_diff, so that the trainer's
// log_policy_churn keys run without a GPU.  The stand-in has no network, so the answer is a closed form that names the two
// sets and the stat: ROWS = num_envs * horizon, NONFINITE_ROWS = 0 and, for k >= 2,
//   stats[k] = (4 * set_a + set_b + k) / 64
// so that a test can tell which sets the trainer compared and that it logs the stat it names.  The batch source only (the
// trainer never uses the other).  Validation follows the header: an armed step, unknown sets, the snapshot as a take's
// source, a set that does not exist yet, stats and the counts.  Every call is RECORDED, one line on stderr
// ("stub: aleppo_snapshot_take source=<s>", "stub: aleppo_policy_diff a=<a> b=<b> fresh=<f>", f = 1 when a take came since the
// last comparison that read the snapshot), the calls are COUNTED and the counts printed when the process ends
// ("stub: aleppo_snapshot_take calls: N", "stub: aleppo_policy_diff calls: N"), so that a run with the key off shows that it
// never called either.  Never linked into anything but trainer/train_pdiff_stub.
#include "aleppo_stub_ema.cc"

namespace {
struct StubPolicyDiff {
  long takes = 0, diffs = 0;
  bool have = false, fresh = false;
  std::vector<float> snapshot;
  ~StubPolicyDiff() {
    std::fprintf(stderr, "stub: aleppo_snapshot_take calls: %ld\nstub: aleppo_policy_diff calls: %ld\n", takes, diffs);
  }
} g_pd;

// ALEPPO_OK, or what the header says about a set that is unknown or does not exist yet
int stub_pd_set(aleppo_ctx *c, int set) {
  if (set == ALEPPO_SET_LIVE)
    return ALEPPO_OK;
  if (set == ALEPPO_SET_AVERAGED)
    return g_ema.open ? ALEPPO_OK : fail(c, ALEPPO_ERR_RUNTIME, "stub: no averaged parameters: call aleppo_ema_open first");
  if (set == ALEPPO_SET_SNAPSHOT)
    return g_pd.have ? ALEPPO_OK : fail(c, ALEPPO_ERR_RUNTIME, "stub: no snapshot: call aleppo_snapshot_take first");
  return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: unknown parameter set");
}
} // namespace

extern "C" {
int aleppo_snapshot_take(aleppo_ctx *c, int source_set) {
  g_pd.takes++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (source_set == ALEPPO_SET_SNAPSHOT)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: snapshot_take: the source must be the live or the averaged set");
  if (int rc = stub_pd_set(c, source_set))
    return rc;
  g_pd.snapshot = source_set == ALEPPO_SET_LIVE ? c->params : g_ema.e;
  g_pd.have = g_pd.fresh = true;
  std::fprintf(stderr, "stub: aleppo_snapshot_take source=%d\n", source_set);
  return ALEPPO_OK;
}
int aleppo_policy_diff(aleppo_ctx *c, const uint8_t *observations, int64_t n, int set_a, int set_b, double *stats,
                       size_t stat_count, double *per_sample, size_t, int64_t *transitions, size_t, float *outputs, size_t) {
  g_pd.diffs++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (!stats || stat_count != ALEPPO_PD_COUNT || observations || n != 0 || per_sample || transitions || outputs)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: policy_diff: bad argument (the stand-in has the batch source and the stats only)");
  if (int rc = stub_pd_set(c, set_a))
    return rc;
  if (int rc = stub_pd_set(c, set_b))
    return rc;
  const bool reads_snapshot = set_a == ALEPPO_SET_SNAPSHOT || set_b == ALEPPO_SET_SNAPSHOT;
  std::fprintf(stderr, "stub: aleppo_policy_diff a=%d b=%d fresh=%d\n", set_a, set_b, g_pd.fresh ? 1 : 0);
  if (reads_snapshot)
    g_pd.fresh = false;
  stats[ALEPPO_PD_ROWS] = (double)c->cfg.num_envs * c->cfg.horizon;
  stats[ALEPPO_PD_NONFINITE_ROWS] = 0.0;
  for (int k = 2; k < ALEPPO_PD_COUNT; ++k)
    stats[k] = (4 * set_a + set_b + k) / 64.0;
  return ALEPPO_OK;
}
}
