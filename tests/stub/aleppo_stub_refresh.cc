// TEST INFRASTRUCTURE - aleppo_stub.cc plus a host-only aleppo_refresh_advantages, so that the trainer's
// recompute_advantages key - where the call goes in the epoch loop, how often, and how it composes with target_kl - runs
// without a GPU.  The stand-in's aleppo_finish_rollout, aleppo_train and aleppo_read_train_metric are renamed while it is
// included and defined again here: every one of the three calls and every refresh is RECORDED, one line on stderr ("stub:
// aleppo_finish_rollout", "stub: aleppo_train epochs=<e>", "stub: aleppo_refresh_advantages set=<s> stats=<n>"), the
// refreshes are COUNTED and the count is printed when the process ends ("stub: aleppo_refresh_advantages calls: N"), so that
// a run with the key off shows that it never called it.  ALEPPO_M_MEAN_APPROX_KL reads 0.01 times the number of
// aleppo_train calls since the last aleppo_finish_rollout in every slot (every other metric stays the stand-in's zero):
// target_kl: 0.015 stops an update after its second epoch.  The statistics are fixed figures of few bits (explained
// variance 0.5, value change std 0.25, max-abs 0.75).  Validation follows the header: a batch from a finished rollout, the
// set, the count, an armed step.  One context per process (the trainer's).  Never linked into anything but
// trainer/train_refresh_stub.
#define aleppo_finish_rollout stub_plain_finish_rollout
#define aleppo_train stub_plain_train
#define aleppo_read_train_metric stub_plain_read_train_metric
#include "aleppo_stub.cc"
#undef aleppo_finish_rollout
#undef aleppo_train
#undef aleppo_read_train_metric

namespace {
struct StubRefresh {
  bool batch = false;   // a rollout has been finished and the next one has not begun
  long trains = 0;      // aleppo_train calls since the last aleppo_finish_rollout
  long calls = 0;
  ~StubRefresh() { std::fprintf(stderr, "stub: aleppo_refresh_advantages calls: %ld\n", calls); }
} g_refresh;
} // namespace

extern "C" {
int aleppo_finish_rollout(aleppo_ctx *c, const float *noise) {
  const int rc = stub_plain_finish_rollout(c, noise);
  if (rc == ALEPPO_OK) {
    g_refresh.batch = true;
    g_refresh.trains = 0;
    std::fprintf(stderr, "stub: aleppo_finish_rollout\n");
  }
  return rc;
}
int aleppo_train(aleppo_ctx *c, double lr, int epochs, int M, aleppo_minibatch_metrics *out) {
  g_refresh.trains++;
  std::fprintf(stderr, "stub: aleppo_train epochs=%d\n", epochs);
  return stub_plain_train(c, lr, epochs, M, out);
}
int aleppo_read_train_metric(aleppo_ctx *c, int field, float *dst, size_t n) {
  const int rc = stub_plain_read_train_metric(c, field, dst, n);
  if (rc == ALEPPO_OK && field == ALEPPO_M_MEAN_APPROX_KL)
    for (size_t i = 0; i < n; ++i)
      dst[i] = 0.01f * (float)g_refresh.trains;
  return rc;
}
int aleppo_refresh_advantages(aleppo_ctx *c, int set, double *stats, size_t stat_count) {
  g_refresh.calls++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (stats ? stat_count != ALEPPO_REFRESH_STATS_COUNT : stat_count != 0)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: refresh_advantages: bad stat_count");
  if (set != ALEPPO_SET_LIVE)
    return fail(c, set == ALEPPO_SET_AVERAGED || set == ALEPPO_SET_SNAPSHOT ? ALEPPO_ERR_RUNTIME : ALEPPO_ERR_INVALID_ARGUMENT,
                "stub: refresh_advantages: the stand-in has the live parameters only");
  if (!g_refresh.batch || c->t != 0)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: refresh_advantages: no rollout batch");
  if (stats) {
    for (size_t i = 0; i < stat_count; ++i)
      stats[i] = 0.0;
    stats[ALEPPO_BS_COUNT] = (double)c->cfg.num_envs * c->cfg.horizon;
    stats[ALEPPO_BS_EXPLAINED_VARIANCE] = 0.5;
    stats[ALEPPO_REFRESH_VALUE_CHANGE_STD] = 0.25;
    stats[ALEPPO_REFRESH_VALUE_CHANGE_MAXABS] = 0.75;
  }
  std::fprintf(stderr, "stub: aleppo_refresh_advantages set=%d stats=%zu\n", set, stat_count);
  return ALEPPO_OK;
}
}
