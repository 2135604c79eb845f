// TEST INFRASTRUCTURE - aleppo_stub_eval_env.cc plus host-only averaged parameters (aleppo_ema_open / _update / _read /
// _export / _import), so that the trainer's ema_decay / ema_warmup / eval_averaged keys - the decay of every update, the
// checkpoint section, the resume - run without a GPU.  The average is kept over the stand-in's own parameter array by the
// header's rule itself: d = (float)decay, w = (float)(1.0 - decay), a = d * e, b = w * p, e' = a + b, three fp32 operations
// (volatile intermediates: the host compiler must not contract them either), and the six statistics in double.  Every
// aleppo_ema_update is RECORDED, one line on stderr ("stub: aleppo_ema_update decay=<%.17g> updates=<n>", n the count after
// the call), the calls are COUNTED and the count is printed when the process ends ("stub: aleppo_ema_update calls: N"), so
// that a run with the key off shows that it never called it.  The stand-in's aleppo_set_option is renamed while it is
// included and defined again here: ALEPPO_OPT_EVAL_PARAMS is validated as the header says and printed ("stub:
// aleppo_set_option ALEPPO_OPT_EVAL_PARAMS value=<v>"), everything else is passed on.  The stand-in's lanes have no
// network, so the option changes nothing they do.  Validation follows the header: before the open, decay, counts, NULL
// pointers, negative updates, an armed step.  One context per process (the trainer's).  Never linked into anything but
// trainer/train_ema_stub.
#define aleppo_set_option stub_plain_set_option
#include "aleppo_stub_eval_env.cc"
#undef aleppo_set_option
#include <cmath>

namespace {
struct StubEma {
  bool open = false;
  std::vector<float> e;
  int64_t updates = 0;
  double stats[ALEPPO_EMA_STATS_COUNT] = {};
  long update_calls = 0;
  ~StubEma() { std::fprintf(stderr, "stub: aleppo_ema_update calls: %ld\n", update_calls); }
} g_ema;

void stub_ema_stats(const aleppo_ctx *c, float d) {
  double se = 0, sp = 0, sd = 0;
  for (size_t i = 0; i < g_ema.e.size(); ++i) {
    const double e = g_ema.e[i], p = c->params[i];
    se += e * e, sp += p * p, sd += (p - e) * (p - e);
  }
  const double s[ALEPPO_EMA_STATS_COUNT] = {(double)g_ema.updates,  (double)d, std::sqrt(se), std::sqrt(sp), std::sqrt(sd),
                                            sp > 0 ? std::sqrt(sd / sp) : 0.0};
  std::memcpy(g_ema.stats, s, sizeof s);
}
int stub_ema_closed(aleppo_ctx *c) {
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (!g_ema.open)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: no averaged parameters: call aleppo_ema_open first");
  return ALEPPO_OK;
}
} // namespace

extern "C" {
int aleppo_set_option(aleppo_ctx *c, int option, int value) {
  if (option != ALEPPO_OPT_EVAL_PARAMS)
    return stub_plain_set_option(c, option, value);
  if (value != 0 && value != 1)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: ALEPPO_OPT_EVAL_PARAMS: 0 or 1");
  if (value == 1 && !g_ema.open)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: ALEPPO_OPT_EVAL_PARAMS: call aleppo_ema_open first");
  std::fprintf(stderr, "stub: aleppo_set_option ALEPPO_OPT_EVAL_PARAMS value=%d\n", value);
  return ALEPPO_OK;
}
int aleppo_ema_open(aleppo_ctx *c) {
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  g_ema.e = c->params;
  g_ema.updates = 0;
  g_ema.open = true;
  stub_ema_stats(c, 0.f);
  std::fprintf(stderr, "stub: aleppo_ema_open\n");
  return ALEPPO_OK;
}
int aleppo_ema_update(aleppo_ctx *c, double decay) {
  g_ema.update_calls++;
  if (int rc = stub_ema_closed(c))
    return rc;
  if (!std::isfinite(decay) || !(decay >= 0.0 && decay < 1.0))
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: ema_update: decay must be finite and in [0, 1)");
  const float d = (float)decay, w = (float)(1.0 - decay);
  for (size_t i = 0; i < g_ema.e.size(); ++i) {
    volatile float a = d * g_ema.e[i];
    volatile float b = w * c->params[i];
    g_ema.e[i] = a + b;
  }
  g_ema.updates++;
  stub_ema_stats(c, d);
  std::fprintf(stderr, "stub: aleppo_ema_update decay=%.17g updates=%lld\n", decay, (long long)g_ema.updates);
  return ALEPPO_OK;
}
int aleppo_ema_read(aleppo_ctx *c, double out[ALEPPO_EMA_STATS_COUNT]) {
  if (int rc = stub_ema_closed(c))
    return rc;
  if (!out)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: ema_read: null out");
  std::memcpy(out, g_ema.stats, sizeof g_ema.stats);
  return ALEPPO_OK;
}
int aleppo_ema_export(aleppo_ctx *c, float *flat, size_t count, int64_t *updates) {
  if (int rc = stub_ema_closed(c))
    return rc;
  if (!flat || !updates || count != g_ema.e.size())
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: ema_export: bad argument");
  std::memcpy(flat, g_ema.e.data(), count * 4);
  *updates = g_ema.updates;
  return ALEPPO_OK;
}
int aleppo_ema_import(aleppo_ctx *c, const float *flat, size_t count, int64_t updates) {
  if (int rc = stub_ema_closed(c))
    return rc;
  if (!flat || count != g_ema.e.size() || updates < 0)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: ema_import: bad argument");
  std::memcpy(g_ema.e.data(), flat, count * 4);
  g_ema.updates = updates;
  stub_ema_stats(c, 0.f);
  std::fprintf(stderr, "stub: aleppo_ema_import updates=%lld\n", (long long)updates);
  return ALEPPO_OK;
}
}
