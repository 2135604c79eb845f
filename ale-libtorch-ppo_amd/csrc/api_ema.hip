// api_ema.hip - C ABI (include/aleppo.h), the exponentially averaged parameters: aleppo_ema_open, aleppo_ema_update,
// aleppo_ema_read, aleppo_ema_export, aleppo_ema_import.  The averaged set (c->averaged, a ParamSet with a compute copy)
// lives next to the live parameters in the same layout; the pass is ema.hip.  Nothing here touches P, the moments, the
// gradient or anything aleppo_train reads, and everything goes onto the context's main stream only.
#include "api_internal.hpp"

using namespace aleppo;

#define CHECK_EMA(c)                                                                                                   \
  do {                                                                                                                 \
    CHECK_CTX(c);                                                                                                      \
    if (!(c)->averaged.on)                                                                                             \
      return set_err((c), ALEPPO_ERR_RUNTIME, NO_AVERAGED);                                                            \
  } while (0)

// the sums of the two sets as they stand and the six doubles; d: what ALEPPO_EMA_DECAY reports
static void ema_stats_enqueue(aleppo_ctx *c, float d) {
  const int nblk =
      launch_ema(c->stream, false, c->P, c->averaged.P, c->averaged.Pc, (long)c->L.total(), 0.f, 0.f, c->ema_blk);
  launch_ema_final(c->stream, nblk, (long long)c->ema_updates, d, c->ema_blk);
}

int aleppo::ema_restart(aleppo_ctx *c) {
  if (int rc = param_set_copy(c, &c->averaged, live_view(c)))
    return rc;
  c->ema_updates = 0;
  ema_stats_enqueue(c, 0.f);
  HIPCHK(c, hipGetLastError());
  return ALEPPO_OK;
}

extern "C" int aleppo_ema_open(aleppo_ctx *c) {
  CHECK_CTX(c);
  void *blk = nullptr; // first use: the set and its block in one step; a later call re-initialises the same storage
  if (int rc = param_set_storage(c, &c->averaged, true, "ema_open", &blk, EMA_BLK_BYTES))
    return rc; // (stays closed)
  if (blk)
    c->ema_blk = static_cast<double *>(blk);
  if (int rc = ema_restart(c))
    return rc;
  c->averaged.on = true;
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_ema_update(aleppo_ctx *c, double decay) {
  CHECK_EMA(c);
  if (!std::isfinite(decay) || !(decay >= 0.0 && decay < 1.0))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "ema_update: decay must be finite and in [0, 1)");
  const float d = (float)decay, w = (float)(1.0 - decay);
  prof_begin(c, ALEPPO_K_EMA);
  const int nblk =
      launch_ema(c->stream, true, c->P, c->averaged.P, c->averaged.Pc, (long)c->L.total(), d, w, c->ema_blk);
  prof_end(c, ALEPPO_K_EMA);
  c->ema_updates++;
  launch_ema_final(c->stream, nblk, (long long)c->ema_updates, d, c->ema_blk);
  HIPCHK(c, hipGetLastError());
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_ema_read(aleppo_ctx *c, double out[ALEPPO_EMA_STATS_COUNT]) {
  CHECK_EMA(c);
  if (!out)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "ema_read: null out");
  double h[ALEPPO_EMA_STATS_COUNT]; // (the caller's memory is never the target of an asynchronous copy)
  HIPCHK(c, copy_sync(c, h, ema_stats(c->ema_blk), sizeof(h), hipMemcpyDeviceToHost));
  std::memcpy(out, h, sizeof(h));
  return ALEPPO_OK;
}

extern "C" int aleppo_ema_export(aleppo_ctx *c, float *flat, size_t count, int64_t *updates) {
  CHECK_EMA(c);
  if (!updates)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "ema_export: null updates");
  if (int rc = param_set_export(c, c->averaged, NO_AVERAGED, flat, count))
    return rc;
  *updates = c->ema_updates;
  return ALEPPO_OK;
}

extern "C" int aleppo_ema_import(aleppo_ctx *c, const float *flat, size_t count, int64_t updates) {
  CHECK_EMA(c);
  static const char *const refusal = "ema_import: wrong element count";
  if (!flat || count != c->L.reference_count()) // (here too: it comes before the refusal of updates)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, refusal);
  if (updates < 0)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "ema_import: updates must not be negative");
  if (int rc = param_set_upload(c, &c->averaged, flat, count, refusal))
    return rc;
  c->ema_updates = updates;
  ema_stats_enqueue(c, 0.f);
  HIPCHK(c, hipGetLastError());
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}
