// TEST INFRASTRUCTURE - aleppo_stub_env.cc plus a host-only aleppo_recycle_dormant, so that the trainer's recycle_dormant
// keys run without a GPU.  The stand-in has no network and recycles nothing: it RECORDS its arguments, one line per call on
// stderr ("stub: aleppo_recycle_dormant tau=<%.17g> layers=<int> key=<hex> flags=<int> batch=<0|1> mask_out=<0|1>"), and
// answers with counts that are a function of them - layer l of the asked-for layers reports l + 1 units, the others 0 - so
// that a test can tell which arguments arrived and that the counts reach the log.  Validation follows the header: counts,
// unit_count, flags, layers, tau, the source (the batch source only: the trainer never uses the other), an armed step.  It
// COUNTS its calls and says so when the process ends ("stub: aleppo_recycle_dormant calls: N"), so that a run with the key
// off shows that it never called it.  Never linked into anything but trainer/train_recycle_stub.
#include "aleppo_stub_env.cc"
#include <cmath>

namespace {
struct RecycleCallCount {
  long n = 0;
  ~RecycleCallCount() { std::fprintf(stderr, "stub: aleppo_recycle_dormant calls: %ld\n", n); }
} g_recycle_calls;
} // namespace

extern "C" int aleppo_recycle_dormant(aleppo_ctx *c, const uint8_t *observations, int64_t n, double tau, int layers,
                                      uint64_t key, int flags, uint8_t *mask_out, size_t unit_count,
                                      int64_t counts[ALEPPO_RECYCLE_COUNTS]) {
  g_recycle_calls.n++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  const int H = c->cfg.hidden_size;
  if (!counts || unit_count != (size_t)(160 + H) || (flags & ~ALEPPO_RECYCLE_KEEP_MOMENTS) || layers <= 0 ||
      (layers & ~ALEPPO_RECYCLE_ALL) || !(tau >= 0) || !std::isfinite(tau) || observations || n != 0)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: recycle_dormant: bad argument (the stand-in has the batch source only)");
  if (c->cfg.world_size > 1)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: recycle_dormant under world_size > 1");
  std::fprintf(stderr, "stub: aleppo_recycle_dormant tau=%.17g layers=%d key=%016llx flags=%d batch=%d mask_out=%d\n", tau,
               layers, (unsigned long long)key, flags, observations ? 0 : 1, mask_out ? 1 : 0);
  counts[4] = 0;
  for (int l = 0; l < 4; ++l) {
    counts[l] = (layers >> l) & 1 ? l + 1 : 0;
    counts[4] += counts[l];
  }
  if (mask_out)
    std::memset(mask_out, 0, unit_count);
  return ALEPPO_OK;
}
