// api_recycle.hip - C ABI (include/aleppo.h), acting on the representation: aleppo_recycle_units, aleppo_recycle_dormant
// (ReDo, Sokar et al. 2023).  Both rewrite P / M1 / M2 in place by one masked pass (recycle.hip) and rebuild every derived
// copy the way aleppo_load_params does (params_rewritten); no pointer changes, so a captured update stays valid.  Own stream only.
#include "api_internal.hpp"

using namespace aleppo;

static inline size_t unit_total(const aleppo_ctx *c) { return (size_t)(A1_C + A2_C + A3_C + c->H); }

static int ensure_mask(aleppo_ctx *c) {
  if (!c->rc_mask)
    HIPCHK(c, dalloc(c, &c->rc_mask, unit_total(c))); // (160 + H is a multiple of 4: the pass loads 4 bytes)
  return ALEPPO_OK;
}

// the pass over P / M1 / M2 with c->rc_mask, then everything derived from P; enqueued, not waited for
static void recycle_enqueue(aleppo_ctx *c, uint64_t key, int flags) {
  prof_begin(c, ALEPPO_K_RECYCLE);
  launch_recycle(c->stream, c->L, c->rc_mask, splitmix64(key), (flags & ALEPPO_RECYCLE_KEEP_MOMENTS) != 0, c->P, c->M1,
                 c->M2);
  prof_end(c, ALEPPO_K_RECYCLE);
  params_rewritten(c);
}

static void count_units(const aleppo_ctx *c, const uint8_t *mask, int64_t counts[ALEPPO_RECYCLE_COUNTS]) {
  const int first[5] = {0, A1_C, A1_C + A2_C, A1_C + A2_C + A3_C, (int)unit_total(c)};
  counts[4] = 0;
  for (int l = 0; l < 4; ++l) {
    counts[l] = 0;
    for (int u = first[l]; u < first[l + 1]; ++u)
      counts[l] += mask[u];
    counts[4] += counts[l];
  }
}

extern "C" int aleppo_recycle_units(aleppo_ctx *c, const uint8_t *mask, size_t unit_count, uint64_t key, int flags,
                                    int64_t counts[ALEPPO_RECYCLE_COUNTS]) {
  CHECK_CTX(c);
  const size_t U = unit_total(c);
  if (!mask || !counts)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "recycle_units: null argument");
  if (unit_count != U)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "recycle_units: unit_count must be 160 + H");
  if (flags & ~ALEPPO_RECYCLE_KEEP_MOMENTS)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "recycle_units: unknown flag bits");
  for (size_t u = 0; u < U; ++u)
    if (mask[u] > 1)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "recycle_units: a mask byte must be 0 or 1");
  std::vector<uint8_t> hm(mask, mask + U); // (the caller's memory is never the source of an asynchronous copy)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = ensure_mask(c))
    return rc;
  HIPCHK(c, copy_sync(c, c->rc_mask, hm.data(), U, hipMemcpyHostToDevice));
  recycle_enqueue(c, key, flags);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  count_units(c, hm.data(), counts);
  return ALEPPO_OK;
}

extern "C" int aleppo_recycle_dormant(aleppo_ctx *c, const uint8_t *observations, int64_t n, double tau, int layers,
                                      uint64_t key, int flags, uint8_t *mask_out, size_t unit_count,
                                      int64_t counts[ALEPPO_RECYCLE_COUNTS]) {
  CHECK_CTX(c);
  const size_t U = unit_total(c);
  if (!counts)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "recycle_dormant: null counts");
  if (unit_count != U)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "recycle_dormant: unit_count must be 160 + H");
  if (flags & ~ALEPPO_RECYCLE_KEEP_MOMENTS)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "recycle_dormant: unknown flag bits");
  if (layers <= 0 || (layers & ~ALEPPO_RECYCLE_ALL))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "recycle_dormant: layers must be a non-empty set of ALEPPO_RECYCLE_* bits");
  if (int rc = act_stats_check_tau(c, tau))
    return rc;
  if (int rc = source_check(c, observations, n))
    return rc;
  if (c->world > 1) // each rank would score its own samples and pick its own units: the replicas would part
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   "recycle_dormant: the scores describe one rank's samples; under world_size > 1 form one mask and "
                   "call aleppo_recycle_units on every rank");
  if (int rc = ensure_mask(c))
    return rc;
  const double *units_dev = nullptr, *layers_dev = nullptr;
  if (int rc = act_stats_measure(c, observations, n, tau, &units_dev, &layers_dev))
    return rc;
  launch_recycle_mask(c->stream, units_dev, c->H, tau, layers, c->rc_mask);
  recycle_enqueue(c, key, flags);
  HIPCHK(c, hipGetLastError());
  std::vector<uint8_t> hm(U);
  HIPCHK(c, copy_sync(c, hm.data(), c->rc_mask, U, hipMemcpyDeviceToHost));
  CHECK_ASYNC(c);
  if (mask_out)
    std::memcpy(mask_out, hm.data(), U);
  count_units(c, hm.data(), counts);
  return ALEPPO_OK;
}
