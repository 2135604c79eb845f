// api_grad_probe.hip - C ABI (include/aleppo.h), gradient probes: aleppo_grad_probe, aleppo_grad_take, aleppo_grad_export,
// aleppo_grad_import, aleppo_grad_gram.  The ALEPPO_GRAD_SLOTS gradient slots (c->grad_slots, padded vectors in the private
// layout) live next to G and only these calls write them.  aleppo_grad_probe runs the gradient half of aleppo_train's
// minibatch (grad_probe_enqueue, api_train.hip) with the slot as its destination and private storage for everything the
// head kernel writes; aleppo_grad_gram is the read-only pass of grad_gram.hip.  Nothing here writes P, the moments, G, the
// per-sample metric planes or anything else aleppo_train, aleppo_state_digest or a checkpoint reads.
#include "api_internal.hpp"

using namespace aleppo;

static bool bad_slot(int slot) { return slot < 0 || slot >= ALEPPO_GRAD_SLOTS; }
static float *slot_ptr(const aleppo_ctx *c, int slot) { return c->grad_slots + (size_t)slot * c->L.total(); }
// the slots, together, on the first call that writes one (zero-filled: pads stay zero under every writer)
static int ensure_slots(aleppo_ctx *c) {
  if (!c->grad_slots)
    HIPCHK(c, dalloc(c, &c->grad_slots, (size_t)ALEPPO_GRAD_SLOTS * c->L.total() * 4));
  return ALEPPO_OK;
}

extern "C" int aleppo_grad_probe(aleppo_ctx *c, int slot, int64_t first, int64_t n, const aleppo_grad_probe_config *cfg,
                                 int64_t *unmasked_out) {
  CHECK_CTX(c);
  if (bad_slot(slot))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "grad_probe: slot must be in [0, ALEPPO_GRAD_SLOTS)");
  aleppo_grad_probe_config g{1, c->hyper.c_v, c->hyper.c_e, 0};
  if (cfg)
    g = *cfg;
  if ((g.policy_term != 0 && g.policy_term != 1) || !std::isfinite(g.value_loss_coef) || g.value_loss_coef < 0.f ||
      !std::isfinite(g.entropy_coef) || g.entropy_coef < 0.f || g.reserved != 0)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "grad_probe: policy_term must be 0 or 1, the two coefficients finite and >= 0, reserved 0");
  if (c->batch_n <= 0)
    return set_err(c, ALEPPO_ERR_RUNTIME, "no batch: call aleppo_finish_rollout or aleppo_set_batch first");
  if (n < 1 || n > c->maxB || first < 0 || first > c->batch_n - n)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "grad_probe: samples [first, first + n) must lie in the batch, 1 <= n <= max(E, max_minibatch)");
  if (c->value_clip && c->val_src == Ctx::VAL_NONE)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   "ALEPPO_OPT_VALUE_CLIP needs the batch's old values: call aleppo_set_batch_values after aleppo_set_batch");
  if (int rc = ensure_slots(c))
    return rc;
  if (!c->gp_blk)
    HIPCHK(c, dalloc(c, &c->gp_blk, GP_BLOCK * 4));
  if (!c->h_gp_blk) // (each on its own: a failure between the two must not leave the next call with half of the pair)
    HIPCHK(c, halloc(c, &c->h_gp_blk, GP_BLOCK * 4, hipHostMallocDefault));
  if (!c->gp_ps)
    HIPCHK(c, dalloc(c, &c->gp_ps, (size_t)8 * c->maxB * 4));
  hipStream_t s = c->stream;
  HIPCHK(c, hipStreamSynchronize(s)); // (also: the pinned block below is no longer being read)
  // the network runs in the shared activation scratch (net_forward drops aleppo_export_backward's mark itself)
  c->pre_acted = -1;
  c->bwd.B = 0;
  acted_clear(c);
  // the private block: clip and value-clip range as aleppo_train uploads them, the call's coefficients, the record
  // (+0.0f, +0.0f) the head reads with policy_term = 0, beta
  float *b = c->h_gp_blk;
  std::memset(b, 0, GP_BLOCK * 4);
  b[GP_HYPER + HYPER_CLIP] = c->hyper.clip;
  b[GP_HYPER + HYPER_VCLIP] = c->vclip_range_set ? c->value_clip_range : c->hyper.clip;
  b[GP_HYPER + HYPER_CV] = g.value_loss_coef;
  b[GP_HYPER + HYPER_CE] = g.entropy_coef;
  std::memcpy(&b[GP_BETA], &c->kl_coef_bits, 4);
  HIPCHK(c, hipMemcpyAsync(c->gp_blk, b, GP_BLOCK * 4, hipMemcpyHostToDevice, s));
  int rc = grad_probe_enqueue(c, (long)first, (long)n, g.policy_term == 1, c->gp_blk, c->gp_ps, slot_ptr(c, slot));
  if (rc == ALEPPO_OK) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
      rc = set_err(c, ALEPPO_ERR_HIP, std::string("grad_probe: ") + hipGetErrorString(e));
  }
  if (rc) { // part of the gradient may be in the slot: it no longer holds what it held
    c->grad_written[slot] = false;
    return rc;
  }
  float count = 0.f;
  HIPCHK(c, hipMemcpyAsync(b + GP_COUNT, c->gp_blk + GP_COUNT, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  CHECK_ASYNC(c);
  count = b[GP_COUNT];
  c->grad_written[slot] = true;
  if (unmasked_out)
    *unmasked_out = (int64_t)count;
  return ALEPPO_OK;
}

extern "C" int aleppo_grad_take(aleppo_ctx *c, int slot, int source, int set) {
  CHECK_CTX(c);
  if (bad_slot(slot))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "grad_take: slot must be in [0, ALEPPO_GRAD_SLOTS)");
  const size_t n = c->L.total();
  if (source == ALEPPO_GRAD_SRC_EXP_AVG) {
    if (set != 0)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "grad_take: set must be 0 with ALEPPO_GRAD_SRC_EXP_AVG");
    if (int rc = ensure_slots(c))
      return rc;
    HIPCHK(c, hipMemcpyAsync(slot_ptr(c, slot), c->M1, n * 4, hipMemcpyDeviceToDevice, c->stream));
  } else if (source == ALEPPO_GRAD_SRC_PARAM_DELTA) {
    if (set != ALEPPO_SET_AVERAGED && set != ALEPPO_SET_SNAPSHOT)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "grad_take: set must be ALEPPO_SET_AVERAGED or ALEPPO_SET_SNAPSHOT with ALEPPO_GRAD_SRC_PARAM_DELTA");
    ParamView view{};
    if (int rc = set_view(c, set, &view))
      return rc;
    if (int rc = ensure_slots(c))
      return rc;
    launch_grad_delta(c->stream, c->P, view.P, slot_ptr(c, slot), (long)n);
    HIPCHK(c, hipGetLastError());
  } else {
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "grad_take: source must be ALEPPO_GRAD_SRC_EXP_AVG or ALEPPO_GRAD_SRC_PARAM_DELTA");
  }
  c->grad_written[slot] = true;
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_grad_export(aleppo_ctx *c, int slot, float *flat, size_t count) {
  CHECK_CTX(c);
  if (bad_slot(slot))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "grad_export: slot must be in [0, ALEPPO_GRAD_SLOTS)");
  if (!c->grad_written[slot])
    return set_err(c, ALEPPO_ERR_RUNTIME, "grad_export: nothing has written this slot");
  return export_flat(c, slot_ptr(c, slot), flat, count);
}

extern "C" int aleppo_grad_import(aleppo_ctx *c, int slot, const float *flat, size_t count) {
  CHECK_CTX(c);
  static const char *const refusal = "grad_import: wrong element count";
  if (bad_slot(slot))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "grad_import: slot must be in [0, ALEPPO_GRAD_SLOTS)");
  if (!flat || count != c->L.reference_count()) // (here too: a refused call allocates nothing)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, refusal);
  if (int rc = ensure_slots(c))
    return rc;
  if (int rc = upload_flat(c, slot_ptr(c, slot), flat, count, refusal))
    return rc;
  c->grad_written[slot] = true;
  return ALEPPO_OK;
}

extern "C" int aleppo_grad_gram(aleppo_ctx *c, const int32_t *slots, int k, double *gram, size_t gram_count,
                                int64_t *nonfinite, size_t nonfinite_count) {
  CHECK_CTX(c);
  const size_t rows = ALEPPO_TENSOR_STATS_ROWS;
  if (!slots || k < 1 || k > ALEPPO_GRAD_SLOTS)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "grad_gram: slots must name 1 to ALEPPO_GRAD_SLOTS slots");
  for (int i = 0; i < k; ++i)
    if (bad_slot(slots[i]))
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "grad_gram: slot must be in [0, ALEPPO_GRAD_SLOTS)");
  if (!gram || gram_count != rows * k * k || (nonfinite ? nonfinite_count != rows : nonfinite_count != 0))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "grad_gram: gram_count must be 13 * k * k, nonfinite_count 13 (0 with a NULL nonfinite)");
  for (int i = 0; i < k; ++i)
    if (!c->grad_written[slots[i]])
      return set_err(c, ALEPPO_ERR_RUNTIME, "grad_gram: nothing has written one of the named slots");
  if (!c->gg_scratch)
    HIPCHK(c, dalloc(c, &c->gg_scratch, grad_gram_scratch_bytes(c->L)));
  const float *vec[ALEPPO_GRAD_SLOTS];
  for (int i = 0; i < k; ++i)
    vec[i] = slot_ptr(c, slots[i]);
  const double *dev = nullptr;
  prof_begin(c, ALEPPO_K_ACT_STATS); // (the class of the read-only diagnostic passes)
  launch_grad_gram(c->stream, vec, k, c->L, c->gg_scratch, &dev);
  prof_end(c, ALEPPO_K_ACT_STATS);
  HIPCHK(c, hipGetLastError());
  // the results pass through a host temporary: a failed call writes nothing
  double out[ALEPPO_TENSOR_STATS_ROWS * (ALEPPO_GRAD_SLOTS * ALEPPO_GRAD_SLOTS + 1)];
  const size_t nd = rows * k * k;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, copy_sync(c, out, dev, (nd + rows) * sizeof(double), hipMemcpyDeviceToHost));
  CHECK_ASYNC(c);
  std::memcpy(gram, out, nd * sizeof(double));
  if (nonfinite)
    std::memcpy(nonfinite, out + nd, rows * sizeof(int64_t));
  return ALEPPO_OK;
}
