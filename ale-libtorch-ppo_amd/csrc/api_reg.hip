// api_reg.hip - C ABI (include/aleppo.h), acting on the parameters from outside the gradient: the anchor of
// ALEPPO_OPT_ANCHOR_COEF (aleppo_anchor_take, aleppo_anchor_import, aleppo_anchor_export) and aleppo_shrink_perturb.  The
// anchor (Pa) is a fourth parameter set in the private layout: fp32 only, never forwarded, written by the first two calls
// alone and read by reg_step_kernel (kernels.hip) inside aleppo_train.  aleppo_shrink_perturb rewrites P in place by one
// pass (recycle.hip) and rebuilds every derived copy the way aleppo_recycle_units does; no pointer changes, so a captured
// update stays valid.  Own stream only.
#include "api_internal.hpp"

using namespace aleppo;

static uint64_t splitmix64(uint64_t x) { // the permutation of aleppo.h (aleppo_read_sample_order)
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// first use: the anchor's storage, zero-filled; a failure leaves the context without one
static int anchor_storage(aleppo_ctx *c) {
  if (c->Pa)
    return ALEPPO_OK;
  float *pa = nullptr;
  const hipError_t e = dalloc(c, &pa, c->L.total() * 4);
  if (e != hipSuccess)
    return set_err(c, ALEPPO_ERR_HIP, std::string("anchor: allocation failed: ") + hipGetErrorString(e));
  c->Pa = pa;
  return ALEPPO_OK;
}

extern "C" int aleppo_anchor_take(aleppo_ctx *c, int source_set) {
  CHECK_CTX(c);
  ParamView src{};
  if (int rc = set_view(c, source_set, &src))
    return rc;
  if (int rc = anchor_storage(c))
    return rc;
  HIPCHK(c, hipMemcpyAsync(c->Pa, src.P, c->L.total() * 4, hipMemcpyDeviceToDevice, c->stream));
  c->anchor_on = true;
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_anchor_export(aleppo_ctx *c, float *flat, size_t count) {
  CHECK_CTX(c);
  if (!c->anchor_on)
    return set_err(c, ALEPPO_ERR_RUNTIME, "no anchor: call aleppo_anchor_take or aleppo_anchor_import first");
  return export_flat(c, c->Pa, flat, count);
}

extern "C" int aleppo_anchor_import(aleppo_ctx *c, const float *flat, size_t count) {
  CHECK_CTX(c);
  if (!flat || count != c->L.reference_count())
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "anchor_import: wrong element count");
  if (int rc = anchor_storage(c))
    return rc;
  std::vector<float> tmp(c->L.total());
  params_to_internal(c->L, flat, tmp.data());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, copy_sync(c, c->Pa, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
  c->anchor_on = true;
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_shrink_perturb(aleppo_ctx *c, double shrink, double sigma, uint64_t key, int flags) {
  CHECK_CTX(c);
  if (!std::isfinite(shrink) || !(shrink >= 0.0 && shrink <= 1.0))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "shrink_perturb: shrink must be finite and in [0, 1]");
  if (!std::isfinite(sigma) || !(sigma >= 0.0))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "shrink_perturb: sigma must be finite and >= 0");
  if (flags & ~ALEPPO_SP_RESET_MOMENTS)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "shrink_perturb: unknown flag bits");
  const float sg = (float)sigma;
  if (!std::isfinite(sg))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "shrink_perturb: sigma does not fit a float");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  prof_begin(c, ALEPPO_K_RECYCLE); // (the class of the in-place passes over the parameters)
  launch_shrink_perturb(c->stream, c->L, splitmix64(key), (float)shrink, sg, c->P);
  prof_end(c, ALEPPO_K_RECYCLE);
  if (flags & ALEPPO_SP_RESET_MOMENTS) {
    HIPCHK(c, hipMemsetAsync(c->M1, 0, c->L.total() * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->M2, 0, c->L.total() * 4, c->stream));
  }
  refresh_compute_copies(c);
  c->pre_acted = -1;        // (what aleppo_step pre-computed used the old parameters)
  c->ts_step_valid = false; // (aleppo_tensor_stats: the parameters are no longer the last step's)
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}
