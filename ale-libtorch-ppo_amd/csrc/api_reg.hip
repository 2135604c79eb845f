// api_reg.hip - C ABI (include/aleppo.h), acting on the parameters from outside the gradient: the anchor of
// ALEPPO_OPT_ANCHOR_COEF (aleppo_anchor_take, aleppo_anchor_import, aleppo_anchor_export) and aleppo_shrink_perturb.  The
// anchor (c->anchor) is a fourth parameter set in the private layout: fp32 only, never forwarded, written by the first two
// calls alone and read by reg_step_kernel (kernels.hip) inside aleppo_train.  aleppo_shrink_perturb rewrites P in place by
// one pass (recycle.hip) and rebuilds every derived copy (params_rewritten); no pointer changes, so a captured update stays
// valid.  Own stream only.
#include "api_internal.hpp"

using namespace aleppo;

extern "C" int aleppo_anchor_take(aleppo_ctx *c, int source_set) {
  CHECK_CTX(c);
  ParamView src{};
  if (int rc = set_view(c, source_set, &src))
    return rc;
  if (int rc = param_set_storage(c, &c->anchor, false, "anchor"))
    return rc;
  if (int rc = param_set_copy(c, &c->anchor, src))
    return rc;
  c->anchor.on = true;
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_anchor_export(aleppo_ctx *c, float *flat, size_t count) {
  CHECK_CTX(c);
  return param_set_export(c, c->anchor, NO_ANCHOR, flat, count);
}

extern "C" int aleppo_anchor_import(aleppo_ctx *c, const float *flat, size_t count) {
  CHECK_CTX(c);
  static const char *const refusal = "anchor_import: wrong element count";
  if (!flat || count != c->L.reference_count()) // (here too: a refused call allocates nothing)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, refusal);
  if (int rc = param_set_storage(c, &c->anchor, false, "anchor"))
    return rc;
  if (int rc = param_set_upload(c, &c->anchor, flat, count, refusal))
    return rc;
  c->anchor.on = true;
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
  params_rewritten(c);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}
