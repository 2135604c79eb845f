// TEST INFRASTRUCTURE - aleppo_stub_env.cc plus a host-only aleppo_tensor_stats, so that the trainer's log_tensor_stats key
// runs without a GPU.  What is real and what is made up: the stand-in keeps parameters (aleppo_stub.cc moves them by
// lr / 2 per aleppo_train) and Adam moments (aleppo_stub_state.cc: zero unless a checkpoint was imported), so SIZE, the
// PARAM_ columns and the UPDATE_ columns are computed from those arrays in double, row by row, with the header's rule
// for non-finite elements.  It keeps NO gradient: GRAD_NORM of row k is the made-up 1 / (k + 1) and GRAD_MAXABS half of
// that, the same on every call.  u uses s = c = 1 (the stand-in has no schedule).  Validation follows the header:
// sections, count, null pointer, an armed step.  Never linked into anything but trainer/train_tstats_stub.
#include "aleppo_stub_env.cc"
#include <cmath>

extern "C" int aleppo_tensor_stats(aleppo_ctx *c, int sections, double *out, size_t count) {
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (!out || count != (size_t)ALEPPO_TENSOR_STATS_ROWS * ALEPPO_TENSOR_STATS_COLS || sections <= 0 ||
      (sections & ~(ALEPPO_TS_SEC_PARAMS | ALEPPO_TS_SEC_STEP)))
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: tensor_stats: bad argument");
  stub_state_init(c);
  const bool params = sections & ALEPPO_TS_SEC_PARAMS, step = sections & ALEPPO_TS_SEC_STEP;
  const size_t H = (size_t)c->cfg.hidden_size, A = (size_t)c->cfg.num_actions;
  const size_t sizes[12] = {32 * 256, 32, 64 * 512, 64, 64 * 576, 64, H * 3136, H, A * H, A, H, 1};
  double tot[ALEPPO_TENSOR_STATS_COLS] = {}, tot_sq_p = 0, tot_sq_g = 0, tot_sq_u = 0;
  size_t at = 0;
  for (int k = 0; k < 12; ++k) {
    double sq_p = 0, sq_u = 0, max_p = 0, max_u = 0, nf_p = 0, nf_s = 0;
    for (size_t i = at; i < at + sizes[k]; ++i) {
      const float p = c->params[i], m = g_m1[i], v = g_m2[i];
      const float u = m / (std::sqrt(v) + 1e-5f);
      if (std::isfinite(p))
        sq_p += (double)p * p, max_p = std::max(max_p, (double)std::fabs(p));
      else
        nf_p += 1;
      if (std::isfinite(m) && std::isfinite(v) && std::isfinite(u))
        sq_u += (double)u * u, max_u = std::max(max_u, (double)std::fabs(u));
      else
        nf_s += 1;
    }
    at += sizes[k];
    const double gn = 1.0 / (k + 1);
    double *o = out + k * ALEPPO_TENSOR_STATS_COLS;
    const double row[ALEPPO_TENSOR_STATS_COLS] = {(double)sizes[k], std::sqrt(sq_p), max_p, nf_p, gn, 0.5 * gn,
                                                  std::sqrt(sq_u), max_u, std::sqrt(sq_u) / std::sqrt(sq_p), nf_s};
    for (int j = 0; j < ALEPPO_TENSOR_STATS_COLS; ++j)
      o[j] = j == 0 || (j <= ALEPPO_TS_PARAM_NONFINITE ? params : step) ? row[j] : 0.0;
    tot[ALEPPO_TS_SIZE] += row[ALEPPO_TS_SIZE], tot[ALEPPO_TS_PARAM_NONFINITE] += nf_p, tot[ALEPPO_TS_STEP_NONFINITE] += nf_s;
    tot[ALEPPO_TS_PARAM_MAXABS] = std::max(tot[ALEPPO_TS_PARAM_MAXABS], max_p);
    tot[ALEPPO_TS_GRAD_MAXABS] = std::max(tot[ALEPPO_TS_GRAD_MAXABS], 0.5 * gn);
    tot[ALEPPO_TS_UPDATE_MAXABS] = std::max(tot[ALEPPO_TS_UPDATE_MAXABS], max_u);
    tot_sq_p += sq_p, tot_sq_g += gn * gn, tot_sq_u += sq_u;
  }
  tot[ALEPPO_TS_PARAM_NORM] = std::sqrt(tot_sq_p), tot[ALEPPO_TS_GRAD_NORM] = std::sqrt(tot_sq_g);
  tot[ALEPPO_TS_UPDATE_NORM] = std::sqrt(tot_sq_u);
  tot[ALEPPO_TS_UPDATE_RATIO] = tot[ALEPPO_TS_UPDATE_NORM] / tot[ALEPPO_TS_PARAM_NORM];
  double *o = out + 12 * ALEPPO_TENSOR_STATS_COLS;
  for (int j = 0; j < ALEPPO_TENSOR_STATS_COLS; ++j)
    o[j] = j == 0 || (j <= ALEPPO_TS_PARAM_NONFINITE ? params : step) ? tot[j] : 0.0;
  return ALEPPO_OK;
}
