// api_acts.hip - C ABI (include/aleppo.h), the representation: aleppo_forward_activations, aleppo_activation_stats,
// aleppo_export_backward, aleppo_export_acting.  The first two run the network over a SampleSource (api_internal.hpp), as
// aleppo_forward does, and then only read a1 / a2 / a3 / h; the third runs nothing and reads what the last update left there
// and in dh / dz3 / dz2 / dz1, the fourth what the rollout's last acting forward left in a1 / a2 / a3 / hpart.  Nothing here
// touches what the rollout or a captured update can observe.
#include "api_internal.hpp"

using namespace aleppo;

extern "C" int aleppo_forward_activations(aleppo_ctx *c, const uint8_t *observations, int64_t n, float *conv1,
                                          float *conv2, float *conv3, float *fc) {
  CHECK_CTX(c);
  if (!observations)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "forward_activations: null observations");
  if (!conv1 && !conv2 && !conv3 && !fc)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "forward_activations: at least one output must be given");
  if (n <= 0 || n > c->maxB)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "forward_activations: n exceeds capacity");
  float *const out[3] = {conv1, conv2, conv3};
  const void *const act[3] = {c->a1, c->a2, c->a3};
  const size_t per[3] = {(size_t)A1_PIX * A1_C, (size_t)A2_PIX * A2_C, (size_t)A3_PIX * A3_C};
  size_t need = 0;
  for (int l = 0; l < 3; ++l)
    need += out[l] ? (size_t)n * per[l] * 4 : 0;
  HIPCHK(c, grow(c, &c->ax_buf, &c->ax_cap, need, ALLOC_RAW));
  SampleSource src;
  if (int rc = source_open(c, observations, 0, n, &src))
    return rc;
  net_forward(c, src.obs, src.map, n); // (one chunk: n <= maxB)
  float *at = c->ax_buf; // (every layer's size is a multiple of 16 bytes: the areas stay aligned)
  for (int l = 0; l < 3; ++l) {
    if (!out[l])
      continue;
    launch_act_export(c->stream, c->prec, l, act[l], at, n);
    HIPCHK(c, hipMemcpyAsync(out[l], at, (size_t)n * per[l] * 4, hipMemcpyDeviceToHost, c->stream));
    at += (size_t)n * per[l];
  }
  if (fc)
    HIPCHK(c, hipMemcpyAsync(fc, c->h, (size_t)n * c->H * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

// What the last minibatch of the last aleppo_train left: the stored tensors of both passes, read and converted, nothing
// else.  One staging area in ax_buf, as large as the largest tensor asked for, reused tensor by tensor (stream order).
extern "C" int aleppo_export_backward(aleppo_ctx *c, int64_t capacity, float *conv1, float *conv2, float *conv3, float *fc,
                                      float *dfc, float *dconv3, float *dconv2, float *dconv1, int64_t *n,
                                      uint32_t *stored) {
  CHECK_CTX(c);
  if (!conv1 && !conv2 && !conv3 && !fc && !dfc && !dconv3 && !dconv2 && !dconv1)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "export_backward: at least one output must be given");
  const Ctx::BwdMark m = c->bwd;
  if (m.B <= 0)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   "export_backward: no update has run, or something else has run the network since the last one");
  if (capacity < m.B)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "export_backward: capacity is smaller than the minibatch");
  const size_t B = (size_t)m.B, H = (size_t)c->H;
  const size_t per[3] = {(size_t)A1_PIX * A1_C, (size_t)A2_PIX * A2_C, (size_t)A3_PIX * A3_C};
  // (layer of launch_act_export, source, destination) - the gradients have their activations' shapes
  struct Conv {
    int layer;
    const void *src;
    float *dst;
  } const convs[6] = {{0, c->a1, conv1},  {1, c->a2, conv2},  {2, c->a3, conv3},
                      {2, c->dz3, dconv3}, {1, c->dz2, dconv2}, {0, m.dz1 ? c->dz1 : nullptr, dconv1}};
  size_t need = (fc || dfc) ? B * H * 4 : 0;
  for (const Conv &t : convs)
    if (t.src && t.dst)
      need = std::max(need, B * per[t.layer] * 4);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, grow(c, &c->ax_buf, &c->ax_cap, need, ALLOC_RAW));
  for (const Conv &t : convs) {
    if (!t.src || !t.dst)
      continue;
    launch_act_export(c->stream, c->prec, t.layer, t.src, c->ax_buf, m.B);
    HIPCHK(c, hipMemcpyAsync(t.dst, c->ax_buf, B * per[t.layer] * 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (fc) {
    launch_h_export(c->stream, c->h, m.hparts, m.B, c->H, c->ax_buf);
    HIPCHK(c, hipMemcpyAsync(fc, c->ax_buf, B * H * 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (dfc) {
    launch_plane_export(c->stream, c->prec, c->dh, c->ax_buf, (long)(B * H));
    HIPCHK(c, hipMemcpyAsync(dfc, c->ax_buf, B * H * 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  if (n)
    *n = m.B;
  if (stored)
    *stored = ALEPPO_BWD_CONV1 | ALEPPO_BWD_CONV2 | ALEPPO_BWD_CONV3 | ALEPPO_BWD_FC | ALEPPO_BWD_DFC | ALEPPO_BWD_DCONV3 |
              ALEPPO_BWD_DCONV2 | (m.dz1 ? ALEPPO_BWD_DCONV1 : 0);
  return ALEPPO_OK;
}

// What the rollout's last acting forward left (Ctx::acted): a1 / a2 where the route stored them, a3 and the split-K slices
// of fc, read and converted, nothing else - the acting twin of aleppo_export_backward, with its staging.
static_assert(ALEPPO_FC_SPLITS == FC_SPLITS, "include/aleppo.h states the number of split-K slices");
extern "C" int aleppo_export_acting(aleppo_ctx *c, int64_t capacity, float *conv1, float *conv2, float *conv3,
                                    float *fc_parts, int64_t *n, uint32_t *stored) {
  CHECK_CTX(c);
  if (!conv1 && !conv2 && !conv3 && !fc_parts)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "export_acting: at least one output must be given");
  const Ctx::ActMark m = c->acted;
  if (m.n <= 0)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   "export_acting: no acting forward has run, or something else has run the network or replaced the "
                   "parameters since the last one");
  if (capacity < m.n)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "export_acting: capacity is smaller than num_envs");
  const size_t ns = (size_t)m.n;
  const size_t per[3] = {(size_t)A1_PIX * A1_C, (size_t)A2_PIX * A2_C, (size_t)A3_PIX * A3_C};
  struct Conv {
    int layer;
    const void *src;
    float *dst;
  } const convs[3] = {{0, m.a12 ? c->a1 : nullptr, conv1}, {1, m.a12 ? c->a2 : nullptr, conv2}, {2, c->a3, conv3}};
  size_t need = 0;
  for (const Conv &t : convs)
    if (t.src && t.dst)
      need = std::max(need, ns * per[t.layer] * 4);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (need)
    HIPCHK(c, grow(c, &c->ax_buf, &c->ax_cap, need, ALLOC_RAW));
  for (const Conv &t : convs) {
    if (!t.src || !t.dst)
      continue;
    launch_act_export(c->stream, c->prec, t.layer, t.src, c->ax_buf, (long)ns);
    HIPCHK(c, hipMemcpyAsync(t.dst, c->ax_buf, ns * per[t.layer] * 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (fc_parts) // fp32 already, [FC_SPLITS][n][H] with n = E: one copy
    HIPCHK(c, hipMemcpyAsync(fc_parts, c->hpart, (size_t)FC_SPLITS * ns * c->H * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  if (n)
    *n = m.n;
  if (stored)
    *stored = ALEPPO_ACTING_CONV3 | ALEPPO_ACTING_FC_PARTS | (m.a12 ? ALEPPO_ACTING_CONV1 | ALEPPO_ACTING_CONV2 : 0);
  return ALEPPO_OK;
}

namespace aleppo {
// what aleppo_activation_stats refuses in tau (aleppo_recycle_dormant measures the same way)
int act_stats_check_tau(aleppo_ctx *c, double tau) {
  if (!(tau >= 0.0) || !std::isfinite(tau))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "activation_stats: tau must be finite and non-negative");
  return ALEPPO_OK;
}
// the measurement itself, arguments already checked (source_check): the source's open, the forward chunks with one pass each
// and the finalising launch, all enqueued; *units_dev / *layers_dev: the two tables in the context's scratch (device memory)
int act_stats_measure(aleppo_ctx *c, const uint8_t *observations, int64_t n, double tau, const double **units_dev,
                      const double **layers_dev) {
  // the scratch holds the largest sample count either source can bring (the record count grows with it)
  if (!c->as_scratch)
    HIPCHK(c, dalloc(c, &c->as_scratch, act_stats_plan(c->prec, c->H, std::max(c->N, c->maxB), c->maxB).bytes));
  SampleSource src;
  if (int rc = source_open(c, observations, 0, n, &src))
    return rc;
  const ActStatsPlan pl = act_stats_plan(c->prec, c->H, src.total, c->maxB);
  size_t done[4] = {0, 0, 0, 0};
  source_walk(c, src, [&](const SampleMap &map, long, long ns) {
    net_forward(c, src.obs, map, ns);
    prof_begin(c, ALEPPO_K_ACT_STATS);
    launch_act_stats_partial(c->stream, c->prec, c->a1, c->a2, c->a3, c->h, c->H, ns, pl, done, c->as_scratch);
    prof_end(c, ALEPPO_K_ACT_STATS);
    return ALEPPO_OK;
  });
  launch_act_stats_final(c->stream, c->H, src.total, tau, pl, done, c->as_scratch, units_dev, layers_dev);
  HIPCHK(c, hipGetLastError());
  return ALEPPO_OK;
}
} // namespace aleppo

extern "C" int aleppo_activation_stats(aleppo_ctx *c, const uint8_t *observations, int64_t n, double tau, double *units,
                                       size_t unit_count, double *layers, size_t layer_count) {
  CHECK_CTX(c);
  const size_t U = (size_t)(A1_C + A2_C + A3_C + c->H);
  constexpr size_t LAYER_COUNT = (size_t)ALEPPO_ACT_LAYER_ROWS * ALEPPO_ACT_LAYER_COLS;
  if (int rc = act_stats_check_tau(c, tau))
    return rc;
  if (!units || !layers)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "activation_stats: null argument");
  if (unit_count != U * ALEPPO_ACT_UNIT_COLS || layer_count != LAYER_COUNT)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "activation_stats: unit_count must be (160 + H) * 5 and layer_count 40");
  if (int rc = source_check(c, observations, n))
    return rc;
  const double *units_dev = nullptr, *layers_dev = nullptr;
  if (int rc = act_stats_measure(c, observations, n, tau, &units_dev, &layers_dev))
    return rc;
  std::vector<double> hu(U * ALEPPO_ACT_UNIT_COLS);
  double hl[LAYER_COUNT];
  HIPCHK(c, hipMemcpyAsync(hu.data(), units_dev, hu.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hl, layers_dev, sizeof(hl), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  std::memcpy(units, hu.data(), hu.size() * sizeof(double));
  std::memcpy(layers, hl, sizeof(hl));
  return ALEPPO_OK;
}
