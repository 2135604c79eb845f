// head_train.hip - the PPO head training kernel's three __global__ entry points and their launcher (the kernel itself is
// described below, "PPO head, training"; its body is head_train_body.inc).  A translation unit of its own: the
// 96 instantiations compile next to kernels.hip.
#include "head_train.hpp"

namespace aleppo {

// ================================================================================================
// PPO head, training.  Fuses: action/value linear layers (train.cc:245-253,262-263), normalize_logits
// (losses.cc:45-47), losses::compute forward (losses.cc:4-26) with its closed-form backward (SURVEY
// app. B: autograd's gradient of the masked-mean loss), the head dgrad (dh) and the head wgrad
// partials.  One wave per sample row, 4 waves per workgroup, rows strided over the grid; every
// workgroup writes ONE partial slab of head-weight gradients (summed later in fixed order).
// 1/N_m uses the GLOBAL unmasked count so that an all-reduce SUM over ranks yields the mean (8e).
// ================================================================================================
// Wide action sets (AMAX = 18: 19 x 8 wgrad accumulators per lane) run 4 waves per workgroup: one wave per SIMD may
// use the whole 512-entry register file; with 8 waves the 256-register cap spilled the accumulators (150 us vs 22).
// VCLIP (ALEPPO_OPT_VALUE_CLIP): the value term is the clipped one of aleppo.h against vold, the values the samples were
// collected with; without it vold is never read.  ps_kl / ps_cf (approx-KL and clip fraction) are written either way.
// ADVN (ALEPPO_OPT_ADV_NORM_MINIBATCH): every row's advantage a becomes (a - advs[0]) * advs[1] in fp32, this minibatch's
// (mean_f, inv_f) from advn_stats_kernel; without it advs is never read.
// KLPEN (ALEPPO_OPT_KL_PENALTY): the exact KL(pi_old || pi) of every row goes to ps_kle, and with beta = klb[0] != 0 the
// loss gains beta KL and its gradient beta (p S - q) (include/aleppo.h).  The body is shared by three entry points:
// head_train_kernel (ADVN and KLPEN off, the default path's instantiations), head_train_advn_kernel (ADVN on) and
// head_train_kl_kernel (KLPEN on, with advantage normalisation a run-time switch: advs may be null).
// Waves per workgroup: 8, or 4 where one wave per SIMD needs more than 256 registers - the wide action sets, and with
// the KL penalty (its S / KL pass and the q_a of the gradient) from AMAX = 10 on (8 waves spilled ~40 registers there).
// The clip range, the value-clip range and the two loss coefficients are slots 0-3 of the device block of
// ALEPPO_OPT_CLIP_PARAM and its kin (common.hpp HYPER_*), read once per workgroup: a captured update follows values changed
// between calls.  The entry points and their launcher, launch_head_train, follow.

template <class T, int AMAX, class RT, bool VCLIP>
__global__ __launch_bounds__(AMAX > 10 ? 256 : 512) void head_train_kernel(HEAD_PARAMS) {
  constexpr bool ADVN = false, KLPEN = false;
  const float *advs = nullptr, *klb = nullptr;
  float *ps_kle = nullptr;
#include "head_train_body.inc"
}
// advs: float [4] of this minibatch (mean_f, inv_f, std, 0)
template <class T, int AMAX, class RT, bool VCLIP>
__global__ __launch_bounds__(AMAX > 10 ? 256 : 512) void head_train_advn_kernel(HEAD_PARAMS,
                                                                                 const float *__restrict__ advs) {
  constexpr bool ADVN = true, KLPEN = false;
  const float *klb = nullptr;
  float *ps_kle = nullptr;
#include "head_train_body.inc"
}
// advs: as above, or nullptr (no minibatch normalisation); klb: float [1], beta; ps_kle: float [B], the exact KL per row
template <class T, int AMAX, class RT, bool VCLIP>
__global__ __launch_bounds__(64 * head_waves(AMAX, true)) void head_train_kl_kernel(HEAD_PARAMS,
                                                                                    const float *__restrict__ advs,
                                                                                    const float *__restrict__ klb,
                                                                                    float *ps_kle) {
  constexpr bool ADVN = true, KLPEN = true;
#define HEAD_TRAIN_PASSES
#include "head_train_body.inc"
#undef HEAD_TRAIN_PASSES
}

template <class T, int AM, class RT, bool VCLIP>
static void head_train_launch(hipStream_t s, const HeadTrainArgs &a, const float *hp) {
  const int H = a.H;
  const size_t sm = ((size_t)((AM + 1) + ((AM + 1) > 8 ? (AM + 1) : 8)) * H + 8 * (AM + 1)) * sizeof(float);
  const void *fn = a.klb    ? reinterpret_cast<const void *>(&head_train_kl_kernel<T, AM, RT, VCLIP>)
                   : a.advs ? reinterpret_cast<const void *>(&head_train_advn_kernel<T, AM, RT, VCLIP>)
                            : reinterpret_cast<const void *>(&head_train_kernel<T, AM, RT, VCLIP>);
  if (sm > 48 * 1024)
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
#define HEAD_ARGS                                                                                                      \
  a.h, a.Wh, a.bh, a.act, static_cast<const RT *>(a.oldlp), static_cast<const RT *>(a.adv),                            \
      static_cast<const RT *>(a.ret), static_cast<const RT *>(a.vold), a.mask, a.mask_count, hp,                       \
      static_cast<T *>(a.dh), a.ps_total, a.ps_clipped, a.ps_value, a.ps_entropy, a.ps_ratio, a.ps_kl, a.ps_cf,        \
      a.slab_w, a.slab_b, a.B, a.H, a.A, a.logits_out, a.values_out, a.hparts
  if (a.klb)
    hipLaunchKernelGGL((head_train_kl_kernel<T, AM, RT, VCLIP>), dim3(a.nblk), dim3(64 * head_waves(AM, true)), sm, s,
                       HEAD_ARGS, a.advs, a.klb, a.ps_kle);
  else if (a.advs)
    hipLaunchKernelGGL((head_train_advn_kernel<T, AM, RT, VCLIP>), dim3(a.nblk), dim3(AM > 10 ? 256 : 512), sm, s,
                       HEAD_ARGS, a.advs);
  else
    hipLaunchKernelGGL((head_train_kernel<T, AM, RT, VCLIP>), dim3(a.nblk), dim3(AM > 10 ? 256 : 512), sm, s,
                       HEAD_ARGS);
#undef HEAD_ARGS
}
template <class T, class RT, bool VCLIP>
static void head_train_amax(hipStream_t s, const HeadTrainArgs &a, const float *hp) {
  if (a.A <= 4)
    head_train_launch<T, 4, RT, VCLIP>(s, a, hp);
  else if (a.A <= 6)
    head_train_launch<T, 6, RT, VCLIP>(s, a, hp);
  else if (a.A <= 10)
    head_train_launch<T, 10, RT, VCLIP>(s, a, hp);
  else
    head_train_launch<T, 18, RT, VCLIP>(s, a, hp);
}
template <class T, class RT> static void head_train_vclip(hipStream_t s, const HeadTrainArgs &a, const float *hp) {
  if (a.vold)
    head_train_amax<T, RT, true>(s, a, hp);
  else
    head_train_amax<T, RT, false>(s, a, hp);
}
// aleppo_export_backward: row r of h as the kernels above fetch it (their zero, their add_h_slabs) -> out [B][H].  One wave
// per row, four rows per workgroup; reads only.
__global__ __launch_bounds__(256) void h_export_kernel(const float *__restrict__ h, int hparts, long B, int H,
                                                       float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B || lane * 8 >= H)
    return;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    acc[i] = 0.f;
  add_h_slabs(h, hparts, B, r, H, lane, acc);
  float *dst = out + (size_t)r * H + lane * 4;
  *reinterpret_cast<f32x4 *>(dst) = f32x4{acc[0], acc[1], acc[2], acc[3]};
  *reinterpret_cast<f32x4 *>(dst + H / 2) = f32x4{acc[4], acc[5], acc[6], acc[7]};
}
void launch_h_export(hipStream_t s, const float *h, int hparts, long B, int H, float *out) {
  hipLaunchKernelGGL(h_export_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, h, hparts, B, H, out);
}

void launch_head_train(hipStream_t s, const HeadTrainArgs &a, const float *hp) {
  if (a.prec == ALEPPO_BF16) {
    if (a.rt16)
      head_train_vclip<bf16, f16>(s, a, hp);
    else
      head_train_vclip<bf16, float>(s, a, hp);
  } else {
    if (a.rt16)
      head_train_vclip<float, f16>(s, a, hp);
    else
      head_train_vclip<float, float>(s, a, hp);
  }
}

} // namespace aleppo
