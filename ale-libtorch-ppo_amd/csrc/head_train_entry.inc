// head_train_entry.inc - the PPO head training kernel's three __global__ entry points and their launcher, as text that is
// instantiated once per way of passing the hyper-parameters (the includer defines, and owns, the macros):
//   HEAD_KERNEL / HEAD_ADVN_KERNEL / HEAD_KL_KERNEL  the entry points' names
//   HEAD_LAUNCH                                       the launcher's name (declared in common.hpp; HeadTrainArgs)
//   HEAD_HP_T                                         the type of the argument `hp`: Hyper by value, or the device block
//   HEAD_HYPER_LOAD                                   defines hp_clip / hp_vclip / hp_cv / hp_ce from `hp`
// kernels.hip: the default route, whose instantiations are the ones that existed before the device block did;
// head_hyper.hip: ALEPPO_OPT_CLIP_PARAM and its kin.  Needs head_train.hpp.
template <class T, int AMAX, class RT, bool VCLIP>
__global__ __launch_bounds__(AMAX > 10 ? 256 : 512) void HEAD_KERNEL(HEAD_PARAMS) {
  constexpr bool ADVN = false, KLPEN = false;
  const float *advs = nullptr, *klb = nullptr;
  float *ps_kle = nullptr;
#include "head_train_body.inc"
}
// advs: float [4] of this minibatch (mean_f, inv_f, std, 0)
template <class T, int AMAX, class RT, bool VCLIP>
__global__ __launch_bounds__(AMAX > 10 ? 256 : 512) void HEAD_ADVN_KERNEL(HEAD_PARAMS,
                                                                           const float *__restrict__ advs) {
  constexpr bool ADVN = true, KLPEN = false;
  const float *klb = nullptr;
  float *ps_kle = nullptr;
#include "head_train_body.inc"
}
// advs: as above, or nullptr (no minibatch normalisation); klb: float [1], beta; ps_kle: float [B], the exact KL per row
template <class T, int AMAX, class RT, bool VCLIP>
__global__ __launch_bounds__(64 * head_waves(AMAX, true)) void HEAD_KL_KERNEL(HEAD_PARAMS,
                                                                              const float *__restrict__ advs,
                                                                              const float *__restrict__ klb,
                                                                              float *ps_kle) {
  constexpr bool ADVN = true, KLPEN = true;
#define HEAD_TRAIN_PASSES
#include "head_train_body.inc"
#undef HEAD_TRAIN_PASSES
}

template <class T, class RT, bool VCLIP>
static void head_train_t(hipStream_t s, const HeadTrainArgs &a, HEAD_HP_T hp) {
  const int H = a.H;
#define HEAD_LAUNCH_ARGS                                                                                               \
  a.h, a.Wh, a.bh, a.act, static_cast<const RT *>(a.oldlp), static_cast<const RT *>(a.adv),                            \
      static_cast<const RT *>(a.ret), static_cast<const RT *>(a.vold), a.mask, a.mask_count, hp,                       \
      static_cast<T *>(a.dh), a.ps_total, a.ps_clipped, a.ps_value, a.ps_entropy, a.ps_ratio, a.ps_kl, a.ps_cf,        \
      a.slab_w, a.slab_b, a.B, a.H, a.A, a.logits_out, a.values_out, a.hparts
#define LAUNCH_HEAD(AM)                                                                                                \
  do {                                                                                                                 \
    const size_t sm = ((size_t)((AM + 1) + ((AM + 1) > 8 ? (AM + 1) : 8)) * H + 8 * (AM + 1)) * sizeof(float);         \
    const void *fn = a.klb    ? reinterpret_cast<const void *>(&HEAD_KL_KERNEL<T, AM, RT, VCLIP>)                      \
                     : a.advs ? reinterpret_cast<const void *>(&HEAD_ADVN_KERNEL<T, AM, RT, VCLIP>)                    \
                              : reinterpret_cast<const void *>(&HEAD_KERNEL<T, AM, RT, VCLIP>);                        \
    if (sm > 48 * 1024)                                                                                                \
      (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);                              \
    if (a.klb)                                                                                                         \
      hipLaunchKernelGGL((HEAD_KL_KERNEL<T, AM, RT, VCLIP>), dim3(a.nblk), dim3(64 * head_waves(AM, true)), sm, s,     \
                         HEAD_LAUNCH_ARGS, a.advs, a.klb, a.ps_kle);                                                   \
    else if (a.advs)                                                                                                   \
      hipLaunchKernelGGL((HEAD_ADVN_KERNEL<T, AM, RT, VCLIP>), dim3(a.nblk), dim3(AM > 10 ? 256 : 512), sm, s,         \
                         HEAD_LAUNCH_ARGS, a.advs);                                                                    \
    else                                                                                                               \
      hipLaunchKernelGGL((HEAD_KERNEL<T, AM, RT, VCLIP>), dim3(a.nblk), dim3(AM > 10 ? 256 : 512), sm, s,              \
                         HEAD_LAUNCH_ARGS);                                                                            \
  } while (0)
  if (a.A <= 4)
    LAUNCH_HEAD(4);
  else if (a.A <= 6)
    LAUNCH_HEAD(6);
  else if (a.A <= 10)
    LAUNCH_HEAD(10);
  else
    LAUNCH_HEAD(18);
#undef LAUNCH_HEAD
#undef HEAD_LAUNCH_ARGS
}
void HEAD_LAUNCH(hipStream_t s, const HeadTrainArgs &a, HEAD_HP_T hp) {
#define HEAD_T(T, RT)                                                                                                  \
  do {                                                                                                                 \
    if (a.vold)                                                                                                        \
      head_train_t<T, RT, true>(s, a, hp);                                                                             \
    else                                                                                                               \
      head_train_t<T, RT, false>(s, a, hp);                                                                            \
  } while (0)
  if (a.prec == ALEPPO_BF16) {
    if (a.rt16)
      HEAD_T(bf16, f16);
    else
      HEAD_T(bf16, float);
  } else {
    if (a.rt16)
      HEAD_T(float, f16);
    else
      HEAD_T(float, float);
  }
#undef HEAD_T
}
