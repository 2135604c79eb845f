// head_train.hpp - what head_train.hip (the PPO head training kernel's entry points; their body is head_train_body.inc)
// shares with kernels.hip: the rollout-plane type and the kernel's waves per workgroup.
#pragma once
#include "block_sum.hpp" // wave_sum
#include "common.hpp"
#include "gemm.hpp" // bf16 / vector typedefs

namespace aleppo {

// Rollout-plane storage type RT: float (the reference's Buffer, buffer.cc:12-38) or IEEE half (BASELINE configs[4],
// "fp16 rollout buffer").  Arithmetic is always fp32: planes are widened on load and rounded (RNE) on store.
typedef _Float16 f16;

// Waves per workgroup of the head training kernel (head_train.hip, "PPO head, training")
constexpr int head_waves(int amax, bool klpen) { return amax > 10 || (klpen && amax > 6) ? 4 : 8; }
// The parameters the three entry points share.  hp: the device block of common.hpp's HYPER_* slots
#define HEAD_PARAMS                                                                                                    \
  const float *__restrict__ h, const float *__restrict__ Wh, const float *__restrict__ bh, const int *__restrict__ act, \
      const RT *__restrict__ oldlp, const RT *__restrict__ adv, const RT *__restrict__ ret,                            \
      const RT *__restrict__ vold, const uint8_t *__restrict__ mask, const float *__restrict__ mask_count,             \
      const float *__restrict__ hp, T *dh, float *ps_total, float *ps_clipped, float *ps_value, float *ps_entropy,     \
      float *ps_ratio, float *ps_kl, float *ps_cf, float *slab_w, float *slab_b, long B, int H, int A,                 \
      float *logits_out, float *values_out, int hparts

} // namespace aleppo
