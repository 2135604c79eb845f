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

// h arrives as `hparts` split-K partial slabs [hparts][B][H] (slab 0 carries the bias).  Lane l owns hidden units
// 4l .. 4l+3 and H/2 + 4l .. H/2 + 4l+3 of row r (H % 8 == 0; call only where lane * 8 < H): their slabs are added onto acc
// one after the other, in slab order.  The head training kernel's fetch and aleppo_export_backward's h (h_export_kernel)
// share these additions.
__device__ __forceinline__ void add_h_slabs(const float *h, int hparts, long B, long r, int H, int lane,
                                            float (&acc)[8]) {
  for (int p = 0; p < hparts; ++p) {
    const float *src = h + ((size_t)p * B + r) * H + lane * 4;
    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(src), v1 = *reinterpret_cast<const f32x4 *>(src + H / 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i] += v0[i];
      acc[4 + i] += v1[i];
    }
  }
}

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
