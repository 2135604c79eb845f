// refresh.hip - the kernel of aleppo_refresh_advantages (the definitions are in aleppo.h): the value head alone on the fc
// rows of one forward chunk, stored where the GAE scan reads its values.
//   value_refresh  one wave per row, four rows per 256-thread workgroup.  The wave sums h[r][:] * w_value[:] exactly as
//                  heads_fwd_kernel sums its value row - lane l takes l, l + 64, ... in turn, the xor butterfly of
//                  block_sum.hpp adds the 64 lanes, then + bias - so the fp32 value is aleppo_forward's bit for bit.  Lane 0
//                  rounds it to the rollout plane type and stores it time-major with an ordinary vector store: sample
//                  n = e*T + t of the batch goes to [t][e], the post-rollout observation of environment e to [T][e].
// No logits, no atomics, no LDS.
#include "block_sum.hpp"
#include "common.hpp"

namespace aleppo {

template <class RT>
__global__ __launch_bounds__(256) void value_refresh_kernel(const float *__restrict__ h, const float *__restrict__ wv,
                                                             const float *__restrict__ bv, RT *__restrict__ fresh_tm,
                                                             long n0, long ns, int H, int E, int T, int boot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long r = (long)blockIdx.x * 4 + wave;
  if (r >= ns) // (uniform over the wave)
    return;
  float s = 0.f;
  for (int j = lane; j < H; j += 64)
    s += h[(size_t)r * H + j] * wv[j];
  s = wave_sum(s);
  if (lane == 0) {
    const unsigned n = (unsigned)(n0 + r); // (n < E*T fits 32 bits: 32-bit division)
    const size_t i = boot ? (size_t)T * E + n : (size_t)(n % (unsigned)T) * E + n / (unsigned)T;
    fresh_tm[i] = (RT)(s + bv[0]);
  }
}

void launch_value_refresh(hipStream_t s, const float *h, const float *wv, const float *bv, void *fresh_tm, long n0,
                          long ns, int H, int E, int T, bool boot, bool rt16) {
  const dim3 grid((unsigned)((ns + 3) / 4));
  if (rt16)
    hipLaunchKernelGGL(value_refresh_kernel<_Float16>, grid, dim3(256), 0, s, h, wv, bv, static_cast<_Float16 *>(fresh_tm),
                       n0, ns, H, E, T, boot ? 1 : 0);
  else
    hipLaunchKernelGGL(value_refresh_kernel<float>, grid, dim3(256), 0, s, h, wv, bv, static_cast<float *>(fresh_tm), n0,
                       ns, H, E, T, boot ? 1 : 0);
}

} // namespace aleppo
