// saliency.hip - the kernels of aleppo_saliency and aleppo_saliency_perturbed (the definitions are in aleppo.h):
// perturbation saliency after Greydanus et al. 2018, in integer pixel arithmetic on the packed stacks.
//   blur     one workgroup per (sample, plane): the plane's 7056 bytes and the 32-bit horizontal intermediate live in LDS
//            (35 KB, four workgroups per CU) - a forward chunk of 4096 pairs touches about 15 samples, so one workgroup per
//            whole stack (141 KB, one per CU) would leave most of the chip idle; per plane it is four times as many, and a
//            plane that `planes` does not name returns at once.  1024 threads: with few workgroups the pass is bound by one
//            workgroup's LDS reads (7056 pixels x (2R + 1) taps, twice), not by the chip.  Horizontal pass, then vertical,
//            both with scipy's reflect rule; the byte goes into lane k of the packed blurred stack.
//   perturb  one workgroup per (sample, position) pair i of a chunk: reads the stack I and its blur B, writes the blend as a
//            packed stack of the staging buffer the forward pass then reads.  Store-bound (28 224 B per pair): a thread
//            handles four consecutive packed pixels of one row (84 = 21 * 4) with one 16-byte load of I, one of B and one
//            16-byte store; the two mask profiles of the pair (|y - cy|, |x - cx|) are looked up once per workgroup.
//   score    one thread per pair of a chunk: 0.5 * sum (z - z')^2 in fp32 in the order a = 0 .. A-1 (no contraction), the
//            value likewise, and - when asked for - the raw outputs.  No atomics; nothing depends on the grid.
// The blur and perturb grids are exactly the launch's counts; the score kernel's last workgroup checks its pair index.
#include "common.hpp"

namespace aleppo {

constexpr int SAL_W = 84, SAL_GROUPS = FRAME_PIX / 4; // 16-byte groups of four packed pixels per stack
static_assert(SAL_W % 4 == 0 && (FRAME_PIX * 4) % 16 == 0, "a group stays inside a row; every stack is 16-byte aligned");

__device__ __forceinline__ int sal_reflect(int i) { return i < 0 ? -1 - i : i > SAL_W - 1 ? 2 * SAL_W - 1 - i : i; }

// sample s0 + blockIdx.x, plane blockIdx.y -> byte lane blockIdx.y of blur[blockIdx.x]
constexpr int SAL_BLUR_THREADS = 1024;
__global__ __launch_bounds__(SAL_BLUR_THREADS) void sal_blur_kernel(const uint32_t *__restrict__ obs, SampleMap map, long s0,
                                                       SalTables tb, int planes, uint32_t *__restrict__ blur) {
  __shared__ uint8_t src[FRAME_PIX];
  __shared__ uint32_t hh[FRAME_PIX];
  __shared__ uint32_t w[SAL_W];
  const int k = blockIdx.y;
  if (!((planes >> k) & 1)) // (uniform over the workgroup)
    return;
  const uint32_t *in = obs + sample_off<false>(map, (long)map.n0 + s0 + (long)blockIdx.x);
  for (int i = threadIdx.x; i < FRAME_PIX; i += SAL_BLUR_THREADS)
    src[i] = (uint8_t)(in[i] >> (8 * k));
  if (threadIdx.x < SAL_W)
    w[threadIdx.x] = tb.w[threadIdx.x];
  __syncthreads();
  const int R = tb.radius;
  for (int i = threadIdx.x; i < FRAME_PIX; i += SAL_BLUR_THREADS) {
    const int y = i / SAL_W, x = i % SAL_W;
    uint32_t acc = 0;
    for (int j = -R; j <= R; ++j)
      acc += w[j < 0 ? -j : j] * (uint32_t)src[y * SAL_W + sal_reflect(x + j)];
    hh[i] = acc;
  }
  __syncthreads();
  uint8_t *out = reinterpret_cast<uint8_t *>(blur + (size_t)blockIdx.x * FRAME_PIX) + k;
  for (int i = threadIdx.x; i < FRAME_PIX; i += SAL_BLUR_THREADS) {
    const int y = i / SAL_W, x = i % SAL_W;
    uint32_t acc = 0;
    for (int j = -R; j <= R; ++j)
      acc += w[j < 0 ? -j : j] * hh[sal_reflect(y + j) * SAL_W + x];
    out[(size_t)i * 4] = (uint8_t)((acc + (1u << 23)) >> 24);
  }
}

// the four lanes of one packed pixel, each one `planes` names: (I * (256 - m) + B * m + 128) >> 8
__device__ __forceinline__ uint32_t sal_blend(uint32_t I, uint32_t B, uint32_t m, int planes) {
  uint32_t o = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t a = (I >> (8 * k)) & 255u, b = (B >> (8 * k)) & 255u;
    const uint32_t v = ((planes >> k) & 1) ? (a * (256u - m) + b * m + 128u) >> 8 : a;
    o |= v << (8 * k);
  }
  return o;
}

// pair j = j0 + blockIdx.x of the call: sample j / per, position p0 + j % per -> stage[blockIdx.x]
__global__ __launch_bounds__(256) void sal_perturb_kernel(const uint32_t *__restrict__ obs, SampleMap map,
                                                          const uint32_t *__restrict__ blur, long blur_s0, SalTables tb,
                                                          int planes, int stride, int G, long j0, int per, int p0,
                                                          uint32_t *__restrict__ stage) {
  __shared__ uint32_t gy[SAL_W], gx[SAL_W];
  const long j = j0 + (long)blockIdx.x, s = j / per;
  const int p = p0 + (int)(j % per), cy = (p / G) * stride, cx = (p % G) * stride;
  if (threadIdx.x < SAL_W) {
    const int t = threadIdx.x, dy = t > cy ? t - cy : cy - t, dx = t > cx ? t - cx : cx - t;
    gy[t] = tb.g[dy], gx[t] = tb.g[dx];
  }
  __syncthreads();
  const uint4 *I4 = reinterpret_cast<const uint4 *>(obs + sample_off<false>(map, (long)map.n0 + s));
  const uint4 *B4 = reinterpret_cast<const uint4 *>(blur + (size_t)(s - blur_s0) * FRAME_PIX);
  uint4 *O4 = reinterpret_cast<uint4 *>(stage + (size_t)blockIdx.x * FRAME_PIX);
  for (int q = threadIdx.x; q < SAL_GROUPS; q += 256) {
    const int y = q / (SAL_W / 4), x = (q % (SAL_W / 4)) * 4;
    const uint4 a = I4[q];
    const uint32_t my = gy[y];
    const uint32_t m0 = (my * gx[x] + 32768u) >> 16, m1 = (my * gx[x + 1] + 32768u) >> 16,
                   m2 = (my * gx[x + 2] + 32768u) >> 16, m3 = (my * gx[x + 3] + 32768u) >> 16;
    uint4 o = a;
    if (m0 | m1 | m2 | m3) { // (where every mask is 0 the pixels are unchanged and B is not read)
      const uint4 b = B4[q];
      o.x = sal_blend(a.x, b.x, m0, planes), o.y = sal_blend(a.y, b.y, m1, planes);
      o.z = sal_blend(a.z, b.z, m2, planes), o.w = sal_blend(a.w, b.w, m3, planes);
    }
    O4[q] = o;
  }
}

// pair i = i0 + thread of the call (sample i / P, position i % P); row `thread` of logits / values is its forward pass
__global__ __launch_bounds__(256) void sal_score_kernel(const float *__restrict__ base_logits,
                                                        const float *__restrict__ base_values,
                                                        const float *__restrict__ logits, const float *__restrict__ values,
                                                        long i0, long ns, int P, int A, float *__restrict__ policy,
                                                        float *__restrict__ value, float *__restrict__ outputs) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= ns)
    return;
  const long i = i0 + q, s = i / P;
  const int p = (int)(i % P);
  const float *z = base_logits + s * A, *zp = logits + q * A;
  float *row = outputs ? outputs + ((size_t)s * (P + 1) + 1 + p) * (A + 1) : nullptr;
  float *row0 = outputs && p == 0 ? outputs + (size_t)s * (P + 1) * (A + 1) : nullptr; // (each sample has one p == 0)
  float acc = 0.f;
  for (int a = 0; a < A; ++a) {
    const float d = __fsub_rn(z[a], zp[a]);
    acc = __fadd_rn(acc, __fmul_rn(d, d));
    if (row)
      row[a] = zp[a];
    if (row0)
      row0[a] = z[a];
  }
  const float v = base_values[s], vp = values[q], dv = __fsub_rn(v, vp);
  policy[i] = 0.5f * acc;
  value[i] = 0.5f * __fmul_rn(dv, dv);
  if (row)
    row[A] = vp;
  if (row0)
    row0[A] = v;
}

void launch_sal_blur(hipStream_t s, const uint32_t *obs, SampleMap map, long s0, long count, const SalTables &tb,
                     int planes, uint32_t *blur) {
  hipLaunchKernelGGL(sal_blur_kernel, dim3((unsigned)count, 4), dim3(SAL_BLUR_THREADS), 0, s, obs, map, s0, tb, planes, blur);
}
void launch_sal_perturb(hipStream_t s, const uint32_t *obs, SampleMap map, const uint32_t *blur, long blur_s0,
                        const SalTables &tb, int planes, int stride, int G, long j0, long ns, int per, int p0,
                        uint32_t *stage) {
  hipLaunchKernelGGL(sal_perturb_kernel, dim3((unsigned)ns), dim3(256), 0, s, obs, map, blur, blur_s0, tb, planes, stride,
                     G, j0, per, p0, stage);
}
void launch_sal_score(hipStream_t s, const float *base_logits, const float *base_values, const float *logits,
                      const float *values, long i0, long ns, int P, int A, float *policy, float *value, float *outputs) {
  hipLaunchKernelGGL(sal_score_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, s, base_logits, base_values,
                     logits, values, i0, ns, P, A, policy, value, outputs);
}
} // namespace aleppo
