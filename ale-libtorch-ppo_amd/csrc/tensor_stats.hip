// tensor_stats.hip - aleppo_tensor_stats (the definition is in aleppo.h): per-tensor norms, maxima and non-finite counts of
// the parameters, the last minibatch's clipped gradient and the last optimizer step, from the private padded layout in
// place.  One bandwidth-bound pass that only reads: the flat vectors are cut into chunks of TS_CHUNK floats PER INTERNAL
// TENSOR (tensors start 64-float aligned, so a chunk never holds two), one workgroup per chunk, every thread four 16-byte
// loads per vector, all issued before the first use.  The exported order differs from the internal one only inside a
// tensor (norms and maxima do not care) and in the two stacked heads: P_WH is [A + 1][H] and P_BH is [A + 1], action rows
// then the value row, so every chunk writes TWO partial records - the elements below the tensor's split and those from it
// on - and the attribution is per element (a 16-byte group of P_BH straddles action.b and value.b whenever A % 4 != 0).
// Stage 2 is one small launch: per exported tensor the partials are added in chunk order (from LDS), then row 12 and the
// ratios.
// Sums are doubles of exact squares; the order is a function of (H, A) only: no atomics, no device-dependent grid.
#include "common.hpp"
#include <algorithm>

namespace aleppo {

constexpr int TS_GROUPS = TS_CHUNK / 4; // 16-byte groups per chunk: 4 per thread
static_assert(TS_GROUPS == 4 * 256, "a chunk is four groups per thread of a 256-thread workgroup");

struct TsRecord { // what one chunk contributes to one exported tensor
  double sq_p, sq_g, sq_u;      // sums of squares over the finite elements of the column group
  float max_p, max_g, max_u;    // maxima of |.| over the same elements
  uint32_t nf_p, nf_s;          // non-finite p; elements whose g, m, v or u is non-finite
  uint32_t pad;
};
static_assert(sizeof(TsRecord) == 48, "TsRecord layout"); // (whole 16-byte words: the reduction copies them as such)

TsLayout ts_layout(const ParamLayout &L) {
  TsLayout t{};
  uint32_t chunks = 0;
  for (int k = 0; k < P_COUNT; ++k) {
    t.off[k] = (uint32_t)L.off[k];
    t.size[k] = t.split[k] = (uint32_t)L.size[k];
    t.first[k] = chunks;
    chunks += (uint32_t)((L.size[k] + TS_CHUNK - 1) / TS_CHUNK);
  }
  t.first[P_COUNT] = chunks;
  t.split[P_WH] = (uint32_t)L.A * (uint32_t)L.H;
  t.split[P_BH] = (uint32_t)L.A;
  return t;
}
size_t tensor_stats_scratch_bytes(const ParamLayout &L) {
  return (size_t)ts_layout(L).first[P_COUNT] * 2 * sizeof(TsRecord) +
         (size_t)ALEPPO_TENSOR_STATS_ROWS * ALEPPO_TENSOR_STATS_COLS * sizeof(double);
}

__device__ __forceinline__ float ts_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v = fmaxf(v, __shfl_down(v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t ts_wave_add(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_down(v, o, 64);
  return v;
}

// STEP = false (ALEPPO_TS_SEC_PARAMS alone): only P is read, the step fields of the records are 0
template <bool STEP>
__global__ __launch_bounds__(256) void tensor_stats_partial_kernel(const float4 *__restrict__ P, const float4 *__restrict__ G,
                                                                    const float4 *__restrict__ M1,
                                                                    const float4 *__restrict__ M2, TsLayout L, float coef,
                                                                    float step_size, float bc2_sqrt, float eps,
                                                                    TsRecord *__restrict__ part) {
  __shared__ double s_sq[4][2][3];
  __shared__ float s_mx[4][2][3];
  __shared__ uint32_t s_nf[4][2][2];
  int k = 0;
#pragma unroll
  for (int q = 1; q < P_COUNT; ++q) // (selects on constant indices: the argument stays in scalar registers)
    if (blockIdx.x >= L.first[q])
      k = q;
  uint32_t off = L.off[0], size = L.size[0], split = L.split[0], first = L.first[0];
#pragma unroll
  for (int q = 1; q < P_COUNT; ++q)
    if (k == q)
      off = L.off[q], size = L.size[q], split = L.split[q], first = L.first[q];
  const uint32_t g_base = off / 4u, g0 = (blockIdx.x - first) * (uint32_t)TS_GROUPS + threadIdx.x;
  // all loads first; a group past the tensor's end reads the tensor's group 0 instead (in bounds) and is not used
  float4 p[4], g[4], m[4], v[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const uint32_t gi = g0 + it * 256u;
    const uint32_t src = g_base + (gi * 4u < size ? gi : 0u);
    p[it] = P[src];
    if constexpr (STEP) {
      g[it] = G[src];
      m[it] = M1[src];
      v[it] = M2[src];
    }
  }
  double sq[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  float mx[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  uint32_t nf[2][2] = {{0u, 0u}, {0u, 0u}};
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const uint32_t j0 = (g0 + it * 256u) * 4u;
    const float pe[4] = {p[it].x, p[it].y, p[it].z, p[it].w};
    float ge[4] = {0.f, 0.f, 0.f, 0.f}, me[4] = {0.f, 0.f, 0.f, 0.f}, ve[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (STEP) {
      ge[0] = g[it].x, ge[1] = g[it].y, ge[2] = g[it].z, ge[3] = g[it].w;
      me[0] = m[it].x, me[1] = m[it].y, me[2] = m[it].z, me[3] = m[it].w;
      ve[0] = v[it].x, ve[1] = v[it].y, ve[2] = v[it].z, ve[3] = v[it].w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t j = j0 + e;
      if (j >= size) // past the tensor: an alignment pad (or a group that was not loaded) is not an element
        continue;
      const bool hi = j >= split;
      // (an added 0.0 leaves a non-negative sum as it is: both sides of the split keep their own order)
      {
        const float x = pe[e];
        const bool ok = ts_finite(x);
        const double d = ok ? (double)x : 0.0, d2 = d * d;
        const float a = ok ? fabsf(x) : 0.f;
        sq[0][0] += hi ? 0.0 : d2;
        sq[1][0] += hi ? d2 : 0.0;
        mx[0][0] = fmaxf(mx[0][0], hi ? 0.f : a);
        mx[1][0] = fmaxf(mx[1][0], hi ? a : 0.f);
        nf[0][0] += (!ok && !hi) ? 1u : 0u;
        nf[1][0] += (!ok && hi) ? 1u : 0u;
      }
      if constexpr (STEP) {
        const float gs = ge[e] * coef;                        // aleppo_export_grads' element
        const float denom = sqrtf(ve[e]) / bc2_sqrt + eps;    // adam_element's expression on the stored moments
        const float u = step_size * (me[e] / denom);
        const bool ok = ts_finite(gs) && ts_finite(me[e]) && ts_finite(ve[e]) && ts_finite(u);
        const double dg = ok ? (double)gs : 0.0, du = ok ? (double)u : 0.0, dg2 = dg * dg, du2 = du * du;
        const float ag = ok ? fabsf(gs) : 0.f, au = ok ? fabsf(u) : 0.f;
        sq[0][1] += hi ? 0.0 : dg2;
        sq[1][1] += hi ? dg2 : 0.0;
        sq[0][2] += hi ? 0.0 : du2;
        sq[1][2] += hi ? du2 : 0.0;
        mx[0][1] = fmaxf(mx[0][1], hi ? 0.f : ag);
        mx[1][1] = fmaxf(mx[1][1], hi ? ag : 0.f);
        mx[0][2] = fmaxf(mx[0][2], hi ? 0.f : au);
        mx[1][2] = fmaxf(mx[1][2], hi ? au : 0.f);
        nf[0][1] += (!ok && !hi) ? 1u : 0u;
        nf[1][1] += (!ok && hi) ? 1u : 0u;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const double a = ts_wave_sum(sq[h][f]);
      const float b = ts_wave_max(mx[h][f]);
      if (lane == 0) {
        s_sq[wave][h][f] = a;
        s_mx[wave][h][f] = b;
      }
    }
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const uint32_t a = ts_wave_add(nf[h][f]);
      if (lane == 0)
        s_nf[wave][h][f] = a;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2) { // the four waves in order
    const int h = threadIdx.x;
    TsRecord r;
    r.sq_p = ((s_sq[0][h][0] + s_sq[1][h][0]) + s_sq[2][h][0]) + s_sq[3][h][0];
    r.sq_g = ((s_sq[0][h][1] + s_sq[1][h][1]) + s_sq[2][h][1]) + s_sq[3][h][1];
    r.sq_u = ((s_sq[0][h][2] + s_sq[1][h][2]) + s_sq[2][h][2]) + s_sq[3][h][2];
    r.max_p = fmaxf(fmaxf(s_mx[0][h][0], s_mx[1][h][0]), fmaxf(s_mx[2][h][0], s_mx[3][h][0]));
    r.max_g = fmaxf(fmaxf(s_mx[0][h][1], s_mx[1][h][1]), fmaxf(s_mx[2][h][1], s_mx[3][h][1]));
    r.max_u = fmaxf(fmaxf(s_mx[0][h][2], s_mx[1][h][2]), fmaxf(s_mx[2][h][2], s_mx[3][h][2]));
    r.nf_p = s_nf[0][h][0] + s_nf[1][h][0] + s_nf[2][h][0] + s_nf[3][h][0];
    r.nf_s = s_nf[0][h][1] + s_nf[1][h][1] + s_nf[2][h][1] + s_nf[3][h][1];
    r.pad = 0u;
    part[(size_t)blockIdx.x * 2 + h] = r;
  }
}

// one workgroup: the partial records pass through LDS in tiles of TS_TILE chunks (whole 16-byte words, every thread
// copying), and thread (row, field) adds its row's partials from there in chunk order - a loop over records in global memory
// paid one dependent memory latency per chunk, 392 of them for fc.w at H = 512; then one thread per output row
constexpr int TS_TILE = 256; // chunks per tile: 512 records, 24 KB
__global__ __launch_bounds__(256) void tensor_stats_reduce_kernel(const TsRecord *__restrict__ part, TsLayout L, int sections,
                                                                   double *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) TsRecord tile[TS_TILE * 2];
  __shared__ double r_sq[12][3];
  __shared__ float r_mx[12][3];
  __shared__ uint32_t r_nf[12][2];
  __shared__ uint32_t r_size[12];
  const int t = threadIdx.x;
  const int r = t >> 3, f = t & 7; // (t < 96)
  const TsRow row = ts_row(t < 96 ? r : 0);
  const uint32_t c0 = L.first[row.tensor], c1 = L.first[row.tensor + 1], chunks = L.first[P_COUNT];
  double ad = 0.0;
  float af = 0.f;
  uint32_t au = 0u;
  for (uint32_t base = 0; base < chunks; base += TS_TILE) {
    const uint32_t n = min((uint32_t)TS_TILE, chunks - base);
    const uint4 *src = reinterpret_cast<const uint4 *>(part + (size_t)base * 2);
    uint4 *dst = reinterpret_cast<uint4 *>(tile);
    for (uint32_t i = t; i < n * 2u * (uint32_t)(sizeof(TsRecord) / 16); i += 256u)
      dst[i] = src[i];
    __syncthreads();
    if (t < 96) {
      const uint32_t lo = max(c0, base), hi = min(c1, base + n);
      for (uint32_t c = lo; c < hi; ++c) {
        const TsRecord &q = tile[(c - base) * 2u + row.half];
        if (f < 3)
          ad += f == 0 ? q.sq_p : f == 1 ? q.sq_g : q.sq_u;
        else if (f < 6)
          af = fmaxf(af, f == 3 ? q.max_p : f == 4 ? q.max_g : q.max_u);
        else
          au += f == 6 ? q.nf_p : q.nf_s;
      }
    }
    __syncthreads();
  }
  if (t < 96) {
    if (f < 3)
      r_sq[r][f] = ad;
    else if (f < 6)
      r_mx[r][f - 3] = af;
    else
      r_nf[r][f - 6] = au;
    if (f == 6) {
      const uint32_t size = L.size[row.tensor], split = L.split[row.tensor];
      r_size[r] = row.half ? size - split : split;
    }
  }
  __syncthreads();
  if (t >= ALEPPO_TENSOR_STATS_ROWS)
    return;
  double sq[3] = {0.0, 0.0, 0.0}, size = 0.0, nfp = 0.0, nfs = 0.0;
  float mx[3] = {0.f, 0.f, 0.f};
  if (t < 12) {
    for (int f = 0; f < 3; ++f)
      sq[f] = r_sq[t][f], mx[f] = r_mx[t][f];
    size = (double)r_size[t], nfp = (double)r_nf[t][0], nfs = (double)r_nf[t][1];
  } else { // the whole model: the twelve rows in row order
    uint32_t n = 0u, a = 0u, b = 0u;
    for (int r = 0; r < 12; ++r) {
      for (int f = 0; f < 3; ++f)
        sq[f] += r_sq[r][f], mx[f] = fmaxf(mx[f], r_mx[r][f]);
      n += r_size[r], a += r_nf[r][0], b += r_nf[r][1];
    }
    size = (double)n, nfp = (double)a, nfs = (double)b;
  }
  const bool params = (sections & ALEPPO_TS_SEC_PARAMS) != 0, step = (sections & ALEPPO_TS_SEC_STEP) != 0;
  const double pn = sqrt(sq[0]), gn = sqrt(sq[1]), un = sqrt(sq[2]);
  double *o = out + t * ALEPPO_TENSOR_STATS_COLS;
  o[ALEPPO_TS_SIZE] = size;
  o[ALEPPO_TS_PARAM_NORM] = params ? pn : 0.0;
  o[ALEPPO_TS_PARAM_MAXABS] = params ? (double)mx[0] : 0.0;
  o[ALEPPO_TS_PARAM_NONFINITE] = params ? nfp : 0.0;
  o[ALEPPO_TS_GRAD_NORM] = step ? gn : 0.0;
  o[ALEPPO_TS_GRAD_MAXABS] = step ? (double)mx[1] : 0.0;
  o[ALEPPO_TS_UPDATE_NORM] = step ? un : 0.0;
  o[ALEPPO_TS_UPDATE_MAXABS] = step ? (double)mx[2] : 0.0;
  o[ALEPPO_TS_UPDATE_RATIO] = step ? un / pn : 0.0;
  o[ALEPPO_TS_STEP_NONFINITE] = step ? nfs : 0.0;
}

void launch_tensor_stats(hipStream_t s, const float *P, const float *G, const float *M1, const float *M2,
                         const ParamLayout &L, int sections, float coef, float step_size, float bc2_sqrt, float eps,
                         void *scratch, const double **out_dev) {
  const TsLayout tl = ts_layout(L);
  const uint32_t chunks = tl.first[P_COUNT];
  TsRecord *part = static_cast<TsRecord *>(scratch);
  double *out = reinterpret_cast<double *>(part + (size_t)chunks * 2);
  if (sections & ALEPPO_TS_SEC_STEP)
    hipLaunchKernelGGL(tensor_stats_partial_kernel<true>, dim3(chunks), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(P), reinterpret_cast<const float4 *>(G),
                       reinterpret_cast<const float4 *>(M1), reinterpret_cast<const float4 *>(M2), tl, coef, step_size,
                       bc2_sqrt, eps, part);
  else
    hipLaunchKernelGGL(tensor_stats_partial_kernel<false>, dim3(chunks), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(P), static_cast<const float4 *>(nullptr),
                       static_cast<const float4 *>(nullptr), static_cast<const float4 *>(nullptr), tl, 1.0f, 0.0f, 1.0f,
                       0.0f, part);
  hipLaunchKernelGGL(tensor_stats_reduce_kernel, dim3(1), dim3(256), 0, s, part, tl, sections, out);
  *out_dev = out;
}
} // namespace aleppo
