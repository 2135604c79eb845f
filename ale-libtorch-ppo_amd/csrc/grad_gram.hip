// grad_gram.hip - aleppo_grad_gram and aleppo_grad_take's difference (the definitions are in aleppo.h): the Gram of up to
// four gradient slots per exported tensor, from the private padded layout in place.  Built like tensor_stats.hip, whose
// chunk grid (TsLayout) it shares: chunks of TS_CHUNK floats PER INTERNAL TENSOR, one 256-thread workgroup per chunk, every
// thread four 16-byte loads per vector, all K x 4 of them issued before the first use.  Every thread keeps the K (K + 1) / 2
// products of the upper triangle in double for EACH side of the tensor's split (the stacked heads: action rows, then the
// value row; the attribution is per element, a 16-byte group of P_BH straddles the two whenever A % 4 != 0), the threads
// are folded by a fixed wave tree and every chunk writes one partial record per side.  Stage 2 is one workgroup: per
// exported tensor the partials are added in chunk order (from LDS tiles), row 12 is the twelve rows added in row order,
// and [i][j] and [j][i] are written from the same sum.
// A product of two widened fp32 values is exact in double (24 + 24 <= 53 bits), so an fma and a multiply-add give the same
// bits and the only rounding is the double additions, in an order that is a function of (H, A, K) only: no atomics, no
// device-dependent grid.  K is a template parameter: at K = 4 a thread holds 16 loaded 16-byte groups and 20 double
// accumulators (about 120 registers: four waves per SIMD, which a pass that only streams memory needs no more than), and
// the instantiations for K = 1 and 2 do not pay for them.
#include "common.hpp"

namespace aleppo {

constexpr int GG_SUMS = ALEPPO_GRAD_SLOTS * (ALEPPO_GRAD_SLOTS + 1) / 2; // upper-triangle entries at K = 4
struct GgRecord {     // what one chunk contributes to one exported tensor
  double s[GG_SUMS];  // entry gg_idx(K, i, j), i <= j; the entries K (K + 1) / 2 .. are written as 0
  uint32_t nf;        // element indices at which any of the K vectors is non-finite
  uint32_t pad[3];
};
static_assert(sizeof(GgRecord) == 96, "GgRecord layout"); // (whole 16-byte words: the reduction copies them as such)

// position of (i, j), i <= j < K, in the packed upper triangle
__host__ __device__ constexpr int gg_idx(int K, int i, int j) { return i * K - i * (i - 1) / 2 + (j - i); }

struct GgSlots {
  const float4 *v[ALEPPO_GRAD_SLOTS]; // the K vectors (entries K .. repeat the first)
};

size_t grad_gram_scratch_bytes(const ParamLayout &L) {
  return (size_t)ts_layout(L).first[P_COUNT] * 2 * sizeof(GgRecord) +
         (size_t)ALEPPO_TENSOR_STATS_ROWS * (ALEPPO_GRAD_SLOTS * ALEPPO_GRAD_SLOTS + 1) * sizeof(double);
}

template <int K>
__global__ __launch_bounds__(256) void grad_gram_partial_kernel(GgSlots X, TsLayout L, GgRecord *__restrict__ part) {
  constexpr int NP = K * (K + 1) / 2;
  __shared__ double s_sum[4][2][NP];
  __shared__ uint32_t s_nf[4][2];
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
  const uint32_t g_base = off / 4u, g0 = (blockIdx.x - first) * (uint32_t)(TS_CHUNK / 4) + threadIdx.x;
  // all loads first; a group past the tensor's end reads the tensor's group 0 instead (in bounds) and is not used
  float4 x[K][4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const uint32_t gi = g0 + it * 256u;
    const uint32_t src = g_base + (gi * 4u < size ? gi : 0u);
#pragma unroll
    for (int v = 0; v < K; ++v)
      x[v][it] = X.v[v][src];
  }
  double acc[2][NP];
#pragma unroll
  for (int q = 0; q < NP; ++q)
    acc[0][q] = acc[1][q] = 0.0;
  uint32_t nf[2] = {0u, 0u};
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const uint32_t j0 = (g0 + it * 256u) * 4u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t j = j0 + e;
      if (j >= size) // past the tensor: an alignment pad (or a group that was not loaded) is not an element
        continue;
      const bool hi = j >= split;
      float xe[K];
      bool ok = true;
#pragma unroll
      for (int v = 0; v < K; ++v) {
        xe[v] = e == 0 ? x[v][it].x : e == 1 ? x[v][it].y : e == 2 ? x[v][it].z : x[v][it].w;
        ok = ok && ts_finite(xe[v]);
      }
      nf[0] += (!ok && !hi) ? 1u : 0u;
      nf[1] += (!ok && hi) ? 1u : 0u;
      double d[K];
#pragma unroll
      for (int v = 0; v < K; ++v) // an index that is left out contributes exact zeros: every entry keeps its own order
        d[v] = ok ? (double)xe[v] : 0.0;
#pragma unroll
      for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = a; b < K; ++b) {
          const double pr = d[a] * d[b];
          acc[0][gg_idx(K, a, b)] += hi ? 0.0 : pr;
          acc[1][gg_idx(K, a, b)] += hi ? pr : 0.0;
        }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const double a = ts_wave_sum(acc[h][q]);
      if (lane == 0)
        s_sum[wave][h][q] = a;
    }
    uint32_t c = nf[h];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
      c += __shfl_down(c, o, 64);
    if (lane == 0)
      s_nf[wave][h] = c;
  }
  __syncthreads();
  if (threadIdx.x < 2) { // the four waves in order
    const int h = threadIdx.x;
    GgRecord r;
#pragma unroll
    for (int q = 0; q < GG_SUMS; ++q)
      r.s[q] = 0.0;
#pragma unroll
    for (int q = 0; q < NP; ++q)
      r.s[q] = ((s_sum[0][h][q] + s_sum[1][h][q]) + s_sum[2][h][q]) + s_sum[3][h][q];
    r.nf = s_nf[0][h] + s_nf[1][h] + s_nf[2][h] + s_nf[3][h];
    r.pad[0] = r.pad[1] = r.pad[2] = 0u;
    part[(size_t)blockIdx.x * 2 + h] = r;
  }
}

// one workgroup: the partial records pass through LDS in tiles of GG_TILE chunks (whole 16-byte words, every thread
// copying), and thread (row, entry) adds its row's partials from there in chunk order; then one thread per output element.
// out: double [13][K][K], then int64 [13]
constexpr int GG_TILE = 128;           // chunks per tile: 256 records, 24 KB
constexpr int GG_ENTRIES = GG_SUMS + 1; // the sums, then the count
__global__ __launch_bounds__(256) void grad_gram_reduce_kernel(const GgRecord *__restrict__ part, TsLayout L, int K,
                                                                double *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) GgRecord tile[GG_TILE * 2];
  __shared__ double r_sum[12][GG_SUMS];
  __shared__ unsigned long long r_nf[12];
  const int t = threadIdx.x;
  const bool adds = t < 12 * GG_ENTRIES;
  const int r = adds ? t / GG_ENTRIES : 0, f = t % GG_ENTRIES;
  const TsRow row = ts_row(r);
  const uint32_t c0 = L.first[row.tensor], c1 = L.first[row.tensor + 1], chunks = L.first[P_COUNT];
  double ad = 0.0;
  unsigned long long au = 0ull;
  for (uint32_t base = 0; base < chunks; base += GG_TILE) {
    const uint32_t n = min((uint32_t)GG_TILE, chunks - base);
    const uint4 *src = reinterpret_cast<const uint4 *>(part + (size_t)base * 2);
    uint4 *dst = reinterpret_cast<uint4 *>(tile);
    for (uint32_t i = t; i < n * 2u * (uint32_t)(sizeof(GgRecord) / 16); i += 256u)
      dst[i] = src[i];
    __syncthreads();
    if (adds) {
      const uint32_t lo = max(c0, base), hi = min(c1, base + n);
      for (uint32_t c = lo; c < hi; ++c) {
        const GgRecord &q = tile[(c - base) * 2u + row.half];
        if (f < GG_SUMS)
          ad += q.s[f];
        else
          au += q.nf;
      }
    }
    __syncthreads();
  }
  if (adds) {
    if (f < GG_SUMS)
      r_sum[r][f] = ad;
    else
      r_nf[r] = au;
  }
  __syncthreads();
  const int rows = ALEPPO_TENSOR_STATS_ROWS;
  if (t < rows * ALEPPO_GRAD_SLOTS * ALEPPO_GRAD_SLOTS) {
    const int o = t / (ALEPPO_GRAD_SLOTS * ALEPPO_GRAD_SLOTS), i = (t / ALEPPO_GRAD_SLOTS) % ALEPPO_GRAD_SLOTS,
              j = t % ALEPPO_GRAD_SLOTS;
    if (i < K && j < K) {
      const int q = gg_idx(K, min(i, j), max(i, j)); // [i][j] and [j][i]: the same sum
      double v = 0.0;
      if (o < 12)
        v = r_sum[o][q];
      else // the whole model: the twelve rows in row order
        for (int rr = 0; rr < 12; ++rr)
          v += r_sum[rr][q];
      out[((size_t)o * K + i) * K + j] = v;
    }
  }
  if (t < rows) {
    unsigned long long v = 0ull;
    if (t < 12)
      v = r_nf[t];
    else
      for (int rr = 0; rr < 12; ++rr)
        v += r_nf[rr];
    reinterpret_cast<long long *>(out + (size_t)rows * K * K)[t] = (long long)v;
  }
}

void launch_grad_gram(hipStream_t s, const float *const *vec, int K, const ParamLayout &L, void *scratch,
                      const double **out_dev) {
  const TsLayout tl = ts_layout(L);
  const uint32_t chunks = tl.first[P_COUNT];
  GgRecord *part = static_cast<GgRecord *>(scratch);
  double *out = reinterpret_cast<double *>(part + (size_t)chunks * 2);
  GgSlots X;
  for (int v = 0; v < ALEPPO_GRAD_SLOTS; ++v)
    X.v[v] = reinterpret_cast<const float4 *>(vec[v < K ? v : 0]);
  switch (K) {
  case 1:
    hipLaunchKernelGGL(grad_gram_partial_kernel<1>, dim3(chunks), dim3(256), 0, s, X, tl, part);
    break;
  case 2:
    hipLaunchKernelGGL(grad_gram_partial_kernel<2>, dim3(chunks), dim3(256), 0, s, X, tl, part);
    break;
  case 3:
    hipLaunchKernelGGL(grad_gram_partial_kernel<3>, dim3(chunks), dim3(256), 0, s, X, tl, part);
    break;
  default:
    hipLaunchKernelGGL(grad_gram_partial_kernel<4>, dim3(chunks), dim3(256), 0, s, X, tl, part);
    break;
  }
  hipLaunchKernelGGL(grad_gram_reduce_kernel, dim3(1), dim3(256), 0, s, part, tl, K, out);
  *out_dev = out;
}

// aleppo_grad_take, ALEPPO_GRAD_SRC_PARAM_DELTA: out[i] = a[i] - b[i], one fp32 subtraction per element of the padded
// vector (n floats, a multiple of 4; a pad gives 0 - 0)
__global__ __launch_bounds__(256) void grad_delta_kernel(const float4 *__restrict__ a, const float4 *__restrict__ b,
                                                          float4 *__restrict__ out, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4)
    return;
  const float4 p = a[i], q = b[i];
  out[i] = make_float4(p.x - q.x, p.y - q.y, p.z - q.z, p.w - q.w);
}
void launch_grad_delta(hipStream_t s, const float *a, const float *b, float *out, long n) {
  const long n4 = n / 4;
  hipLaunchKernelGGL(grad_delta_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const float4 *>(a), reinterpret_cast<const float4 *>(b),
                     reinterpret_cast<float4 *>(out), n4);
}
} // namespace aleppo
