// feature_rank.hip - the kernels of aleppo_feature_rank (the definitions and the summation order are in aleppo.h): the
// Gram matrix G = Phi^T Phi and the column sums of the fc output h [ns][H] (fp32), in double, from the activation scratch
// in place.  Three launches per forward chunk, all of which only read h:
//   flags   one wave per row: flag[r] = 1 if every feature of row r is finite.
//   gram    grid (tiles + H / 64 column-sum blocks rounded up, S row splits).  A Gram workgroup owns one 64 x 64 block
//           (bi <= bj) of G over the rows of its split: four waves, each a 2 x 2 arrangement of 16 x 16 f64 accumulators
//           (32 x 32 of the block).  Both operands are the same matrix read along K, so there is no LDS and no transpose:
//           lane l loads h[k0 + (l >> 4)][i0 + (l & 15)] for A and h[k0 + (l >> 4)][j0 + (l & 15)] for B - 64-byte runs of
//           four consecutive rows -, widens with a convert and issues v_mfma_f64_16x16x4_f64 (A[i][k] in lane 16 k + i,
//           B[k][j] in lane 16 k + j, D[(l >> 4) + 4 reg][l & 15] in register reg of lane l).  Four K steps (16 rows) are
//           loaded while the 16 MFMAs of the four steps before them run.  A flagged-out row and a row past the split
//           enter as zeros and are not read.  A wave whose 32 columns do not exist (H % 64 == 32), or that lies below the
//           diagonal of a diagonal block, does nothing; its quarter of the partial block is never read either.
//           A column-sum workgroup takes 64 columns: thread (q, c) adds rows q, q + 4, ... of the split, then the four are
//           added in order from LDS.
//   reduce  element e of the result: the S partials in split order, then set (first chunk) or added to the result; the
//           rows left out are counted with integer atomics in LDS by workgroup 0.
// Doubles throughout, no floating-point atomics, a grid that is a function of (ns, H) only.
#include "common.hpp"
#include <algorithm>

namespace aleppo {

typedef double fr_d4 __attribute__((ext_vector_type(4)));

FeatureRankPlan feature_rank_plan(int H, long maxB) {
  FeatureRankPlan pl{};
  pl.H = H;
  pl.nb = (H + 63) / 64;
  pl.tiles = pl.nb * (pl.nb + 1) / 2;
  pl.result_doubles = (size_t)pl.tiles * 4096 + (size_t)H + 2;
  pl.bytes = pl.result_doubles * sizeof(double) * (1 + FR_MAX_SPLITS) + (size_t)maxB * sizeof(uint32_t);
  return pl;
}

__device__ __forceinline__ bool fr_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(256) void fr_flags_kernel(const float *__restrict__ h, int H, uint32_t ns,
                                                        uint32_t *__restrict__ flag) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= ns) // (the whole wave)
    return;
  bool bad = false;
  for (uint32_t c = lane; c < (uint32_t)H; c += 64u)
    bad |= !fr_finite(h[(size_t)row * H + c]);
  const bool any = __ballot(bad) != 0ull;
  if (lane == 0)
    flag[row] = any ? 0u : 1u;
}

struct FrPass {
  const float *h;       // [ns][H]
  const uint32_t *flag; // [ns]
  double *part;         // [S][result_doubles]
  size_t stride;        // result_doubles
  int H, nb, tiles;
  uint32_t ns, rps;     // rows of the chunk, rows per split
};

__global__ __launch_bounds__(256) void fr_gram_kernel(FrPass p) {
  __shared__ double cs[4][64];
  const uint32_t b = blockIdx.x, s = blockIdx.y;
  const uint32_t r0 = s * p.rps, rend = min(p.ns, r0 + p.rps);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = p.H;
  double *out = p.part + (size_t)s * p.stride;
  if (b < (uint32_t)p.tiles) {
    int bi = 0, rem = (int)b;
    while (rem >= p.nb - bi) {
      rem -= p.nb - bi;
      ++bi;
    }
    const int bj = bi + rem, wi = wave >> 1, wj = wave & 1;
    const int i0 = bi * 64 + wi * 32, j0 = bj * 64 + wj * 32;
    if (i0 >= H || j0 >= H || (bi == bj && wi > wj)) // (wave-uniform)
      return;
    const int kl = lane >> 4, cl = lane & 15;
    const float *ha = p.h + i0 + cl, *hb = p.h + j0 + cl;
    fr_d4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
        acc[x][y] = fr_d4{0.0, 0.0, 0.0, 0.0};
    // the sixteen loads of four K steps (16 rows); a row that does not enter is not read
    auto load16 = [&](uint32_t k0, float (&a)[4][2], float (&bb)[4][2]) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t row = k0 + 4u * u + (uint32_t)kl;
        const bool live = row < rend && p.flag[row] != 0u;
        const size_t at = (size_t)row * H;
        a[u][0] = live ? ha[at] : 0.f;
        a[u][1] = live ? ha[at + 16] : 0.f;
        bb[u][0] = live ? hb[at] : 0.f;
        bb[u][1] = live ? hb[at + 16] : 0.f;
      }
    };
    float a[4][2], bb[4][2];
    load16(r0, a, bb);
    for (uint32_t k0 = r0; k0 < rend; k0 += 16u) {
      float na[4][2], nb[4][2]; // the next 16 rows are in flight while these 16 MFMAs run (past the split: zeros, no read)
      load16(k0 + 16u, na, nb);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int y = 0; y < 2; ++y)
            acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[u][x], (double)bb[u][y], acc[x][y], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int x = 0; x < 2; ++x)
          a[u][x] = na[u][x], bb[u][x] = nb[u][x];
    }
    double *blk = out + (size_t)b * 4096;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int ii = wi * 32 + x * 16 + kl + 4 * reg, jj = wj * 32 + y * 16 + cl;
          blk[ii * 64 + jj] = acc[x][y][reg];
        }
    return;
  }
  // column sums: columns [64 cb, 64 cb + 64)
  const int col = (int)(b - (uint32_t)p.tiles) * 64 + lane;
  double sum = 0.0;
  if (col < H)
    for (uint32_t r = r0 + (uint32_t)wave; r < rend; r += 4u)
      if (p.flag[r] != 0u)
        sum += (double)p.h[(size_t)r * H + col];
  cs[wave][lane] = sum;
  __syncthreads();
  if (wave == 0 && col < H)
    out[(size_t)p.tiles * 4096 + col] = ((cs[0][lane] + cs[1][lane]) + cs[2][lane]) + cs[3][lane];
}

__global__ __launch_bounds__(256) void fr_reduce_kernel(const double *__restrict__ part, const uint32_t *__restrict__ flag,
                                                         double *__restrict__ result, size_t stride, size_t elements,
                                                         uint32_t splits, uint32_t ns, int first) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < elements) {
    double t = part[e];
    for (uint32_t s = 1; s < splits; ++s)
      t += part[(size_t)s * stride + e];
    result[e] = first ? t : result[e] + t;
  }
  if (blockIdx.x == 0) { // the rows this chunk leaves out (an integer count: any order)
    __shared__ unsigned int bad;
    if (threadIdx.x == 0)
      bad = 0u;
    __syncthreads();
    unsigned int mine = 0u;
    for (uint32_t r = threadIdx.x; r < ns; r += 256u)
      mine += flag[r] == 0u ? 1u : 0u;
    if (mine)
      atomicAdd(&bad, mine);
    __syncthreads();
    if (threadIdx.x == 0)
      result[elements] = (first ? 0.0 : result[elements]) + (double)bad;
  }
}

void launch_feature_rank_chunk(hipStream_t s, const float *h, long ns, bool first, const FeatureRankPlan &pl,
                               void *scratch) {
  double *result = static_cast<double *>(scratch);
  double *part = result + pl.result_doubles;
  uint32_t *flag = reinterpret_cast<uint32_t *>(part + pl.result_doubles * FR_MAX_SPLITS);
  const uint32_t splits = (uint32_t)std::min<long>(FR_MAX_SPLITS, (ns + FR_SPLIT_ROWS - 1) / FR_SPLIT_ROWS);
  const uint32_t rps = (uint32_t)(((ns + splits - 1) / splits + 3) / 4 * 4);
  hipLaunchKernelGGL(fr_flags_kernel, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, s, h, pl.H, (uint32_t)ns, flag);
  FrPass p{};
  p.h = h, p.flag = flag, p.part = part, p.stride = pl.result_doubles;
  p.H = pl.H, p.nb = pl.nb, p.tiles = pl.tiles, p.ns = (uint32_t)ns, p.rps = rps;
  hipLaunchKernelGGL(fr_gram_kernel, dim3((unsigned)(pl.tiles + pl.nb), splits), dim3(256), 0, s, p);
  const size_t elements = (size_t)pl.tiles * 4096 + (size_t)pl.H;
  hipLaunchKernelGGL(fr_reduce_kernel, dim3((unsigned)((elements + 255) / 256)), dim3(256), 0, s, part, flag, result,
                     pl.result_doubles, elements, splits, (uint32_t)ns, first ? 1 : 0);
}
} // namespace aleppo
