// activation_stats.hip - the kernels of aleppo_forward_activations and aleppo_activation_stats (the definitions are in
// aleppo.h): what the four hidden layers emit, from the private NHWC layout in place.
//   export   [n][PIX][C] of T -> float [n][C][PIX] (the reference's tensor order): one workgroup per sample, 16-byte loads of
//            one pixel's channel group, the transpose through LDS, 16-byte stores of the sample's contiguous output.
//   partial  one bandwidth-bound pass that only reads.  A layer is a matrix [rows][C] (rows = samples * PIX; fc: rows =
//            samples, C = H, always float); a 16-byte load is one channel group of one row (8 bf16 / 4 fp32 channels).  A
//            workgroup takes a chunk of AS_GROUPS 16-byte groups of whole rows: thread t owns channel group t % CG and the rows
//            t / CG, t / CG + RL, ... of the chunk (CG groups per row, RL = 256 / CG), so the 256 loads of one step are 4 KB
//            of consecutive addresses and a thread's accumulators never change channel.  fc (CG = H / 4 is not a power of
//            two) is tiled instead: 64 channel groups by 4 rows, AS_FC_ROWS rows per workgroup.  The threads of a channel
//            group are folded by a fixed tree (wave shuffles, then the four waves in order from LDS); one record per
//            (workgroup, channel).  One launch covers the four layers: the grid is a function of the shapes only.
//   final    one workgroup: thread u adds unit u's records in chunk order, then one thread per layer adds the units in unit
//            order, forms the scores and the two tables.
// Sums are doubles of exactly widened |a|: no atomics, no device-dependent grid.  Rows of samples >= n are never read.
#include "common.hpp"
#include <algorithm>

namespace aleppo {

struct AsRecord { // what one workgroup contributes to one unit
  double s;       // sum of |a| over the finite elements
  uint32_t p;     // finite elements > 0
  float x;        // max |a| over the finite elements
  uint32_t nf;    // non-finite elements
  uint32_t pad;
};
static_assert(sizeof(AsRecord) == 24, "AsRecord layout");

constexpr int AS_GROUPS = 16384; // 16-byte groups per conv workgroup: 64 per thread, 256 KB
constexpr int AS_FC_ROWS = 256;  // rows per fc workgroup: 64 per wave
constexpr int AS_PIX[3] = {A1_PIX, A2_PIX, A3_PIX};
constexpr int AS_C[3] = {A1_C, A2_C, A3_C};

// rows of a conv layer one workgroup takes
static inline uint32_t as_conv_rows_per_wg(int prec, int layer) {
  const int G = prec == ALEPPO_BF16 ? 8 : 4;
  return (uint32_t)(AS_GROUPS / (AS_C[layer] / G));
}
// workgroups of layer l (0-2 conv, 3 fc) for one forward chunk of ns samples
static inline uint32_t as_layer_wgs(int prec, int H, int l, long ns) {
  if (l == 3)
    return (uint32_t)((ns + AS_FC_ROWS - 1) / AS_FC_ROWS) * (uint32_t)((H / 4 + 63) / 64);
  const uint32_t rpw = as_conv_rows_per_wg(prec, l);
  return (uint32_t)(((size_t)ns * AS_PIX[l] + rpw - 1) / rpw);
}
// records of layer l for one forward chunk of ns samples: one per (row chunk, channel)
static inline size_t as_layer_records(int prec, int H, int l, long ns) {
  if (l == 3)
    return (size_t)((ns + AS_FC_ROWS - 1) / AS_FC_ROWS) * (size_t)H;
  return (size_t)as_layer_wgs(prec, H, l, ns) * AS_C[l];
}

ActStatsPlan act_stats_plan(int prec, int H, long total, long maxB) {
  ActStatsPlan pl{};
  size_t at = 0;
  for (int l = 0; l < 4; ++l) {
    size_t recs = 0;
    for (long n0 = 0; n0 < total; n0 += maxB)
      recs += as_layer_records(prec, H, l, std::min(maxB, total - n0));
    pl.rec_base[l] = at;
    at += recs;
  }
  pl.records = at;
  pl.units = (size_t)(A1_C + A2_C + A3_C + H);
  pl.bytes = at * sizeof(AsRecord) +
             (pl.units * ALEPPO_ACT_UNIT_COLS + (size_t)ALEPPO_ACT_LAYER_ROWS * ALEPPO_ACT_LAYER_COLS) * sizeof(double);
  return pl;
}

__device__ __forceinline__ bool as_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

struct AsAcc {
  double s = 0.0;
  uint32_t p = 0u;
  float x = 0.f;
  uint32_t nf = 0u;
  __device__ __forceinline__ void add(float a) {
    const bool ok = as_finite(a);
    const float m = ok ? fabsf(a) : 0.f;
    s += (double)m; // (an added 0.0 leaves a non-negative sum as it is)
    x = fmaxf(x, m);
    p += (ok && a > 0.f) ? 1u : 0u;
    nf += ok ? 0u : 1u;
  }
  // the other operand of one step of the fixed tree (sums of non-negative doubles: the order is the tree's)
  __device__ __forceinline__ void fold(int offset) {
    s += __shfl_down(s, offset, 64);
    p += __shfl_down(p, offset, 64);
    x = fmaxf(x, __shfl_down(x, offset, 64));
    nf += __shfl_down(nf, offset, 64);
  }
};

// the G channels of one 16-byte group, widened exactly
template <class T> struct AsGroup;
template <> struct AsGroup<float> {
  static constexpr int G = 4;
  static __device__ __forceinline__ void widen(const uint4 &v, float (&a)[4]) {
    a[0] = __uint_as_float(v.x), a[1] = __uint_as_float(v.y), a[2] = __uint_as_float(v.z), a[3] = __uint_as_float(v.w);
  }
};
template <> struct AsGroup<uint16_t> { // bf16 as its bits: the value is the bits in the high half of a float
  static constexpr int G = 8;
  static __device__ __forceinline__ void widen(const uint4 &v, float (&a)[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[2 * k] = __uint_as_float(w[k] << 16);
      a[2 * k + 1] = __uint_as_float(w[k] & 0xFFFF0000u);
    }
  }
};

struct AsShared { // the wave totals of a workgroup: [wave][channel slot]
  double s[4][256];
  uint32_t p[4][256];
  float x[4][256];
  uint32_t nf[4][256];
};

// slots channels of this workgroup, slot q in LDS; thread q < slots adds the four waves in order and writes its record
__device__ __forceinline__ void as_write_records(const AsShared &sh, int slots, AsRecord *__restrict__ out) {
  const int q = threadIdx.x;
  if (q >= slots)
    return;
  AsRecord r;
  r.s = ((sh.s[0][q] + sh.s[1][q]) + sh.s[2][q]) + sh.s[3][q];
  r.p = sh.p[0][q] + sh.p[1][q] + sh.p[2][q] + sh.p[3][q];
  r.x = fmaxf(fmaxf(sh.x[0][q], sh.x[1][q]), fmaxf(sh.x[2][q], sh.x[3][q]));
  r.nf = sh.nf[0][q] + sh.nf[1][q] + sh.nf[2][q] + sh.nf[3][q];
  r.pad = 0u;
  out[q] = r;
}

// chunk `chunk` of a conv layer [rows][C] of T -> C records at out
template <class T, int C>
__device__ __forceinline__ void as_conv_partial(const uint4 *__restrict__ a, uint32_t rows, uint32_t chunk, AsShared &sh,
                                                AsRecord *__restrict__ out) {
  constexpr int G = AsGroup<T>::G, CG = C / G, RL = 256 / CG, RPW = AS_GROUPS / CG;
  static_assert(C % G == 0 && 64 % CG == 0 && AS_GROUPS % (4 * 256) == 0, "a wave holds whole rows; four loads a step");
  const uint32_t cg = threadIdx.x % CG, rl = threadIdx.x / CG;
  const uint32_t r0 = chunk * (uint32_t)RPW, rend = min(rows, r0 + (uint32_t)RPW);
  AsAcc acc[G];
  for (uint32_t r = r0 + rl; r < rend; r += 4u * RL) {
    uint4 v[4]; // all four loads before the first use; a row past the chunk is not read and adds nothing
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t rk = r + (uint32_t)k * RL;
      v[k] = rk < rend ? a[(size_t)rk * CG + cg] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float e[G];
      AsGroup<T>::widen(v[k], e);
#pragma unroll
      for (int j = 0; j < G; ++j)
        acc[j].add(e[j]);
    }
  }
  // lanes l, l + CG, l + 2 CG, ... of a wave hold the same channel group
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < G; ++j) {
#pragma unroll
    for (int o = 32; o >= CG; o >>= 1)
      acc[j].fold(o);
    if (lane < CG) {
      const int q = lane * G + j; // = the channel
      sh.s[wave][q] = acc[j].s, sh.p[wave][q] = acc[j].p, sh.x[wave][q] = acc[j].x, sh.nf[wave][q] = acc[j].nf;
    }
  }
  __syncthreads();
  as_write_records(sh, C, out);
}

// fc: tile (bx, by) = rows [bx * AS_FC_ROWS, ...) by channel groups [by * 64, ...) of h [rows][H]; wave w takes rows
// w, w + 4, ... of the chunk, lane l channel group by * 64 + l
__device__ __forceinline__ void as_fc_partial(const uint4 *__restrict__ h, uint32_t rows, int H, uint32_t bx, uint32_t by,
                                              AsShared &sh, AsRecord *__restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t CG = (uint32_t)H / 4u, cg = by * 64u + lane;
  const bool live = cg < CG;
  const uint32_t r0 = bx * (uint32_t)AS_FC_ROWS, rend = min(rows, r0 + (uint32_t)AS_FC_ROWS);
  AsAcc acc[4];
  for (uint32_t r = r0 + wave; r < rend; r += 16u) {
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t rk = r + 4u * k;
      v[k] = (live && rk < rend) ? h[(size_t)rk * CG + cg] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float e[4];
      AsGroup<float>::widen(v[k], e);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j].add(e[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = lane * 4 + j;
    sh.s[wave][q] = acc[j].s, sh.p[wave][q] = acc[j].p, sh.x[wave][q] = acc[j].x, sh.nf[wave][q] = acc[j].nf;
  }
  __syncthreads();
  const int slots = min(256, H - (int)by * 256); // (channels of this tile that exist)
  as_write_records(sh, slots, out + (size_t)bx * H + (size_t)by * 256);
}

struct AsPass {            // one forward chunk
  const void *a[3];        // a1, a2, a3 of T
  const float *h;          // [ns][H]
  uint32_t rows[4];        // ns * PIX; fc: ns
  uint32_t first[5];       // first workgroup of each layer; first[4] = the grid
  unsigned long long rec[4]; // where this chunk's records of each layer start
  int H;
};

template <class T>
__global__ __launch_bounds__(256) void act_stats_partial_kernel(AsPass p, AsRecord *__restrict__ part) {
  __shared__ AsShared sh;
  const uint32_t b = blockIdx.x;
  if (b < p.first[1])
    as_conv_partial<T, A1_C>(static_cast<const uint4 *>(p.a[0]), p.rows[0], b, sh, part + p.rec[0] + (size_t)b * A1_C);
  else if (b < p.first[2])
    as_conv_partial<T, A2_C>(static_cast<const uint4 *>(p.a[1]), p.rows[1], b - p.first[1], sh,
                             part + p.rec[1] + (size_t)(b - p.first[1]) * A2_C);
  else if (b < p.first[3])
    as_conv_partial<T, A3_C>(static_cast<const uint4 *>(p.a[2]), p.rows[2], b - p.first[2], sh,
                             part + p.rec[2] + (size_t)(b - p.first[2]) * A3_C);
  else {
    const uint32_t tiles = ((uint32_t)p.H / 4u + 63u) / 64u, q = b - p.first[3];
    as_fc_partial(reinterpret_cast<const uint4 *>(p.h), p.rows[3], p.H, q / tiles, q % tiles, sh, part + p.rec[3]);
  }
}

struct AsFinal {
  unsigned long long rec[4];   // first record of each layer
  uint32_t chunks[4];          // records per unit of each layer
  unsigned long long K[4];     // positions per unit: samples * PIX
  int H;
  double tau;
};
constexpr int AS_MAX_UNITS = A1_C + A2_C + A3_C + 512;
// first unit of layer q (q = 4: the unit count); selects, so that nothing is indexed by a thread's own layer in registers
__device__ __forceinline__ int as_first(int q, int H) {
  return q == 0 ? 0 : q == 1 ? A1_C : q == 2 ? A1_C + A2_C : q == 3 ? A1_C + A2_C + A3_C : A1_C + A2_C + A3_C + H;
}
template <class V> __device__ __forceinline__ V as_pick(const V (&a)[4], int l) {
  return l == 0 ? a[0] : l == 1 ? a[1] : l == 2 ? a[2] : a[3];
}

__global__ __launch_bounds__(1024) void act_stats_final_kernel(const AsRecord *__restrict__ part, AsFinal f,
                                                                double *__restrict__ units, double *__restrict__ layers) {
  __shared__ double u_s[AS_MAX_UNITS], u_mean[AS_MAX_UNITS];
  __shared__ unsigned long long u_p[AS_MAX_UNITS], u_nf[AS_MAX_UNITS];
  __shared__ float u_x[AS_MAX_UNITS];
  __shared__ double l_mean[4], l_s[4], l_max[4];
  __shared__ unsigned long long l_p[4], l_nf[4], l_dead[4], l_dormant[4];
  const int U = as_first(4, f.H), u = threadIdx.x;
  const int l = u < A1_C ? 0 : u < A1_C + A2_C ? 1 : u < A1_C + A2_C + A3_C ? 2 : 3; // this thread's unit's layer
  const int lo = as_first(l, f.H), hi = as_first(l + 1, f.H);
  const double K = (double)as_pick(f.K, l);
  if (u < U) {
    const uint32_t C = (uint32_t)(hi - lo), chunks = as_pick(f.chunks, l);
    const AsRecord *src = part + as_pick(f.rec, l) + (u - lo);
    double s = 0.0;
    unsigned long long p = 0ull, nf = 0ull;
    float x = 0.f;
    uint32_t c = 0;
    for (; c + 8 <= chunks; c += 8) { // eight records in flight; added in chunk order
      AsRecord r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        r[k] = src[(size_t)(c + k) * C];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        s += r[k].s, p += r[k].p, x = fmaxf(x, r[k].x), nf += r[k].nf;
    }
    for (; c < chunks; ++c) {
      const AsRecord r = src[(size_t)c * C];
      s += r.s, p += r.p, x = fmaxf(x, r.x), nf += r.nf;
    }
    u_s[u] = s, u_p[u] = p, u_x[u] = x, u_nf[u] = nf;
    u_mean[u] = s / K;
  }
  __syncthreads();
  if (u < 4) { // layer u: its units in unit order
    const int lo = as_first(u, f.H), hi = as_first(u + 1, f.H);
    double sm = 0.0, ss = 0.0;
    unsigned long long p = 0ull, nf = 0ull, dead = 0ull, dormant = 0ull;
    float x = 0.f;
    for (int i = lo; i < hi; ++i) { // (lo / hi: of the LAYER u here)
      sm += u_mean[i], ss += u_s[i], p += u_p[i], nf += u_nf[i];
      x = fmaxf(x, u_x[i]);
      dead += u_x[i] == 0.f ? 1ull : 0ull;
    }
    const double lm = sm / (double)(hi - lo);
    for (int i = lo; i < hi; ++i) {
      const double score = lm == 0.0 ? 0.0 : u_mean[i] / lm;
      dormant += score <= f.tau ? 1ull : 0ull;
    }
    l_mean[u] = lm, l_s[u] = ss, l_max[u] = (double)x, l_p[u] = p, l_nf[u] = nf, l_dead[u] = dead, l_dormant[u] = dormant;
  }
  __syncthreads();
  if (u < U) {
    double *o = units + (size_t)u * ALEPPO_ACT_UNIT_COLS;
    const double lm = l_mean[l];
    o[ALEPPO_ACT_MEAN_ABS] = u_mean[u];
    o[ALEPPO_ACT_POSITIVE_FRACTION] = (double)u_p[u] / K;
    o[ALEPPO_ACT_MAX_ABS] = (double)u_x[u];
    o[ALEPPO_ACT_SCORE] = lm == 0.0 ? 0.0 : u_mean[u] / lm;
    o[ALEPPO_ACT_NONFINITE] = (double)u_nf[u];
  }
  if (u < 4) {
    double *o = layers + u * ALEPPO_ACT_LAYER_COLS;
    const double n_units = (double)(as_first(u + 1, f.H) - as_first(u, f.H)), elements = n_units * (double)as_pick(f.K, u);
    o[ALEPPO_ACT_L_UNITS] = n_units;
    o[ALEPPO_ACT_L_ELEMENTS] = elements;
    o[ALEPPO_ACT_L_MEAN_ABS] = l_s[u] / elements;
    o[ALEPPO_ACT_L_POSITIVE_FRACTION] = (double)l_p[u] / elements;
    o[ALEPPO_ACT_L_MAX_ABS] = l_max[u];
    o[ALEPPO_ACT_L_DEAD] = (double)l_dead[u];
    o[ALEPPO_ACT_L_DORMANT] = (double)l_dormant[u];
    o[ALEPPO_ACT_L_NONFINITE] = (double)l_nf[u];
  }
  if (u == 4) { // the total row: the four rows in row order
    double n_units = 0.0, elements = 0.0, ss = 0.0, mx = 0.0;
    unsigned long long p = 0ull, nf = 0ull, dead = 0ull, dormant = 0ull;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double nu = (double)(as_first(q + 1, f.H) - as_first(q, f.H));
      n_units += nu, elements += nu * (double)f.K[q], ss += l_s[q];
      mx = fmax(mx, l_max[q]);
      p += l_p[q], nf += l_nf[q], dead += l_dead[q], dormant += l_dormant[q];
    }
    double *o = layers + 4 * ALEPPO_ACT_LAYER_COLS;
    o[ALEPPO_ACT_L_UNITS] = n_units;
    o[ALEPPO_ACT_L_ELEMENTS] = elements;
    o[ALEPPO_ACT_L_MEAN_ABS] = ss / elements;
    o[ALEPPO_ACT_L_POSITIVE_FRACTION] = (double)p / elements;
    o[ALEPPO_ACT_L_MAX_ABS] = mx;
    o[ALEPPO_ACT_L_DEAD] = (double)dead;
    o[ALEPPO_ACT_L_DORMANT] = (double)dormant;
    o[ALEPPO_ACT_L_NONFINITE] = (double)nf;
  }
}

void launch_act_stats_partial(hipStream_t s, int prec, const void *a1, const void *a2, const void *a3, const float *h,
                              int H, long ns, const ActStatsPlan &pl, size_t done[4], void *scratch) {
  AsPass p{};
  p.a[0] = a1, p.a[1] = a2, p.a[2] = a3, p.h = h, p.H = H;
  uint32_t grid = 0;
  for (int l = 0; l < 4; ++l) {
    p.rows[l] = (uint32_t)(l < 3 ? (size_t)ns * AS_PIX[l] : (size_t)ns);
    p.first[l] = grid;
    grid += as_layer_wgs(prec, H, l, ns);
    p.rec[l] = pl.rec_base[l] + done[l];
    done[l] += as_layer_records(prec, H, l, ns);
  }
  p.first[4] = grid;
  AsRecord *part = static_cast<AsRecord *>(scratch);
  if (prec == ALEPPO_BF16)
    hipLaunchKernelGGL(act_stats_partial_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, p, part);
  else
    hipLaunchKernelGGL(act_stats_partial_kernel<float>, dim3(grid), dim3(256), 0, s, p, part);
}

void launch_act_stats_final(hipStream_t s, int H, long total, double tau, const ActStatsPlan &pl, const size_t done[4],
                            void *scratch, const double **units_dev, const double **layers_dev) {
  AsFinal f{};
  const int C[4] = {A1_C, A2_C, A3_C, H};
  for (int l = 0; l < 4; ++l) {
    f.rec[l] = pl.rec_base[l];
    f.chunks[l] = (uint32_t)(done[l] / C[l]);
    f.K[l] = (unsigned long long)total * (l < 3 ? AS_PIX[l] : 1);
  }
  f.H = H;
  f.tau = tau;
  AsRecord *part = static_cast<AsRecord *>(scratch);
  double *units = reinterpret_cast<double *>(part + pl.records);
  double *layers = units + pl.units * ALEPPO_ACT_UNIT_COLS;
  hipLaunchKernelGGL(act_stats_final_kernel, dim3(1), dim3(1024), 0, s, part, f, units, layers);
  *units_dev = units;
  *layers_dev = layers;
}

// ------------------------------------------------------------------ export
// sample blockIdx.x: [PIX][C] of T -> float [C][PIX]
template <class T, int PIX, int C>
__global__ __launch_bounds__(256) void act_export_kernel(const uint4 *__restrict__ a, float4 *__restrict__ out) {
  constexpr int G = AsGroup<T>::G, CG = C / G, PP = PIX | 1; // (an odd pitch spreads a pixel's channels over the banks)
  static_assert((PIX * C) % 4 == 0, "a sample's output is whole 16-byte words");
  __shared__ float t[C * PP];
  const size_t n = blockIdx.x;
  const uint4 *src = a + n * (size_t)(PIX * CG);
  for (int g = threadIdx.x; g < PIX * CG; g += 256) {
    const int pix = g / CG, c0 = (g % CG) * G;
    float e[G];
    AsGroup<T>::widen(src[g], e);
#pragma unroll
    for (int j = 0; j < G; ++j)
      t[(c0 + j) * PP + pix] = e[j];
  }
  __syncthreads();
  float4 *dst = out + n * (size_t)(PIX * C / 4);
  for (int w = threadIdx.x; w < PIX * C / 4; w += 256) {
    float e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = 4 * w + k;
      e[k] = t[(i / PIX) * PP + i % PIX];
    }
    dst[w] = make_float4(e[0], e[1], e[2], e[3]);
  }
}

// groups 16-byte groups of T in row-major order -> the same elements as float
template <class T>
__global__ __launch_bounds__(256) void plane_export_kernel(const uint4 *__restrict__ a, float4 *__restrict__ out,
                                                           long groups) {
  constexpr int G = AsGroup<T>::G;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups)
    return;
  float e[G];
  AsGroup<T>::widen(a[g], e);
#pragma unroll
  for (int k = 0; k < G / 4; ++k)
    out[g * (G / 4) + k] = make_float4(e[4 * k], e[4 * k + 1], e[4 * k + 2], e[4 * k + 3]);
}

void launch_plane_export(hipStream_t s, int prec, const void *src, float *out, long n) {
  const bool bf = prec == ALEPPO_BF16;
  const long groups = n / (bf ? 8 : 4); // (n is a multiple of 8: whole groups)
  const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
  if (bf)
    hipLaunchKernelGGL(plane_export_kernel<uint16_t>, grid, block, 0, s, static_cast<const uint4 *>(src),
                       reinterpret_cast<float4 *>(out), groups);
  else
    hipLaunchKernelGGL(plane_export_kernel<float>, grid, block, 0, s, static_cast<const uint4 *>(src),
                       reinterpret_cast<float4 *>(out), groups);
}

void launch_act_export(hipStream_t s, int prec, int layer, const void *a, float *out, long ns) {
  const uint4 *src = static_cast<const uint4 *>(a);
  float4 *dst = reinterpret_cast<float4 *>(out);
  const dim3 grid((unsigned)ns), block(256);
  const bool bf = prec == ALEPPO_BF16;
  if (layer == 0) {
    if (bf)
      hipLaunchKernelGGL((act_export_kernel<uint16_t, A1_PIX, A1_C>), grid, block, 0, s, src, dst);
    else
      hipLaunchKernelGGL((act_export_kernel<float, A1_PIX, A1_C>), grid, block, 0, s, src, dst);
  } else if (layer == 1) {
    if (bf)
      hipLaunchKernelGGL((act_export_kernel<uint16_t, A2_PIX, A2_C>), grid, block, 0, s, src, dst);
    else
      hipLaunchKernelGGL((act_export_kernel<float, A2_PIX, A2_C>), grid, block, 0, s, src, dst);
  } else {
    if (bf)
      hipLaunchKernelGGL((act_export_kernel<uint16_t, A3_PIX, A3_C>), grid, block, 0, s, src, dst);
    else
      hipLaunchKernelGGL((act_export_kernel<float, A3_PIX, A3_C>), grid, block, 0, s, src, dst);
  }
}
} // namespace aleppo
