// recycle.hip - the kernels of aleppo_recycle_units / aleppo_recycle_dormant (the definition is in aleppo.h): ReDo's
// re-initialisation and reset of masked units, on the master parameters and both Adam moments, in the private flat layout.
//   mask     one small launch: unit u of the device-side table of aleppo_activation_stats -> mask[u] = (its layer is asked
//            for) && SCORE_u <= tau, the comparison ALEPPO_ACT_L_DORMANT counts by.
//   pass     one launch over the whole layout.  A thread owns 4 consecutive floats (a quad) of one tensor; every tensor starts
//            64-float aligned, so a quad never spans two.  Every tensor is read as rows [o][p][c] with c innermost: conv
//            weights [oc][(kh,kw)][c], the fc weight [o][position][c], the stacked heads [a][1][j], a bias [1][1][o].  o
//            indexes the tensor's OWN units, c the units that FEED it (for a bias: its own units, whose rule is "zero").  The
//            channel count of every tensor a rule can select is a multiple of 4, so a quad is 4 consecutive c of one (o, p):
//            one own-mask byte, one aligned 4-byte load of feed-mask bytes.  Element: zero if mask[feed + c], otherwise
//            re-initialised if mask[own + o], otherwise not selected.  A wholly selected quad is one 16-byte store to P (and
//            one each of zeros to M1 / M2); a partly selected one stores its selected elements alone.  Nothing is loaded from
//            P / M1 / M2, nothing unselected, no pad and nothing past a tensor's size is written.
// No atomics, no LDS; the grid is a function of the layout only.
// aleppo_shrink_perturb's pass (Ash & Adams 2020) is here too: it draws with the same rc_value at the same exported index
// (rc_export_index), from the same tensor table (rc_tensors).  A thread owns a quad as above, loads it, forms
// p' = lam * p + sg * xi as three explicit fp32 operations and stores it; xi = 0 for a bias.
#include "common.hpp"
#include <cmath>

namespace aleppo {

struct RcTensor {
  uint32_t K;     // elements per own unit (row length): PIX * C
  uint32_t C;     // feeding channels, innermost
  uint32_t PIX;   // positions per (own unit, feeding channel) in the reference's order
  int own, feed;  // first mask byte of the own / the feeding units; -1: the tensor has no such rule
  uint32_t ref;   // index of the tensor's first element in the flat aleppo_export_params vector
  float a;        // sqrt(6 / fan_in) of the re-initialisation (tensors with own >= 0)
  uint32_t vrow, vskip; // rows o >= vrow are exported vskip elements later (the stacked heads: the action bias lies between
                        // the action rows and the value row); ~0u, 0 elsewhere
};
// index in the flat aleppo_export_params vector of element (own unit o, position pos, feeding channel c) of a weight tensor
__device__ __forceinline__ uint32_t rc_export_index(const RcTensor &d, uint32_t o, uint32_t pos, uint32_t c) {
  return d.ref + (o * d.C + c) * d.PIX + pos + (o >= d.vrow ? d.vskip : 0u);
}
struct RcPass {
  uint32_t off[P_COUNT + 1], size[P_COUNT];
  RcTensor t[P_COUNT];
  unsigned long long key; // splitmix64(key of the call)
  int keep_moments;
};

__device__ __forceinline__ unsigned long long rc_splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// element i of the exported vector: a * (k * 2^-23), k uniform in [-2^23, 2^23) - the inner product is exact
__device__ __forceinline__ float rc_value(unsigned long long key, uint32_t i, float a) {
  const unsigned long long r = rc_splitmix64(key ^ (unsigned long long)i);
  const int k = (int)(r >> 40) - 8388608;
  return a * ((float)k * 0x1p-23f);
}

static float rc_bound(int fan_in) { return (float)std::sqrt(6.0 / (double)fan_in); } // He-uniform's a_l

__global__ __launch_bounds__(256) void recycle_kernel(RcPass p, const uint8_t *__restrict__ mask, float *__restrict__ P,
                                                      float *__restrict__ M1, float *__restrict__ M2) {
  const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
  if (i0 >= p.off[P_COUNT])
    return;
  RcTensor d = p.t[0];
  uint32_t base = 0, size = p.size[0];
#pragma unroll
  for (int t = 1; t < P_COUNT; ++t)
    if (i0 >= p.off[t])
      d = p.t[t], base = p.off[t], size = p.size[t];
  const uint32_t j = i0 - base;
  if (j >= size || (d.own < 0 && d.feed < 0)) // an alignment pad, or a tensor no rule selects (the head biases)
    return;
  const uint32_t o = j / d.K, r = j - o * d.K, pos = r / d.C, c0 = r - pos * d.C; // (c0 % 4 == 0: C % 4 == 0)
  const bool own = d.own >= 0 && mask[d.own + o] != 0;
  const uint32_t feed = d.feed >= 0 ? *reinterpret_cast<const uint32_t *>(mask + d.feed + c0) : 0u;
  if (!own && feed == 0u)
    return;
  const uint32_t valid = min(4u, size - j);
  float v[4];
  bool sel[4];
  bool all = valid == 4u;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const bool z = ((feed >> (8 * k)) & 0xFFu) != 0u;
    sel[k] = k < valid && (z || own);
    v[k] = z || !own ? 0.0f : rc_value(p.key, rc_export_index(d, o, pos, c0 + k), d.a);
    all = all && sel[k];
  }
  if (all) {
    *reinterpret_cast<float4 *>(P + i0) = make_float4(v[0], v[1], v[2], v[3]);
    if (!p.keep_moments) {
      *reinterpret_cast<float4 *>(M1 + i0) = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4 *>(M2 + i0) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k)
    if (sel[k]) {
      P[i0 + k] = v[k];
      if (!p.keep_moments)
        M1[i0 + k] = 0.f, M2[i0 + k] = 0.f;
    }
}

__global__ __launch_bounds__(256) void recycle_mask_kernel(const double *__restrict__ units, int H, double tau, int layers,
                                                           uint8_t *__restrict__ mask) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= A1_C + A2_C + A3_C + H)
    return;
  const int l = u < A1_C ? 0 : u < A1_C + A2_C ? 1 : u < A1_C + A2_C + A3_C ? 2 : 3;
  const bool on = ((layers >> l) & 1) != 0 && units[(size_t)u * ALEPPO_ACT_UNIT_COLS + ALEPPO_ACT_SCORE] <= tau;
  mask[u] = on ? 1 : 0;
}

void launch_recycle_mask(hipStream_t s, const double *units_dev, int H, double tau, int layers, uint8_t *mask) {
  const int U = A1_C + A2_C + A3_C + H;
  hipLaunchKernelGGL(recycle_mask_kernel, dim3((U + 255) / 256), dim3(256), 0, s, units_dev, H, tau, layers, mask);
}

// aleppo_shrink_perturb: sa[t] = sqrt(6 / fan_in) of the tensors that are drawn for (the four trunk weights, the stacked
// head rows with fan_in = H), 0 for a bias
struct SpPass {
  uint32_t off[P_COUNT + 1], size[P_COUNT];
  RcTensor t[P_COUNT];
  float sa[P_COUNT];
  unsigned long long key; // splitmix64(key of the call)
  float lam, sg;
};
// p' = __fadd_rn(__fmul_rn(lam, p), __fmul_rn(sg, xi)) of aleppo.h: THREE fp32 operations, each rounded to nearest.  Written
// with the plain operators under contract(off), like ema_step: the header's __fmul_rn / __fadd_rn are inline functions
// compiled with contraction allowed, so a product made by one of them is still fused into the sum (v_pk_fma_f32 on
// part of the elements), which rounds once less than a host does
__device__ __forceinline__ float sp_element(float lam, float p, float sg, float xi) {
#pragma clang fp contract(off)
  const float a = lam * p;
  const float b = sg * xi;
  return a + b;
}
__global__ __launch_bounds__(256) void shrink_perturb_kernel(SpPass p, float *__restrict__ P) {
  const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
  if (i0 >= p.off[P_COUNT])
    return;
  RcTensor d = p.t[0];
  uint32_t base = 0, size = p.size[0];
  float a = p.sa[0];
#pragma unroll
  for (int t = 1; t < P_COUNT; ++t)
    if (i0 >= p.off[t])
      d = p.t[t], base = p.off[t], size = p.size[t], a = p.sa[t];
  const uint32_t j = i0 - base;
  if (j >= size) // an alignment pad
    return;
  const uint32_t valid = min(4u, size - j);
  const float4 q = *reinterpret_cast<const float4 *>(P + i0); // (i0 + 3 is inside the tensor's 64-float aligned extent)
  float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k)
    if (k < valid) {
      float xi = 0.0f;
      if (a != 0.0f) {
        const uint32_t e = j + k, o = e / d.K, r = e - o * d.K, pos = r / d.C, c = r - pos * d.C;
        xi = rc_value(p.key, rc_export_index(d, o, pos, c), a);
      }
      v[k] = sp_element(p.lam, v[k], p.sg, xi);
    }
  *reinterpret_cast<float4 *>(P + i0) = make_float4(v[0], v[1], v[2], v[3]); // (elements past `valid` are the pad's zeros)
}

// the tensor table both passes share: row shapes, mask bytes and where each tensor starts in the exported vector
static void rc_tensors(const ParamLayout &L, RcTensor t[P_COUNT]) {
  const int H = L.H, A = L.A;
  const int m1 = 0, m2 = A1_C, m3 = A1_C + A2_C, m4 = A1_C + A2_C + A3_C; // first mask byte of conv1, conv2, conv3, fc
  // the tensors' first elements in the exported vector (libtorch's parameters() order)
  const uint32_t r_w1 = 0, r_w2 = r_w1 + 32 * 256 + 32, r_w3 = r_w2 + 64 * 512 + 64, r_wfc = r_w3 + 64 * 576 + 64;
  const uint32_t r_aw = r_wfc + (uint32_t)H * FC_IN + (uint32_t)H; // (the recycle never draws for the heads)
  const uint32_t none = ~0u;
  auto bias = [&](int units, int first) {
    return RcTensor{(uint32_t)units, (uint32_t)units, 1u, -1, first, 0u, 0.f, none, 0u};
  };
  t[P_W1] = RcTensor{256u, 4u, 64u, m1, -1, r_w1, rc_bound(256), none, 0u};
  t[P_W2] = RcTensor{512u, 32u, 16u, m2, m1, r_w2, rc_bound(512), none, 0u};
  t[P_W3] = RcTensor{576u, 64u, 9u, m3, m2, r_w3, rc_bound(576), none, 0u};
  t[P_WFC] = RcTensor{(uint32_t)FC_IN, 64u, 49u, m4, m3, r_wfc, rc_bound(FC_IN), none, 0u};
  // action rows, then the value row: zero where m4[j]
  t[P_WH] = RcTensor{(uint32_t)H, (uint32_t)H, 1u, -1, m4, r_aw, 0.f, (uint32_t)A, (uint32_t)A};
  t[P_BH] = RcTensor{(uint32_t)(A + 1), (uint32_t)(A + 1), 1u, -1, -1, 0u, 0.f, none, 0u}; // never touched
  t[P_B1] = bias(A1_C, m1);
  t[P_B2] = bias(A2_C, m2);
  t[P_B3] = bias(A3_C, m3);
  t[P_BFC] = bias(H, m4);
}

void launch_recycle(hipStream_t s, const ParamLayout &L, const uint8_t *mask, unsigned long long key, bool keep_moments,
                    float *P, float *M1, float *M2) {
  RcPass p{};
  for (int t = 0; t <= P_COUNT; ++t)
    p.off[t] = (uint32_t)L.off[t];
  for (int t = 0; t < P_COUNT; ++t)
    p.size[t] = (uint32_t)L.size[t];
  rc_tensors(L, p.t);
  p.key = key;
  p.keep_moments = keep_moments ? 1 : 0;
  const uint32_t quads = (uint32_t)(L.total() / 4); // (every offset is a multiple of 64)
  hipLaunchKernelGGL(recycle_kernel, dim3((quads + 255) / 256), dim3(256), 0, s, p, mask, P, M1, M2);
}

void launch_shrink_perturb(hipStream_t s, const ParamLayout &L, unsigned long long key, float lam, float sg, float *P) {
  SpPass p{};
  for (int t = 0; t <= P_COUNT; ++t)
    p.off[t] = (uint32_t)L.off[t];
  for (int t = 0; t < P_COUNT; ++t)
    p.size[t] = (uint32_t)L.size[t];
  rc_tensors(L, p.t);
  for (int t = 0; t < P_COUNT; ++t)
    p.sa[t] = p.t[t].a; // the trunk weights; 0 for the biases
  p.sa[P_WH] = rc_bound(L.H);
  p.key = key;
  p.lam = lam;
  p.sg = sg;
  const uint32_t quads = (uint32_t)(L.total() / 4);
  hipLaunchKernelGGL(shrink_perturb_kernel, dim3((quads + 255) / 256), dim3(256), 0, s, p, P);
}

} // namespace aleppo
