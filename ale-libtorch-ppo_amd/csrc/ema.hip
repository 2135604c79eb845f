// ema.hip - the kernels of aleppo_ema_open / aleppo_ema_update / aleppo_ema_import (the definition is in aleppo.h): the
// exponentially averaged copy of the master parameters, in the private flat layout.
//   pass     one launch over the whole padded vector, a grid-stride loop of quads (4 consecutive floats; every tensor
//            starts 64-float aligned and the total is a multiple of 64).  Per quad: one 16-byte load of P, one of Pe, the
//            rule e' = d * e + w * p as THREE fp32 operations (contraction off: a fused multiply-add would round once
//            where the definition rounds twice), one 16-byte store of Pe and - bf16 contexts - one 8-byte store of four
//            packed bf16 to Pec, the conversion of cast_params_kernel.  Pads are zero in P and Pe and stay zero.  14 bytes
//            per element in bf16 (4 + 4 read, 4 + 2 written), 12 in fp32.
//            The same pass accumulates sum e'^2, sum p^2 and sum (p - e')^2 in double per thread, in the order of its
//            loop; block_sum.hpp gives one partial triple per workgroup.  UPDATE = false is the pass without its stores
//            (the statistics of the sets as they stand: open, import).
//   final    one workgroup: thread k < 3 adds partial k of every workgroup in index order; thread 0 writes the six doubles.
// No atomics; the grid is a function of the element count alone, so every figure is a function of the inputs alone.
#include "block_sum.hpp"
#include "common.hpp"
#include <algorithm>

namespace aleppo {

typedef __attribute__((ext_vector_type(4))) __bf16 ema_bf16x4;

__device__ __forceinline__ float ema_step(float d, float e, float w, float p) {
#pragma clang fp contract(off) // three roundings, as aleppo.h defines the rule (no fma)
  const float a = d * e;
  const float b = w * p;
  return a + b;
}

template <bool BF16, bool UPDATE>
__global__ __launch_bounds__(256) void ema_kernel(const float4 *__restrict__ P, float4 *__restrict__ Pe,
                                                  ema_bf16x4 *__restrict__ Pec, float d, float w, uint32_t quads,
                                                  double *__restrict__ part) {
  double se = 0.0, sp = 0.0, sd = 0.0;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < quads; q += gridDim.x * 256u) {
    const float4 p = P[q];
    float4 e = Pe[q];
    if constexpr (UPDATE) {
      e.x = ema_step(d, e.x, w, p.x);
      e.y = ema_step(d, e.y, w, p.y);
      e.z = ema_step(d, e.z, w, p.z);
      e.w = ema_step(d, e.w, w, p.w);
      Pe[q] = e;
      if constexpr (BF16) {
        ema_bf16x4 c;
        c[0] = (__bf16)e.x;
        c[1] = (__bf16)e.y;
        c[2] = (__bf16)e.z;
        c[3] = (__bf16)e.w;
        Pec[q] = c;
      }
    }
    const double pv[4] = {p.x, p.y, p.z, p.w}, ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double df = pv[k] - ev[k];
      se += ev[k] * ev[k];
      sp += pv[k] * pv[k];
      sd += df * df;
    }
  }
  __shared__ double s4[4];
  se = block_sum_256(se, s4);
  sp = block_sum_256(sp, s4);
  sd = block_sum_256(sd, s4);
  if (threadIdx.x == 0) {
    part[(size_t)blockIdx.x * 3 + 0] = se;
    part[(size_t)blockIdx.x * 3 + 1] = sp;
    part[(size_t)blockIdx.x * 3 + 2] = sd;
  }
}

__global__ __launch_bounds__(64) void ema_final_kernel(const double *__restrict__ part, int nblk, long long updates, float d,
                                                       double *__restrict__ out) {
  __shared__ double s[3];
  if (threadIdx.x < 3) {
    double a = 0.0;
    for (int b = 0; b < nblk; ++b) // index order
      a += part[(size_t)b * 3 + threadIdx.x];
    s[threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[ALEPPO_EMA_UPDATES] = (double)updates;
    out[ALEPPO_EMA_DECAY] = (double)d;
    out[ALEPPO_EMA_NORM] = sqrt(s[0]);
    out[ALEPPO_EMA_PARAM_NORM] = sqrt(s[1]);
    out[ALEPPO_EMA_DISTANCE] = sqrt(s[2]);
    out[ALEPPO_EMA_RELATIVE_DISTANCE] = s[1] > 0.0 ? sqrt(s[2] / s[1]) : 0.0;
  }
}

// A bandwidth-bound pass: one quad per thread up to 8 workgroups of 256 threads per CU on 256 CUs, the loop strides the rest.
int launch_ema(hipStream_t s, bool update, const float *P, float *Pe, void *Pec, long n, float d, float w, double *blk) {
  const uint32_t quads = (uint32_t)(n / 4);
  const int nblk = (int)std::max<uint32_t>(1u, std::min<uint32_t>((quads + 255u) / 256u, (uint32_t)EMA_MAX_BLOCKS));
  const float4 *p4 = reinterpret_cast<const float4 *>(P);
  float4 *e4 = reinterpret_cast<float4 *>(Pe);
  ema_bf16x4 *c4 = static_cast<ema_bf16x4 *>(Pec);
  const bool bf = Pec != static_cast<void *>(Pe);
  if (!update)
    hipLaunchKernelGGL((ema_kernel<false, false>), dim3(nblk), dim3(256), 0, s, p4, e4, c4, d, w, quads, blk);
  else if (bf)
    hipLaunchKernelGGL((ema_kernel<true, true>), dim3(nblk), dim3(256), 0, s, p4, e4, c4, d, w, quads, blk);
  else
    hipLaunchKernelGGL((ema_kernel<false, true>), dim3(nblk), dim3(256), 0, s, p4, e4, c4, d, w, quads, blk);
  return nblk;
}

void launch_ema_final(hipStream_t s, int nblk, long long updates, float d, double *blk) {
  hipLaunchKernelGGL(ema_final_kernel, dim3(1), dim3(64), 0, s, blk, nblk, updates, d, ema_stats(blk));
}

} // namespace aleppo
