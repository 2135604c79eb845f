// block_sum.hpp - the wave and workgroup sums every reduction kernel shares.  One fixed tree for every element type, so
// that a sum's bits depend on its inputs alone: run-to-run deterministic, and equal wherever two kernels sum the same values.
#pragma once
#include <hip/hip_runtime.h>

namespace aleppo {

// xor butterfly over the 64 lanes: every lane ends with the same sum
template <class V> __device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_xor(v, o, 64);
  return v;
}

// deterministic sum over a workgroup of 256 threads, valid in every thread: the butterfly, then the four waves' sums as
// (s0 + s1) + (s2 + s3).  s4: 4 elements of LDS (may be reused by the next call: the leading barrier orders them)
template <class V> __device__ __forceinline__ V block_sum_256(V v, V *s4) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0)
    s4[wave] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

} // namespace aleppo
