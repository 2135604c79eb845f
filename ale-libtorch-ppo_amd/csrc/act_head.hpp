// act_head.hpp - the acting head's pieces: what infer_head_kernel (the rollout, kernels.hip) and eval_head_kernel (the
// evaluation lanes, kernels.hip) are both built from, so that "a lane computes what an environment of aleppo_act
// computes, bit for bit" holds by construction.  One wave per environment / lane, four waves per workgroup; lane k < A
// owns action k (softmax term, noise, p / q), lane A the value.  Device code only.
#pragma once
#include "common.hpp"
#include "gemm.hpp"       // f32x4
#include "block_sum.hpp" // wave_sum

namespace aleppo {

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
// U(w) = ((w >> 8) + 0.5) / 2^24 in fp32: u in (0,1)  (include/aleppo.h)
__device__ __forceinline__ float philox_unit(uint32_t w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// The workgroup's dynamic LDS is the head-weight tile sWh [(A+1)][H] floats (the launch asks for exactly that): written by
// head_hidden, read by head_dot behind the caller's __syncthreads().  Both name the array itself, not a pointer handed
// in: the compiler then knows the address space and the array's alignment when it first sees the accesses.

// hv = the fc bias + the fc split-K slices z = 0 .. NSPLIT-1 (in that order), formed on the fly, and the head weights Wh
// staged into sWh by the whole workgroup - ONE parallel round trip: every load is issued before the first add.
// Lane l owns hidden units 4l .. 4l+3 and H/2 + 4l .. (H <= 512, H % 8 == 0): two 16-byte loads per split-K slice
// instead of eight scalar ones (the kernel is latency-bound on ~70 vector-memory instructions per wave; now 18),
// consecutive lanes on consecutive 16-byte pieces (coalesced, conflict-free LDS reads of the head weights).
template <int NSPLIT>
__device__ __forceinline__ void head_hidden(const float *__restrict__ hpart, const float *__restrict__ bfc,
                                            const float *__restrict__ Wh, int e, int E, int H, int A, int lane,
                                            float hv[8]) {
  extern __shared__ float sWh[];
  f32x4 part[NSPLIT][2];
  const bool own = e < E && lane * 8 < H;
#pragma unroll
  for (int z = 0; z < NSPLIT; ++z) { // issue every split-K partial load first (independent)
    const float *src = hpart + ((size_t)z * E + (own ? e : 0)) * H + (own ? lane * 4 : 0);
    part[z][0] = *reinterpret_cast<const f32x4 *>(src);
    part[z][1] = *reinterpret_cast<const f32x4 *>(src + H / 2);
  }
  {
    const float *b = bfc + (own ? lane * 4 : 0);
    const f32x4 b0 = *reinterpret_cast<const f32x4 *>(b), b1 = *reinterpret_cast<const f32x4 *>(b + H / 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hv[i] = b0[i];
      hv[4 + i] = b1[i];
    }
  }
  for (int k = threadIdx.x; k < (A + 1) * H / 4; k += 256)
    reinterpret_cast<f32x4 *>(sWh)[k] = reinterpret_cast<const f32x4 *>(Wh)[k];
#pragma unroll
  for (int z = 0; z < NSPLIT; ++z)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hv[i] += part[z][0][i];
      hv[4 + i] += part[z][1][i];
    }
}

// Head output a of the wave's hidden vector - logit a (a < A) / the value (a == A) - into lane a's zmine: the lanes'
// partial dot products (two 4-wide sums, in this order), the wave sum, then the bias.  The callers loop a = 0 .. A.
__device__ __forceinline__ void head_dot(const float *__restrict__ bh, const float hv[8], int H, int a, int lane,
                                         float &zmine) {
  extern __shared__ float sWh[];
  float s = 0.f;
  if (lane * 8 < H) {
    const f32x4 w0 = *reinterpret_cast<const f32x4 *>(sWh + a * H + lane * 4);
    const f32x4 w1 = *reinterpret_cast<const f32x4 *>(sWh + a * H + H / 2 + lane * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      s += hv[i] * w0[i];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      s += hv[4 + i] * w1[i];
  }
  s = wave_sum(s) + bh[a];
  if (lane == a)
    zmine = s;
}

// softmax(z * scale) over the action lanes (train.cc:374): lane k's p_k = the returned numerator / sum (the caller
// divides, after it has put the noise load in flight); scale = 1 is a literal at the rollout's call and folds away
__device__ __forceinline__ float softmax_term(float zmine, bool isact, float scale, float &sum) {
  float mx = isact ? zmine : -3.0e38f;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1)
    mx = fmaxf(mx, __shfl_xor(mx, o, 64)); // A <= 18 < 32
  const float ex = isact ? expf((zmine - mx) * scale) : 0.f;
  sum = ex;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1)
    sum += __shfl_xor(sum, o, 64);
  return ex;
}

// lane k's q_k ~ Exp(1) (Q10): the caller's noise[e][k], or -logf(U(c[k % 4])) of the Philox4x32-10 block with counter
// words { counter lo, counter hi, e, k / 4 } - four actions share a block.  1 on the lanes that own no action.
__device__ __forceinline__ float exp1_noise(const float *__restrict__ noise, uint64_t key, uint64_t counter, int e, int A,
                                            int lane) {
  float q = 1.f;
  if (lane < A) {
    if (noise) {
      q = noise[(size_t)e * A + lane];
    } else {
      uint32_t c[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)e, (uint32_t)(lane >> 2)};
      philox4x32_10(c, (uint32_t)key, (uint32_t)(key >> 32));
      const uint32_t w = (lane & 3) == 0 ? c[0] : (lane & 3) == 1 ? c[1] : (lane & 3) == 2 ? c[2] : c[3];
      q = -logf(philox_unit(w));
    }
  }
  return q;
}

// arg-max of r over the wave's lanes 0 .. 31 (A <= 18 < 32), ties -> lowest index (first maximum wins)
__device__ __forceinline__ int wave_argmax_first(float r, int lane) {
  int best = lane;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    const float ro = __shfl_xor(r, o, 64);
    const int bo = __shfl_xor(best, o, 64);
    if (ro > r || (ro == r && bo < best)) {
      r = ro;
      best = bo;
    }
  }
  return best;
}

// one lane per wave: the action to the device plane and straight to the mapped host buffer with a system-scope (sc0 sc1,
// write-through) store, which publish_ticket's drain then waits for
__device__ __forceinline__ void store_action(int *actions, int64_t *pinned, int e, int best) {
  actions[e] = best;
  __hip_atomic_store(pinned + e, (int64_t)best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Publish: ONE ticket word (pinned[E]) after every wave's action stores are system-visible - the host polls the ticket
// instead of synchronising the stream, so PCIe write latency overlaps the host's next enqueue.  Every wave of every
// workgroup calls this, the waves that own no environment included (they must reach the barrier).
// The host only needs the actions; they were written with system-scope stores, so a full system-scope release (an L2
// write-back of everything this rollout slot dirtied, ~4 us) is not needed: every storing wave drains its stores
// (vmcnt(0): acknowledged), the workgroup meets, one thread bumps the device counter and the last arriver - which
// therefore runs after every wave's acknowledged stores - writes the ticket, again at system scope.  All atomics are
// RELAXED on purpose (an agent / system release would emit the buffer_wbl2 this path exists to avoid); the order comes
// from the explicit vmcnt(0) drain, the barrier and the data dependency of the ticket store on the counter's return value.
// (Measured and rejected: one self-describing 8-byte word { ticket | action } per environment, no drain / counter /
// ticket store, the host sweeping all E words - 5.4-5.6 vs 4.9-5.3 ms per 128-slot rollout on the same box: the host
// then reads the very lines the device is still writing.)
__device__ __forceinline__ void publish_ticket(int64_t *pinned, unsigned int *done_ctr, long long ticket, int E) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int prev = __hip_atomic_fetch_add(done_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      __hip_atomic_store(done_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(reinterpret_cast<long long *>(pinned + E), ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

} // namespace aleppo
