// kernels.hip - HBM-bound / latency-bound kernels of the PPO-over-ALE hot path for gfx950:
// frame ingest (LUT + area resize + 2-frame max + 4-frame stack + rollout-slot write), action head +
// categorical sampling, reward clamp + GAE + returns + old log-probs, PPO loss forward/backward fused
// with the head linear layers, split-K slab reduction, global-norm clip + Adam, and the layout
// conversions used only at the C-ABI boundary.  Each kernel cites the reference code it replaces.
#include "common.hpp"
#include "gemm.hpp" // bf16 / vector typedefs
#include "block_sum.hpp" // wave_sum, block_sum_256
#include "head_train.hpp" // f16, and what the head kernel's entry points share
#include "act_head.hpp" // what the acting head's two entry points are built from
#include <algorithm>

namespace aleppo {

// ================================================================================================
// Frame ingest.  Replaces, per env-step: gray LUT (environment.cc:48-55) + resize (vision.cc:86-95 on
// the env threads; here the area spec of vision.cc:8-32) + 2-frame max (max_and_skip.cc:33-42) +
// Rollout::update_observations (rollout.cc:184-196) + Buffer::add's observation copy (buffer.cc:47).
// The 4-frame stack of one pixel is ONE u32 (byte 0 = newest frame, Q11), so "shift + insert" is
// (old << 8) | new and "broadcast on episode start" is new * 0x01010101.  The stack for slot t+1
// is written straight into the rollout buffer; slot t is never copied again.
// grid (28 x E) workgroups of 256 threads, one thread per output pixel (a 4-pixels-per-thread variant with
// dword loads measured slower: 20 vs 17 us - fewer threads to hide the LUT read latency).
// ================================================================================================
template <bool RAW>
__global__ __launch_bounds__(256) void ingest_kernel(const uint8_t *__restrict__ frames, const uint8_t *__restrict__ lut,
                                                      const uint8_t *__restrict__ start, StartBits sbits, uint32_t *obs,
                                                      int slots, int t_src, int t_dst) {
  // one thread per output pixel: every load of a thread (6 raw dwords, the old packed pixel, the start flag)
  // is independent and issued up front - one memory round trip, no staging barrier on the frame data; the
  // 256-entry LUT sits in LDS.  A wave's 64 adjacent output pixels read ~122 adjacent raw bytes per row.
  const int e = blockIdx.y, tid = threadIdx.x;
  const int pix = blockIdx.x * 256 + tid;
  __shared__ uint8_t slut[256];
  const bool live = pix < FRAME_PIX;
  const int i = live ? pix / 84 : 0, j = live ? pix - i * 84 : 0;
  uint32_t old = 0;
  if (live)
    old = obs[((size_t)e * slots + t_src) * FRAME_PIX + pix];
  // episode-start flag: from the kernel-argument bitmask (no upload on the critical path) or from memory
  const bool st = start ? start[e] != 0 : ((sbits.w[e >> 5] >> (e & 31)) & 1u) != 0;
  uint32_t v = 0;
  if (RAW) {
    const int y0 = (i * RAW_H) / 84, x0 = (j * RAW_W) / 84, x1 = ((j + 1) * RAW_W + 83) / 84; // 3 rows, 2-3 cols
    const bool wide = (x1 - x0) == 3;
    // ONE unaligned dword per (frame, row) instead of 2-3 byte loads: the kernel is bound by the number of
    // vector-memory instructions (20 -> 8 per pixel).  The dword starts at min(x0, RAW_W - 4) so it never leaves
    // the row; the wanted bytes are shifted down.
    typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
    const int xa = min(x0, RAW_W - 4), sh = (x0 - xa) * 8;
    uint32_t roww[2][3];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const uint8_t *src = frames + ((size_t)e * 2 + f) * (RAW_H * RAW_W) + (size_t)y0 * RAW_W + xa;
#pragma unroll
      for (int y = 0; y < 3; ++y)
        roww[f][y] = live ? *reinterpret_cast<const u32_unaligned *>(src + y * RAW_W) : 0u;
    }
    slut[tid] = lut[tid];
    __syncthreads();
    int best = 0;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      int s = 0;
#pragma unroll
      for (int y = 0; y < 3; ++y) {
        const uint32_t w = roww[f][y] >> sh;
        s += slut[w & 255u] + slut[(w >> 8) & 255u] + (wide ? slut[(w >> 16) & 255u] : 0);
      }
      // adaptive-average (area) mean in f32 like interpolate(mode=area), round-half-even to u8
      const int q = (int)rintf((float)s / (wide ? 9.0f : 6.0f));
      best = max(best, q);
    }
    v = (uint32_t)min(best, 255);
  } else if (live) {
    v = frames[(size_t)e * FRAME_PIX + pix];
  }
  if (live)
    obs[((size_t)e * slots + t_dst) * FRAME_PIX + pix] = st ? v * 0x01010101u : ((old << 8) | v);
}

void launch_ingest(hipStream_t s, bool raw, const uint8_t *frames, const uint8_t *lut, const uint8_t *start,
                   const StartBits *sbits, uint32_t *obs, int E, int slots, int t_src, int t_dst) {
  const dim3 g((FRAME_PIX + 255) / 256, E);
  StartBits sb{};
  if (sbits)
    sb = *sbits;
  if (raw)
    hipLaunchKernelGGL(ingest_kernel<true>, g, dim3(256), 0, s, frames, lut, start, sb, obs, slots, t_src, t_dst);
  else
    hipLaunchKernelGGL(ingest_kernel<false>, g, dim3(256), 0, s, frames, lut, start, sb, obs, slots, t_src, t_dst);
}

__global__ void copy_slot_kernel(uint32_t *obs, int slots, int src, int dst) {
  const int e = blockIdx.y;
  const u32x4 *s = reinterpret_cast<const u32x4 *>(obs + ((size_t)e * slots + src) * FRAME_PIX);
  u32x4 *d = reinterpret_cast<u32x4 *>(obs + ((size_t)e * slots + dst) * FRAME_PIX);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < FRAME_PIX / 4)
    d[i] = s[i];
}
void launch_copy_slot(hipStream_t s, uint32_t *obs, int E, int slots, int src, int dst) {
  hipLaunchKernelGGL(copy_slot_kernel, dim3((FRAME_PIX / 4 + 255) / 256, E), dim3(256), 0, s, obs, slots, src, dst);
}

// ================================================================================================
// The slot-ahead hand-off's gate (rollout.cc:204-208 / :312-313: the next forward pass may only start once the host has
// the actions and the emulators have delivered the frames).  The next slot's kernels are enqueued BEHIND this one-wave
// kernel; it returns when the host has stored a sequence number >= seq into the release word (mapped page-locked host
// memory, read with system-scope loads: every poll is a bus round trip, nothing is cached).
// Exit condition every wave reaches: after timeout_ticks of the 100 MHz wall clock the kernel gives up, reports the
// sequence number it was waiting for in go[1] and returns - the stream drains, the host finds the report and fails the
// context; the GPU never waits for ever on a host that has gone away.
// (Replaces hipStreamWaitValue32, which this runtime implements as the same kind of polling kernel - but without an
// exit condition, behind a capability flag, and on a 32-bit word that wraps.)
// ================================================================================================
__global__ __launch_bounds__(64) void gate_kernel(unsigned long long *go, unsigned long long seq,
                                                   unsigned long long timeout_ticks) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < seq) {
      __builtin_amdgcn_s_sleep(2);
      if (wall_clock64() - t0 > timeout_ticks) {
        __hip_atomic_store(go + 1, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
    }
  }
}
void launch_gate(hipStream_t s, unsigned long long *go_dev, unsigned long long seq, unsigned long long timeout_ticks) {
  hipLaunchKernelGGL(gate_kernel, dim3(1), dim3(64), 0, s, go_dev, seq, timeout_ticks);
}

// ================================================================================================
// Action head + categorical sampling (action selector closure, train.cc:367-379): logits / value from
// the hidden vector, softmax, multinomial(1, replacement) == argmax_k(p_k / q_k), q ~ Exp(1) (Q10),
// first maximum wins.  One wave per environment.  Actions go to the rollout slot AND to pinned host
// memory (replaces the per-env .item<int64_t>() of rollout.cc:312-313).
// ================================================================================================
// h = sum of the fc split-K slices + fc bias, formed on the fly (all NSPLIT*8 loads of a lane are independent).
// Lane k < A owns action k (softmax term, noise, p/q); a wave arg-max picks the first maximum.  The pieces are
// act_head.hpp's, shared with the evaluation lanes' head below.
// Hand-off to the host: actions go to pinned memory, then ONE ticket word is published (publish_ticket).
// probs_in != nullptr (the stateless aleppo_sample operator, train.cc:374-375 alone): the head is skipped and lane k
// takes p_k from probs_in[e][k]; the division, the arg-max and the stores are the very same instructions.
template <int NSPLIT, class RT>
__global__ __launch_bounds__(256) void infer_head_kernel(const float *__restrict__ hpart, const float *__restrict__ bfc,
                                                          const float *__restrict__ Wh, const float *__restrict__ bh,
                                                          const float *__restrict__ noise, uint64_t seed,
                                                          uint64_t counter, RT *logits_t, RT *values_t,
                                                          int *actions_t, int64_t *pinned, unsigned int *done_ctr,
                                                          long long ticket, int E, int H, int A,
                                                          const float *__restrict__ probs_in) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * 4 + wave;
  float hv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool heads = probs_in == nullptr; // workgroup-uniform
  if (heads)
    head_hidden<NSPLIT>(hpart, bfc, Wh, e, E, H, A, lane, hv);
  __syncthreads();
  if (e < E) {
    float zmine = 0.f; // lane a keeps logit a (a < A) / the value (a == A)
    for (int a = 0; heads && a <= A; ++a)
      head_dot(bh, hv, H, a, lane, zmine);
    const bool isact = lane < A;
    float sum;
    const float ex = softmax_term(zmine, isact, 1.0f, sum);
    const float q = exp1_noise(noise, seed, counter, e, A, lane);
    float pk = ex / sum; // softmax (train.cc:374)
    if (!heads)
      pk = isact ? probs_in[(size_t)e * A + lane] : 0.f;
    const float r = isact ? pk / q : -1.f; // p_k / q_k (train.cc:374-375)
    const int best = wave_argmax_first(r, lane);
    if (heads && isact)
      logits_t[(size_t)e * A + lane] = (RT)zmine;
    if (heads && lane == A)
      values_t[e] = (RT)zmine;
    if (lane == 0) {
      if (pinned)
        store_action(actions_t, pinned, e, best);
      else // (the stateless operator, the --profile mode that does not publish)
        actions_t[e] = best;
    }
  }
  if (done_ctr && pinned)
    publish_ticket(pinned, done_ctr, ticket, E);
}
void launch_infer_head(hipStream_t s, const float *hpart, const float *bfc, const float *Wh, const float *bh,
                       const float *noise, uint64_t seed, uint64_t counter, void *logits_t, void *values_t,
                       int *actions_t, int64_t *pinned, unsigned int *done_ctr, long long ticket, int E, int H, int A,
                       const float *probs_in, bool rt16) {
  const dim3 g((E + 3) / 4), b(256);
  const size_t sm = (size_t)(A + 1) * H * sizeof(float);
  if (rt16)
    hipLaunchKernelGGL((infer_head_kernel<FC_SPLITS, f16>), g, b, sm, s, hpart, bfc, Wh, bh, noise, seed, counter,
                       static_cast<f16 *>(logits_t), static_cast<f16 *>(values_t), actions_t, pinned, done_ctr, ticket, E,
                       H, A, probs_in);
  else
    hipLaunchKernelGGL((infer_head_kernel<FC_SPLITS, float>), g, b, sm, s, hpart, bfc, Wh, bh, noise, seed, counter,
                       static_cast<float *>(logits_t), static_cast<float *>(values_t), actions_t, pinned, done_ctr, ticket,
                       E, H, A, probs_in);
}

// ================================================================================================
// Head of the evaluation lanes (aleppo_eval_act; the reference has no evaluation loop - SB3's predict(deterministic) /
// EvalCallback, the epsilon-greedy evaluation of the DQN / PPO papers).  The forward half is infer_head_kernel's, call
// for call (act_head.hpp): at rule = SAMPLE with 1 / tau = 1 (an exact multiplication) a lane computes what an
// environment of aleppo_act computes, bit for bit.  One wave per lane; the rule is workgroup-uniform.  Outputs are
// always fp32 (they are not rollout planes).
//   GREEDY          r_k = z_k                                      -> first maximum
//   SAMPLE          r_k = p_k / q_k, p = softmax(z * inv_tau)      -> first maximum (multinomial via Exp(1) noise)
//   EPSILON_GREEDY  u < epsilon ? min((int)(w * A), A - 1) : the greedy action
// Built-in noise (noise == nullptr): Philox4x32-10 under the key the host derived from config.seed and the evaluation
// domain constant, counter words { n lo, n hi, lane, block } with n the evaluation counter; SAMPLE: block = action / 4,
// EPSILON_GREEDY: block = 0, words 0 and 1 (include/aleppo.h).
// The hand-off to the host is publish_ticket on the lanes' OWN pinned buffer and arrival counter.
// ================================================================================================
template <int NSPLIT>
__global__ __launch_bounds__(256) void eval_head_kernel(const float *__restrict__ hpart, const float *__restrict__ bfc,
                                                         const float *__restrict__ Wh, const float *__restrict__ bh,
                                                         const float *__restrict__ noise, uint64_t key, uint64_t counter,
                                                         int rule, float param, float *logits_o, float *values_o,
                                                         int *actions_o, int64_t *pinned, unsigned int *done_ctr,
                                                         long long ticket, int E, int H, int A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * 4 + wave;
  float hv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  head_hidden<NSPLIT>(hpart, bfc, Wh, e, E, H, A, lane, hv);
  __syncthreads();
  if (e < E) {
    float zmine = 0.f; // lane a keeps logit a (a < A) / the value (a == A)
    for (int a = 0; a <= A; ++a)
      head_dot(bh, hv, H, a, lane, zmine);
    const bool isact = lane < A;
    float r = isact ? zmine : -INFINITY; // GREEDY / EPSILON_GREEDY: the logit itself
    float u0 = 1.f, u1 = 0.f;            // EPSILON_GREEDY's (u, w)
    if (rule == ALEPPO_EVAL_SAMPLE) {    // workgroup-uniform
      float sum;
      const float ex = softmax_term(zmine, isact, param, sum); // param = 1 / tau
      const float q = exp1_noise(noise, key, counter, e, A, lane);
      const float pk = ex / sum;
      r = isact ? pk / q : -1.f;
    } else if (rule == ALEPPO_EVAL_EPSILON_GREEDY) { // (every lane holds the lane's two uniforms: no broadcast needed)
      if (noise) {
        u0 = noise[(size_t)e * 2];
        u1 = noise[(size_t)e * 2 + 1];
      } else {
        uint32_t c[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)e, 0u};
        philox4x32_10(c, (uint32_t)key, (uint32_t)(key >> 32));
        u0 = philox_unit(c[0]);
        u1 = philox_unit(c[1]);
      }
    }
    int best = wave_argmax_first(r, lane);
    if (rule == ALEPPO_EVAL_EPSILON_GREEDY && u0 < param) // param = epsilon
      best = min((int)(u1 * (float)A), A - 1);
    if (isact)
      logits_o[(size_t)e * A + lane] = zmine;
    if (lane == A)
      values_o[e] = zmine;
    if (lane == 0)
      store_action(actions_o, pinned, e, best);
  }
  publish_ticket(pinned, done_ctr, ticket, E);
}
void launch_eval_head(hipStream_t s, const float *hpart, const float *bfc, const float *Wh, const float *bh,
                      const float *noise, uint64_t key, uint64_t counter, int rule, float param, float *logits,
                      float *values, int *actions, int64_t *pinned, unsigned int *done_ctr, long long ticket, int L, int H,
                      int A) {
  const size_t sm = (size_t)(A + 1) * H * sizeof(float);
  hipLaunchKernelGGL((eval_head_kernel<FC_SPLITS>), dim3((L + 3) / 4), dim3(256), sm, s, hpart, bfc, Wh, bh, noise, key,
                     counter, rule, param, logits, values, actions, pinned, done_ctr, ticket, L, H, A);
}

// ================================================================================================
// Reward clamp + GAE + returns + masks + old log-probs in ONE pass: Buffer::get (buffer.cc:58-77),
// ai::gae::gae (gae.cc:49-79) and prepare_batch's normalize_logits (train.cc:272-283).
// Rollout scalars are time-major [T][E] so each wave reads 64 consecutive environments per slot
// (coalesced); one thread owns one environment and scans t = T-1..0.  Outputs are the env-major
// (n = e*T + t) training arrays the minibatch slices index (Q1, Q5).  The float op order of
// gae.cc:61-66 is pinned (fp contract off) so no fma contraction changes the rounding.
// ================================================================================================
__device__ __forceinline__ float gae_step(float r, float v, float nv, float last, float gamma, float gl, bool st,
                                          bool te, bool tr) {
#pragma clang fp contract(off) // keep the reference's separate mul / add roundings (no fma)
  const float t1 = gamma * nv;
  const float t2 = r + t1;
  const float boot = t2 - v;                                           // (r + g*nv) - v
  const float t3 = gl * last;
  float a = boot + t3;                                                 // running,   gae.cc:61-63
  if (st)
    a = 0.f;                                                           // start,     gae.cc:68-69
  if (te)
    a = r - v;                                                         // terminal,  gae.cc:64,70-71
  if (tr)
    a = boot;                                                          // truncated, gae.cc:65-66,72-73
  return a;
}

// One thread = one environment, scanning t = T-1 .. 0.  The scan itself is a short dependent chain; what costs is
// memory latency, so the inputs of 16 time steps are loaded together and the NEXT 16 are already in flight (second
// register set) while a chunk is processed.  A chunk is processed branch-free (all 16 steps valid, the flag check
// accumulates into a register): with per-step branches the compiler sinks every load into its step's block and each
// step then pays a full memory round trip behind the previous step's scattered stores (54 us for T = 128).
struct GaeChunk {
  static constexpr int CH = 16;
  float r[CH], v[CH];
  uint8_t te[CH], tr[CH], st[CH];
};
// The scan is ONE text with two entry points: gae_kernel (SCALED = false: the reference's clamp, or none) and
// gae_scaled_kernel (SCALED = true, ALEPPO_OPT_REWARD_SCALE: step 5 of aleppo.h in place of the clamp - every reward
// becomes min(max(r * s, -c), c) in fp32, s from the reward-scale state block, and the rewards the clip changed are
// counted).  Everything SCALED adds is behind `if constexpr`, so gae_kernel's instruction stream is what it was.
template <class RT, bool SCALED>
__device__ __forceinline__ void gae_scan(uint8_t *rec, size_t rb, const RT *__restrict__ values_tm, RT *adv_n, RT *ret_n,
                                         uint8_t *mask_n, int *err, int E, int T, float gamma, float lambda, int clamp,
                                         float rs_s, float rs_c, unsigned long long *rs_clipped) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E)
    return;
  constexpr int CH = GaeChunk::CH;
  const float gl = gamma * lambda;
  float last = 0.f, nv = (float)values_tm[(size_t)T * E + e];
  int bad = 0;
  [[maybe_unused]] unsigned int nclip = 0;
  auto step = [&](int t, float r, float v, bool bte, bool btr, bool bst) {
    float rc;
    if constexpr (SCALED) {
      const float p = r * rs_s;
      rc = fminf(fmaxf(p, -rs_c), rs_c);
      nclip += fabsf(p) > rs_c ? 1u : 0u;
      reinterpret_cast<float *>(rec + (size_t)t * rb)[e] = rc;
    } else {
      // buffer.cc:67 clamp_, in place (Buffer::get).  clamp == 0: ai::gae::gae alone (the stateless aleppo_gae
      // operator) - rewards are used as given and left untouched.
      rc = clamp ? fminf(fmaxf(r, -1.0f), 1.0f) : r;
      if (clamp)
        reinterpret_cast<float *>(rec + (size_t)t * rb)[e] = rc;
    }
    bad |= ((int)bte + (int)btr + (int)bst > 1) ? 1 : 0; // gae.cc:49-53
    const float a = gae_step(rc, v, nv, last, gamma, gl, bst, bte, btr);
    const size_t n = (size_t)e * T + t;
    adv_n[n] = (RT)a;        // (the recursion keeps the unrounded fp32 value)
    ret_n[n] = (RT)(a + v);  // buffer.cc:70-71
    mask_n[n] = bst ? 0 : 1; // buffer.cc:74
    last = a;
    nv = v;
  };
  auto load = [&](GaeChunk &c, int t1) { // steps t1-1 .. t1-CH, all valid
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int t = t1 - 1 - k;
      const uint8_t *fl = rec + (size_t)t * rb + 4 * (size_t)E;
      c.r[k] = reinterpret_cast<const float *>(rec + (size_t)t * rb)[e];
      c.v[k] = (float)values_tm[(size_t)t * E + e];
      c.te[k] = fl[e];
      c.tr[k] = fl[E + e];
      c.st[k] = fl[2 * E + e];
    }
  };
  auto process = [&](const GaeChunk &c, int t1) {
#pragma unroll
    for (int k = 0; k < CH; ++k)
      step(t1 - 1 - k, c.r[k], c.v[k], c.te[k] != 0, c.tr[k] != 0, c.st[k] != 0);
  };
  int t1 = T;
  for (int rem = T % CH; rem > 0; --rem) { // the ragged top of the horizon, one step at a time
    const int t = --t1;
    const uint8_t *fl = rec + (size_t)t * rb + 4 * (size_t)E;
    step(t, reinterpret_cast<const float *>(rec + (size_t)t * rb)[e], (float)values_tm[(size_t)t * E + e], fl[e] != 0,
         fl[E + e] != 0, fl[2 * E + e] != 0);
  }
  if (t1 > 0) { // t1 is a multiple of CH (uniform control flow: T is a kernel argument)
    GaeChunk ca, cb;
    load(ca, t1);
    while (true) {
      const bool more_b = t1 - CH > 0;
      if (more_b)
        load(cb, t1 - CH);
      process(ca, t1);
      if (!more_b)
        break;
      const bool more_a = t1 - 2 * CH > 0;
      if (more_a)
        load(ca, t1 - 2 * CH);
      process(cb, t1 - CH);
      if (!more_a)
        break;
      t1 -= 2 * CH;
    }
  }
  if (bad)
    *err = 1;
  if constexpr (SCALED) {
    if (nclip) // an integer vector atomic: the total does not depend on the order of arrival
      atomicAdd(rs_clipped, (unsigned long long)nclip);
  }
}
template <class RT>
__global__ __launch_bounds__(64) void gae_kernel(uint8_t *rec, size_t rb, const RT *__restrict__ values_tm, RT *adv_n,
                                                  RT *ret_n, uint8_t *mask_n, int *err, int E, int T, float gamma,
                                                  float lambda, int clamp) {
  gae_scan<RT, false>(rec, rb, values_tm, adv_n, ret_n, mask_n, err, E, T, gamma, lambda, clamp, 0.f, 0.f, nullptr);
}
// rs: the reward-scale state block (RS_SCALE: the float s, widened; RS_CLIPPED: the counter, zeroed by the second stage)
template <class RT>
__global__ __launch_bounds__(64) void gae_scaled_kernel(uint8_t *rec, size_t rb, const RT *__restrict__ values_tm,
                                                         RT *adv_n, RT *ret_n, uint8_t *mask_n, int *err, int E, int T,
                                                         float gamma, float lambda, double *rs, float clip) {
  gae_scan<RT, true>(rec, rb, values_tm, adv_n, ret_n, mask_n, err, E, T, gamma, lambda, 1, (float)rs[RS_SCALE], clip,
                     reinterpret_cast<unsigned long long *>(rs + RS_CLIPPED));
}
// the embarrassingly parallel part of prepare_batch (train.cc:272-283): old log-probs + actions, one thread
// per (t, e) slot, written env-major
template <class RT>
__global__ void oldlp_kernel(const RT *__restrict__ logits_tm, const int *__restrict__ actions_tm, RT *oldlp_n,
                             int *act_n, int E, int T, int A) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x; // time-major index t*E + e
  if (i >= (long)E * T)
    return;
  const int t = (int)(i / E), e = (int)(i - (long)t * E);
  const size_t n = (size_t)e * T + t;
  act_n[n] = actions_tm[i];
  const RT *z = logits_tm + i * A;
  float mx = (float)z[0];
  for (int k = 1; k < A; ++k)
    mx = fmaxf(mx, (float)z[k]);
  float s = 0.f;
  for (int k = 0; k < A; ++k)
    s += expf((float)z[k] - mx);
  const float lse = mx + logf(s);
  for (int k = 0; k < A; ++k)
    oldlp_n[n * A + k] = (RT)((float)z[k] - lse); // train.cc:279 normalize_logits
}
template <class RT>
static void launch_gae_t(hipStream_t s, uint8_t *step_rec, size_t rec_bytes, const void *values_tm, const void *logits_tm,
                         const int *actions_tm, void *adv_n, void *ret_n, void *oldlp_n, int *act_n, uint8_t *mask_n,
                         int *err, int E, int T, int A, float gamma, float lambda, bool clamp, double *rs,
                         float rs_clip) {
  if (logits_tm) // (the stateless aleppo_gae operator has no logits / actions)
    hipLaunchKernelGGL(oldlp_kernel<RT>, dim3((unsigned)(((long)E * T + 255) / 256)), dim3(256), 0, s,
                       static_cast<const RT *>(logits_tm), actions_tm, static_cast<RT *>(oldlp_n), act_n, E, T, A);
  if (rs)
    hipLaunchKernelGGL(gae_scaled_kernel<RT>, dim3((E + 63) / 64), dim3(64), 0, s, step_rec, rec_bytes,
                       static_cast<const RT *>(values_tm), static_cast<RT *>(adv_n), static_cast<RT *>(ret_n), mask_n,
                       err, E, T, gamma, lambda, rs, rs_clip);
  else
    hipLaunchKernelGGL(gae_kernel<RT>, dim3((E + 63) / 64), dim3(64), 0, s, step_rec, rec_bytes,
                       static_cast<const RT *>(values_tm), static_cast<RT *>(adv_n), static_cast<RT *>(ret_n), mask_n,
                       err, E, T, gamma, lambda, clamp ? 1 : 0);
}
void launch_gae(hipStream_t s, uint8_t *step_rec, size_t rec_bytes, const void *values_tm, const void *logits_tm,
                const int *actions_tm, void *adv_n, void *ret_n, void *oldlp_n, int *act_n, uint8_t *mask_n, int *err,
                int E, int T, int A, float gamma, float lambda, bool clamp, bool rt16) {
  if (rt16)
    launch_gae_t<f16>(s, step_rec, rec_bytes, values_tm, logits_tm, actions_tm, adv_n, ret_n, oldlp_n, act_n, mask_n, err,
                      E, T, A, gamma, lambda, clamp, nullptr, 0.f);
  else
    launch_gae_t<float>(s, step_rec, rec_bytes, values_tm, logits_tm, actions_tm, adv_n, ret_n, oldlp_n, act_n, mask_n,
                        err, E, T, A, gamma, lambda, clamp, nullptr, 0.f);
}
void launch_gae_scaled(hipStream_t s, uint8_t *step_rec, size_t rec_bytes, const void *values_tm, const void *logits_tm,
                       const int *actions_tm, void *adv_n, void *ret_n, void *oldlp_n, int *act_n, uint8_t *mask_n,
                       int *err, int E, int T, int A, float gamma, float lambda, double *rs, float clip, bool rt16) {
  if (rt16)
    launch_gae_t<f16>(s, step_rec, rec_bytes, values_tm, logits_tm, actions_tm, adv_n, ret_n, oldlp_n, act_n, mask_n, err,
                      E, T, A, gamma, lambda, true, rs, clip);
  else
    launch_gae_t<float>(s, step_rec, rec_bytes, values_tm, logits_tm, actions_tm, adv_n, ret_n, oldlp_n, act_n, mask_n,
                        err, E, T, A, gamma, lambda, true, rs, clip);
}

// optional advantage normalisation over unmasked samples (NOT in the reference, Q2; off by default).
// phase 0: stats[0..2] += {sum, sumsq, count} (one block, deterministic); phase 1: apply.
template <class RT>
__global__ __launch_bounds__(256) void adv_norm_kernel(RT *adv, const uint8_t *mask, float *stats, long n, int phase) {
  __shared__ float s4[4];
  if (phase == 0) {
    float s = 0.f, q = 0.f, c = 0.f;
    for (long i = threadIdx.x; i < n; i += 256)
      if (mask[i]) {
        const float a = (float)adv[i];
        s += a;
        q += a * a;
        c += 1.f;
      }
    s = block_sum_256(s, s4);
    q = block_sum_256(q, s4);
    c = block_sum_256(c, s4);
    if (threadIdx.x == 0) {
      stats[0] = s;
      stats[1] = q;
      stats[2] = c;
    }
  } else {
    const float c = stats[2];
    if (!(c > 0.f)) // every sample masked: nothing to normalise (and nothing enters the loss)
      return;
    const float mean = stats[0] / c;
    const float var = fmaxf((stats[1] - c * mean * mean) / fmaxf(c - 1.f, 1.f), 0.f);
    const float inv = 1.0f / (sqrtf(var) + 1e-8f);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
      adv[i] = (RT)(((float)adv[i] - mean) * inv);
  }
}
void launch_adv_norm(hipStream_t s, void *adv_n, const uint8_t *mask_n, float *stats, long n, int phase, bool rt16) {
  const dim3 g(phase == 0 ? 1 : (unsigned)((n + 255) / 256));
  if (rt16)
    hipLaunchKernelGGL(adv_norm_kernel<f16>, g, dim3(256), 0, s, static_cast<f16 *>(adv_n), mask_n, stats, n, phase);
  else
    hipLaunchKernelGGL(adv_norm_kernel<float>, g, dim3(256), 0, s, static_cast<float *>(adv_n), mask_n, stats, n, phase);
}

// boundary conversions of a rollout plane (aleppo_set_batch / aleppo_read_batch)
template <class S, class D> __global__ void cast_plane_kernel(const S *src, D *dst, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    dst[i] = (D)(float)src[i];
}
void launch_plane_to_float(hipStream_t s, const void *src, float *dst, long n, bool rt16) {
  const dim3 g((unsigned)std::min<long>((n + 255) / 256, 1024));
  if (rt16)
    hipLaunchKernelGGL((cast_plane_kernel<f16, float>), g, dim3(256), 0, s, static_cast<const f16 *>(src), dst, n);
  else
    hipLaunchKernelGGL((cast_plane_kernel<float, float>), g, dim3(256), 0, s, static_cast<const float *>(src), dst, n);
}
void launch_plane_from_float(hipStream_t s, const float *src, void *dst, long n, bool rt16) {
  const dim3 g((unsigned)std::min<long>((n + 255) / 256, 1024));
  if (rt16)
    hipLaunchKernelGGL((cast_plane_kernel<float, f16>), g, dim3(256), 0, s, src, static_cast<f16 *>(dst), n);
  else
    hipLaunchKernelGGL((cast_plane_kernel<float, float>), g, dim3(256), 0, s, src, static_cast<float *>(dst), n);
}

// unmasked-sample count per minibatch (losses.cc:19 masks.sum()); block per minibatch
__global__ __launch_bounds__(256) void mask_count_kernel(const uint8_t *mask, float *counts, long B) {
  __shared__ float s4[4];
  const uint8_t *m = mask + (size_t)blockIdx.x * B;
  float c = 0.f;
  for (long i = threadIdx.x; i < B; i += 256)
    c += m[i] ? 1.f : 0.f;
  c = block_sum_256(c, s4);
  if (threadIdx.x == 0)
    counts[blockIdx.x] = c;
}
void launch_mask_count(hipStream_t s, const uint8_t *mask_n, float *counts, long B, int M) {
  hipLaunchKernelGGL(mask_count_kernel, dim3(M), dim3(256), 0, s, mask_n, counts, B);
}

// ALEPPO_OPT_ADV_NORM_MINIBATCH: (n, S, Q) = count, sum and sum of squares of the unmasked advantages of one minibatch, in
// double (aleppo.h), block per minibatch.  Fixed order: thread t sums samples t, t + 256, ... in turn, then the block
// reduces with the same shuffle tree every time (block_sum_256).  a*a of a widened float is exact in double, so a
// contracted fma is too.
// advn_finalise: (mean_f, inv_f, std, 0) of aleppo.h from the (all-reduced) sums; n = 0: (0, 1, 0, 0)
__device__ __forceinline__ void advn_finalise(double n, double S, double Q, float *out) {
  if (!(n > 0.0)) {
    out[0] = 0.f;
    out[1] = 1.f;
    out[2] = 0.f;
    out[3] = 0.f;
    return;
  }
  const double mean = S / n;
  const double var = fmax(0.0, (Q - S * S / n) / fmax(n - 1.0, 1.0));
  const double sd = sqrt(var);
  out[0] = (float)mean;
  out[1] = (float)(1.0 / (sd + 1e-8));
  out[2] = (float)sd;
  out[3] = 0.f;
}
template <class RT>
__global__ __launch_bounds__(256) void advn_stats_kernel(const RT *__restrict__ adv, const uint8_t *__restrict__ mask,
                                                         long B, double *part, float *stats) {
  __shared__ double s4[4];
  const RT *a = adv + (size_t)blockIdx.x * B;
  const uint8_t *m = mask + (size_t)blockIdx.x * B;
  double n = 0.0, S = 0.0, Q = 0.0;
  for (long i = threadIdx.x; i < B; i += 256)
    if (m[i]) {
      const double x = (double)(float)a[i];
      n += 1.0;
      S += x;
      Q += x * x;
    }
  n = block_sum_256(n, s4);
  S = block_sum_256(S, s4);
  Q = block_sum_256(Q, s4);
  if (threadIdx.x == 0) {
    if (part) { // data parallel: the partial sums, all-reduced and then finalised by advn_finalise_kernel
      part[(size_t)blockIdx.x * 4 + 0] = n;
      part[(size_t)blockIdx.x * 4 + 1] = S;
      part[(size_t)blockIdx.x * 4 + 2] = Q;
      part[(size_t)blockIdx.x * 4 + 3] = 0.0;
    } else {
      advn_finalise(n, S, Q, stats + (size_t)blockIdx.x * 4);
    }
  }
}
__global__ __launch_bounds__(256) void advn_finalise_kernel(const double *part, float *stats, int nmb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nmb)
    advn_finalise(part[(size_t)i * 4], part[(size_t)i * 4 + 1], part[(size_t)i * 4 + 2], stats + (size_t)i * 4);
}
void launch_advn_stats(hipStream_t s, const void *adv, const uint8_t *mask, long B, int nmb, double *part, float *stats,
                       bool rt16) {
  if (rt16)
    hipLaunchKernelGGL(advn_stats_kernel<f16>, dim3(nmb), dim3(256), 0, s, static_cast<const f16 *>(adv), mask, B, part,
                       stats);
  else
    hipLaunchKernelGGL(advn_stats_kernel<float>, dim3(nmb), dim3(256), 0, s, static_cast<const float *>(adv), mask, B,
                       part, stats);
}
void launch_advn_finalise(hipStream_t s, const double *part, float *stats, int nmb) {
  hipLaunchKernelGGL(advn_finalise_kernel, dim3((unsigned)((nmb + 255) / 256)), dim3(256), 0, s, part, stats, nmb);
}

// ================================================================================================
// ALEPPO_F_BATCH_STATS (aleppo.h): count, sum and sum of squares of the stored values v, returns R, advantages a and of
// d = R - v over the unmasked samples of the batch, in double, in two stages whose order depends on the sample count only.
// Stage 1: workgroup b sums the samples [b * BSTAT_CHUNK, (b + 1) * BSTAT_CHUNK): thread t takes t, t + 256, ... in turn,
// then the block folds with the shuffle tree of block_sum_256.  x * x of a widened float is exact in double (a
// contracted fma is too); d is one rounded double subtraction of two widened floats.  The values of a rollout batch are
// time-major ([T+1][E], sample n = e*T + t sits at t*E + e: E > 0); those of a caller batch are sample-major (E == 0).
// REFRESH (aleppo_refresh_advantages): val0 is the collected plane next to the fresh one in val, and a partial grows by S
// and Q of d' = v - v0 and the maximum of |d'| (RSTAT_SUMS); everything it adds is behind `if constexpr`.
template <class RT, bool REFRESH>
__device__ __forceinline__ void bstat_partial(const RT *__restrict__ val, const RT *__restrict__ val0,
                                              const RT *__restrict__ ret, const RT *__restrict__ adv,
                                              const uint8_t *__restrict__ mask, long n, int E, int T,
                                              double *__restrict__ part) {
  __shared__ double s4[4];
  constexpr int SUMS = REFRESH ? RSTAT_SUMS - 1 : BSTAT_SUMS, REC = REFRESH ? RSTAT_SUMS : BSTAT_SUMS;
  const long i0 = (long)blockIdx.x * BSTAT_CHUNK;
  const long i1 = i0 + BSTAT_CHUNK < n ? i0 + BSTAT_CHUNK : n;
  double acc[SUMS];
  [[maybe_unused]] double mx = 0.0;
#pragma unroll
  for (int k = 0; k < SUMS; ++k)
    acc[k] = 0.0;
  for (long i = i0 + threadIdx.x; i < i1; i += 256)
    if (mask[i]) {
      const unsigned u = (unsigned)i; // (n <= E*T fits 32 bits: 32-bit division)
      const long iv = E > 0 ? (long)(u % (unsigned)T) * E + u / (unsigned)T : i;
      const double v = (double)(float)val[iv], r = (double)(float)ret[i], a = (double)(float)adv[i];
      const double d = r - v;
      acc[0] += 1.0;
      acc[1] += v;
      acc[2] += v * v;
      acc[3] += r;
      acc[4] += r * r;
      acc[5] += a;
      acc[6] += a * a;
      acc[7] += d;
      acc[8] += d * d;
      if constexpr (REFRESH) {
        const double dp = v - (double)(float)val0[iv];
        acc[9] += dp;
        acc[10] += dp * dp;
        mx = fmax(mx, fabs(dp));
      }
    }
#pragma unroll
  for (int k = 0; k < SUMS; ++k)
    acc[k] = block_sum_256(acc[k], s4);
  if constexpr (REFRESH) { // the maximum is order-free: the butterfly, then the four waves through LDS
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
      mx = fmax(mx, __shfl_xor(mx, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
      s4[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmax(fmax(s4[0], s4[1]), fmax(s4[2], s4[3]));
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < SUMS; ++k)
      part[(size_t)blockIdx.x * REC + k] = acc[k];
    if constexpr (REFRESH)
      part[(size_t)blockIdx.x * REC + SUMS] = mx;
  }
}
template <class RT>
__global__ __launch_bounds__(256) void bstat_partial_kernel(const RT *__restrict__ val, const RT *__restrict__ ret,
                                                            const RT *__restrict__ adv, const uint8_t *__restrict__ mask,
                                                            long n, int E, int T, double *__restrict__ part) {
  bstat_partial<RT, false>(val, nullptr, ret, adv, mask, n, E, T, part);
}
template <class RT>
__global__ __launch_bounds__(256) void rstat_partial_kernel(const RT *__restrict__ val, const RT *__restrict__ val0,
                                                            const RT *__restrict__ ret, const RT *__restrict__ adv,
                                                            const uint8_t *__restrict__ mask, long n, int E, int T,
                                                            double *__restrict__ part) {
  bstat_partial<RT, true>(val, val0, ret, adv, mask, n, E, T, part);
}
// The ten results of aleppo.h from the nine (all-reduced) sums: population variance max(0, Q / n - mean^2), without
// contraction so that every instance of this function rounds alike; n == 0: zeros and a NaN explained variance.
__device__ __forceinline__ void bstat_finalise(const double *sums, double *out) {
#pragma clang fp contract(off)
  const double n = sums[0];
  double var[4];
  out[ALEPPO_BS_COUNT] = n;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double S = sums[1 + 2 * k], Q = sums[2 + 2 * k];
    const double mean = n > 0.0 ? S / n : 0.0;
    var[k] = n > 0.0 ? fmax(0.0, Q / n - mean * mean) : 0.0;
    out[2 + 2 * k] = mean;
    out[3 + 2 * k] = sqrt(var[k]);
  }
  out[ALEPPO_BS_EXPLAINED_VARIANCE] = (n > 0.0 && var[1] > 0.0) ? 1.0 - var[3] / var[1] : __builtin_nan("");
}
// Stage 2, one workgroup: thread k < 9 adds sum k of the nblk partials in index order; then either the sums (for the
// all-reduce, finalised by bstat_finalise_kernel) or the results.
__global__ __launch_bounds__(64) void bstat_reduce_kernel(const double *__restrict__ part, int nblk, double *sums_out,
                                                          double *result) {
  __shared__ double sums[BSTAT_SUMS];
  if (threadIdx.x < BSTAT_SUMS) {
    double acc = 0.0;
    for (int b = 0; b < nblk; ++b)
      acc += part[(size_t)b * BSTAT_SUMS + threadIdx.x];
    sums[threadIdx.x] = acc;
    if (sums_out)
      sums_out[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0 && result)
    bstat_finalise(sums, result);
}
// aleppo_refresh_advantages' stage 2: thread k < 11 adds sum k of the nblk partials in index order, thread 11 takes the
// maximum; then the ten results of bstat_finalise and the mean, population std and maximum of d'
__global__ __launch_bounds__(64) void rstat_reduce_kernel(const double *__restrict__ part, int nblk, double *result) {
#pragma clang fp contract(off)
  __shared__ double sums[RSTAT_SUMS];
  if (threadIdx.x < RSTAT_SUMS) {
    const bool is_max = threadIdx.x == RSTAT_SUMS - 1;
    double acc = 0.0;
    for (int b = 0; b < nblk; ++b) {
      const double x = part[(size_t)b * RSTAT_SUMS + threadIdx.x];
      acc = is_max ? fmax(acc, x) : acc + x;
    }
    sums[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    bstat_finalise(sums, result);
    const double n = sums[0];
    const double mean = n > 0.0 ? sums[9] / n : 0.0;
    const double var = n > 0.0 ? fmax(0.0, sums[10] / n - mean * mean) : 0.0;
    result[ALEPPO_REFRESH_VALUE_CHANGE_MEAN] = mean;
    result[ALEPPO_REFRESH_VALUE_CHANGE_STD] = sqrt(var);
    result[ALEPPO_REFRESH_VALUE_CHANGE_MAXABS] = sums[RSTAT_SUMS - 1];
  }
}
__global__ __launch_bounds__(64) void bstat_finalise_kernel(const double *sums, double *result) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    bstat_finalise(sums, result);
}
int bstat_blocks(long n) { return (int)((n + BSTAT_CHUNK - 1) / BSTAT_CHUNK); }
void launch_bstat_partial(hipStream_t s, const void *val, const void *ret, const void *adv, const uint8_t *mask, long n,
                          int E, int T, double *part, bool rt16) {
  const dim3 grid((unsigned)bstat_blocks(n));
  if (rt16)
    hipLaunchKernelGGL(bstat_partial_kernel<f16>, grid, dim3(256), 0, s, static_cast<const f16 *>(val),
                       static_cast<const f16 *>(ret), static_cast<const f16 *>(adv), mask, n, E, T, part);
  else
    hipLaunchKernelGGL(bstat_partial_kernel<float>, grid, dim3(256), 0, s, static_cast<const float *>(val),
                       static_cast<const float *>(ret), static_cast<const float *>(adv), mask, n, E, T, part);
}
void launch_rstat_partial(hipStream_t s, const void *val, const void *val0, const void *ret, const void *adv,
                          const uint8_t *mask, long n, int E, int T, double *part, bool rt16) {
  const dim3 grid((unsigned)bstat_blocks(n));
  if (rt16)
    hipLaunchKernelGGL(rstat_partial_kernel<f16>, grid, dim3(256), 0, s, static_cast<const f16 *>(val),
                       static_cast<const f16 *>(val0), static_cast<const f16 *>(ret), static_cast<const f16 *>(adv), mask,
                       n, E, T, part);
  else
    hipLaunchKernelGGL(rstat_partial_kernel<float>, grid, dim3(256), 0, s, static_cast<const float *>(val),
                       static_cast<const float *>(val0), static_cast<const float *>(ret), static_cast<const float *>(adv),
                       mask, n, E, T, part);
}
void launch_rstat_reduce(hipStream_t s, const double *part, int nblk, double *result) {
  hipLaunchKernelGGL(rstat_reduce_kernel, dim3(1), dim3(64), 0, s, part, nblk, result);
}
void launch_bstat_reduce(hipStream_t s, const double *part, int nblk, double *sums, double *result) {
  hipLaunchKernelGGL(bstat_reduce_kernel, dim3(1), dim3(64), 0, s, part, nblk, sums, result);
}
void launch_bstat_finalise(hipStream_t s, const double *sums, double *result) {
  hipLaunchKernelGGL(bstat_finalise_kernel, dim3(1), dim3(64), 0, s, sums, result);
}

// ================================================================================================
// ALEPPO_OPT_REWARD_SCALE (aleppo.h): the running discounted return per environment, the count, sum and sum of squares of
// its samples over one rollout, and the merge into the running mean / variance that gives the scale s - all in double.
// Stage 1, rs_scan_kernel: one thread = one environment, scanning t = 0 .. T-1 over the time-major step records (a wave
// reads 64 consecutive environments per slot), with gae_kernel's loading discipline: the rewards and flags of 16 slots
// are loaded together, the next 16 are already in flight, and a chunk is processed branch-free (selects, no per-step
// branches: see the comment above GaeChunk for what the naive form costs).  G * gamma + r keeps its two roundings
// (contraction off), so the samples are the bits a host restatement in double gets.  The wave then folds (n, S, Q) with
// xor butterflies (the wave stage of block_sum_256) and writes one partial per workgroup.  The order of every addition
// is a function of (E, T) only.
// ================================================================================================
struct RsChunk {
  static constexpr int CH = 16;
  float r[CH];
  uint8_t te[CH], tr[CH], st[CH];
};
__device__ __forceinline__ void rs_step(double &G, double &n, double &S, double &Q, int &bad, double g, float r, bool te,
                                        bool tr, bool st) {
#pragma clang fp contract(off)
  bad |= ((int)te + (int)tr + (int)st > 1) ? 1 : 0; // gae.cc:49-53, as gae_kernel checks it
  const double x = G * g + (double)r;
  const bool live = !st; // an episode-start slot carries the stale reward: no sample, G untouched
  G = live ? x : G;
  n += live ? 1.0 : 0.0;
  S += live ? x : 0.0;
  Q += live ? x * x : 0.0;
  G = (live && (te || tr)) ? 0.0 : G;
}
__global__ __launch_bounds__(64) void rs_scan_kernel(const uint8_t *__restrict__ rec, size_t rb,
                                                     const double *__restrict__ g_in, double *__restrict__ g_out,
                                                     double *__restrict__ part, int *err, int E, int T, float gamma) {
  constexpr int CH = RsChunk::CH;
  const int e = blockIdx.x * 64 + threadIdx.x;
  double G = 0.0, n = 0.0, S = 0.0, Q = 0.0;
  if (e < E) {
    const double g = (double)gamma;
    int bad = 0;
    G = g_in[e];
    auto load = [&](RsChunk &c, int t0) { // slots t0 .. t0+CH-1, all valid
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        const uint8_t *row = rec + (size_t)(t0 + k) * rb;
        const uint8_t *fl = row + 4 * (size_t)E;
        c.r[k] = reinterpret_cast<const float *>(row)[e];
        c.te[k] = fl[e];
        c.tr[k] = fl[E + e];
        c.st[k] = fl[2 * E + e];
      }
    };
    auto process = [&](const RsChunk &c) {
#pragma unroll
      for (int k = 0; k < CH; ++k)
        rs_step(G, n, S, Q, bad, g, c.r[k], c.te[k] != 0, c.tr[k] != 0, c.st[k] != 0);
    };
    int t0 = 0;
    for (const int rem = T % CH; t0 < rem; ++t0) { // the ragged start of the horizon, one slot at a time
      const uint8_t *row = rec + (size_t)t0 * rb;
      const uint8_t *fl = row + 4 * (size_t)E;
      rs_step(G, n, S, Q, bad, g, reinterpret_cast<const float *>(row)[e], fl[e] != 0, fl[E + e] != 0,
              fl[2 * E + e] != 0);
    }
    if (t0 < T) { // T - t0 is a multiple of CH (uniform control flow: T is a kernel argument)
      RsChunk ca, cb;
      load(ca, t0);
      while (true) {
        const bool more_b = t0 + CH < T;
        if (more_b)
          load(cb, t0 + CH);
        process(ca);
        if (!more_b)
          break;
        const bool more_a = t0 + 2 * CH < T;
        if (more_a)
          load(ca, t0 + 2 * CH);
        process(cb);
        if (!more_a)
          break;
        t0 += 2 * CH;
      }
    }
    g_out[e] = G;
    if (bad)
      *err = 1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { // lanes past E hold zeros
    n += __shfl_xor(n, o, 64);
    S += __shfl_xor(S, o, 64);
    Q += __shfl_xor(Q, o, 64);
  }
  if (threadIdx.x == 0) {
    double *p = part + (size_t)blockIdx.x * 4;
    p[0] = n;
    p[1] = S;
    p[2] = Q;
    p[3] = 0.0;
  }
}
// gym's / SB3's RunningMeanStd.update_from_moments on the state block, then the scale; without contraction so that the
// direct and the all-reduced path round alike (a 1-rank communicator gives the single-GPU bits).  n == 0: the statistics
// stay.  A rollout whose flags overlap (*err set by the scan; aleppo_finish_rollout refuses it) changes nothing.
__device__ __forceinline__ void rs_merge(double *rs, double n, double S, double Q, const int *err) {
#pragma clang fp contract(off)
  if (*err)
    return;
  double count = rs[RS_COUNT], mean = rs[RS_MEAN], var = rs[RS_VAR];
  if (n > 0.0) {
    const double mean_b = S / n;
    const double var_b = fmax(0.0, Q / n - mean_b * mean_b);
    const double d = mean_b - mean, tot = count + n;
    mean = mean + d * n / tot;
    var = (var * count + var_b * n + d * d * count * n / tot) / tot;
    count = tot;
  }
  const float s = (float)(1.0 / sqrt(var + 1e-8));
  rs[RS_COUNT] = count;
  rs[RS_MEAN] = mean;
  rs[RS_VAR] = var;
  rs[RS_SCALE] = (double)s;
  rs[RS_BATCH_COUNT] = n;
  reinterpret_cast<unsigned long long *>(rs)[RS_CLIPPED] = 0ull; // gae_scaled_kernel counts from here
}
// Stage 2, one workgroup: thread k < 3 adds sum k of the partials in index order; then either the merge, or (sums_out:
// data parallel) the three sums for the all-reduce, merged by rs_finalise_kernel afterwards.
__global__ __launch_bounds__(64) void rs_reduce_kernel(const double *__restrict__ part, int nblk, double *sums_out,
                                                       double *rs, const int *err) {
  __shared__ double sums[3];
  if (threadIdx.x < 3) {
    double acc = 0.0;
    for (int b = 0; b < nblk; ++b)
      acc += part[(size_t)b * 4 + threadIdx.x];
    sums[threadIdx.x] = acc;
    if (sums_out)
      sums_out[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0 && !sums_out)
    rs_merge(rs, sums[0], sums[1], sums[2], err);
}
__global__ __launch_bounds__(64) void rs_finalise_kernel(const double *sums, double *rs, const int *err) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    rs_merge(rs, sums[0], sums[1], sums[2], err);
}
int rs_blocks(int E) { return (E + 63) / 64; }
void launch_rs_scan(hipStream_t s, const uint8_t *step_rec, size_t rec_bytes, const double *g_in, double *g_out,
                    double *part, int *err, int E, int T, float gamma) {
  hipLaunchKernelGGL(rs_scan_kernel, dim3(rs_blocks(E)), dim3(64), 0, s, step_rec, rec_bytes, g_in, g_out, part, err, E,
                     T, gamma);
}
void launch_rs_reduce(hipStream_t s, const double *part, int nblk, double *sums_out, double *rs, const int *err) {
  hipLaunchKernelGGL(rs_reduce_kernel, dim3(1), dim3(64), 0, s, part, nblk, sums_out, rs, err);
}
void launch_rs_finalise(hipStream_t s, const double *sums, double *rs, const int *err) {
  hipLaunchKernelGGL(rs_finalise_kernel, dim3(1), dim3(64), 0, s, sums, rs, err);
}

// ================================================================================================
// Per-epoch minibatch shuffling (ALEPPO_OPT_MINIBATCH_SHUFFLE; the permutation is specified in aleppo.h).  One thread per
// position i of epoch e = blockIdx.y: a four-round Feistel network on [0, 2^(2h)) walked until it lands in [0, N).  The
// small per-sample planes are gathered into the new order (coalesced writes; oldlp's A elements per sample go through
// LDS-held indices so that consecutive threads write consecutive elements).  The observations are NOT moved: the
// update's kernels read them through SampleMap::idx = order[e].
// ================================================================================================
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ uint32_t feistel4(uint32_t x, const uint32_t k[4], int h) {
  const uint32_t mask = (1u << h) - 1u;
  uint32_t L = x >> h, R = x & mask;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t t = R;
    R = L ^ (fmix32(R ^ k[r]) & mask);
    L = t;
  }
  return (L << h) | R;
}
template <class RT>
__global__ __launch_bounds__(256) void shuffle_gather_kernel(const uint32_t *__restrict__ rk, int h, long N, int A,
                                                             int32_t *order, const int *__restrict__ act_n,
                                                             const RT *__restrict__ oldlp_n, const RT *__restrict__ adv_n,
                                                             const RT *__restrict__ ret_n, const RT *__restrict__ val_n,
                                                             const uint8_t *__restrict__ mask_n, int *act_p, RT *oldlp_p,
                                                             RT *adv_p, RT *ret_p, RT *val_p, uint8_t *mask_p) {
  __shared__ int sj[256];
  const int e = blockIdx.y;
  const long i0 = (long)blockIdx.x * 256, i = i0 + threadIdx.x;
  const uint32_t k[4] = {rk[4 * e], rk[4 * e + 1], rk[4 * e + 2], rk[4 * e + 3]};
  const size_t row = (size_t)e * N;
  if (i < N) {
    uint32_t y = feistel4((uint32_t)i, k, h);
    while (y >= (uint32_t)N) // cycle-walking: the cycle through i returns to [0, N)
      y = feistel4(y, k, h);
    const long j = (long)y;
    sj[threadIdx.x] = (int)j;
    order[row + i] = (int32_t)j;
    act_p[row + i] = act_n[j];
    adv_p[row + i] = adv_n[j];
    ret_p[row + i] = ret_n[j];
    if (val_n) // ALEPPO_OPT_VALUE_CLIP: the old values travel with their samples
      val_p[row + i] = val_n[j];
    mask_p[row + i] = mask_n[j];
  }
  __syncthreads();
  const long cnt = min(256L, N - i0);
  for (long t = threadIdx.x; t < cnt * A; t += 256) {
    const long s = t / A, a = t - s * A;
    oldlp_p[(row + i0 + s) * A + a] = oldlp_n[(long)sj[s] * A + a];
  }
}
void launch_shuffle_gather(hipStream_t s, const uint32_t *rk, int h, long N, int epochs, int A, int32_t *order,
                           const int *act_n, const void *oldlp_n, const void *adv_n, const void *ret_n,
                           const void *val_n, const uint8_t *mask_n, int *act_p, void *oldlp_p, void *adv_p,
                           void *ret_p, void *val_p, uint8_t *mask_p, bool rt16) {
  const dim3 g((unsigned)((N + 255) / 256), (unsigned)epochs);
  if (rt16)
    hipLaunchKernelGGL(shuffle_gather_kernel<f16>, g, dim3(256), 0, s, rk, h, N, A, order, act_n,
                       static_cast<const f16 *>(oldlp_n), static_cast<const f16 *>(adv_n),
                       static_cast<const f16 *>(ret_n), static_cast<const f16 *>(val_n), mask_n, act_p,
                       static_cast<f16 *>(oldlp_p), static_cast<f16 *>(adv_p), static_cast<f16 *>(ret_p),
                       static_cast<f16 *>(val_p), mask_p);
  else
    hipLaunchKernelGGL(shuffle_gather_kernel<float>, g, dim3(256), 0, s, rk, h, N, A, order, act_n,
                       static_cast<const float *>(oldlp_n), static_cast<const float *>(adv_n),
                       static_cast<const float *>(ret_n), static_cast<const float *>(val_n), mask_n, act_p,
                       static_cast<float *>(oldlp_p), static_cast<float *>(adv_p), static_cast<float *>(ret_p),
                       static_cast<float *>(val_p), mask_p);
}

// ================================================================================================
// Split-K slab reduction -> flat gradient (fixed summation order => run-to-run deterministic).
// ================================================================================================
struct ReduceArgs {
  ReduceSeg seg[12];
  int cprefix[13]; // prefix of workgroups per segment
  int wide[12];    // segment runs the 16-byte path (1024 outputs per workgroup)
  int nseg;
};
// Two shapes of work in one launch, chosen per segment on the host:
//  * narrow (small n, many slabs - the conv wgrads): one workgroup per 64 consecutive outputs, thread
//    (o = tid&63, q = tid>>6) sums slabs q, q+4, ... and the four partials are combined in fixed order
//    -> 4x the memory-level parallelism of a serial scan;
//  * wide (the fc weight: 1.6 M outputs, <= 4 slabs): one workgroup per 1024 outputs, every thread sums a
//    float4 column with 16-byte loads, keeping the same four interleaved partial sums per output.
// Both give the value ((s0+s4+..) + (s1+s5+..)) + ((s2+..) + (s3+..)) -> identical bits, run-to-run deterministic.

// The narrow shape's sum of output j over S slabs of n floats, for a workgroup of 256 threads that owns 64 consecutive
// outputs: thread (o = tid & 63, q = tid >> 6) sums slabs q, q + 4, ... of its output j, then the four partials combine
// through LDS as (p0 + p1) + (p2 + p3).  Every thread of the workgroup calls it (one barrier); j >= n: 0.
__device__ __forceinline__ float slab_column_sum(const float *slab, int S, long n, long j, float (*part)[64]) {
  const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
  float acc = 0.f;
  if (j < n) {
    const float *p = slab + j;
#pragma unroll 4
    for (int k = q; k < S; k += 4)
      acc += p[(long)k * n];
  }
  part[q][o] = acc;
  __syncthreads();
  return (part[0][o] + part[1][o]) + (part[2][o] + part[3][o]);
}
__global__ __launch_bounds__(256) void reduce_slabs_kernel(ReduceArgs a, float *G) {
  __shared__ float part[4][64];
  int s = 0;
  while ((int)blockIdx.x >= a.cprefix[s + 1])
    ++s;
  const long n = a.seg[s].n;
  const int S = a.seg[s].S;
  if (a.wide[s]) { // workgroup-uniform
    const long j = ((long)((int)blockIdx.x - a.cprefix[s]) * 256 + threadIdx.x) * 4;
    if (j >= n)
      return;
    const float *p = a.seg[s].slab + j;
    float4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    int k = 0;
    for (; k + 4 <= S; k += 4) {
      float4 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        v[q] = *reinterpret_cast<const float4 *>(p + (long)(k + q) * n);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[q].x += v[q].x;
        acc[q].y += v[q].y;
        acc[q].z += v[q].z;
        acc[q].w += v[q].w;
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (k + q < S) {
        const float4 v = *reinterpret_cast<const float4 *>(p + (long)(k + q) * n);
        acc[q].x += v.x;
        acc[q].y += v.y;
        acc[q].z += v.z;
        acc[q].w += v.w;
      }
    float4 r;
    r.x = (acc[0].x + acc[1].x) + (acc[2].x + acc[3].x);
    r.y = (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y);
    r.z = (acc[0].z + acc[1].z) + (acc[2].z + acc[3].z);
    r.w = (acc[0].w + acc[1].w) + (acc[2].w + acc[3].w);
    *reinterpret_cast<float4 *>(G + a.seg[s].dst + j) = r;
    return;
  }
  const long j = (long)((int)blockIdx.x - a.cprefix[s]) * 64 + (threadIdx.x & 63);
  const float g = slab_column_sum(a.seg[s].slab, S, n, j, part);
  if (threadIdx.x < 64 && j < n)
    G[a.seg[s].dst + j] = g;
}
void launch_reduce_slabs(hipStream_t s, const ReduceSeg *segs, int nseg, float *G) {
  constexpr long wide_min = 1L << 18; // smallest segment that takes the 16-byte path
  ReduceArgs a;
  a.nseg = nseg;
  a.cprefix[0] = 0;
  for (int i = 0; i < nseg; ++i) {
    a.seg[i] = segs[i];
    const bool aligned = segs[i].n % 4 == 0 && segs[i].dst % 4 == 0 && ((uintptr_t)segs[i].slab & 15) == 0 &&
                         ((uintptr_t)G & 15) == 0;
    a.wide[i] = aligned && segs[i].n >= wide_min;
    a.cprefix[i + 1] = a.cprefix[i] + (int)(a.wide[i] ? (segs[i].n + 1023) / 1024 : (segs[i].n + 63) / 64);
  }
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3(a.cprefix[nseg]), dim3(256), 0, s, a, G);
}

// ================================================================================================
// clip_grad_norm_ (train.cc:12-46) + torch::optim::Adam (eps 1e-5, train.cc:360-362) in two kernels:
// per-block sum of squares, then every Adam block re-reduces the <=1024 partials in the same order
// (identical norm everywhere), scales by min(1, max_norm/(norm+1e-6)) and applies the update.  The
// bf16 compute copy of the weights is refreshed in the same pass.
// ================================================================================================
// Blocks [0, nmain) square G[0, n).  The blocks after them own the LAST gradient tensors (conv1 weight + bias, 64
// outputs per block) and either sum their split-K slabs first - the update's last slab reduce fused into this pass, one
// launch less on the serial tail of every minibatch - or, when the slabs were reduced before (data parallelism: the
// all-reduce needs G complete), read G.  Same partition and same summation order in both modes: identical partials.
struct SumsqTail {
  ReduceSeg seg[2]; // slab == nullptr: the tensor is already in G
  int chunks[2];    // 64-output chunks per tensor
};
__global__ __launch_bounds__(256) void sumsq_kernel(float *__restrict__ G, long n, float *partials, int nmain,
                                                    SumsqTail tail) {
  __shared__ float s4[4];
  __shared__ float part[4][64];
  float s = 0.f;
  const int blk = (int)blockIdx.x;
  if (blk < nmain) {
    const long per = (n + nmain - 1) / nmain;
    const long b = (long)blk * per, e = min(n, b + per);
    for (long i = b + threadIdx.x; i < e; i += 256)
      s += G[i] * G[i];
  } else {
    int c = blk - nmain, t = 0;
    if (c >= tail.chunks[0]) {
      c -= tail.chunks[0];
      t = 1;
    }
    const ReduceSeg sg = tail.seg[t];
    const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long j = (long)c * 64 + o;
    float g = 0.f;
    if (sg.slab) { // workgroup-uniform; reduce_slabs_kernel's narrow path
      const float sum = slab_column_sum(sg.slab, sg.S, sg.n, j, part);
      if (q == 0 && j < sg.n) {
        g = sum;
        G[sg.dst + j] = g;
      }
    } else if (q == 0 && j < sg.n) {
      g = G[sg.dst + j];
    }
    s = g * g;
  }
  s = block_sum_256(s, s4);
  if (threadIdx.x == 0)
    partials[blk] = s;
}
// One launch covers every block.  Splitting the pass - main blocks on the weight-gradient stream beside conv1 wgrad, tail
// blocks after the join - measured slower (454.7 vs 450.0 us per minibatch: the tail launch alone still costs 7.8 us and
// the join gap stays).
int launch_sumsq(hipStream_t s, float *G, long n_main, float *partials, int nblk_main, const ReduceSeg tail[2]) {
  SumsqTail t;
  for (int i = 0; i < 2; ++i) {
    t.seg[i] = tail[i];
    t.chunks[i] = (int)((tail[i].n + 63) / 64);
  }
  const int ntail = t.chunks[0] + t.chunks[1], nblk = nblk_main + ntail;
  hipLaunchKernelGGL(sumsq_kernel, dim3(nblk), dim3(256), 0, s, G, n_main, partials, nblk_main, t);
  return nblk; // partials written once every block has run
}

struct long4_ranges {
  long begin[4], len[4];
};
// One Adam step of one element (train.cc:42-44 clip scale always applied; torch::optim::Adam's update form)
struct AdamScalars {
  float coef, step_size, bc2_sqrt, beta1, beta2, omb1, omb2, eps;
};
struct AdamElement {
  float p, m, v;
};
// g: the raw gradient; m1, m2, p0: the element's moments and parameter before the step.  The one copy of the update's
// arithmetic: both paths of both entry points call it, so their bits agree by construction.  The three fused
// multiply-adds are WRITTEN OUT and contraction is off: m = fma(m1, beta1, fl(omb1 g)), v = fma(m2, beta2, fl(omb2 fl(g g))),
// p = fma(-step_size, fl(m / denom), p0).  These are the forms hipcc chose at every site of adam_kernel while the
// expressions were left to it; which product of a sum of two it fuses is its choice, and it chose the other one for v at
// 30 of 34 sites once this function was inlined through optimizer_step - one ulp in v, and a different run.
__device__ __forceinline__ AdamElement adam_element(float g, float m1, float m2, float p0, const AdamScalars &a) {
#pragma clang fp contract(off)
  g *= a.coef;
  const float m = __builtin_fmaf(m1, a.beta1, a.omb1 * g);
  const float v = __builtin_fmaf(m2, a.beta2, a.omb2 * (g * g));
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  return {__builtin_fmaf(-a.step_size, m / denom, p0), m, v};
}
// The dgrad-side weight layouts are TRANSPOSES of three weight tensors (W3d[c][(tap,oc)], W2d[class][c][(ab,oc)],
// WfcT[j][o]): the blocks that own those tensors walk them in 64-row tiles, write the updated weight to the compute copy
// in place and - through an LDS transpose, so that both sides are whole lines - to its transposed home.  (Until round 3
// two extra kernels re-read P on a side stream after every optimizer step: 28 us and 9.6 MB per step.)
struct AdamTiles {
  // tile t of tensor k: rows r0..r0+63 (row stride rs), cols c0..c0+cols-1 contiguous at src = off + r*rs + c;
  // transposed element (c, r) at dst + c*ds + r
  long off[3];      // Wfc, W3, W2 offsets in the flat vector
  int first[4];     // first tile index of each tensor (+ total)
  int H;
};
// ALEPPO_OPT_WEIGHT_DECAY / ALEPPO_OPT_ANCHOR_COEF (aleppo.h): the decoupled terms r = f_wd * p0 + f_an * (p0 - a) leave the
// parameter Adam produced, q.  They never pass through the clip or the moments.  The one copy of their arithmetic.
__device__ __forceinline__ float reg_element(float q, float p0, float a, float f_wd, float f_an) {
#pragma clang fp contract(off) // (as in adam_element: the one fused multiply-add is written out)
  const float r = __builtin_fmaf(f_wd, p0, f_an * (p0 - a));
  return q - r;
}
// The optimizer step, the body of both entry points below.  REG = false is adam_kernel as it always was: anchor and the
// two hyper slots are never read and no instruction of the decoupled terms exists in it.  REG = true (reg_step_kernel)
// also reads slots HYPER_WD / HYPER_ANCHOR and, where there is one, the anchor (nullptr: a reads as +0.0f, and f_an is 0).
// hpd: the device block of the hyper-parameter options (common.hpp HYPER_*): slot HYPER_MAX_NORM is the gradient-norm
// limit, a device value so that a captured update follows ALEPPO_OPT_MAX_GRAD_NORM
template <class T, bool REG>
__device__ __forceinline__ void optimizer_step(float *P, const float *G, float *M1, float *M2, T *Pc, T *WfcT, T *W3d,
                                               T *W2d, const AdamTiles &tl, long n_flat, const long4_ranges &fr,
                                               const float *partials, int nblk, const float *hpd, const float *sched,
                                               float beta1, float beta2, float eps, float *grad_norm_out,
                                               const float *anchor) { // (__restrict__: on the entry points' parameters)
  const float max_norm = hpd[HYPER_MAX_NORM];
  float f_wd = 0.f, f_an = 0.f;
  if constexpr (REG) {
    f_wd = hpd[HYPER_WD];
    f_an = hpd[HYPER_ANCHOR];
  }
  __shared__ float s4[4];
  __shared__ float tile[64][65];
  float s = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 256)
    s += partials[i];
  s = block_sum_256(s, s4);
  const float norm = sqrtf(s);
  float coef = max_norm / (norm + 1e-6f); // train.cc:39
  coef = fminf(coef, 1.0f);               // train.cc:40-41
  if (blockIdx.x == 0 && threadIdx.x == 0 && grad_norm_out)
    *grad_norm_out = norm;                // pre-clip norm is what the reference reports (Q9)
  // lr / (1 - beta1^t) and sqrt(1 - beta2^t) of THIS optimizer step: device scalars (a captured hipGraph of the update
  // follows the annealed rate and the step count; the reference's captured graph bakes both, train.h:163-195)
  const AdamScalars a{coef, sched[0], sched[1], beta1, beta2, 1.0f - beta1, 1.0f - beta2, eps};
  const int ntile = tl.first[3];
  if ((int)blockIdx.x < ntile) { // a 64-row tile of Wfc / W3 / W2
    const int t = blockIdx.x;
    long src;      // flat index of tile element (0, 0)
    int rs, rows, cols;
    T *dst;        // transposed element (c, r) at dst[c * ds + r]
    int ds;
    if (t < tl.first[1]) {          // Wfc[o][j] -> WfcT[j][o]: tile (o-block, j-block of 64; 3136 = 49 * 64)
      const int ob = t / 49, jb = t - ob * 49;
      rs = FC_IN;
      rows = min(64, tl.H - ob * 64);
      cols = 64;
      src = tl.off[0] + (long)ob * 64 * FC_IN + jb * 64;
      dst = WfcT + (long)jb * 64 * tl.H + ob * 64;
      ds = tl.H;
    } else if (t < tl.first[2]) {   // W3[oc][tap][c] -> W3d[c][tap][oc]: one tile per tap
      const int tap = t - tl.first[1];
      rs = 576;
      rows = 64;
      cols = 64;
      src = tl.off[1] + tap * 64;
      dst = W3d + tap * 64;
      ds = 576;
    } else {                        // W2[oc][(kh,kw)][c] -> W2d[class][c][(ab)][oc]: one 64 x 32 tile per (kh, kw)
      const int k = t - tl.first[2], kh = k >> 2, kw = k & 3;
      const int cls = (kh & 1) * 2 + (kw & 1), ab = (kh >> 1) * 2 + (kw >> 1);
      rs = 512;
      rows = 64;
      cols = 32;
      src = tl.off[2] + k * 32;
      dst = W2d + cls * (32 * 256) + ab * 64;
      ds = 256;
    }
    const int c = threadIdx.x & 63, r4 = threadIdx.x >> 6;
    if (c < cols) {
      // all 64 loads of a thread's 16 elements are issued before the first store (P / M1 / M2 are read and written through
      // the same pointers, so the compiler may not hoist them itself; a dependent load-compute-store chain per element made
      // this kernel latency-bound: 23 vs 13 us).  REG: the 16 anchor loads join the batch - issued after the first store
      // they would wait behind it, one more dependent round trip per element
      float g[16], m1[16], m2[16], p0[16], an[REG ? 16 : 1];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int r = r4 + 4 * k;
        const long i = src + (long)(r < rows ? r : 0) * rs + c;
        g[k] = G[i];
        m1[k] = M1[i];
        m2[k] = M2[i];
        p0[k] = P[i];
        if constexpr (REG)
          an[k] = anchor ? anchor[i] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int r = r4 + 4 * k;
        if (r < rows) {
          const long i = src + (long)r * rs + c;
          AdamElement e = adam_element(g[k], m1[k], m2[k], p0[k], a);
          if constexpr (REG)
            e.p = reg_element(e.p, p0[k], an[k], f_wd, f_an);
          M1[i] = e.m;
          M2[i] = e.v;
          P[i] = e.p;
          if (Pc)
            Pc[i] = (T)e.p;
          tile[r][c] = e.p;
        }
      }
    }
    __syncthreads();
    const int r = threadIdx.x & 63, c4 = threadIdx.x >> 6;
    if (r < rows)
      for (int cc = c4; cc < cols; cc += 4)
        dst[(long)cc * ds + r] = (T)tile[r][cc];
    return;
  }
  // everything else, flat: index k of the compacted space of the (at most four) ranges between the tiled tensors
  const long stride = (long)(gridDim.x - ntile) * 256;
  for (long k = (long)((int)blockIdx.x - ntile) * 256 + threadIdx.x; k < n_flat; k += stride) {
    long i = k;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (i < fr.len[q]) {
        i += fr.begin[q];
        break;
      }
      i -= fr.len[q];
    }
    float p0 = 0.f, an = 0.f;
    if constexpr (REG) { // (both loads before the stores below, like the tile path's)
      p0 = P[i];
      an = anchor ? anchor[i] : 0.f;
    }
    AdamElement e = adam_element(G[i], M1[i], M2[i], P[i], a);
    if constexpr (REG)
      e.p = reg_element(e.p, p0, an, f_wd, f_an);
    M1[i] = e.m;
    M2[i] = e.v;
    P[i] = e.p;
    if (Pc)
      Pc[i] = (T)e.p;
  }
}
template <class T>
__global__ __launch_bounds__(256) void adam_kernel(float *P, const float *__restrict__ G, float *M1, float *M2, T *Pc,
                                                    T *WfcT, T *W3d, T *W2d, AdamTiles tl, long n_flat,
                                                    long4_ranges fr, const float *__restrict__ partials, int nblk,
                                                    const float *__restrict__ hpd, const float *__restrict__ sched,
                                                    float beta1, float beta2, float eps, float *grad_norm_out) {
  optimizer_step<T, false>(P, G, M1, M2, Pc, WfcT, W3d, W2d, tl, n_flat, fr, partials, nblk, hpd, sched, beta1, beta2,
                           eps, grad_norm_out, nullptr);
}
// adam_kernel with the decoupled terms of ALEPPO_OPT_WEIGHT_DECAY / ALEPPO_OPT_ANCHOR_COEF: launched in its place by a
// context in which either coefficient is not zero, and by no other
template <class T>
__global__ __launch_bounds__(256) void reg_step_kernel(float *P, const float *__restrict__ G, float *M1, float *M2, T *Pc,
                                                        T *WfcT, T *W3d, T *W2d, AdamTiles tl, long n_flat,
                                                        long4_ranges fr, const float *__restrict__ partials, int nblk,
                                                        const float *__restrict__ hpd,
                                                        const float *__restrict__ sched, float beta1, float beta2,
                                                        float eps, float *grad_norm_out,
                                                        const float *__restrict__ anchor) {
  optimizer_step<T, true>(P, G, M1, M2, Pc, WfcT, W3d, W2d, tl, n_flat, fr, partials, nblk, hpd, sched, beta1, beta2, eps,
                          grad_norm_out, anchor);
}
void launch_adam(hipStream_t s, float *P, const float *G_in, float *M1, float *M2, void *Pc,
                 void *WfcT, void *W3d, void *W2d, const ParamLayout &L, int prec, const float *partials, int nblk,
                 const float *hpd, const float *sched, float beta1, float beta2, float eps, float *grad_norm_out,
                 bool reg, const float *anchor) {
  AdamTiles tl;
  tl.off[0] = (long)L.off[P_WFC];
  tl.off[1] = (long)L.off[P_W3];
  tl.off[2] = (long)L.off[P_W2];
  tl.H = L.H;
  tl.first[0] = 0;
  tl.first[1] = (L.H + 63) / 64 * 49;
  tl.first[2] = tl.first[1] + 9;
  tl.first[3] = tl.first[2] + 16;
  // flat ranges: [0, Wfc) heads, [bfc, W3), [b3, W2), [b2, end) (pads between tensors included: zero and stay zero)
  long4_ranges fr;
  const long edges[8] = {0, (long)L.off[P_WFC], (long)L.off[P_BFC], (long)L.off[P_W3], (long)L.off[P_B3],
                         (long)L.off[P_W2], (long)L.off[P_B2], (long)L.total()};
  long n_flat = 0;
  for (int q = 0; q < 4; ++q) {
    fr.begin[q] = edges[2 * q];
    fr.len[q] = edges[2 * q + 1] - edges[2 * q];
    n_flat += fr.len[q];
  }
  const int nb = tl.first[3] + (int)std::min<long>((n_flat + 255) / 256, 1024);
  if (reg) { // same grid, same arguments, and the anchor behind them
    if (prec == ALEPPO_BF16)
      hipLaunchKernelGGL(reg_step_kernel<bf16>, dim3(nb), dim3(256), 0, s, P, G_in, M1, M2, static_cast<bf16 *>(Pc),
                         static_cast<bf16 *>(WfcT), static_cast<bf16 *>(W3d), static_cast<bf16 *>(W2d), tl, n_flat, fr,
                         partials, nblk, hpd, sched, beta1, beta2, eps, grad_norm_out, anchor);
    else
      hipLaunchKernelGGL(reg_step_kernel<float>, dim3(nb), dim3(256), 0, s, P, G_in, M1, M2,
                         static_cast<float *>(nullptr), static_cast<float *>(WfcT), static_cast<float *>(W3d),
                         static_cast<float *>(W2d), tl, n_flat, fr, partials, nblk, hpd, sched, beta1, beta2, eps,
                         grad_norm_out, anchor);
    return;
  }
  if (prec == ALEPPO_BF16)
    hipLaunchKernelGGL(adam_kernel<bf16>, dim3(nb), dim3(256), 0, s, P, G_in, M1, M2,
                       static_cast<bf16 *>(Pc), static_cast<bf16 *>(WfcT), static_cast<bf16 *>(W3d),
                       static_cast<bf16 *>(W2d), tl, n_flat, fr, partials, nblk, hpd, sched, beta1, beta2, eps,
                       grad_norm_out);
  else
    hipLaunchKernelGGL(adam_kernel<float>, dim3(nb), dim3(256), 0, s, P, G_in, M1, M2,
                       static_cast<float *>(nullptr), static_cast<float *>(WfcT), static_cast<float *>(W3d),
                       static_cast<float *>(W2d), tl, n_flat, fr, partials, nblk, hpd, sched, beta1, beta2, eps,
                       grad_norm_out);
}

__global__ void cast_params_kernel(const float *P, bf16 *Pc, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    Pc[i] = (bf16)P[i];
}
void launch_cast_params(hipStream_t s, const float *P, void *Pc, long n) {
  hipLaunchKernelGGL(cast_params_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 2048)), dim3(256), 0, s, P,
                     static_cast<bf16 *>(Pc), n);
}

// dgrad-side weight copies: W3d[c][(kh,kw,oc)], W2d[class][c][(a,b,oc)], WfcT[j][o]   (all in T)
template <class T> __global__ void pack_conv_dgrad_kernel(const float *W3, const float *W2, T *W3d, T *W2d) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 64 * 576) {
    const int c = i / 576, rem = i - c * 576, tap = rem >> 6, oc = rem & 63;
    W3d[i] = (T)W3[oc * 576 + tap * 64 + c];
  } else if (i < 64 * 576 + 4 * 32 * 256) {
    const int k = i - 64 * 576;
    const int cls = k / (32 * 256), c = (k / 256) % 32, rem = k & 255, ab = rem >> 6, oc = rem & 63;
    const int kh = (cls >> 1) + 2 * (ab >> 1), kw = (cls & 1) + 2 * (ab & 1);
    W2d[k] = (T)W2[oc * 512 + (kh * 4 + kw) * 32 + c];
  }
}
template <class T> __global__ void transpose_cast_kernel(const float *in, T *out, int R, int C) { // out[C][R]
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32x8
  for (int k = ty; k < 32; k += 8)
    if (r0 + k < R && c0 + tx < C)
      tile[k][tx] = in[(size_t)(r0 + k) * C + c0 + tx];
  __syncthreads();
  for (int k = ty; k < 32; k += 8)
    if (c0 + k < C && r0 + tx < R)
      out[(size_t)(c0 + k) * R + r0 + tx] = (T)tile[tx][k];
}
void launch_pack_dgrad(hipStream_t s, const float *P, const ParamLayout &L, void *W2d, void *W3d, void *WfcT,
                       int prec) {
  const int n = 64 * 576 + 4 * 32 * 256;
  const dim3 tg((FC_IN + 31) / 32, (L.H + 31) / 32);
  if (prec == ALEPPO_BF16) {
    hipLaunchKernelGGL(pack_conv_dgrad_kernel<bf16>, dim3((n + 255) / 256), dim3(256), 0, s, P + L.off[P_W3],
                       P + L.off[P_W2], static_cast<bf16 *>(W3d), static_cast<bf16 *>(W2d));
    hipLaunchKernelGGL(transpose_cast_kernel<bf16>, tg, dim3(256), 0, s, P + L.off[P_WFC], static_cast<bf16 *>(WfcT),
                       L.H, FC_IN);
  } else {
    hipLaunchKernelGGL(pack_conv_dgrad_kernel<float>, dim3((n + 255) / 256), dim3(256), 0, s, P + L.off[P_W3],
                       P + L.off[P_W2], static_cast<float *>(W3d), static_cast<float *>(W2d));
    hipLaunchKernelGGL(transpose_cast_kernel<float>, tg, dim3(256), 0, s, P + L.off[P_WFC],
                       static_cast<float *>(WfcT), L.H, FC_IN);
  }
}

// masked sums of the per-sample metric arrays (log_data's masked means, train.cc:163-210): block per (epoch, mb).
// Record [mi][8]: the sums of fields 0-4 (total, clipped, value, entropy, ratio), the count, then the sums of fields 5-6
// (approx-KL, clip fraction)
// kle: the exact-KL plane of ALEPPO_OPT_KL_PENALTY ([mi][B], like one field of ps), summed into slot 8; nullptr: 0 there
__global__ __launch_bounds__(256) void metrics_reduce_kernel(const float *ps, size_t field_stride, const uint8_t *mask_n,
                                                              long B, int M, const float *kle, float *out) {
  __shared__ float s4[4];
  const int mi = blockIdx.x, mb = mi % M;
  const uint8_t *m = mask_n + (size_t)mb * B;
  float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, cnt = 0.f, kacc = 0.f;
  for (long i = threadIdx.x; i < B; i += 256)
    if (m[i]) {
      cnt += 1.f;
#pragma unroll
      for (int f = 0; f < 7; ++f)
        acc[f] += ps[f * field_stride + (size_t)mi * B + i];
      if (kle)
        kacc += kle[(size_t)mi * B + i];
    }
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    const float v = block_sum_256(acc[f], s4);
    if (threadIdx.x == 0)
      out[mi * METRIC_REC + f] = v;
  }
  cnt = block_sum_256(cnt, s4);
  if (threadIdx.x == 0)
    out[mi * METRIC_REC + 5] = cnt;
#pragma unroll
  for (int f = 5; f < 7; ++f) {
    const float v = block_sum_256(acc[f], s4);
    if (threadIdx.x == 0)
      out[mi * METRIC_REC + 1 + f] = v;
  }
  if (kle) // (uniform: the whole workgroup takes the branch)
    kacc = block_sum_256(kacc, s4);
  if (threadIdx.x == 0)
    out[mi * METRIC_REC + 8] = kacc;
}
void launch_metrics_reduce(hipStream_t s, const float *ps, size_t field_stride, const uint8_t *mask_n, long B, int M,
                           int epochs, float *out, const float *kle) {
  hipLaunchKernelGGL(metrics_reduce_kernel, dim3(epochs * M), dim3(256), 0, s, ps, field_stride, mask_n, B, M, kle,
                     out);
}

// ================================================================================================
// Boundary-only layout conversions (parity dumps / caller-supplied batches; not on the hot path).
// ================================================================================================
__global__ void obs_unpack_kernel(const uint32_t *obs, uint8_t *out, SampleMap map) { // -> NCHW u8 [n][4][7056]
  const long n = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= FRAME_PIX)
    return;
  const uint32_t w = obs[(n / map.TP) * map.s1 + (n % map.TP) * map.s0 + map.base + i];
  uint8_t *o = out + (size_t)n * 4 * FRAME_PIX + i;
  o[0] = w & 255u;
  o[FRAME_PIX] = (w >> 8) & 255u;
  o[2 * FRAME_PIX] = (w >> 16) & 255u;
  o[3 * FRAME_PIX] = w >> 24;
}
__global__ void obs_pack_kernel(const uint8_t *in, uint32_t *obs, SampleMap map) {
  const long n = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= FRAME_PIX)
    return;
  const uint8_t *p = in + (size_t)n * 4 * FRAME_PIX + i;
  obs[(n / map.TP) * map.s1 + (n % map.TP) * map.s0 + map.base + i] =
      (uint32_t)p[0] | ((uint32_t)p[FRAME_PIX] << 8) | ((uint32_t)p[2 * FRAME_PIX] << 16) |
      ((uint32_t)p[3 * FRAME_PIX] << 24);
}
void launch_obs_unpack(hipStream_t s, const uint32_t *obs, uint8_t *out, long nsamp, SampleMap map) {
  hipLaunchKernelGGL(obs_unpack_kernel, dim3((FRAME_PIX + 255) / 256, (unsigned)nsamp), dim3(256), 0, s, obs, out, map);
}
void launch_obs_pack(hipStream_t s, const uint8_t *in, uint32_t *obs, long nsamp, SampleMap map) {
  hipLaunchKernelGGL(obs_pack_kernel, dim3((FRAME_PIX + 255) / 256, (unsigned)nsamp), dim3(256), 0, s, in, obs, map);
}

// [T][E][inner] (elements of `elem` bytes, row pitch src_pitch bytes per t) -> [E][T][inner]
__global__ void transpose_tm_kernel(const uint8_t *src, size_t src_pitch, uint8_t *dst, int E, int T, int inner,
                                    int elem) {
  const long total = (long)E * T * inner;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int k = (int)(i % inner);
    const long et = i / inner;
    const int t = (int)(et % T), e = (int)(et / T);
    const uint8_t *s = src + (size_t)t * src_pitch + ((size_t)e * inner + k) * elem;
    uint8_t *d = dst + (size_t)i * elem;
    for (int b = 0; b < elem; ++b)
      d[b] = s[b];
  }
}
void launch_transpose_tm_pitched(hipStream_t s, const void *src_tm, size_t pitch, void *dst_em, int E, int T, int inner,
                                 int elem) {
  hipLaunchKernelGGL(transpose_tm_kernel, dim3(256), dim3(256), 0, s, static_cast<const uint8_t *>(src_tm), pitch,
                     static_cast<uint8_t *>(dst_em), E, T, inner, elem);
}

// action/value heads only (aleppo_forward): one wave per row
__global__ __launch_bounds__(256) void heads_fwd_kernel(const float *__restrict__ h, const float *__restrict__ Wh,
                                                         const float *__restrict__ bh, float *logits, float *values,
                                                         long n, int H, int A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long r = (long)blockIdx.x * 4 + wave;
  if (r >= n)
    return;
  for (int a = 0; a <= A; ++a) {
    float s = 0.f;
    for (int j = lane; j < H; j += 64)
      s += h[(size_t)r * H + j] * Wh[(size_t)a * H + j];
    s = wave_sum(s);
    if (lane == 0) {
      if (a < A)
        logits[r * A + a] = s + bh[a];
      else
        values[r] = s + bh[a];
    }
  }
}
void launch_heads_fwd(hipStream_t s, const float *h, const float *Wh, const float *bh, float *logits, float *values,
                      long n, int H, int A) {
  hipLaunchKernelGGL(heads_fwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, h, Wh, bh, logits, values, n, H,
                     A);
}

__global__ void logsoftmax_rows_kernel(const float *in, float *out, long rows, int A) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows)
    return;
  const float *z = in + r * A;
  float mx = z[0];
  for (int k = 1; k < A; ++k)
    mx = fmaxf(mx, z[k]);
  float s = 0.f;
  for (int k = 0; k < A; ++k)
    s += expf(z[k] - mx);
  const float lse = mx + logf(s);
  for (int k = 0; k < A; ++k)
    out[r * A + k] = z[k] - lse;
}
void launch_logsoftmax_rows(hipStream_t s, const float *in, float *out, long rows, int A) {
  hipLaunchKernelGGL(logsoftmax_rows_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, in, out, rows, A);
}

// ================================================================================================
// Stateless operators of the reference's free functions (parity tests).
// ================================================================================================
// vision.cc:8-32 interpolate(mode=area) 210x160 -> 84x84, float in / float out
__global__ void area_resize_kernel(const float *in, float *out) {
  const long n = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= FRAME_PIX)
    return;
  const int i = pix / 84, j = pix - i * 84;
  const int y0 = (i * RAW_H) / 84, y1 = ((i + 1) * RAW_H + 83) / 84, x0 = (j * RAW_W) / 84,
            x1 = ((j + 1) * RAW_W + 83) / 84;
  const float *src = in + (size_t)n * RAW_H * RAW_W;
  float s = 0.f;
  for (int y = y0; y < y1; ++y)
    for (int x = x0; x < x1; ++x)
      s += src[y * RAW_W + x];
  out[(size_t)n * FRAME_PIX + pix] = s / (float)((y1 - y0) * (x1 - x0));
}
void launch_area_resize(hipStream_t s, const float *in, float *out, long n) {
  hipLaunchKernelGGL(area_resize_kernel, dim3((FRAME_PIX + 255) / 256, (unsigned)n), dim3(256), 0, s, in, out);
}
// vision.cc:51,71-84
__global__ void rgb_to_gray_kernel(const float *in, float *out) {
  const long n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= FRAME_PIX)
    return;
  const float *s = in + (size_t)n * 3 * FRAME_PIX + p;
  {
#pragma clang fp contract(off)
    const float a = s[0] * 0.2125f, b = s[FRAME_PIX] * 0.7154f, c = s[2 * FRAME_PIX] * 0.0721f;
    out[(size_t)n * FRAME_PIX + p] = (a + b) + c;
  }
}
void launch_rgb_to_gray(hipStream_t s, const float *in, float *out, long n) {
  hipLaunchKernelGGL(rgb_to_gray_kernel, dim3((FRAME_PIX + 255) / 256, (unsigned)n), dim3(256), 0, s, in, out);
}

// ================================================================================================
// aleppo_state_digest (the definition is in aleppo.h): D(tag, w) = sum_i splitmix64(splitmix64(tag) ^ (i << 32 | w_i))
// over the EXPORTED representation, computed from the private layouts in place.  One bandwidth-bound pass: every thread
// takes 16-byte loads in a grid-stride loop, maps each word to its index in the exported order, and keeps a 64-bit sum;
// a workgroup folds its sums (wave shuffles, then LDS) and adds them to the section's word with ONE 64-bit integer
// atomic.  Integer addition mod 2^64 commutes, so the grid and the order of arrival do not show in the result.
// Everything is only read; the four words of `out` are the only stores.
// ================================================================================================
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned long long digest_term(unsigned long long tagkey, uint32_t i, uint32_t w) {
  return splitmix64(tagkey ^ (((unsigned long long)i << 32) | w));
}
// internal parameter layout -> libtorch parameters() index (the inverse of params_to_internal, api_core.hip): tensor k
// holds `size` elements from internal offset `off`; element j = (oc, kk, c) of a [oc][KK][C] weight is exported at
// base + (oc * C + c) * KK + kk (C = KK = 1: a plain copy); the stacked heads split at `split` (action rows | value row)
struct DigestSeg {
  uint32_t off, size, base, C, KK, split, base2;
};
struct DigestLayout {
  DigestSeg seg[P_COUNT];
  uint32_t groups; // 16-byte groups of the padded flat vector
};
__global__ __launch_bounds__(256) void digest_learner_kernel(const u32x4 *__restrict__ P, const u32x4 *__restrict__ M1,
                                                              const u32x4 *__restrict__ M2, DigestLayout L,
                                                              unsigned long long step, unsigned long long *out) {
  __shared__ unsigned long long s4[4];
  const unsigned long long k1 = splitmix64(1), k2 = splitmix64(2), k3 = splitmix64(3);
  unsigned long long ap = 0, am = 0;
  for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < L.groups; g += gridDim.x * 256u) {
    const uint32_t i0 = g * 4u;
    DigestSeg sg = L.seg[0]; // (selects on constant indices: the argument stays in scalar registers)
#pragma unroll
    for (int q = 1; q < P_COUNT; ++q) // (tensors start 64-float aligned: a group never straddles two)
      if (i0 >= L.seg[q].off)
        sg = L.seg[q];
    const uint32_t j0 = i0 - sg.off;
    if (j0 >= sg.size) // alignment pad: not part of the exported state
      continue;
    const u32x4 p = P[g], m = M1[g], v = M2[g];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t j = j0 + e;
      if (j < sg.size) {
        uint32_t ref;
        if (j >= sg.split)
          ref = sg.base2 + (j - sg.split);
        else {
          const uint32_t c = j % sg.C, r = j / sg.C, kk = r % sg.KK, oc = r / sg.KK;
          ref = sg.base + (oc * sg.C + c) * sg.KK + kk;
        }
        ap += digest_term(k1, ref, p[e]);
        am += digest_term(k2, ref, m[e]) + digest_term(k3, ref, v[e]);
      }
    }
  }
  ap = block_sum_256(ap, s4);
  am = block_sum_256(am, s4);
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0)
      am += splitmix64(splitmix64(4) ^ step);
    atomicAdd(out + ALEPPO_DG_PARAMS, ap);
    atomicAdd(out + ALEPPO_DG_OPTIMIZER, am);
  }
}
// the stacks of slot `slot`: the packed word of a pixel IS s[e * 7056 + p] of the definition
__global__ __launch_bounds__(256) void digest_rollout_kernel(const uint32_t *__restrict__ obs, int slots, int slot, int E,
                                                              unsigned long long counter, unsigned long long *out) {
  __shared__ unsigned long long s4[4];
  constexpr uint32_t GPE = FRAME_PIX / 4; // 16-byte groups per environment
  const unsigned long long k5 = splitmix64(5);
  const uint32_t groups = (uint32_t)E * GPE;
  unsigned long long a = 0;
  for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < groups; g += gridDim.x * 256u) {
    const uint32_t e = g / GPE, q = g - e * GPE;
    const u32x4 w = *reinterpret_cast<const u32x4 *>(obs + ((size_t)e * slots + slot) * FRAME_PIX + q * 4u);
    const uint32_t i = e * (uint32_t)FRAME_PIX + q * 4u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      a += digest_term(k5, i + k, w[k]);
  }
  a = block_sum_256(a, s4);
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0)
      a += splitmix64(splitmix64(6) ^ counter);
    atomicAdd(out + ALEPPO_DG_ROLLOUT, a);
  }
}
// (count, mean, var) of the state block and the E running returns, each double as its low then its high word
__global__ __launch_bounds__(256) void digest_rs_kernel(const double *__restrict__ blk, const double *__restrict__ g, int E,
                                                         unsigned long long *out) {
  __shared__ unsigned long long s4[4];
  const unsigned long long k7 = splitmix64(7);
  unsigned long long a = 0;
  for (int d = threadIdx.x; d < 3 + E; d += 256) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d < 3 ? blk[d] : g[d - 3]);
    a += digest_term(k7, 2u * d, (uint32_t)b) + digest_term(k7, 2u * d + 1u, (uint32_t)(b >> 32));
  }
  a = block_sum_256(a, s4);
  if (threadIdx.x == 0)
    atomicAdd(out + ALEPPO_DG_REWARD_SCALE, a);
}
void launch_state_digest(hipStream_t s, const float *P, const float *M1, const float *M2, const ParamLayout &L,
                         int64_t step, const uint32_t *obs, int slots, int slot, int E, uint64_t counter,
                         const double *rs_blk, const double *rs_g, unsigned long long *out) {
  DigestLayout dl{};
  const uint32_t H = (uint32_t)L.H, A = (uint32_t)L.A;
  // reference offsets: c1w c1b c2w c2b c3w c3b fcw fcb aw ab vw vb
  const uint32_t r_b1 = 32 * 256, r_w2 = r_b1 + 32, r_b2 = r_w2 + 64 * 512, r_w3 = r_b2 + 64, r_b3 = r_w3 + 64 * 576,
                 r_fc = r_b3 + 64, r_bfc = r_fc + H * FC_IN, r_aw = r_bfc + H, r_ab = r_aw + A * H, r_vw = r_ab + A,
                 r_vb = r_vw + H;
  auto seg = [&](ParamId id, uint32_t base, uint32_t C, uint32_t KK, uint32_t split = ~0u, uint32_t base2 = 0) {
    dl.seg[id] = DigestSeg{(uint32_t)L.off[id], (uint32_t)L.size[id], base, C, KK, split, base2};
  };
  seg(P_WH, r_aw, 1, 1, A * H, r_vw);
  seg(P_BH, r_ab, 1, 1, A, r_vb);
  seg(P_WFC, r_fc, 64, 49);
  seg(P_BFC, r_bfc, 1, 1);
  seg(P_W3, r_w3, 64, 9);
  seg(P_B3, r_b3, 1, 1);
  seg(P_W2, r_w2, 32, 16);
  seg(P_B2, r_b2, 1, 1);
  seg(P_W1, 0, 4, 64);
  seg(P_B1, r_b1, 1, 1);
  dl.groups = (uint32_t)(L.total() / 4);
  // one 16-byte group per thread up to 2048 workgroups (8 per CU), a grid-stride loop beyond
  auto grid = [](uint32_t groups) { return dim3(std::min<uint32_t>((groups + 255u) / 256u, 2048u)); };
  hipMemsetAsync(out, 0, ALEPPO_DIGEST_COUNT * sizeof(unsigned long long), s);
  hipLaunchKernelGGL(digest_learner_kernel, grid(dl.groups), dim3(256), 0, s, reinterpret_cast<const u32x4 *>(P),
                     reinterpret_cast<const u32x4 *>(M1), reinterpret_cast<const u32x4 *>(M2), dl,
                     (unsigned long long)step, out);
  hipLaunchKernelGGL(digest_rollout_kernel, grid((uint32_t)E * (FRAME_PIX / 4)), dim3(256), 0, s, obs, slots, slot, E,
                     (unsigned long long)counter, out);
  hipLaunchKernelGGL(digest_rs_kernel, dim3(1), dim3(256), 0, s, rs_blk, rs_g, E, out);
}
} // namespace aleppo
