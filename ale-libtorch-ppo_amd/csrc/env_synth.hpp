// env_synth.hpp - the device-resident synthetic environment (include/aleppo.h: aleppo_env_open / aleppo_env_rollout).
// The specification is trainer/emulator.hpp read literally (SyntheticAtari::reset / step / next / render, EnvSet::step) plus
// the slot bookkeeping of the trainer's collect(); the functions below restate it on one aleppo_env_state and compute a
// frame's pixels analytically.  They are plain C++ (ENV_HD is empty outside hipcc), so a host program can run them
// against emulator.hpp itself; env_step_kernel at the end is the only device-only part.
#pragma once
#include "../../include/aleppo.h"
#include <stdint.h>
#ifdef __HIPCC__
#define ENV_HD __host__ __device__ __forceinline__
#else
#define ENV_HD inline
#endif

namespace aleppo {

// what one slot of one environment hands to the rollout: the step record's entries and the episode log's
struct EnvSlotOut {
  float reward;                  // recorded reward (a start slot: the stale one)
  uint8_t term, trunc, start;    // recorded flags; start = the flag at ENTRY of the slot
  float ep_ret, game_ret;        // the episode / game that ended in this slot ...
  uint32_t ep_len, game_len;     // ... 0: none did
};

ENV_HD uint64_t env_next(aleppo_env_state &s) { // SyntheticAtari::next
  s.rng ^= s.rng << 13;
  s.rng ^= s.rng >> 7;
  s.rng ^= s.rng << 17;
  return s.rng;
}

// EnvSet::step + the per-environment body of collect()'s two loops, on one environment
ENV_HD EnvSlotOut env_slot(aleppo_env_state &s, int action, uint64_t max_steps, float max_return) {
  EnvSlotOut o;
  o.start = s.start;
  bool terminated = false, truncated = false;
  if (s.start) { // SyntheticAtari::reset: a full reset only after game over
    if (s.lives == 0) {
      s.lives = 5;
      s.steps = 0;
      s.episode_return = 0.f;
      s.bricks = 0;
    }
    s.ball_x = 42;
    s.ball_y = 60;
    s.prev_x = s.ball_x;
    s.prev_y = s.ball_y;
    s.dx = (env_next(s) & 1) ? 1 : -1;
    s.dy = -1;
  } else { // SyntheticAtari::step
    float reward = 0.f;
    s.paddle += (action == 2 ? 3 : action == 3 ? -3 : 0);
    s.paddle = s.paddle < 4 ? 4 : s.paddle > 79 ? 79 : s.paddle;
    for (int k = 0; k < 4; ++k) {
      s.prev_x = s.ball_x;
      s.prev_y = s.ball_y;
      s.ball_x += s.dx * 2;
      s.ball_y += s.dy * 2;
      if (s.ball_x <= 1 || s.ball_x >= 82)
        s.dx = -s.dx;
      if (s.ball_y <= 20) {
        s.dy = 1;
        reward += (float)(1 + 3 * (s.bricks % 3 == 2));
        ++s.bricks;
      }
      if (s.ball_y >= 78) {
        const int d = s.ball_x - s.paddle;
        if ((d < 0 ? -d : d) <= 8 || (env_next(s) % 3) == 0)
          s.dy = -1;
        else {
          --s.lives;
          terminated = true;
          break;
        }
      }
    }
    s.steps += 4; // (also after the break)
    s.episode_return += reward;
    bool game_over = s.lives == 0;
    if (!terminated && (s.steps >= max_steps || (max_return > 0 && s.episode_return >= max_return))) {
      truncated = true;
      s.lives = 0;
      game_over = true;
    }
    // collect(): rollout.cc:214-226
    s.reward = reward;
    s.game_over = game_over;
    s.ep_ret += reward;
    s.ep_len++;
    s.game_ret += reward;
    s.game_len++;
  }
  o.reward = s.reward;
  o.term = terminated;
  o.trunc = truncated;
  o.ep_ret = o.game_ret = 0.f;
  o.ep_len = o.game_len = 0;
  if (terminated || truncated) { // rollout.cc:239-265
    s.start = 1;
    o.ep_ret = s.ep_ret;
    o.ep_len = (uint32_t)s.ep_len;
    s.ep_ret = 0.f;
    s.ep_len = 0;
    if (s.game_over) {
      o.game_ret = s.game_ret;
      o.game_len = (uint32_t)s.game_len;
      s.game_ret = 0.f;
      s.game_len = 0;
    }
  } else if (s.start) {
    s.start = 0;
  }
  return o;
}

// ---- render, one pixel at a time: what the memset + overdraw of SyntheticAtari::render leaves at (x, y)
// 84x84: brick rows coloured by the PIXEL row's y / 3, the paddle over them, the ball over everything
ENV_HD uint32_t env_pixel_84(const aleppo_env_state &s, int x, int y) {
  uint32_t v = 0;
  if (y >= 8 && y < 20)
    v = ((uint32_t)(x / 6 + y / 3 + s.bricks) & 3u) * 50u + 60u;
  if ((y == 80 || y == 81) && x >= s.paddle - 6 && x <= s.paddle + 6)
    v = 200;
  if (y >= s.ball_y && y < s.ball_y + 2 && x >= s.ball_x && x < s.ball_x + 2)
    v = 236;
  return v;
}
// What one raw frame's pixels are tested against: rect(x0, x1, y0, y1) of render() covers the pixel rows
// [y0 * 210 / 84, y1 * 210 / 84) and columns [x0 * 160 / 84, x1 * 160 / 84), the divisions truncating toward zero as C's do
// (the paddle's left edge can be negative)
struct EnvRawRects {
  int pad_x0, pad_x1;             // paddle: rows 200..204
  int ball_x0, ball_x1, ball_y0, ball_y1;
  int bricks;
};
ENV_HD EnvRawRects env_raw_rects(const aleppo_env_state &s, int k) { // k = 0: the ball where it was one emulator frame ago
  EnvRawRects r;
  r.pad_x0 = (s.paddle - 6) * 160 / 84;
  r.pad_x1 = (s.paddle + 7) * 160 / 84;
  const int bx = k == 0 ? s.prev_x : s.ball_x, by = k == 0 ? s.prev_y : s.ball_y;
  r.ball_x0 = bx * 160 / 84;
  r.ball_x1 = (bx + 2) * 160 / 84;
  r.ball_y0 = by * 210 / 84;
  r.ball_y1 = (by + 2) * 210 / 84;
  r.bricks = s.bricks;
  return r;
}
// a pixel row that no rectangle touches is all zero
ENV_HD bool env_raw_row_live(const EnvRawRects &r, int y) {
  return (y >= 20 && y < 50) || (y >= 200 && y < 205) || (y >= r.ball_y0 && y < r.ball_y1);
}
ENV_HD uint32_t env_pixel_raw(const EnvRawRects &r, int x, int y) {
  uint32_t v = 0;
  if (y >= 20 && y < 50) {
    // brick block (i, j): columns [floor(80 i / 7), floor(80 (i + 1) / 7)), rows [floor((40 + 15 j) / 2), ...) - the
    // 84-grid rectangles x = 6 i, y = 8 + 3 j of render(); whole blocks are coloured by the block's y0 / 3 = 2 + j
    const int i = (7 * x + 6) / 80, j = (2 * y - 39) / 15;
    v = (((uint32_t)(i + 2 + j + r.bricks) & 3u) * 50u + 60u) & ~1u;
  }
  if (y >= 200 && y < 205 && x >= r.pad_x0 && x < r.pad_x1)
    v = 200;
  if (y >= r.ball_y0 && y < r.ball_y1 && x >= r.ball_x0 && x < r.ball_x1)
    v = 236;
  return v;
}

#ifdef __HIPCC__
typedef __attribute__((ext_vector_type(4))) unsigned int env_u32x4;
constexpr int ENV_RAW_PARTS = 4;
// the frame of environment e from its state s, shared out over gridDim.y workgroups: all 256 lanes of each store
// 16 bytes at a time (env_step_kernel below, and eval_env_step_kernel of env_eval.hpp)
template <bool RAW> __device__ __forceinline__ void env_render(uint8_t *__restrict__ frames, int e, const aleppo_env_state &s) {
  const int tid = threadIdx.x;
  if (RAW) {
    constexpr int ROW16 = 160 / 16, FRAME16 = 210 * ROW16; // 16-byte stores per row / per frame
    env_u32x4 *dst = reinterpret_cast<env_u32x4 *>(frames + (size_t)e * (2 * 210 * 160));
    const EnvRawRects r0 = env_raw_rects(s, 0), r1 = env_raw_rects(s, 1);
    for (int c = blockIdx.y * 256 + tid; c < 2 * FRAME16; c += 256 * gridDim.y) {
      const int k = c >= FRAME16, q = c - k * FRAME16, y = q / ROW16, x0 = (q - y * ROW16) * 16;
      const EnvRawRects &r = k ? r1 : r0;
      env_u32x4 v = {0u, 0u, 0u, 0u};
      if (env_raw_row_live(r, y)) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          uint32_t word = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b)
            word |= env_pixel_raw(r, x0 + 4 * w + b, y) << (8 * b);
          v[w] = word;
        }
      }
      dst[c] = v;
    }
  } else {
    constexpr int FRAME16 = 84 * 84 / 16; // 441
    env_u32x4 *dst = reinterpret_cast<env_u32x4 *>(frames + (size_t)e * (84 * 84));
    for (int c = blockIdx.y * 256 + tid; c < FRAME16; c += 256 * gridDim.y) {
      env_u32x4 v;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int p = c * 16 + 4 * w + b, y = p / 84;
          word |= env_pixel_84(s, p - y * 84, y) << (8 * b);
        }
        v[w] = word;
      }
      dst[c] = v;
    }
  }
}
// ================================================================================================
// One agent step of every environment and its frame.  Grid (E, parts): environment e is blockIdx.x, and its frame is
// shared out over `parts` workgroups (ENV_RAW_PARTS for a raw pair, whose 67 KB of stores would otherwise run on one CU per
// environment; 1 for an 84x84 frame).  The game logic is a few dozen uniform integer operations: every lane of every part
// computes it redundantly from the state of the previous slot (in) - no LDS broadcast, no barrier - and lane 0 of part 0
// writes the new state to the OTHER state array (out: the two alternate, so no lane can read what has already been
// written), the slot's step record entries and the episode-log entries.  Then all lanes render: each byte of the frame is
// computed from (paddle, ball, previous ball, bricks) and written exactly once, 16 at a time; a raw row of 160 bytes is
// ten such stores, so a store never crosses a row.
// rec: the device step record of this slot { float r[E]; u8 term[E]; u8 trunc[E]; u8 start[E] }; log_*: row t of the
// four [T][E] planes; actions: the int32 actions the acting head wrote for this slot.
// ================================================================================================
template <bool RAW>
__global__ __launch_bounds__(256) void env_step_kernel(const aleppo_env_state *__restrict__ in, aleppo_env_state *__restrict__ out,
                                                        const int *__restrict__ actions, uint8_t *__restrict__ frames,
                                                        uint8_t *__restrict__ rec, float *__restrict__ log_ep_ret,
                                                        uint32_t *__restrict__ log_ep_len, float *__restrict__ log_game_ret,
                                                        uint32_t *__restrict__ log_game_len, int E, uint64_t max_steps,
                                                        float max_return) {
  const int e = blockIdx.x, tid = threadIdx.x;
  aleppo_env_state s = in[e];
  const EnvSlotOut o = env_slot(s, actions[e], max_steps, max_return);
  if (tid == 0 && blockIdx.y == 0) {
    out[e] = s;
    reinterpret_cast<float *>(rec)[e] = o.reward;
    rec[4 * (size_t)E + e] = o.term;
    rec[5 * (size_t)E + e] = o.trunc;
    rec[6 * (size_t)E + e] = o.start;
    log_ep_ret[e] = o.ep_ret;
    log_ep_len[e] = o.ep_len;
    log_game_ret[e] = o.game_ret;
    log_game_len[e] = o.game_len;
  }
  env_render<RAW>(frames, e, s);
}
#endif

} // namespace aleppo
