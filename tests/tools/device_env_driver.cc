// device_env_driver - runs trainer/emulator.hpp itself on scripted actions and dumps what every slot produced, for
// tests/test_device_env_ref.py (which pins tests/device_env_ref.py against it); and runs the plain-C++ half of
// csrc/env_synth.hpp (the game logic and per-pixel renderers the device kernel is made of) next to it, failing on the
// first difference.  Host only; no GPU, no HIP.
//   device_env_driver <raw 0|1> <max_steps> <max_return> <E> <T> <seed_base> <actions.bin int32 [T][E]> <out.bin>
// out.bin, per slot: frames [E][frame_bytes], rewards f32 [E], terminated / truncated / start-at-entry / game_over u8 [E],
// episode return f32 [E], episode length u32 [E], game return f32 [E], game length u32 [E] (0: none ended); then the
// final aleppo_env_state [E].
//   device_env_driver sweep <raw 0|1>
// renders hand-made states (every ball position, the paddle at both ends, every brick phase) with the header's render() and
// with env_synth.hpp's per-pixel functions, and fails on the first difference.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>
#define private public // (the sweep calls SyntheticAtari::render on states no scripted run reaches; the standard headers are in already)
#include "../../trainer/emulator.hpp"
#undef private
#include "../../ale-libtorch-ppo_amd/csrc/env_synth.hpp"

struct Fields { // SyntheticAtari::visit's order
  aleppo_env_state *s;
  void operator()(uint64_t &rng, int &lives, int &paddle, int &bx, int &by, int &px, int &py, int &dx, int &dy, int &bricks,
                  uint64_t &steps, float &ret) {
    s->rng = rng, s->lives = lives, s->paddle = paddle, s->ball_x = bx, s->ball_y = by, s->prev_x = px, s->prev_y = py;
    s->dx = dx, s->dy = dy, s->bricks = bricks, s->steps = steps, s->episode_return = ret;
  }
};

static bool same_pixels(const aleppo_env_state &s, bool raw, const uint8_t *want, std::vector<uint8_t> &pix) {
  bool ok = true;
  if (raw) {
    for (int k = 0; k < 2; ++k) {
      const aleppo::EnvRawRects r = aleppo::env_raw_rects(s, k);
      for (int y = 0; y < 210; ++y)
        for (int x = 0; x < 160; ++x) {
          const uint32_t v = aleppo::env_pixel_raw(r, x, y);
          pix[((size_t)k * 210 + y) * 160 + x] = (uint8_t)v;
          ok = ok && (v == 0 || aleppo::env_raw_row_live(r, y)); // (the kernel stores zeros for a row that is not live)
        }
    }
  } else {
    for (int y = 0; y < 84; ++y)
      for (int x = 0; x < 84; ++x)
        pix[(size_t)y * 84 + x] = (uint8_t)aleppo::env_pixel_84(s, x, y);
  }
  return ok && std::memcmp(pix.data(), want, pix.size()) == 0;
}
static int sweep(bool raw) {
  const size_t fb = SyntheticAtari::frame_bytes(raw);
  std::vector<uint8_t> want(fb), pix(fb);
  SyntheticAtari env(0, 1000, -1.f, 4, raw);
  long n = 0;
  for (int paddle : {4, 5, 41, 78, 79})
    for (int bricks = 0; bricks < 5; ++bricks)
      for (int by = 0; by < 84; by += (paddle == 4 ? 1 : 7))
        for (int bx = 0; bx < 84; ++bx) {
          aleppo_env_state s{};
          s.paddle = env.paddle_ = paddle;
          s.bricks = env.bricks_ = bricks;
          s.ball_x = env.ball_x_ = bx, s.ball_y = env.ball_y_ = by;
          s.prev_x = env.prev_x_ = 83 - bx, s.prev_y = env.prev_y_ = (by * 5 + 3) % 84;
          env.render(want.data());
          if (!same_pixels(s, raw, want.data(), pix)) {
            std::fprintf(stderr, "render differs: paddle %d bricks %d ball %d,%d\n", paddle, bricks, bx, by);
            return 1;
          }
          ++n;
        }
  std::printf("sweep ok: %ld states\n", n);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && std::string(argv[1]) == "sweep")
    return sweep(std::atoi(argv[2]) != 0);
  if (argc != 9) {
    std::cerr << "usage: device_env_driver raw max_steps max_return E T seed_base actions.bin out.bin\n";
    return 2;
  }
  const bool raw = std::atoi(argv[1]) != 0;
  const size_t max_steps = std::strtoull(argv[2], nullptr, 10);
  const float max_return = std::strtof(argv[3], nullptr);
  const size_t E = std::strtoull(argv[4], nullptr, 10), T = std::strtoull(argv[5], nullptr, 10);
  const uint64_t seed_base = std::strtoull(argv[6], nullptr, 10);
  std::vector<int32_t> script(E * T);
  {
    std::ifstream f(argv[7], std::ios::binary);
    if (!f.read(reinterpret_cast<char *>(script.data()), (std::streamsize)(script.size() * 4))) {
      std::cerr << "cannot read " << argv[7] << "\n";
      return 2;
    }
  }
  std::ofstream out(argv[8], std::ios::binary | std::ios::trunc);
  const size_t fb = SyntheticAtari::frame_bytes(raw);
  EnvSet set(E);
  std::vector<uint8_t> frames(E * fb);
  std::vector<int64_t> actions(E);
  set.frames = frames.data();
  set.frame_bytes = fb;
  set.num_actions = 4;
  set.actions = actions.data();
  for (size_t i = 0; i < E; ++i)
    set.envs.emplace_back(seed_base + i, max_steps, max_return, 4, raw);
  // the trainer-side state of collect() (TrainerState)
  std::vector<uint8_t> term(E, 0), trunc(E, 0), game_over(E, 0);
  std::vector<float> rewards(E, 0.f), ep_ret(E, 0.f), game_ret(E, 0.f);
  std::vector<uint64_t> ep_len(E, 0), game_len(E, 0);
  auto snapshot = [&](size_t i) {
    aleppo_env_state s{};
    Fields f{&s};
    set.envs[i].visit(f);
    s.start = set.start[i], s.game_over = game_over[i], s.reward = rewards[i];
    s.ep_ret = ep_ret[i], s.game_ret = game_ret[i], s.ep_len = ep_len[i], s.game_len = game_len[i];
    return s;
  };
  std::vector<aleppo_env_state> mine(E); // env_synth.hpp's copy of the environments
  for (size_t i = 0; i < E; ++i)
    mine[i] = snapshot(i);
  auto put = [&](const void *p, size_t n) { out.write(static_cast<const char *>(p), (std::streamsize)n); };
  std::vector<uint8_t> pix(fb);
  for (size_t t = 0; t < T; ++t) {
    for (size_t i = 0; i < E; ++i)
      actions[i] = script[t * E + i];
    const std::vector<uint8_t> start_at_entry = set.start;
    std::vector<uint8_t> go_step(E, 0);
    std::vector<float> l_ep_ret(E, 0.f), l_game_ret(E, 0.f);
    std::vector<uint32_t> l_ep_len(E, 0), l_game_len(E, 0);
    for (size_t i = 0; i < E; ++i)
      set.step(i);
    for (size_t i = 0; i < E; ++i) // collect(): rollout.cc:214-226
      if (!set.start[i]) {
        const StepOut &o = set.results[i];
        rewards[i] = o.reward, term[i] = o.terminated, trunc[i] = o.truncated, game_over[i] = o.game_over;
        go_step[i] = o.game_over;
        ep_ret[i] += o.reward, ep_len[i]++, game_ret[i] += o.reward, game_len[i]++;
      }
    put(frames.data(), frames.size());
    put(rewards.data(), E * 4);
    put(term.data(), E);
    put(trunc.data(), E);
    put(start_at_entry.data(), E);
    put(go_step.data(), E);
    for (size_t i = 0; i < E; ++i) { // rollout.cc:239-265
      if (set.results[i].terminated || set.results[i].truncated) {
        set.start[i] = 1;
        term[i] = trunc[i] = 0;
        l_ep_ret[i] = ep_ret[i], l_ep_len[i] = (uint32_t)ep_len[i];
        ep_ret[i] = 0, ep_len[i] = 0;
        if (game_over[i]) {
          l_game_ret[i] = game_ret[i], l_game_len[i] = (uint32_t)game_len[i];
          game_ret[i] = 0, game_len[i] = 0;
        }
      } else if (set.start[i]) {
        set.start[i] = 0;
      }
    }
    put(l_ep_ret.data(), E * 4);
    put(l_ep_len.data(), E * 4);
    put(l_game_ret.data(), E * 4);
    put(l_game_len.data(), E * 4);
    // env_synth.hpp on the same slot: records, log entries, state and every pixel
    for (size_t i = 0; i < E; ++i) {
      const aleppo::EnvSlotOut o = aleppo::env_slot(mine[i], (int)actions[i], max_steps, max_return);
      const aleppo_env_state want = snapshot(i);
      bool ok = std::memcmp(&want, &mine[i], sizeof(want)) == 0 && o.start == start_at_entry[i] &&
                std::memcmp(&o.reward, &rewards[i], 4) == 0 && o.term == set.results[i].terminated &&
                o.trunc == set.results[i].truncated && std::memcmp(&o.ep_ret, &l_ep_ret[i], 4) == 0 &&
                o.ep_len == l_ep_len[i] && std::memcmp(&o.game_ret, &l_game_ret[i], 4) == 0 && o.game_len == l_game_len[i];
      ok = ok && same_pixels(mine[i], raw, &frames[i * fb], pix);
      if (!ok) {
        std::fprintf(stderr, "env_synth.hpp differs from emulator.hpp at slot %zu environment %zu\n", t, i);
        return 1;
      }
    }
  }
  for (size_t i = 0; i < E; ++i) {
    const aleppo_env_state s = snapshot(i);
    put(&s, sizeof(s));
  }
  out.flush();
  return out ? 0 : 2;
}
