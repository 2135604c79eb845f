// Synthetic Atari-shaped emulator (stands in for the ALE wrapper chain) and the environment set the workers step
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

struct StepOut {
  float reward = 0.f;
  bool terminated = false, truncated = false, game_over = false;
};
class SyntheticAtari {
public:
  // raw = true: the emulator hands over what ALE itself produces - the last TWO 210x160 palette-code frames of the skip
  // window - and the gray LUT, the 84x84 resize and the 2-frame max (environment.cc:48-55, resize.cc:34-41,
  // max_and_skip.cc:33-42) run on the device (ALEPPO_FRAMES_RAW_PAIR); raw = false: one finished 84x84 gray frame.
  SyntheticAtari(uint64_t seed, size_t max_steps, float max_return, size_t actions, bool raw = false)
      : rng_(seed * 0x9E3779B97F4A7C15ull + 12345), max_steps_(max_steps), max_return_(max_return), actions_(actions),
        raw_(raw) {}
  static size_t frame_bytes(bool raw) { return raw ? 2 * 210 * 160 : 84 * 84; }
  // FireReset / EpisodeLife semantics: a full reset only after game over, otherwise continue with the next life
  void reset(uint8_t *frame) {
    if (lives_ == 0) {
      lives_ = 5;
      steps_ = 0;
      episode_return_ = 0.f;
      bricks_ = 0;
    }
    ball_x_ = 42;
    ball_y_ = 60;
    prev_x_ = ball_x_;
    prev_y_ = ball_y_;
    dx_ = (next() & 1) ? 1 : -1;
    dy_ = -1;
    render(frame);
  }
  StepOut step(int action, uint8_t *frame) {
    StepOut o;
    paddle_ += (action == 2 ? 3 : action == 3 ? -3 : 0); // NOOP FIRE RIGHT LEFT like Breakout's minimal set
    paddle_ = std::clamp(paddle_, 4, 79);
    for (int k = 0; k < 4; ++k) { // frame_skip emulator frames per agent step
      prev_x_ = ball_x_;
      prev_y_ = ball_y_;
      ball_x_ += dx_ * 2;
      ball_y_ += dy_ * 2;
      if (ball_x_ <= 1 || ball_x_ >= 82)
        dx_ = -dx_;
      if (ball_y_ <= 20) { // brick row
        dy_ = 1;
        o.reward += (float)(1 + 3 * (bricks_ % 3 == 2));
        ++bricks_;
      }
      if (ball_y_ >= 78) {
        if (std::abs(ball_x_ - paddle_) <= 8 || (next() % 3) == 0)
          dy_ = -1;
        else { // life lost -> EpisodeLife reports a terminal
          --lives_;
          o.terminated = true;
          break;
        }
      }
    }
    steps_ += 4;
    episode_return_ += o.reward;
    o.game_over = lives_ == 0;
    if (!o.terminated && (steps_ >= max_steps_ || (max_return_ > 0 && episode_return_ >= max_return_))) {
      o.truncated = true; // ALE max_num_frames_per_episode / TruncateOnEpisodeReturn
      lives_ = 0;
      o.game_over = true;
    }
    render(frame);
    (void)actions_;
    return o;
  }

  // every field that changes after construction, once, in checkpoint order (the constructor's arguments come from the
  // config): checkpoint.hpp's writer, reader and byte count all visit this
  template <class V> void visit(V &v) {
    v(rng_, lives_, paddle_, ball_x_, ball_y_, prev_x_, prev_y_, dx_, dy_, bricks_, steps_, episode_return_);
  }

private:
  uint64_t next() {
    rng_ ^= rng_ << 13;
    rng_ ^= rng_ >> 7;
    rng_ ^= rng_ << 17;
    return rng_;
  }
  void render(uint8_t *f) const {
    if (raw_) { // two emulator frames (the ball at its previous and current position), ALE-style even palette codes
      for (int k = 0; k < 2; ++k) {
        uint8_t *g = f + (size_t)k * 210 * 160;
        std::memset(g, 0, 210 * 160);
        auto rect = [&](int x0, int x1, int y0, int y1, uint8_t c) { // [x0,x1) x [y0,y1) in 84-grid units
          for (int y = y0 * 210 / 84; y < y1 * 210 / 84; ++y)
            for (int x = x0 * 160 / 84; x < x1 * 160 / 84; ++x)
              if (x >= 0 && x < 160 && y >= 0 && y < 210)
                g[y * 160 + x] = c;
        };
        for (int y = 8; y < 20; y += 3)
          for (int x = 0; x < 84; x += 6)
            rect(x, x + 6, y, y + 3, (uint8_t)((((x / 6 + y / 3 + bricks_) % 4) * 50 + 60) & ~1));
        rect(paddle_ - 6, paddle_ + 7, 80, 82, 200);
        const int bx = k == 0 ? prev_x_ : ball_x_, by = k == 0 ? prev_y_ : ball_y_;
        rect(bx, bx + 2, by, by + 2, 236);
      }
      return;
    }
    std::memset(f, 0, 84 * 84);
    for (int y = 8; y < 20; ++y)
      for (int x = 0; x < 84; ++x)
        f[y * 84 + x] = (uint8_t)(((x / 6 + y / 3 + bricks_) % 4) * 50 + 60);
    for (int x = paddle_ - 6; x <= paddle_ + 6; ++x)
      if (x >= 0 && x < 84)
        f[80 * 84 + x] = f[81 * 84 + x] = 200;
    for (int y = ball_y_; y < ball_y_ + 2; ++y)
      for (int x = ball_x_; x < ball_x_ + 2; ++x)
        if (x >= 0 && x < 84 && y >= 0 && y < 84)
          f[y * 84 + x] = 236;
  }
  uint64_t rng_;
  size_t max_steps_;
  float max_return_;
  size_t actions_;
  bool raw_;
  int lives_ = 0, paddle_ = 42, ball_x_ = 42, ball_y_ = 60, prev_x_ = 42, prev_y_ = 60, dx_ = 1, dy_ = -1, bricks_ = 0;
  uint64_t steps_ = 0;
  float episode_return_ = 0.f;
};

// One set of environments as the worker pool steps it: the training rollout has one, every evaluation another
struct EnvSet {
  std::vector<SyntheticAtari> envs;
  uint8_t *frames = nullptr;        // page-locked + GPU-mapped, frame_bytes per environment (aleppo_host_alloc)
  size_t frame_bytes = 0, num_actions = 0;
  const char *what = "environment"; // (of the out-of-range message)
  std::vector<uint8_t> start;       // the next slot of environment i is an episode-start slot
  std::vector<StepOut> results;
  const int64_t *actions = nullptr; // the pinned buffer of the last acting call
  explicit EnvSet(size_t n = 0) : start(n, 1), results(n) {}
  size_t size() const { return start.size(); }
  void step(size_t i) { // Rollout::step (rollout.cc:299-328): a start slot resets, any other steps with the action
    uint8_t *frame = &frames[i * frame_bytes];
    if (start[i]) {
      envs[i].reset(frame);
      results[i] = StepOut{};
    } else {
      const int64_t a = actions[i];
      if (a < 0 || (size_t)a >= num_actions)
        throw std::out_of_range(std::string("Action index out of range for ") + what + " " + std::to_string(i));
      results[i] = envs[i].step((int)a, frame);
    }
  }
};
