// TEST INFRASTRUCTURE - aleppo_stub_state.cc plus host-only stand-ins for the device-resident environments
// (aleppo_env_open / aleppo_env_rollout / aleppo_env_export_state / aleppo_env_import_state / aleppo_env_read), so that the
// trainer's device_environments mode - its counters, its episode log, what it writes into a checkpoint and reads back -
// runs without a GPU.  The environments are trainer/emulator.hpp ITSELF, stepped the way the trainer's collect() steps its
// own; a rollout is T times the stub's aleppo_act and aleppo_step, so the stub's "device state" (tick, checksum) moves as
// it does under the host loop.  Never linked into anything but trainer/train_env_stub.
#include "aleppo_stub_state.cc"
#include "../../trainer/emulator.hpp"

static bool g_env_open = false;
static aleppo_env_config g_env_cfg{};
static EnvSet g_set;
static std::vector<uint8_t> g_frames, g_term, g_trunc, g_game_over;
static std::vector<float> g_rewards, g_ep_ret, g_game_ret;
static std::vector<uint64_t> g_ep_len, g_game_len;
static std::vector<uint32_t> g_log; // [4][T][E]: float planes stored as their bits
struct StubEnvFields { // SyntheticAtari::visit's order <-> aleppo_env_state
  aleppo_env_state &s;
  bool out;
  template <class A, class B> void one(A &emu, B &st) {
    if (out)
      st = (B)emu;
    else
      emu = (A)st;
  }
  void operator()(uint64_t &rng, int &lives, int &paddle, int &bx, int &by, int &px, int &py, int &dx, int &dy, int &bricks,
                  uint64_t &steps, float &ret) {
    one(rng, s.rng), one(lives, s.lives), one(paddle, s.paddle), one(bx, s.ball_x), one(by, s.ball_y), one(px, s.prev_x);
    one(py, s.prev_y), one(dx, s.dx), one(dy, s.dy), one(bricks, s.bricks), one(steps, s.steps), one(ret, s.episode_return);
  }
};
static void stub_env_fields(aleppo_env_state *st, bool out) {
  for (size_t i = 0; i < g_set.size(); ++i) {
    StubEnvFields f{st[i], out};
    g_set.envs[i].visit(f);
    f.one(g_set.start[i], st[i].start), f.one(g_game_over[i], st[i].game_over), f.one(g_rewards[i], st[i].reward);
    f.one(g_ep_ret[i], st[i].ep_ret), f.one(g_game_ret[i], st[i].game_ret), f.one(g_ep_len[i], st[i].ep_len);
    f.one(g_game_len[i], st[i].game_len);
  }
}
extern "C" {
int aleppo_env_open(aleppo_ctx *c, const aleppo_env_config *cfg) {
  if (!cfg || cfg->kind != ALEPPO_ENV_SYNTHETIC || cfg->reserved ||
      (cfg->frame_kind != ALEPPO_FRAMES_84 && cfg->frame_kind != ALEPPO_FRAMES_RAW_PAIR))
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: bad environment config");
  if (g_env_open && std::memcmp(cfg, &g_env_cfg, sizeof(*cfg)) != 0)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: the device environments are already open with another config");
  const size_t E = (size_t)c->cfg.num_envs, T = (size_t)c->cfg.horizon;
  const bool raw = cfg->frame_kind == ALEPPO_FRAMES_RAW_PAIR;
  g_env_cfg = *cfg;
  g_set = EnvSet(E);
  for (size_t i = 0; i < E; ++i)
    g_set.envs.emplace_back(cfg->seed_base + i, (size_t)cfg->max_steps, cfg->max_return, (size_t)c->cfg.num_actions, raw);
  g_set.frame_bytes = SyntheticAtari::frame_bytes(raw);
  g_set.num_actions = (size_t)c->cfg.num_actions;
  g_frames.assign(E * g_set.frame_bytes, 0);
  g_term.assign(E, 0), g_trunc.assign(E, 0), g_game_over.assign(E, 0);
  g_rewards.assign(E, 0.f), g_ep_ret.assign(E, 0.f), g_game_ret.assign(E, 0.f);
  g_ep_len.assign(E, 0), g_game_len.assign(E, 0);
  g_log.assign(4 * T * E, 0);
  g_env_open = true;
  return ALEPPO_OK;
}
int aleppo_env_rollout(aleppo_ctx *c) {
  if (!g_env_open || c->armed || c->t != 0)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: env_rollout out of order");
  const size_t E = g_set.size(), T = (size_t)c->cfg.horizon;
  g_set.frames = g_frames.data();
  for (size_t t = 0; t < T; ++t) { // the trainer's collect(), slot for slot
    if (int rc = aleppo_act(c, nullptr, &g_set.actions))
      return rc;
    const std::vector<uint8_t> start_at_entry = g_set.start;
    for (size_t i = 0; i < E; ++i)
      g_set.step(i);
    for (size_t i = 0; i < E; ++i)
      if (!g_set.start[i]) {
        const StepOut &o = g_set.results[i];
        g_rewards[i] = o.reward, g_term[i] = o.terminated, g_trunc[i] = o.truncated, g_game_over[i] = o.game_over;
        g_ep_ret[i] += o.reward, g_ep_len[i]++, g_game_ret[i] += o.reward, g_game_len[i]++;
      }
    if (int rc = aleppo_step(c, g_frames.data(), g_env_cfg.frame_kind, ALEPPO_DEVICE, g_rewards.data(), g_term.data(),
                             g_trunc.data(), start_at_entry.data()))
      return rc;
    uint32_t *log = g_log.data() + t * E;
    for (size_t i = 0; i < E; ++i) {
      for (int k = 0; k < 4; ++k)
        log[k * T * E + i] = 0;
      if (g_set.results[i].terminated || g_set.results[i].truncated) {
        g_set.start[i] = 1;
        g_term[i] = g_trunc[i] = 0;
        std::memcpy(&log[i], &g_ep_ret[i], 4);
        log[T * E + i] = (uint32_t)g_ep_len[i];
        g_ep_ret[i] = 0, g_ep_len[i] = 0;
        if (g_game_over[i]) {
          std::memcpy(&log[2 * T * E + i], &g_game_ret[i], 4);
          log[3 * T * E + i] = (uint32_t)g_game_len[i];
          g_game_ret[i] = 0, g_game_len[i] = 0;
        }
      } else if (g_set.start[i]) {
        g_set.start[i] = 0;
      }
    }
  }
  return ALEPPO_OK;
}
int aleppo_env_export_state(aleppo_ctx *c, aleppo_env_state *st, size_t E) {
  if (!g_env_open || c->armed || c->t != 0)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: env_export_state out of order");
  if (!st || E != g_set.size())
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: bad argument");
  std::memset(st, 0, E * sizeof(*st));
  stub_env_fields(st, true);
  return ALEPPO_OK;
}
int aleppo_env_import_state(aleppo_ctx *c, const aleppo_env_state *st, size_t E) {
  if (!g_env_open || c->armed || c->t != 0)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: env_import_state out of order");
  if (!st || E != g_set.size())
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: bad argument");
  stub_env_fields(const_cast<aleppo_env_state *>(st), false); // (only read in this direction)
  return ALEPPO_OK;
}
int aleppo_env_read(aleppo_ctx *c, int field, void *dst, size_t bytes) {
  if (!g_env_open || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: env_read out of order");
  const size_t plane = g_log.size() / 4;
  if (field == ALEPPO_ENV_F_FRAMES && bytes == g_frames.size())
    std::memcpy(dst, g_frames.data(), bytes);
  else if (field >= ALEPPO_ENV_F_EPISODE_RETURNS && field <= ALEPPO_ENV_F_GAME_LENGTHS && bytes == plane * 4)
    std::memcpy(dst, g_log.data() + (size_t)(field - ALEPPO_ENV_F_EPISODE_RETURNS) * plane, bytes);
  else
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: env_read: unknown field or wrong byte count");
  return ALEPPO_OK;
}
}
