// TEST INFRASTRUCTURE - aleppo_stub_env.cc plus host-only evaluation lanes (aleppo_eval_open / aleppo_eval_act /
// aleppo_eval_push_frames / aleppo_eval_read / aleppo_eval_set_counter) and host-only device-resident evaluation
// environments (aleppo_eval_env_open / aleppo_eval_env_run / aleppo_eval_env_export_state / aleppo_eval_env_import_state /
// aleppo_eval_env_read), so that the trainer's device_evaluation mode - its chunking, its compaction of the log planes,
// the evaluation counter it sets back - runs without a GPU next to its host evaluation.  There is no network: the action
// of lane l at evaluation counter n is a fixed hash of (seed, n, l) in [0, A), whichever path asks for it.  The
// environments are trainer/emulator.hpp ITSELF.  Never linked into anything but trainer/train_eval_stub.
#include "aleppo_stub_env.cc"

static size_t g_ev_L = 0;
static uint64_t g_ev_counter = 0, g_ev_checksum = 0;
static std::vector<int64_t> g_ev_actions;
static bool g_ee_open = false;
static aleppo_env_config g_ee_cfg{};
static size_t g_ee_S = 0;
static EnvSet g_ee_set;
static std::vector<uint8_t> g_ee_frames, g_ee_game_over;
static std::vector<float> g_ee_reward, g_ee_ep_ret, g_ee_game_ret;
static std::vector<uint64_t> g_ee_ep_len, g_ee_game_len;
static std::vector<uint32_t> g_ee_log; // [4][S][L]: float planes stored as their bits

static void stub_eval_actions(aleppo_ctx *c) { // one acting call: every lane's action at counter n, then n + 1 (stub_mix: aleppo_stub_state.cc)
  for (size_t l = 0; l < g_ev_L; ++l)
    g_ev_actions[l] = (int64_t)(stub_mix(stub_mix(c->cfg.seed ^ g_ev_counter) + l) % (uint64_t)c->cfg.num_actions);
  g_ev_counter++;
}
static bool stub_rule_ok(int rule, float param) {
  return (rule == ALEPPO_EVAL_GREEDY && param == 0.f) || (rule == ALEPPO_EVAL_SAMPLE && param > 0.f) ||
         (rule == ALEPPO_EVAL_EPSILON_GREEDY && param >= 0.f && param <= 1.f);
}
static void stub_ee_fields(aleppo_env_state *st, bool out) {
  for (size_t i = 0; i < g_ee_set.size(); ++i) {
    StubEnvFields f{st[i], out};
    g_ee_set.envs[i].visit(f);
    f.one(g_ee_set.start[i], st[i].start), f.one(g_ee_game_over[i], st[i].game_over), f.one(g_ee_reward[i], st[i].reward);
    f.one(g_ee_ep_ret[i], st[i].ep_ret), f.one(g_ee_game_ret[i], st[i].game_ret), f.one(g_ee_ep_len[i], st[i].ep_len);
    f.one(g_ee_game_len[i], st[i].game_len);
  }
}
extern "C" {
int aleppo_eval_open(aleppo_ctx *c, int32_t L) {
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (L < 1 || L > 4096)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: eval_open: num_lanes must be in [1, 4096]");
  if (g_ev_L && g_ev_L != (size_t)L)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: the evaluation lanes are already open with another lane count");
  g_ev_L = (size_t)L;
  g_ev_actions.assign(g_ev_L, 0);
  g_ev_counter = 0;
  return ALEPPO_OK;
}
int aleppo_eval_act(aleppo_ctx *c, int rule, float param, const float *, const int64_t **out) {
  if (!g_ev_L || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: eval_act out of order");
  if (!stub_rule_ok(rule, param))
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: eval_act: bad rule or param");
  stub_eval_actions(c);
  if (out)
    *out = g_ev_actions.data();
  return ALEPPO_OK;
}
int aleppo_eval_push_frames(aleppo_ctx *c, const uint8_t *frames, int kind, int, const uint8_t *start) {
  if (!g_ev_L || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: eval_push_frames out of order");
  const size_t per = kind == ALEPPO_FRAMES_RAW_PAIR ? 2 * 210 * 160 : 84 * 84;
  for (size_t i = 0; i < g_ev_L * per; i += 97) // what the ingest kernel would read
    g_ev_checksum = g_ev_checksum * 31 + frames[i];
  for (size_t l = 0; l < g_ev_L; ++l)
    g_ev_checksum += start[l];
  return ALEPPO_OK;
}
int aleppo_eval_read(aleppo_ctx *c, int field, void *dst, size_t bytes) {
  if (!g_ev_L || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: eval_read out of order");
  if (field == ALEPPO_EF_ACTIONS && bytes == g_ev_L * 8)
    std::memcpy(dst, g_ev_actions.data(), bytes);
  else
    std::memset(dst, 0, bytes); // (no network: no logits, no values)
  return ALEPPO_OK;
}
int aleppo_eval_set_counter(aleppo_ctx *c, uint64_t n) {
  if (!g_ev_L || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: eval_set_counter out of order");
  g_ev_counter = n;
  return ALEPPO_OK;
}
int aleppo_eval_env_open(aleppo_ctx *c, const aleppo_env_config *cfg, int32_t S) {
  if (!g_ev_L || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: eval_env_open out of order");
  if (!cfg || cfg->kind != ALEPPO_ENV_SYNTHETIC || cfg->reserved || S < 1 || S > 1024 ||
      (cfg->frame_kind != ALEPPO_FRAMES_84 && cfg->frame_kind != ALEPPO_FRAMES_RAW_PAIR))
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: bad evaluation environment config");
  if (g_ee_open && (cfg->frame_kind != g_ee_cfg.frame_kind || cfg->max_steps != g_ee_cfg.max_steps ||
                    std::memcmp(&cfg->max_return, &g_ee_cfg.max_return, 4) != 0 || (size_t)S != g_ee_S))
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: the evaluation environments are already open with another config");
  const size_t L = g_ev_L;
  const bool raw = cfg->frame_kind == ALEPPO_FRAMES_RAW_PAIR;
  g_ee_cfg = *cfg;
  g_ee_S = (size_t)S;
  g_ee_set = EnvSet(L);
  for (size_t i = 0; i < L; ++i)
    g_ee_set.envs.emplace_back(cfg->seed_base + i, (size_t)cfg->max_steps, cfg->max_return, (size_t)c->cfg.num_actions, raw);
  g_ee_set.frame_bytes = SyntheticAtari::frame_bytes(raw);
  g_ee_set.num_actions = (size_t)c->cfg.num_actions;
  g_ee_set.what = "evaluation environment";
  g_ee_frames.assign(L * g_ee_set.frame_bytes, 0);
  g_ee_game_over.assign(L, 0);
  g_ee_reward.assign(L, 0.f), g_ee_ep_ret.assign(L, 0.f), g_ee_game_ret.assign(L, 0.f);
  g_ee_ep_len.assign(L, 0), g_ee_game_len.assign(L, 0);
  g_ee_log.assign(4 * g_ee_S * L, 0);
  g_ee_open = true;
  return ALEPPO_OK;
}
int aleppo_eval_env_run(aleppo_ctx *c, int rule, float param, int32_t steps) {
  if (!g_ee_open || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: eval_env_run out of order");
  if (!stub_rule_ok(rule, param) || steps < 1 || (size_t)steps > g_ee_S)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: eval_env_run: bad rule, param or steps");
  const size_t L = g_ev_L, plane = g_ee_S * L;
  std::fill(g_ee_log.begin(), g_ee_log.end(), 0u);
  g_ee_set.frames = g_ee_frames.data();
  g_ee_set.actions = g_ev_actions.data();
  for (size_t s = 0; s < (size_t)steps; ++s) { // one host-driven evaluation step, lane for lane
    stub_eval_actions(c);
    const std::vector<uint8_t> start_at_entry = g_ee_set.start;
    for (size_t i = 0; i < L; ++i)
      g_ee_set.step(i);
    if (int rc = aleppo_eval_push_frames(c, g_ee_frames.data(), g_ee_cfg.frame_kind, ALEPPO_DEVICE, start_at_entry.data()))
      return rc;
    uint32_t *log = g_ee_log.data() + s * L;
    for (size_t i = 0; i < L; ++i) {
      const StepOut &o = g_ee_set.results[i];
      if (!start_at_entry[i]) {
        g_ee_reward[i] = o.reward, g_ee_game_over[i] = o.game_over;
        g_ee_ep_ret[i] += o.reward, g_ee_ep_len[i]++, g_ee_game_ret[i] += o.reward, g_ee_game_len[i]++;
      }
      if (o.terminated || o.truncated) {
        g_ee_set.start[i] = 1;
        std::memcpy(&log[i], &g_ee_ep_ret[i], 4);
        log[plane + i] = (uint32_t)g_ee_ep_len[i];
        g_ee_ep_ret[i] = 0, g_ee_ep_len[i] = 0;
        if (g_ee_game_over[i]) {
          std::memcpy(&log[2 * plane + i], &g_ee_game_ret[i], 4);
          log[3 * plane + i] = (uint32_t)g_ee_game_len[i];
          g_ee_game_ret[i] = 0, g_ee_game_len[i] = 0;
        }
      } else if (start_at_entry[i]) {
        g_ee_set.start[i] = 0;
      }
    }
  }
  return ALEPPO_OK;
}
int aleppo_eval_env_export_state(aleppo_ctx *c, aleppo_env_state *st, size_t L) {
  if (!g_ee_open || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: eval_env_export_state out of order");
  if (!st || L != g_ev_L)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: bad argument");
  std::memset(st, 0, L * sizeof(*st));
  stub_ee_fields(st, true);
  return ALEPPO_OK;
}
int aleppo_eval_env_import_state(aleppo_ctx *c, const aleppo_env_state *st, size_t L) {
  if (!g_ee_open || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: eval_env_import_state out of order");
  if (!st || L != g_ev_L)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: bad argument");
  stub_ee_fields(const_cast<aleppo_env_state *>(st), false); // (only read in this direction)
  return ALEPPO_OK;
}
int aleppo_eval_env_read(aleppo_ctx *c, int field, void *dst, size_t bytes) {
  if (!g_ee_open || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: eval_env_read out of order");
  const size_t plane = g_ee_log.size() / 4;
  if (field == ALEPPO_EEF_FRAMES && bytes == g_ee_frames.size())
    std::memcpy(dst, g_ee_frames.data(), bytes);
  else if (field >= ALEPPO_EEF_EPISODE_RETURNS && field <= ALEPPO_EEF_GAME_LENGTHS && bytes == plane * 4)
    std::memcpy(dst, g_ee_log.data() + (size_t)(field - ALEPPO_EEF_EPISODE_RETURNS) * plane, bytes);
  else
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: eval_env_read: unknown field or wrong byte count");
  return ALEPPO_OK;
}
}
