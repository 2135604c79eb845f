// TEST INFRASTRUCTURE - aleppo_stub_eval_env.cc plus host-only episode recorders (aleppo_rec_open / aleppo_rec_count /
// aleppo_rec_read / aleppo_rec_clear), so that the trainer's record_video / record_evaluation / record_interval keys - its
// draining, its episode splitting across rollout and chunk boundaries, its files - run without a GPU.  The stand-ins'
// aleppo_env_rollout and aleppo_eval_env_run are renamed while they are included and defined again here: the same loops,
// slot for slot, with the recorded environment's row taken behind every slot's aleppo_step / aleppo_eval_push_frames.
// Frames and step records come from trainer/emulator.hpp ITSELF; there is no network, so logits and values are zero; the
// observation plane of 84x84 frames is the frame, of raw pairs the first frame's top-left 84x84 corner (not the library's:
// no CPU test reads it).  Host-driven steps do not advance the ordinal here (the trainer never drives a recorded source
// from the host).  Never linked into anything but trainer/train_rec_stub.
#define aleppo_env_rollout stub_unrecorded_env_rollout
#define aleppo_eval_env_run stub_unrecorded_eval_env_run
#include "aleppo_stub_eval_env.cc"
#undef aleppo_env_rollout
#undef aleppo_eval_env_run

struct StubRecorder {
  bool open = false;
  aleppo_rec_config cfg{};
  size_t frame_bytes = 0, A = 0;
  uint64_t rows = 0, dropped = 0, ordinal = 0;
  std::vector<aleppo_rec_step> steps;
  std::vector<uint8_t> frames, obs;
  std::vector<float> logits;
};
static StubRecorder g_rec[2];

struct StubLives { // SyntheticAtari::visit's second field
  int lives = 0;
  void operator()(uint64_t &, int &l, int &, int &, int &, int &, int &, int &, int &, int &, uint64_t &, float &) { lives = l; }
};
// one device-driven step of `source`: row `rows` (or a drop), ordinal + 1
static void stub_rec_capture(int source, const uint8_t *frame, SyntheticAtari &env, int action, float reward, bool start,
                             bool term, bool trunc, bool game_over) {
  StubRecorder &R = g_rec[source];
  if (!R.open)
    return;
  const uint64_t ordinal = R.ordinal++;
  if (R.rows >= (uint64_t)R.cfg.capacity) {
    R.dropped++;
    return;
  }
  const size_t r = (size_t)R.rows++;
  StubLives lv;
  env.visit(lv);
  aleppo_rec_step s{};
  s.ordinal = ordinal;
  s.action = action;
  s.reward = reward;
  s.start = start, s.terminated = term, s.truncated = trunc, s.game_over = (term || trunc) && game_over;
  s.lives = lv.lives;
  R.steps[r] = s;
  if (R.cfg.content & ALEPPO_REC_FRAMES)
    std::memcpy(&R.frames[r * R.frame_bytes], frame, R.frame_bytes);
  if (R.cfg.content & ALEPPO_REC_OBSERVATION)
    for (size_t y = 0; y < 84; ++y)
      std::memcpy(&R.obs[(r * 84 + y) * 84], frame + y * (R.frame_bytes == 84 * 84 ? 84 : 160), 84);
}

extern "C" {
int aleppo_env_rollout(aleppo_ctx *c) { // aleppo_stub_env.cc's loop + the capture
  if (!g_env_open || c->armed || c->t != 0)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: env_rollout out of order");
  const size_t E = g_set.size(), T = (size_t)c->cfg.horizon, rec = (size_t)g_rec[ALEPPO_REC_ROLLOUT].cfg.index;
  g_set.frames = g_frames.data();
  for (size_t t = 0; t < T; ++t) {
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
    stub_rec_capture(ALEPPO_REC_ROLLOUT, g_frames.data() + rec * g_set.frame_bytes, g_set.envs[rec], (int)g_set.actions[rec],
                     g_rewards[rec], start_at_entry[rec], g_term[rec], g_trunc[rec], g_game_over[rec]);
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
int aleppo_eval_env_run(aleppo_ctx *c, int rule, float param, int32_t steps) { // aleppo_stub_eval_env.cc's loop + the capture
  if (!g_ee_open || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: eval_env_run out of order");
  if (!stub_rule_ok(rule, param) || steps < 1 || (size_t)steps > g_ee_S)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: eval_env_run: bad rule, param or steps");
  const size_t L = g_ev_L, plane = g_ee_S * L, rec = (size_t)g_rec[ALEPPO_REC_EVAL].cfg.index;
  std::fill(g_ee_log.begin(), g_ee_log.end(), 0u);
  g_ee_set.frames = g_ee_frames.data();
  g_ee_set.actions = g_ev_actions.data();
  for (size_t s = 0; s < (size_t)steps; ++s) {
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
      if (i == rec)
        stub_rec_capture(ALEPPO_REC_EVAL, g_ee_frames.data() + rec * g_ee_set.frame_bytes, g_ee_set.envs[rec],
                         (int)g_ev_actions[rec], g_ee_reward[rec], start_at_entry[rec], o.terminated, o.truncated,
                         g_ee_game_over[rec]);
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
int aleppo_rec_open(aleppo_ctx *c, const aleppo_rec_config *cfg) {
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (!cfg || (cfg->source != ALEPPO_REC_ROLLOUT && cfg->source != ALEPPO_REC_EVAL))
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: rec_open: bad config");
  const bool rollout = cfg->source == ALEPPO_REC_ROLLOUT;
  if (rollout ? !g_env_open : !g_ee_open)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: rec_open: the source's environments are not open");
  const size_t n = rollout ? g_set.size() : g_ee_set.size();
  if (cfg->index < 0 || (size_t)cfg->index >= n || cfg->content < 1 || cfg->content > 3 || cfg->capacity < 1 ||
      cfg->capacity > 65536 || cfg->reserved[0] || cfg->reserved[1] || cfg->reserved[2] || cfg->reserved[3])
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: rec_open: bad config");
  StubRecorder &R = g_rec[cfg->source];
  if (R.open && std::memcmp(&R.cfg, cfg, sizeof(*cfg)) != 0)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: this source's recorder is already open with another config");
  if (!R.open) {
    R.cfg = *cfg;
    R.frame_bytes = rollout ? g_set.frame_bytes : g_ee_set.frame_bytes;
    R.A = (size_t)c->cfg.num_actions;
    const size_t cap = (size_t)cfg->capacity;
    R.steps.assign(cap, aleppo_rec_step{});
    R.logits.assign(cap * R.A, 0.f);
    if (cfg->content & ALEPPO_REC_FRAMES)
      R.frames.assign(cap * R.frame_bytes, 0);
    if (cfg->content & ALEPPO_REC_OBSERVATION)
      R.obs.assign(cap * 84 * 84, 0);
    R.open = true;
  }
  R.rows = R.dropped = R.ordinal = 0;
  return ALEPPO_OK;
}
int aleppo_rec_count(aleppo_ctx *c, int source, aleppo_rec_counts *out) {
  if (!out || (source != ALEPPO_REC_ROLLOUT && source != ALEPPO_REC_EVAL))
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: rec_count: bad argument");
  const StubRecorder &R = g_rec[source];
  aleppo_rec_counts n{};
  if (R.open) {
    n.rows = R.rows, n.dropped = R.dropped, n.next_ordinal = R.ordinal;
    n.capacity = R.cfg.capacity;
    n.frame_bytes = (R.cfg.content & ALEPPO_REC_FRAMES) ? (int32_t)R.frame_bytes : 0;
    n.observation_bytes = (R.cfg.content & ALEPPO_REC_OBSERVATION) ? 84 * 84 : 0;
    n.actions = (int32_t)R.A;
  }
  *out = n;
  return ALEPPO_OK;
}
int aleppo_rec_read(aleppo_ctx *c, int source, int field, uint64_t first, uint64_t rows, void *dst, size_t bytes) {
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (source != ALEPPO_REC_ROLLOUT && source != ALEPPO_REC_EVAL)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: rec_read: unknown source");
  const StubRecorder &R = g_rec[source];
  if (!R.open)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: rec_read: no recorder");
  const uint8_t *src = nullptr;
  size_t row = 0;
  if (field == ALEPPO_REC_F_STEPS)
    src = reinterpret_cast<const uint8_t *>(R.steps.data()), row = sizeof(aleppo_rec_step);
  else if (field == ALEPPO_REC_F_LOGITS)
    src = reinterpret_cast<const uint8_t *>(R.logits.data()), row = R.A * 4;
  else if (field == ALEPPO_REC_F_FRAMES && (R.cfg.content & ALEPPO_REC_FRAMES))
    src = R.frames.data(), row = R.frame_bytes;
  else if (field == ALEPPO_REC_F_OBSERVATIONS && (R.cfg.content & ALEPPO_REC_OBSERVATION))
    src = R.obs.data(), row = 84 * 84;
  if (!src || !dst || first > R.rows || rows > R.rows - first || bytes != (size_t)rows * row)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: rec_read: bad field, range or byte count");
  std::memcpy(dst, src + (size_t)first * row, bytes);
  return ALEPPO_OK;
}
int aleppo_rec_clear(aleppo_ctx *c, int source) {
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (source != ALEPPO_REC_ROLLOUT && source != ALEPPO_REC_EVAL)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: rec_clear: unknown source");
  if (!g_rec[source].open)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: rec_clear: no recorder");
  g_rec[source].rows = g_rec[source].dropped = 0;
  return ALEPPO_OK;
}
}
