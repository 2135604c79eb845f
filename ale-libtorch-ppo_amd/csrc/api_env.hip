// api_env.hip - C ABI (include/aleppo.h), the device-resident environments: aleppo_env_open, aleppo_env_rollout,
// aleppo_env_export_state / aleppo_env_import_state, aleppo_env_read.  The game and its kernel are env_synth.hpp.
#include "api_internal.hpp"
#include "env_synth.hpp"

using namespace aleppo;

static_assert(sizeof(aleppo_env_config) == 32, "aleppo_env_config is 32 bytes (include/aleppo.h)");
static_assert(sizeof(aleppo_env_state) == 88 && offsetof(aleppo_env_state, lives) == 32 &&
                  offsetof(aleppo_env_state, episode_return) == 68 && offsetof(aleppo_env_state, start) == 84,
              "aleppo_env_state is 88 bytes without padding (include/aleppo.h)");

#define CHECK_ENV(c)                                                                                                   \
  do {                                                                                                                 \
    CHECK_CTX(c);                                                                                                      \
    if (!(c)->env_open)                                                                                                \
      return set_err((c), ALEPPO_ERR_RUNTIME, "no device environments: call aleppo_env_open first");                   \
  } while (0)

static size_t env_frame_bytes(const aleppo_ctx *c) { // per environment
  return c->env_cfg.frame_kind == ALEPPO_FRAMES_RAW_PAIR ? (size_t)2 * RAW_H * RAW_W : (size_t)FRAME_PIX;
}
static size_t env_plane(const aleppo_ctx *c) { return (size_t)c->T * c->E; } // elements of one log plane

// the constructor's state (emulator.hpp: SyntheticAtari's member initialisers) with start = 1 and reward 0
void aleppo::env_initial(const aleppo_env_config &cfg, std::vector<aleppo_env_state> &st) {
  for (size_t e = 0; e < st.size(); ++e) {
    aleppo_env_state s{};
    s.rng = (cfg.seed_base + e) * 0x9E3779B97F4A7C15ull + 12345;
    s.paddle = s.ball_x = s.prev_x = 42;
    s.ball_y = s.prev_y = 60;
    s.dx = 1;
    s.dy = -1;
    s.start = 1;
    st[e] = s;
  }
}
// what a run cannot reach (aleppo_env_import_state, aleppo_eval_env_import_state)
const char *aleppo::env_state_invalid(const aleppo_env_state &s) {
  auto pix = [](int v) { return v >= 0 && v <= 83; };
  if (s.lives < 0 || s.lives > 5)
    return "lives must be in 0..5";
  if (s.paddle < 4 || s.paddle > 79)
    return "paddle must be in 4..79";
  if (!pix(s.ball_x) || !pix(s.ball_y) || !pix(s.prev_x) || !pix(s.prev_y))
    return "ball coordinates must be in 0..83";
  if ((s.dx != 1 && s.dx != -1) || (s.dy != 1 && s.dy != -1))
    return "dx and dy must be +1 or -1";
  if (s.bricks < 0)
    return "bricks must not be negative";
  if (s.start > 1 || s.game_over > 1)
    return "flags must be 0 or 1";
  if (s.reserved[0] || s.reserved[1])
    return "reserved bytes must be 0";
  if (!std::isfinite(s.episode_return) || !std::isfinite(s.reward) || !std::isfinite(s.ep_ret) ||
      !std::isfinite(s.game_ret))
    return "a float is not finite";
  return nullptr;
}
static int env_upload(aleppo_ctx *c, const aleppo_env_state *st) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, copy_sync(c, c->env_state[c->env_cur], st, (size_t)c->E * sizeof(aleppo_env_state), hipMemcpyHostToDevice));
  return ALEPPO_OK;
}

extern "C" int aleppo_env_open(aleppo_ctx *c, const aleppo_env_config *cfg) {
  CHECK_CTX(c);
  if (!cfg)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_open: null config");
  if (cfg->kind != ALEPPO_ENV_SYNTHETIC)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_open: unknown environment kind");
  if (cfg->frame_kind != ALEPPO_FRAMES_84 && cfg->frame_kind != ALEPPO_FRAMES_RAW_PAIR)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_open: unknown frame kind");
  if (cfg->reserved != 0)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_open: reserved must be 0");
  if (c->env_open && (cfg->kind != c->env_cfg.kind || cfg->frame_kind != c->env_cfg.frame_kind ||
                      cfg->seed_base != c->env_cfg.seed_base || cfg->max_steps != c->env_cfg.max_steps ||
                      float_bits(cfg->max_return) != float_bits(c->env_cfg.max_return)))
    return set_err(c, ALEPPO_ERR_RUNTIME, "env_open: the device environments are already open with another config");
  std::vector<aleppo_env_state> init((size_t)c->E);
  env_initial(*cfg, init);
  if (!c->env_open) {
    const aleppo_env_config keep = c->env_cfg;
    c->env_cfg = *cfg;
    // frames | state[2][E] | logs [4][T][E]: every part starts 16-byte aligned (88 E and the frame strides are multiples of 8 / 16)
    const size_t fb = (size_t)c->E * env_frame_bytes(c), sb = ((size_t)c->E * sizeof(aleppo_env_state) + 15) / 16 * 16;
    uint8_t *blk = nullptr;
    const hipError_t e = dalloc(c, &blk, fb + 2 * sb + 4 * env_plane(c) * 4); // (zeroed: empty logs)
    if (e != hipSuccess) {
      c->env_cfg = keep;
      return set_err(c, ALEPPO_ERR_HIP, std::string("env_open: allocation failed: ") + hipGetErrorString(e));
    }
    c->env_blk = blk;
    c->env_state[0] = reinterpret_cast<aleppo_env_state *>(blk + fb);
    c->env_state[1] = reinterpret_cast<aleppo_env_state *>(blk + fb + sb);
    c->env_log = reinterpret_cast<float *>(blk + fb + 2 * sb);
    c->env_cur = 0;
    c->env_open = true;
  }
  return env_upload(c, init.data());
}

extern "C" int aleppo_env_rollout(aleppo_ctx *c) {
  CHECK_ENV(c);
  if (c->t != 0)
    return set_err(c, ALEPPO_ERR_RUNTIME, "env_rollout needs an empty rollout buffer");
  const int E = c->E, T = c->T, kind = c->env_cfg.frame_kind;
  const size_t plane = env_plane(c);
  uint32_t *const log_u = reinterpret_cast<uint32_t *>(c->env_log);
  c->act_queued_slot = -1;
  c->rec_on_device = true;
  for (int t = 0; t < T; ++t) {
    int rc = act_enqueue(c, nullptr, t); // conv stack (unless the previous step ran it) + the head: slot t's actions
    if (rc == ALEPPO_OK) {
      uint8_t *rec = c->step_rec + (size_t)t * c->step_rec_bytes;
      const aleppo_env_state *in = c->env_state[c->env_cur];
      aleppo_env_state *out = c->env_state[c->env_cur ^ 1];
      const size_t o = (size_t)t * E;
      const bool timed = c->prof_on;
      if (timed) {
        ProfClass &p = c->env_prof;
        if (p.used == p.start.size()) {
          hipEvent_t a = nullptr, b = nullptr;
          note(c, hipEventCreate(&a));
          note(c, hipEventCreate(&b));
          p.start.push_back(a);
          p.stop.push_back(b);
        }
        note(c, hipEventRecord(p.start[p.used], c->stream));
      }
      if (kind == ALEPPO_FRAMES_RAW_PAIR)
        hipLaunchKernelGGL(env_step_kernel<true>, dim3(E, ENV_RAW_PARTS), dim3(256), 0, c->stream, in, out, c->actions_tm + o,
                           c->env_blk, rec, c->env_log + o, log_u + plane + o, c->env_log + 2 * plane + o, log_u + 3 * plane + o, E,
                           c->env_cfg.max_steps, c->env_cfg.max_return);
      else
        hipLaunchKernelGGL(env_step_kernel<false>, dim3(E), dim3(256), 0, c->stream, in, out, c->actions_tm + o, c->env_blk,
                           rec, c->env_log + o, log_u + plane + o, c->env_log + 2 * plane + o, log_u + 3 * plane + o, E,
                           c->env_cfg.max_steps, c->env_cfg.max_return);
      if (timed)
        note(c, hipEventRecord(c->env_prof.stop[c->env_prof.used++], c->stream));
      c->env_cur ^= 1;
      // slot t's frames -> observation slot t + 1, with the start-at-entry bytes the kernel just wrote into the record
      rc = step_enqueue(c, c->env_blk, kind, ALEPPO_DEVICE, nullptr, nullptr, t, rec + 6 * (size_t)E);
      // the recorded environment's row: behind the ingest, in front of the next slot's environment kernel (which
      // overwrites `in`)
      if (rc == ALEPPO_OK && c->rec[ALEPPO_REC_ROLLOUT].open)
        rec_capture(c, ALEPPO_REC_ROLLOUT, in, t);
    }
    if (rc == ALEPPO_OK && hipGetLastError() != hipSuccess)
      rc = set_err(c, ALEPPO_ERR_HIP, "a launch failed");
    if (rc) // part of a rollout is on the stream: the environments and the buffer no longer agree
      return fail_ctx(c, rc, "aleppo_env_rollout: " + c->err);
    c->t++;
  }
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

static int env_between_rollouts(aleppo_ctx *c, const char *who) {
  if (c->t != 0)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   std::string(who) + ": valid between rollouts only (a rollout is in progress: finish it first)");
  return ALEPPO_OK;
}
extern "C" int aleppo_env_export_state(aleppo_ctx *c, aleppo_env_state *states, size_t num_envs) {
  CHECK_ENV(c);
  if (!states)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_export_state: null argument");
  if (num_envs != (size_t)c->E)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_export_state: num_envs is not the context's");
  if (int rc = env_between_rollouts(c, "env_export_state"))
    return rc;
  HIPCHK(c, copy_sync(c, states, c->env_state[c->env_cur], num_envs * sizeof(aleppo_env_state), hipMemcpyDeviceToHost));
  return ALEPPO_OK;
}
extern "C" int aleppo_env_import_state(aleppo_ctx *c, const aleppo_env_state *states, size_t num_envs) {
  CHECK_ENV(c);
  if (!states)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_import_state: null argument");
  if (num_envs != (size_t)c->E)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_import_state: num_envs is not the context's");
  if (int rc = env_between_rollouts(c, "env_import_state"))
    return rc;
  for (size_t e = 0; e < num_envs; ++e) // what a run cannot reach is refused before anything changes
    if (const char *bad = env_state_invalid(states[e]))
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "env_import_state: environment " + std::to_string(e) + ": " + bad);
  return env_upload(c, states);
}

extern "C" int aleppo_env_read(aleppo_ctx *c, int field, void *dst, size_t bytes) {
  CHECK_ENV(c);
  if (!dst)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_read: null dst");
  const void *src = nullptr;
  size_t need = 0;
  switch (field) {
  case ALEPPO_ENV_F_FRAMES:
    src = c->env_blk;
    need = (size_t)c->E * env_frame_bytes(c);
    break;
  case ALEPPO_ENV_F_EPISODE_RETURNS:
  case ALEPPO_ENV_F_EPISODE_LENGTHS:
  case ALEPPO_ENV_F_GAME_RETURNS:
  case ALEPPO_ENV_F_GAME_LENGTHS:
    src = c->env_log + (size_t)(field - ALEPPO_ENV_F_EPISODE_RETURNS) * env_plane(c);
    need = env_plane(c) * 4;
    break;
  case ALEPPO_ENV_F_STEP_MS: {
    if (bytes != 2 * sizeof(double))
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_read: wrong byte count");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double tot = 0;
    for (size_t i = 0; i < c->env_prof.used; ++i) {
      float ms = 0;
      HIPCHK(c, hipEventElapsedTime(&ms, c->env_prof.start[i], c->env_prof.stop[i]));
      tot += ms;
    }
    double *o = static_cast<double *>(dst);
    o[0] = c->env_prof.used ? tot / (double)c->env_prof.used : 0.0;
    o[1] = (double)c->env_prof.used;
    return ALEPPO_OK;
  }
  default:
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_read: unknown field");
  }
  if (bytes != need)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "env_read: wrong byte count");
  HIPCHK(c, copy_sync(c, dst, src, need, hipMemcpyDeviceToHost));
  return ALEPPO_OK;
}
