// api_eval_env.hip - C ABI (include/aleppo.h), the device-resident evaluation environments: aleppo_eval_env_open,
// aleppo_eval_env_run, aleppo_eval_env_export_state / aleppo_eval_env_import_state, aleppo_eval_env_read.  One
// SyntheticAtari per evaluation lane; the game is env_synth.hpp, the kernel env_eval.hpp, the acting half and the ingest
// are the evaluation lanes' own (api_eval.hip).  Works on the ee_* members and, through eval_act_enqueue and the ingest,
// on the ev_* ones only.
#include "api_internal.hpp"
#include "env_eval.hpp"

using namespace aleppo;

constexpr int MAX_EVAL_RUN_STEPS = 1024;
#define CHECK_EVAL_ENV(c)                                                                                              \
  do {                                                                                                                 \
    CHECK_CTX(c);                                                                                                      \
    if (!(c)->ee_open)                                                                                                 \
      return set_err((c), ALEPPO_ERR_RUNTIME, "no evaluation environments: call aleppo_eval_env_open first");          \
  } while (0)

static size_t ee_frame_bytes(const aleppo_ctx *c) { // per lane
  return c->ee_cfg.frame_kind == ALEPPO_FRAMES_RAW_PAIR ? (size_t)2 * RAW_H * RAW_W : (size_t)FRAME_PIX;
}
static size_t ee_plane(const aleppo_ctx *c) { return (size_t)c->ee_S * c->ev_L; } // elements of one log plane

extern "C" int aleppo_eval_env_open(aleppo_ctx *c, const aleppo_env_config *cfg, int32_t max_run_steps) {
  CHECK_CTX(c);
  if (!c->ev_L)
    return set_err(c, ALEPPO_ERR_RUNTIME, "eval_env_open: no evaluation lanes: call aleppo_eval_open first");
  if (!cfg)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_open: null config");
  if (cfg->kind != ALEPPO_ENV_SYNTHETIC)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_open: unknown environment kind");
  if (cfg->frame_kind != ALEPPO_FRAMES_84 && cfg->frame_kind != ALEPPO_FRAMES_RAW_PAIR)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_open: unknown frame kind");
  if (cfg->reserved != 0)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_open: reserved must be 0");
  if (max_run_steps < 1 || max_run_steps > MAX_EVAL_RUN_STEPS)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_open: max_run_steps must be in [1, 1024]");
  if (c->ee_open && (cfg->kind != c->ee_cfg.kind || cfg->frame_kind != c->ee_cfg.frame_kind ||
                     cfg->max_steps != c->ee_cfg.max_steps ||
                     float_bits(cfg->max_return) != float_bits(c->ee_cfg.max_return) || max_run_steps != c->ee_S))
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   "eval_env_open: the evaluation environments are already open with another config (only seed_base may "
                   "change)");
  const size_t L = (size_t)c->ev_L;
  std::vector<aleppo_env_state> init(L);
  env_initial(*cfg, init);
  if (!c->ee_open) {
    const aleppo_env_config keep = c->ee_cfg;
    c->ee_cfg = *cfg;
    c->ee_S = max_run_steps;
    // frames | state[2][L] | logs [4][S][L] | start [L]: every part but the last starts 16-byte aligned
    const size_t fb = L * ee_frame_bytes(c), sb = (L * sizeof(aleppo_env_state) + 15) / 16 * 16, lb = 4 * ee_plane(c) * 4;
    uint8_t *blk = nullptr;
    const hipError_t e = dalloc(c, &blk, fb + 2 * sb + lb + L); // (zeroed: empty logs)
    if (e != hipSuccess) {
      c->ee_cfg = keep;
      c->ee_S = 0;
      return set_err(c, ALEPPO_ERR_HIP, std::string("eval_env_open: allocation failed: ") + hipGetErrorString(e));
    }
    c->ee_blk = blk;
    c->ee_state[0] = reinterpret_cast<aleppo_env_state *>(blk + fb);
    c->ee_state[1] = reinterpret_cast<aleppo_env_state *>(blk + fb + sb);
    c->ee_log = reinterpret_cast<float *>(blk + fb + 2 * sb);
    c->ee_start = blk + fb + 2 * sb + lb;
    c->ee_cur = 0;
    c->ee_open = true;
  } else { // re-seed: the constructor's state of the new seeds, an empty log; stacks, counter and ticket stay
    HIPCHK(c, hipMemsetAsync(c->ee_log, 0, 4 * ee_plane(c) * 4, c->stream));
    c->ee_cfg.seed_base = cfg->seed_base;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, copy_sync(c, c->ee_state[c->ee_cur], init.data(), L * sizeof(aleppo_env_state), hipMemcpyHostToDevice));
  return ALEPPO_OK;
}

extern "C" int aleppo_eval_env_run(aleppo_ctx *c, int rule, float param, int32_t steps) {
  CHECK_EVAL_ENV(c);
  float kparam = 0.f;
  if (int rc = eval_check_rule(c, rule, param, false, &kparam))
    return rc;
  if (steps < 1 || steps > c->ee_S)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_run: steps must be in [1, max_run_steps]");
  const int L = c->ev_L, kind = c->ee_cfg.frame_kind;
  const size_t plane = ee_plane(c);
  uint32_t *const log_u = reinterpret_cast<uint32_t *>(c->ee_log);
  if (steps < c->ee_S) // rows [steps, S) are zero (rows [0, steps) are written whole by the kernel)
    HIPCHK(c, hipMemsetAsync(c->ee_log, 0, 4 * plane * 4, c->stream));
  for (int s = 0; s < steps; ++s) {
    int rc = eval_act_enqueue(c, rule, kparam, nullptr); // conv stack + the evaluation head: this step's actions
    if (rc) // part of a run is on the stream: the environments, the stacks and the log no longer agree
      return fail_ctx(c, rc, "aleppo_eval_env_run: " + c->err);
    const aleppo_env_state *in = c->ee_state[c->ee_cur];
    aleppo_env_state *out = c->ee_state[c->ee_cur ^ 1];
    const size_t o = (size_t)s * L;
    if (kind == ALEPPO_FRAMES_RAW_PAIR)
      hipLaunchKernelGGL(eval_env_step_kernel<true>, dim3(L, ENV_RAW_PARTS), dim3(256), 0, c->stream, in, out, c->ev_actions,
                         c->ee_blk, c->ee_start, c->ee_log + o, log_u + plane + o, c->ee_log + 2 * plane + o,
                         log_u + 3 * plane + o, c->ee_cfg.max_steps, c->ee_cfg.max_return);
    else
      hipLaunchKernelGGL(eval_env_step_kernel<false>, dim3(L), dim3(256), 0, c->stream, in, out, c->ev_actions, c->ee_blk,
                         c->ee_start, c->ee_log + o, log_u + plane + o, c->ee_log + 2 * plane + o, log_u + 3 * plane + o,
                         c->ee_cfg.max_steps, c->ee_cfg.max_return);
    c->ee_cur ^= 1;
    // this step's frames -> the lanes' stacks with the start-at-entry bytes the kernel just wrote: aleppo_eval_push_frames'
    // ingest on a one-slot "rollout"
    launch_ingest(c->stream, kind == ALEPPO_FRAMES_RAW_PAIR, c->ee_blk, c->lut, c->ee_start, nullptr, c->ev_obs, L, 1, 0, 0);
    if (c->rec[ALEPPO_REC_EVAL].open) // the recorded lane's row, in front of the next step's kernels
      rec_capture(c, ALEPPO_REC_EVAL, in, 0);
    if (hipGetLastError() != hipSuccess)
      return fail_ctx(c, ALEPPO_ERR_HIP, "aleppo_eval_env_run: a launch failed");
  }
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_eval_env_export_state(aleppo_ctx *c, aleppo_env_state *states, size_t num_lanes) {
  CHECK_EVAL_ENV(c);
  if (!states)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_export_state: null argument");
  if (num_lanes != (size_t)c->ev_L)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_export_state: num_lanes is not the lanes' count");
  HIPCHK(c, copy_sync(c, states, c->ee_state[c->ee_cur], num_lanes * sizeof(aleppo_env_state), hipMemcpyDeviceToHost));
  return ALEPPO_OK;
}
extern "C" int aleppo_eval_env_import_state(aleppo_ctx *c, const aleppo_env_state *states, size_t num_lanes) {
  CHECK_EVAL_ENV(c);
  if (!states)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_import_state: null argument");
  if (num_lanes != (size_t)c->ev_L)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_import_state: num_lanes is not the lanes' count");
  for (size_t l = 0; l < num_lanes; ++l) // what a run cannot reach is refused before anything changes
    if (const char *bad = env_state_invalid(states[l]))
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_import_state: lane " + std::to_string(l) + ": " + bad);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, copy_sync(c, c->ee_state[c->ee_cur], states, num_lanes * sizeof(aleppo_env_state), hipMemcpyHostToDevice));
  return ALEPPO_OK;
}

extern "C" int aleppo_eval_env_read(aleppo_ctx *c, int field, void *dst, size_t bytes) {
  CHECK_EVAL_ENV(c);
  if (!dst)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_read: null dst");
  const void *src = nullptr;
  size_t need = 0;
  switch (field) {
  case ALEPPO_EEF_FRAMES:
    src = c->ee_blk;
    need = (size_t)c->ev_L * ee_frame_bytes(c);
    break;
  case ALEPPO_EEF_EPISODE_RETURNS:
  case ALEPPO_EEF_EPISODE_LENGTHS:
  case ALEPPO_EEF_GAME_RETURNS:
  case ALEPPO_EEF_GAME_LENGTHS:
    src = c->ee_log + (size_t)(field - ALEPPO_EEF_EPISODE_RETURNS) * ee_plane(c);
    need = ee_plane(c) * 4;
    break;
  default:
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_read: unknown field");
  }
  if (bytes != need)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_env_read: wrong byte count");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, copy_sync(c, dst, src, need, hipMemcpyDeviceToHost));
  return ALEPPO_OK;
}
