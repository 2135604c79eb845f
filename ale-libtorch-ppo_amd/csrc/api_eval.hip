// api_eval.hip - C ABI (include/aleppo.h), the evaluation lanes.
#include "api_internal.hpp"

using namespace aleppo;

// ------------------------------------------------------------------ evaluation lanes (include/aleppo.h)
// Everything here works on the ev_* members only: own stacks, own acting scratch (aleppo_step may already have filled
// a3 / hpart for the rollout's next slot: pre_acted), own staging, own pinned buffer / ticket / arrival counter, own
// counter of the sampling stream.  The kernels go onto the context's main stream, behind whatever the rollout enqueued.
constexpr int MAX_EVAL_LANES = 4096;
constexpr uint64_t EVAL_KEY_DOMAIN = 0x4556414C4C414E45ull; // "EVALLANE"
#define CHECK_EVAL(c)                                                                                                  \
  do {                                                                                                                 \
    CHECK_CTX(c);                                                                                                      \
    if (!(c)->ev_L)                                                                                                    \
      return set_err((c), ALEPPO_ERR_RUNTIME, "no evaluation lanes: call aleppo_eval_open first");                    \
  } while (0)
static SampleMap eval_map() { return SampleMap{1, (long)FRAME_PIX, 0, 0, 0}; } // lane l at ev_obs + l * 7056

extern "C" int aleppo_eval_open(aleppo_ctx *c, int32_t num_lanes) {
  CHECK_CTX(c);
  if (num_lanes < 1 || num_lanes > MAX_EVAL_LANES)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_open: num_lanes must be in [1, 4096]");
  if (c->ev_L && c->ev_L != num_lanes)
    return set_err(c, ALEPPO_ERR_RUNTIME, "eval_open: the evaluation lanes are already open with another lane count");
  const size_t L = (size_t)num_lanes;
  if (c->ev_L) { // reset: zero stacks, the sampling stream from its start, no act to read
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemsetAsync(c->ev_obs, 0, L * FRAME_PIX * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ev_counter = 0;
    c->ev_acted = false;
    return ALEPPO_OK;
  }
  const bool unfused = !(c->prec == ALEPPO_BF16 && use_patch_kernels()); // conv1 / conv2 outputs pass through memory
  const size_t ts = tsz(c), nz = L * (size_t)std::max(c->A, 2) * 4, fb = L * 2 * RAW_H * RAW_W;
  hipError_t e = hipSuccess;
  const auto ok = [&e](hipError_t r) { return (e = r) == hipSuccess; }; // (the chain below ends at the first failure)
  ok(dalloc(c, &c->ev_obs, L * FRAME_PIX * 4)) &&
      (!unfused || (ok(dalloc(c, &c->ev_a1, L * A1_PIX * A1_C * ts)) && ok(dalloc(c, &c->ev_a2, L * A2_PIX * A2_C * ts)))) &&
      ok(dalloc(c, &c->ev_a3, L * FC_IN * ts)) && ok(dalloc(c, &c->ev_hpart, (size_t)FC_SPLITS * L * c->H * 4)) &&
      ok(dalloc(c, &c->ev_logits, L * c->A * 4)) && ok(dalloc(c, &c->ev_values, L * 4)) &&
      ok(dalloc(c, &c->ev_actions, L * 4)) && ok(dalloc(c, &c->ev_d_frames, fb)) && ok(dalloc(c, &c->ev_d_start, L)) &&
      ok(dalloc(c, &c->ev_d_noise, nz)) && ok(dalloc(c, &c->ev_d_done, 16)) &&
      ok(halloc(c, &c->ev_h_frames, fb, hipHostMallocDefault)) && ok(halloc(c, &c->ev_h_start, L, hipHostMallocDefault)) &&
      ok(halloc(c, &c->ev_h_noise, nz, hipHostMallocDefault)) &&
      ok(halloc(c, &c->ev_h_actions, (L + 8) * 8, hipHostMallocMapped)) &&
      (c->ev_staged || ok(hipEventCreateWithFlags(&c->ev_staged, hipEventDisableTiming)));
  if (e != hipSuccess) { // stay closed; what was allocated is the registry's until aleppo_destroy
    c->ev_obs = nullptr;
    c->ev_a1 = c->ev_a2 = c->ev_a3 = nullptr;
    c->ev_hpart = c->ev_logits = c->ev_values = c->ev_d_noise = c->ev_h_noise = nullptr;
    c->ev_actions = nullptr;
    c->ev_d_frames = c->ev_h_frames = c->ev_d_start = c->ev_h_start = nullptr;
    c->ev_d_done = nullptr;
    c->ev_h_actions = nullptr;
    return set_err(c, ALEPPO_ERR_HIP, std::string("eval_open: allocation failed: ") + hipGetErrorString(e));
  }
  std::memset(c->ev_h_actions, 0, (L + 8) * 8);
  c->ev_ticket = 0;
  c->ev_counter = 0;
  c->ev_acted = false;
  c->ev_L = num_lanes;
  return ALEPPO_OK;
}

extern "C" int aleppo_eval_push_frames(aleppo_ctx *c, const uint8_t *frames, int kind, int location,
                                       const uint8_t *episode_start) {
  CHECK_EVAL(c);
  if (!frames || !episode_start)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  if (kind != ALEPPO_FRAMES_84 && kind != ALEPPO_FRAMES_RAW_PAIR)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "unknown frame kind");
  const size_t L = (size_t)c->ev_L;
  const uint8_t *df = nullptr;
  if (int rc = resolve_frames(c, frames, location, &df)) // (before the staging buffers or the stream are touched)
    return rc;
  HIPCHK(c, hipEventSynchronize(c->ev_staged)); // the staging buffers are reused: the previous upload has run
  std::memcpy(c->ev_h_start, episode_start, L);
  HIPCHK(c, hipMemcpyAsync(c->ev_d_start, c->ev_h_start, L, hipMemcpyHostToDevice, c->stream));
  if (!df) { // ALEPPO_HOST
    const size_t bytes = L * (kind == ALEPPO_FRAMES_RAW_PAIR ? 2 * RAW_H * RAW_W : FRAME_PIX);
    std::memcpy(c->ev_h_frames, frames, bytes);
    HIPCHK(c, hipMemcpyAsync(c->ev_d_frames, c->ev_h_frames, bytes, hipMemcpyHostToDevice, c->stream));
    df = c->ev_d_frames;
  }
  // the rollout's ingest kernel on a one-slot "rollout": slot 0 is read and rewritten in place, pixel by pixel
  launch_ingest(c->stream, kind == ALEPPO_FRAMES_RAW_PAIR, df, c->lut, c->ev_d_start, nullptr, c->ev_obs, c->ev_L, 1, 0, 0);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev_staged, c->stream));
  rec_tick(c, ALEPPO_REC_EVAL);
  return ALEPPO_OK;
}

// the one check of an evaluation rule and its parameter (aleppo_eval_act, aleppo_eval_env_run)
int aleppo::eval_check_rule(aleppo_ctx *c, int rule, float param, bool has_noise, float *kparam) {
  *kparam = 0.f;
  if (rule == ALEPPO_EVAL_GREEDY) {
    if (param != 0.f || has_noise) // (a NaN param compares unequal too)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_act: the greedy rule takes param = 0 and no noise");
  } else if (rule == ALEPPO_EVAL_SAMPLE) {
    if (!(param > 0.f) || !std::isfinite(param) || !std::isfinite(1.0f / param))
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_act: the temperature must be finite and > 0");
    *kparam = 1.0f / param; // once, in fp32
  } else if (rule == ALEPPO_EVAL_EPSILON_GREEDY) {
    if (!(param >= 0.f && param <= 1.f))
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_act: epsilon must be in [0, 1]");
    *kparam = param;
  } else {
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_act: unknown rule");
  }
  const bool patch = c->prec == ALEPPO_BF16 && use_patch_kernels();
  if (!patch && !c->ev_a1)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   "eval_act: the lanes were opened without conv1 / conv2 scratch (set ALEPPO_OPT_GENERIC_CONV before "
                   "aleppo_eval_open)");
  return ALEPPO_OK;
}
// the acting half of one evaluation step: nothing here waits for the device
int aleppo::eval_act_enqueue(aleppo_ctx *c, int rule, float kparam, const float *dn) {
  const int L = c->ev_L;
  int64_t *pinned_dev = nullptr;
  HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void **>(&pinned_dev), c->ev_h_actions, 0));
  // the rollout's acting forward at L samples on the lanes' stacks, into the lanes' scratch, on the live parameters or -
  // ALEPPO_OPT_EVAL_PARAMS = 1 - on the averaged set of aleppo_ema_open
  const ParamView pv = eval_view(c);
  act_forward(c, pv, c->ev_obs, eval_map(), c->ev_a1, c->ev_a2, c->ev_a3, c->ev_hpart, L, false);
  launch_eval_head(c->stream, c->ev_hpart, Pf(c, pv, P_BFC), Pf(c, pv, P_WH), Pf(c, pv, P_BH), dn, c->cfg.seed ^ EVAL_KEY_DOMAIN,
                   c->ev_counter, rule, kparam, c->ev_logits, c->ev_values, c->ev_actions, pinned_dev, c->ev_d_done,
                   c->ev_ticket + 1, L, c->H, c->A);
  HIPCHK(c, hipGetLastError());
  c->ev_ticket++;
  c->ev_counter++;
  c->ev_acted = true;
  return ALEPPO_OK;
}

extern "C" int aleppo_eval_act(aleppo_ctx *c, int rule, float param, const float *noise, const int64_t **actions_pinned) {
  CHECK_EVAL(c);
  float kparam = 0.f;
  if (int rc = eval_check_rule(c, rule, param, noise != nullptr, &kparam))
    return rc;
  const int L = c->ev_L;
  const float *dn = nullptr;
  if (noise) { // (the previous call's head has finished - its ticket was waited for - so the staging is free)
    const size_t bytes = (size_t)L * (rule == ALEPPO_EVAL_SAMPLE ? c->A : 2) * 4;
    std::memcpy(c->ev_h_noise, noise, bytes);
    HIPCHK(c, hipMemcpyAsync(c->ev_d_noise, c->ev_h_noise, bytes, hipMemcpyHostToDevice, c->stream));
    dn = c->ev_d_noise;
  }
  if (int rc = eval_act_enqueue(c, rule, kparam, dn))
    return rc;
  // wait for the ticket the head publishes after the actions (bounded spin, then a real synchronise)
  volatile long long *tk = reinterpret_cast<volatile long long *>(c->ev_h_actions + L);
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 1; *tk != c->ev_ticket; ++spins) {
    __builtin_ia32_pause();
    if ((spins & 1023u) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2e-3) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      break;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  if (*tk != c->ev_ticket)
    return set_err(c, ALEPPO_ERR_RUNTIME, "eval_act: the evaluation head's ticket did not arrive");
  if (actions_pinned)
    *actions_pinned = c->ev_h_actions;
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_eval_set_counter(aleppo_ctx *c, uint64_t counter) {
  CHECK_EVAL(c);
  c->ev_counter = counter; // (host state only: every head launch takes the counter as an argument)
  return ALEPPO_OK;
}

extern "C" int aleppo_eval_read(aleppo_ctx *c, int field, void *dst, size_t bytes) {
  CHECK_EVAL(c);
  if (!dst)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null dst");
  const size_t L = (size_t)c->ev_L;
  size_t need = 0;
  switch (field) {
  case ALEPPO_EF_OBSERVATIONS:
    need = L * 4 * FRAME_PIX;
    break;
  case ALEPPO_EF_LOGITS:
    need = L * c->A * 4;
    break;
  case ALEPPO_EF_VALUES:
    need = L * 4;
    break;
  case ALEPPO_EF_ACTIONS:
    need = L * 8;
    break;
  default:
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_read: unknown field");
  }
  if (bytes != need)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "eval_read: wrong byte count");
  if (field != ALEPPO_EF_OBSERVATIONS && !c->ev_acted)
    return set_err(c, ALEPPO_ERR_RUNTIME, "eval_read: no aleppo_eval_act yet");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (field == ALEPPO_EF_OBSERVATIONS) {
    // unpacked into the (idle: the stream has drained) frame staging, which holds L raw pairs >= L NCHW stacks
    static_assert(2 * RAW_H * RAW_W >= 4 * FRAME_PIX, "frame staging holds an unpacked stack per lane");
    launch_obs_unpack(c->stream, c->ev_obs, c->ev_d_frames, (long)L, eval_map());
    HIPCHK(c, copy_sync(c, dst, c->ev_d_frames, need, hipMemcpyDeviceToHost));
  } else if (field == ALEPPO_EF_ACTIONS) {
    std::vector<int> a(L);
    HIPCHK(c, copy_sync(c, a.data(), c->ev_actions, L * 4, hipMemcpyDeviceToHost));
    int64_t *o = static_cast<int64_t *>(dst);
    for (size_t i = 0; i < L; ++i)
      o[i] = a[i];
  } else {
    HIPCHK(c, copy_sync(c, dst, field == ALEPPO_EF_LOGITS ? c->ev_logits : c->ev_values, need, hipMemcpyDeviceToHost));
  }
  return ALEPPO_OK;
}
