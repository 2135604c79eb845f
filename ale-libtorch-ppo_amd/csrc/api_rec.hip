// api_rec.hip - C ABI (include/aleppo.h), the episode recorders: aleppo_rec_open, aleppo_rec_count, aleppo_rec_read,
// aleppo_rec_clear, and rec_capture, which aleppo_env_rollout / aleppo_eval_env_run call behind every step's ingest.  The
// kernel is rec_capture.hpp.  Works on the rec[] members only; reads (never writes) the sources' buffers.
#include "api_internal.hpp"
#include "rec_capture.hpp"

using namespace aleppo;

static_assert(sizeof(aleppo_rec_config) == 32, "aleppo_rec_config is 32 bytes (include/aleppo.h)");
static_assert(sizeof(aleppo_rec_step) == 32 && offsetof(aleppo_rec_step, action) == 8 && offsetof(aleppo_rec_step, value) == 16 &&
                  offsetof(aleppo_rec_step, start) == 20 && offsetof(aleppo_rec_step, lives) == 24,
              "aleppo_rec_step is 32 bytes without padding (include/aleppo.h)");
static_assert(sizeof(aleppo_rec_counts) == 40, "aleppo_rec_counts is 40 bytes (include/aleppo.h)");

constexpr int MAX_REC_CAPACITY = 65536;

static bool rec_source_ok(int source) { return source == ALEPPO_REC_ROLLOUT || source == ALEPPO_REC_EVAL; }
static bool rec_raw(const aleppo_ctx *c, int source) {
  return (source == ALEPPO_REC_ROLLOUT ? c->env_cfg.frame_kind : c->ee_cfg.frame_kind) == ALEPPO_FRAMES_RAW_PAIR;
}

extern "C" int aleppo_rec_open(aleppo_ctx *c, const aleppo_rec_config *cfg) {
  CHECK_CTX(c);
  if (!cfg)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_open: null config");
  if (!rec_source_ok(cfg->source))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_open: unknown source");
  const bool rollout = cfg->source == ALEPPO_REC_ROLLOUT;
  if (rollout ? !c->env_open : !c->ee_open)
    return set_err(c, ALEPPO_ERR_RUNTIME, rollout ? "rec_open: no device environments: call aleppo_env_open first"
                                                  : "rec_open: no evaluation environments: call aleppo_eval_env_open first");
  if (cfg->index < 0 || cfg->index >= (rollout ? c->E : c->ev_L))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_open: index out of range");
  if (cfg->content == 0 || (cfg->content & ~(ALEPPO_REC_FRAMES | ALEPPO_REC_OBSERVATION)))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_open: content must be ALEPPO_REC_FRAMES and / or ALEPPO_REC_OBSERVATION");
  if (cfg->capacity < 1 || cfg->capacity > MAX_REC_CAPACITY)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_open: capacity must be in [1, 65536]");
  for (int32_t r : cfg->reserved)
    if (r != 0)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_open: reserved must be 0");
  Ctx::Recorder &R = c->rec[cfg->source];
  if (R.open && std::memcmp(&R.cfg, cfg, sizeof *cfg) != 0)
    return set_err(c, ALEPPO_ERR_RUNTIME, "rec_open: this source's recorder is already open with another config");
  if (!R.open) {
    // steps | frames | observations | logits: every plane starts 16-byte aligned (32, 7056 and 67200 are multiples of 16)
    const size_t cap = (size_t)cfg->capacity, fb = rec_raw(c, cfg->source) ? (size_t)2 * RAW_H * RAW_W : (size_t)FRAME_PIX;
    const size_t sb = cap * sizeof(aleppo_rec_step), pf = (cfg->content & ALEPPO_REC_FRAMES) ? cap * fb : 0,
                 po = (cfg->content & ALEPPO_REC_OBSERVATION) ? cap * FRAME_PIX : 0;
    uint8_t *blk = nullptr;
    const hipError_t e = dalloc(c, &blk, sb + pf + po + cap * (size_t)c->A * 4);
    if (e != hipSuccess) {
      return set_err(c, ALEPPO_ERR_HIP, std::string("rec_open: allocation failed: ") + hipGetErrorString(e));
    }
    R.cfg = *cfg;
    R.blk = blk;
    R.steps = reinterpret_cast<aleppo_rec_step *>(blk);
    R.frames = pf ? blk + sb : nullptr;
    R.obs = po ? blk + sb + pf : nullptr;
    R.logits = reinterpret_cast<float *>(blk + sb + pf + po);
    R.frame_bytes = fb;
    R.open = true;
  }
  R.rows = R.dropped = R.ordinal = 0;
  return ALEPPO_OK;
}

// Every step of a source takes exactly one row, so the row is known here: the kernel gets finished pointers.
void aleppo::rec_capture(aleppo_ctx *c, int source, const aleppo_env_state *in, int t) {
  Ctx::Recorder &R = c->rec[source];
  const uint64_t ordinal = R.ordinal++;
  if (R.rows >= (uint64_t)R.cfg.capacity) {
    R.dropped++;
    return;
  }
  const size_t r = (size_t)R.rows++, i = (size_t)R.cfg.index, A = (size_t)c->A;
  const bool raw = rec_raw(c, source);
  RecCaptureArgs a{};
  a.in = in + i;
  if (source == ALEPPO_REC_ROLLOUT) {
    const size_t o = (size_t)t * c->E + i;
    a.frame_src = c->env_blk + i * R.frame_bytes;
    a.stack = c->obs + (i * (size_t)(c->T + 1) + (size_t)t + 1) * FRAME_PIX; // slot t + 1: what the ingest just formed
    a.logits = rp(c, c->logits_tm, o * A);
    a.value = rp(c, c->values_tm, o);
    a.action = c->actions_tm + o;
    a.max_steps = c->env_cfg.max_steps;
    a.max_return = c->env_cfg.max_return;
    a.rt16 = c->rt16;
  } else {
    a.frame_src = c->ee_blk + i * R.frame_bytes;
    a.stack = c->ev_obs + i * FRAME_PIX;
    a.logits = c->ev_logits + i * A;
    a.value = c->ev_values + i;
    a.action = c->ev_actions + i;
    a.max_steps = c->ee_cfg.max_steps;
    a.max_return = c->ee_cfg.max_return;
    a.rt16 = 0;
  }
  a.frame_dst = R.frames ? R.frames + r * R.frame_bytes : nullptr;
  a.obs_dst = R.obs ? R.obs + r * FRAME_PIX : nullptr;
  a.logits_dst = R.logits + r * A;
  a.step_dst = R.steps + r;
  a.ordinal = ordinal;
  a.A = c->A;
  const bool timed = source == ALEPPO_REC_ROLLOUT; // (the evaluation's launches are not bracketed: act_forward)
  if (timed)
    prof_begin(c, ALEPPO_K_REC_CAPTURE);
  if (raw) // a raw pair's 4200 16-byte words over ENV_RAW_PARTS workgroups, like its render; else one workgroup
    hipLaunchKernelGGL(rec_capture_kernel<true>, dim3(R.frames ? ENV_RAW_PARTS : 1), dim3(256), 0, c->stream, a);
  else
    hipLaunchKernelGGL(rec_capture_kernel<false>, dim3(1), dim3(256), 0, c->stream, a);
  if (timed)
    prof_end(c, ALEPPO_K_REC_CAPTURE);
}

extern "C" int aleppo_rec_count(aleppo_ctx *c, int source, aleppo_rec_counts *out) {
  CHECK_CTX_ANY(c); // host state only: valid while a step is armed
  if (!out)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_count: null argument");
  if (!rec_source_ok(source))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_count: unknown source");
  const Ctx::Recorder &R = c->rec[source];
  aleppo_rec_counts n{};
  if (R.open) {
    n.rows = R.rows;
    n.dropped = R.dropped;
    n.next_ordinal = R.ordinal;
    n.capacity = R.cfg.capacity;
    n.frame_bytes = R.frames ? (int32_t)R.frame_bytes : 0;
    n.observation_bytes = R.obs ? FRAME_PIX : 0;
    n.actions = c->A;
  }
  *out = n;
  return ALEPPO_OK;
}

extern "C" int aleppo_rec_read(aleppo_ctx *c, int source, int field, uint64_t first_row, uint64_t rows, void *dst,
                               size_t bytes) {
  CHECK_CTX(c);
  if (!rec_source_ok(source))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_read: unknown source");
  const Ctx::Recorder &R = c->rec[source];
  if (!R.open)
    return set_err(c, ALEPPO_ERR_RUNTIME, "rec_read: this source has no recorder: call aleppo_rec_open first");
  if (!dst)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_read: null dst");
  const uint8_t *src = nullptr;
  size_t row = 0;
  switch (field) {
  case ALEPPO_REC_F_STEPS:
    src = reinterpret_cast<const uint8_t *>(R.steps);
    row = sizeof(aleppo_rec_step);
    break;
  case ALEPPO_REC_F_LOGITS:
    src = reinterpret_cast<const uint8_t *>(R.logits);
    row = (size_t)c->A * 4;
    break;
  case ALEPPO_REC_F_FRAMES:
    src = R.frames;
    row = R.frame_bytes;
    break;
  case ALEPPO_REC_F_OBSERVATIONS:
    src = R.obs;
    row = FRAME_PIX;
    break;
  default:
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_read: unknown field");
  }
  if (!src)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_read: the field is not part of the recorder's content");
  if (first_row > R.rows || rows > R.rows - first_row)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_read: rows out of range");
  if (bytes != (size_t)rows * row)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_read: wrong byte count");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (rows)
    HIPCHK(c, copy_sync(c, dst, src + (size_t)first_row * row, bytes, hipMemcpyDeviceToHost));
  return ALEPPO_OK;
}

extern "C" int aleppo_rec_clear(aleppo_ctx *c, int source) {
  CHECK_CTX(c);
  if (!rec_source_ok(source))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "rec_clear: unknown source");
  Ctx::Recorder &R = c->rec[source];
  if (!R.open)
    return set_err(c, ALEPPO_ERR_RUNTIME, "rec_clear: this source has no recorder: call aleppo_rec_open first");
  R.rows = R.dropped = 0; // (captures already on the stream wrote their rows; later ones are ordered behind them)
  return ALEPPO_OK;
}
