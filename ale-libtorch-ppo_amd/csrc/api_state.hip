// api_state.hip - C ABI (include/aleppo.h), the run state beyond the learner: the rollout side of a checkpoint
// (aleppo_export_rollout_state / aleppo_import_rollout_state) and the device-side digest of the whole run state
// (aleppo_state_digest).  All three are valid between rollouts only and synchronise the context's own stream only.
// Also the other read-only pass over the learner state: aleppo_tensor_stats (valid at any time no step is armed).
#include "api_internal.hpp"

using namespace aleppo;

// between rollouts: the next slot to fill is 0 (after aleppo_create, after aleppo_finish_rollout with or without
// aleppo_train); CHECK_CTX has already refused an armed step
static int between_rollouts(aleppo_ctx *c, const char *who) {
  if (c->t != 0)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   std::string(who) + ": valid between rollouts only (a rollout is in progress: finish it first)");
  return ALEPPO_OK;
}
// the slot that holds the observation the next aleppo_act acts on (what ALEPPO_F_CURRENT_OBS reads)
static inline int current_slot(const aleppo_ctx *c) { return (c->t == 0 && c->need_carry) ? c->T : c->t; }

extern "C" int aleppo_export_rollout_state(aleppo_ctx *c, uint8_t *observations, uint64_t words[4], size_t num_envs) {
  CHECK_CTX(c);
  if (!observations || !words)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "export_rollout_state: null argument");
  if (num_envs != (size_t)c->E)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "export_rollout_state: num_envs is not the context's");
  if (int rc = between_rollouts(c, "export_rollout_state"))
    return rc;
  if (int rc = aleppo_read_batch(c, ALEPPO_F_CURRENT_OBS, observations, num_envs * 4 * FRAME_PIX)) // (the same bytes)
    return rc;
  words[0] = c->rng_counter;
  words[1] = words[2] = words[3] = 0;
  return ALEPPO_OK;
}

extern "C" int aleppo_import_rollout_state(aleppo_ctx *c, const uint8_t *observations, const uint64_t words[4],
                                           size_t num_envs) {
  CHECK_CTX(c);
  if (!observations || !words)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "import_rollout_state: null argument");
  if (num_envs != (size_t)c->E)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "import_rollout_state: num_envs is not the context's");
  if (words[1] || words[2] || words[3])
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "import_rollout_state: a reserved word is not 0");
  if (int rc = between_rollouts(c, "import_rollout_state"))
    return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = stage_observations(c, observations, (int64_t)num_envs))
    return rc;
  // The stacks go where a finished rollout leaves its last observation, slot T, and the next rollout's first aleppo_act
  // carries them into slot 0 - the launches the exporting context would run.  Slots 0 .. T-1 may hold a batch that has not
  // been trained on yet: they are not written.
  launch_obs_pack(c->stream, c->stage_u8, c->obs, (long)num_envs, slot_map(c, c->T));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->need_carry = true;
  c->pre_acted = -1;       // (aleppo_step's pre-computed acting scratch belongs to the stacks that were replaced)
  c->act_queued_slot = -1;
  c->rng_counter = words[0];
  return ALEPPO_OK;
}

extern "C" int aleppo_state_digest(aleppo_ctx *c, uint64_t out[ALEPPO_DIGEST_COUNT]) {
  CHECK_CTX(c);
  if (!out)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "state_digest: null argument");
  if (int rc = between_rollouts(c, "state_digest"))
    return rc;
  if (int rc = ensure_rs_storage(c)) // (before the option was ever used: the initial state)
    return rc;
  if (!c->dg_out)
    HIPCHK(c, dalloc(c, &c->dg_out, ALEPPO_DIGEST_COUNT * sizeof(unsigned long long)));
  launch_state_digest(c->stream, c->P, c->M1, c->M2, c->L, c->adam_step, c->obs, c->T + 1, current_slot(c), c->E,
                      c->rng_counter, c->rs_blk, c->rs_g[c->rs_cur], c->dg_out);
  HIPCHK(c, hipGetLastError());
  unsigned long long host[ALEPPO_DIGEST_COUNT];
  HIPCHK(c, copy_sync(c, host, c->dg_out, sizeof(host), hipMemcpyDeviceToHost));
  for (int k = 0; k < ALEPPO_DIGEST_COUNT; ++k)
    out[k] = host[k];
  return ALEPPO_OK;
}

// Per-tensor norms of the parameters, the last minibatch's clipped gradient and the last optimizer step (aleppo.h), read
// the way the digest is: computed when called, by kernels that only read, on the context's stream.  Nothing here touches
// what a captured update bakes in, and no other entry point knows about it.
extern "C" int aleppo_tensor_stats(aleppo_ctx *c, int sections, double *out, size_t count) {
  CHECK_CTX(c);
  constexpr size_t COUNT = (size_t)ALEPPO_TENSOR_STATS_ROWS * ALEPPO_TENSOR_STATS_COLS;
  if (!out)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "tensor_stats: null argument");
  if (count != COUNT)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "tensor_stats: count must be 130");
  if (sections <= 0 || (sections & ~(ALEPPO_TS_SEC_PARAMS | ALEPPO_TS_SEC_STEP)))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "tensor_stats: sections must be ALEPPO_TS_SEC_PARAMS and / or _STEP");
  const bool step = (sections & ALEPPO_TS_SEC_STEP) != 0;
  if (step && !c->ts_step_valid)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   "tensor_stats: the step section needs an aleppo_train on this context with no aleppo_load_params / "
                   "aleppo_import_optimizer since");
  if (!c->ts_scratch)
    HIPCHK(c, dalloc(c, &c->ts_scratch, tensor_stats_scratch_bytes(c->L)));
  const double *dev = nullptr;
  launch_tensor_stats(c->stream, c->P, c->G, c->M1, c->M2, c->L, sections, step ? last_clip_coef(c) : 1.0f, c->ts_sched[0],
                      c->ts_sched[1], c->cfg.adam_eps, c->ts_scratch, &dev);
  HIPCHK(c, hipGetLastError());
  double host[COUNT];
  HIPCHK(c, copy_sync(c, host, dev, sizeof(host), hipMemcpyDeviceToHost));
  std::memcpy(out, host, sizeof(host));
  return ALEPPO_OK;
}
