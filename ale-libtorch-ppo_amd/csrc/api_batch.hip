// api_batch.hip - C ABI (include/aleppo.h), the batch boundary: aleppo_set_batch, aleppo_set_batch_values,
// aleppo_forward, aleppo_read_batch.
#include "api_internal.hpp"

using namespace aleppo;

// NCHW uint8 observations of the caller -> c->stage_u8 (device)
int aleppo::stage_observations(aleppo_ctx *c, const uint8_t *observations, int64_t n) {
  const size_t bytes = (size_t)n * 4 * FRAME_PIX;
  HIPCHK(c, grow(c, &c->stage_u8, &c->stage_u8_cap, bytes, ALLOC_RAW));
  HIPCHK(c, copy_sync(c, c->stage_u8, observations, bytes, hipMemcpyHostToDevice));
  return ALEPPO_OK;
}

extern "C" int aleppo_set_batch(aleppo_ctx *c, const uint8_t *observations, const int64_t *actions,
                                const float *log_probabilities, const float *advantages, const float *returns,
                                const uint8_t *masks, int64_t n) {
  CHECK_CTX(c);
  if (!observations || !actions || !log_probabilities || !advantages || !returns || !masks)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  if (n <= 0 || n > c->N)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "set_batch: n must be in [1, E*T]");
  std::vector<int> a32(n);
  for (int64_t i = 0; i < n; ++i) {
    if (actions[i] < 0 || actions[i] >= c->A)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "action index out of range");
    a32[i] = (int)actions[i];
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->pre_acted = -1;
  int rc = stage_observations(c, observations, n);
  if (rc)
    return rc;
  launch_obs_pack(c->stream, c->stage_u8, c->obs, n, train_map(c, 0));
  HIPCHK(c, copy_sync(c, c->act_n, a32.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  if (!c->rt16) {
    HIPCHK(c, copy_sync(c, c->oldlp_n, log_probabilities, (size_t)n * c->A * 4, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->adv_n, advantages, (size_t)n * 4, hipMemcpyHostToDevice));
    HIPCHK(c, copy_sync(c, c->ret_n, returns, (size_t)n * 4, hipMemcpyHostToDevice));
  } else { // half planes: upload as float into the (idle) metric scratch area, round on the device
    rc = ensure_metric_storage(c, 1, 1, (long)n * std::max(c->A, 1));
    if (rc)
      return rc;
    const struct {
      const float *src;
      void *dst;
      size_t cnt;
    } pl[3] = {{log_probabilities, c->oldlp_n, (size_t)n * c->A}, {advantages, c->adv_n, (size_t)n}, {returns, c->ret_n, (size_t)n}};
    for (const auto &q : pl) {
      HIPCHK(c, copy_sync(c, c->metric_ps, q.src, q.cnt * 4, hipMemcpyHostToDevice));
      launch_plane_from_float(c->stream, c->metric_ps, q.dst, (long)q.cnt, true);
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  HIPCHK(c, copy_sync(c, c->mask_n, masks, (size_t)n, hipMemcpyHostToDevice));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->batch_n = n;
  c->caller_batch = true;
  c->val_src = Ctx::VAL_NONE; // (values supplied for an earlier batch are forgotten)
  return ALEPPO_OK;
}

extern "C" int aleppo_set_batch_values(aleppo_ctx *c, const float *values, int64_t n) {
  CHECK_CTX(c);
  if (!values)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  if (!c->caller_batch)
    return set_err(c, ALEPPO_ERR_RUNTIME, "set_batch_values: no caller batch (call aleppo_set_batch first)");
  if (n != c->batch_n)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "set_batch_values: n must be the n of the last aleppo_set_batch");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc = ensure_val_storage(c);
  if (rc)
    return rc;
  if (!c->rt16) {
    HIPCHK(c, copy_sync(c, c->val_n, values, (size_t)n * 4, hipMemcpyHostToDevice));
  } else { // half plane: upload as float into the (idle) metric scratch area, round on the device (as aleppo_set_batch)
    if ((rc = ensure_metric_storage(c, 1, 1, (long)n)))
      return rc;
    HIPCHK(c, copy_sync(c, c->metric_ps, values, (size_t)n * 4, hipMemcpyHostToDevice));
    launch_plane_from_float(c->stream, c->metric_ps, c->val_n, (long)n, true);
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  c->val_src = Ctx::VAL_CALLER;
  return ALEPPO_OK;
}

extern "C" int aleppo_forward(aleppo_ctx *c, const uint8_t *observations, int64_t n, float *logits, float *values) {
  CHECK_CTX(c);
  if (!observations || !logits || !values)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  if (n <= 0 || n > c->maxB)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "forward: n exceeds capacity");
  SampleSource src;
  if (int rc = source_open(c, observations, 0, n, &src))
    return rc;
  net_forward(c, src.obs, src.map, n); // (one chunk: n <= maxB)
  launch_heads_fwd(c->stream, c->h, Pf(c, P_WH), Pf(c, P_BH), c->logits_b, c->values_b, n, c->H, c->A);
  HIPCHK(c, hipMemcpyAsync(logits, c->logits_b, (size_t)n * c->A * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(values, c->values_b, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_read_batch(aleppo_ctx *c, int field, void *dst, size_t bytes) {
  CHECK_CTX(c);
  if (!dst)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null dst");
  const int E = c->E, T = c->T, A = c->A;
  const size_t N = (size_t)c->N;
  hipStream_t s = c->stream;
  size_t need = 0;
  // device scratch owned by the context, grown on demand
  auto scratch = [&](int k, size_t nbytes, void **out) -> int {
    HIPCHK(c, grow(c, &c->rb_tmp[k], &c->rb_cap[k], nbytes, ALLOC_RAW));
    *out = c->rb_tmp[k];
    return ALEPPO_OK;
  };
  void *tmp = nullptr;
  auto fin = [&](const void *src) -> int {
    if (bytes != need)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_batch: wrong byte count");
    HIPCHK(c, copy_sync(c, dst, src, need, hipMemcpyDeviceToHost));
    return ALEPPO_OK;
  };
  auto transposed = [&](const void *src, size_t pitch, int inner, int elem) -> int {
    need = N * inner * elem;
    if (int rc = scratch(0, need, &tmp))
      return rc;
    launch_transpose_tm_pitched(s, src, pitch, tmp, E, T, inner, elem);
    return fin(tmp);
  };
  // float planes stored as RT: [count] elements, env-major already (tm = false) or time-major [T][E][inner]
  auto plane = [&](const void *src, size_t count, bool tm, int inner) -> int {
    need = count * 4;
    if (bytes != need)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_batch: wrong byte count");
    if (!c->rt16 && !tm)
      return fin(src);
    if (int rc = scratch(0, need, &tmp))
      return rc;
    if (tm) {
      void *em = nullptr;
      if (int rc = scratch(1, count * c->rsz, &em))
        return rc;
      launch_transpose_tm_pitched(s, src, (size_t)E * inner * c->rsz, em, E, T, inner, (int)c->rsz);
      src = em;
    }
    launch_plane_to_float(s, src, static_cast<float *>(tmp), (long)count, c->rt16);
    return fin(tmp);
  };
  switch (field) {
  case ALEPPO_F_OBSERVATIONS: {
    need = N * 4 * FRAME_PIX;
    if (int rc = scratch(0, need, &tmp))
      return rc;
    launch_obs_unpack(s, c->obs, static_cast<uint8_t *>(tmp), (long)N, train_map(c, 0));
    return fin(tmp);
  }
  case ALEPPO_F_CURRENT_OBS: {
    need = (size_t)E * 4 * FRAME_PIX;
    if (int rc = scratch(0, need, &tmp))
      return rc;
    const int slot = (c->t == 0 && c->need_carry) ? T : c->t;
    launch_obs_unpack(s, c->obs, static_cast<uint8_t *>(tmp), E, slot_map(c, slot));
    return fin(tmp);
  }
  case ALEPPO_F_ACTIONS: {
    need = N * 8;
    if (bytes != need)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_batch: wrong byte count");
    std::vector<int> a(N);
    HIPCHK(c, copy_sync(c, a.data(), c->act_n, N * 4, hipMemcpyDeviceToHost));
    int64_t *o = static_cast<int64_t *>(dst);
    for (size_t i = 0; i < N; ++i)
      o[i] = a[i];
    return ALEPPO_OK;
  }
  case ALEPPO_F_REWARDS:
    return transposed(c->step_rec, c->step_rec_bytes, 1, 4);
  case ALEPPO_F_TERMINALS:
    return transposed(c->step_rec + 4 * (size_t)E, c->step_rec_bytes, 1, 1);
  case ALEPPO_F_TRUNCATIONS:
    return transposed(c->step_rec + 5 * (size_t)E, c->step_rec_bytes, 1, 1);
  case ALEPPO_F_LOGITS:
    return plane(c->logits_tm, N * A, true, A);
  case ALEPPO_F_VALUES:
    return plane(c->values_tm, N, true, 1);
  case ALEPPO_F_MASKS:
    need = N;
    return fin(c->mask_n);
  case ALEPPO_F_ADVANTAGES:
    return plane(c->adv_n, N, false, 1);
  case ALEPPO_F_RETURNS:
    return plane(c->ret_n, N, false, 1);
  case ALEPPO_F_LOG_PROBS:
    return plane(c->oldlp_n, N * A, false, A);
  case ALEPPO_F_NEXT_VALUES:
    return plane(rp(c, c->values_tm, (size_t)T * E), (size_t)E, false, 1);
  case ALEPPO_F_BATCH_STATS: { // computed here, when it is read (aleppo.h): nothing is enqueued anywhere else for it
    need = ALEPPO_BATCH_STATS_COUNT * sizeof(double);
    if (bytes != need)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_batch: wrong byte count");
    const long n = c->batch_n;
    if (n <= 0)
      return set_err(c, ALEPPO_ERR_RUNTIME, "no batch: call aleppo_finish_rollout or aleppo_set_batch first");
    if (c->val_src == Ctx::VAL_NONE)
      return set_err(c, ALEPPO_ERR_RUNTIME,
                     "ALEPPO_F_BATCH_STATS needs the batch's values: call aleppo_set_batch_values after aleppo_set_batch");
    if (c->world > 1 && !c->nccl_comm)
      return set_err(c, ALEPPO_ERR_RUNTIME, "world_size > 1 but aleppo_comm_init was not called");
    const bool dp = c->world > 1 || (c->nccl_comm && c->force_comm);
    // scratch: [0, 16) the results, [16, 32) the sums (all-reduced in place), then the partials of stage 1
    const int nblk = bstat_blocks(n);
    if (int rc = scratch(1, (32 + (size_t)nblk * BSTAT_SUMS) * sizeof(double), &tmp))
      return rc;
    double *result = static_cast<double *>(tmp), *sums = result + 16, *part = result + 32;
    // a rollout batch's values are slots 0..T-1 of values_tm ([T+1][E], time-major), indexed in place: val_n stays what
    // the last update or aleppo_set_batch_values made it
    const bool tm = c->val_src == Ctx::VAL_ROLLOUT;
    launch_bstat_partial(s, tm ? c->values_tm : c->val_n, c->ret_n, c->adv_n, c->mask_n, n, tm ? E : 0, tm ? T : 0, part,
                         c->rt16);
    launch_bstat_reduce(s, part, nblk, dp ? sums : nullptr, dp ? nullptr : result);
    if (dp) {
      NCCLCHK(c, ncclAllReduce(sums, sums, BSTAT_SUMS, ncclDouble, ncclSum, static_cast<ncclComm_t>(c->nccl_comm), s));
      launch_bstat_finalise(s, sums, result);
    }
    return fin(result);
  }
  case ALEPPO_F_REWARD_SCALE: {
    need = ALEPPO_REWARD_SCALE_COUNT * sizeof(double);
    if (bytes != need)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_batch: wrong byte count");
    if (int rc = ensure_rs_storage(c))
      return rc;
    double blk[RS_BLOCK];
    HIPCHK(c, copy_sync(c, blk, c->rs_blk, sizeof(blk), hipMemcpyDeviceToHost));
    unsigned long long clipped;
    std::memcpy(&clipped, &blk[RS_CLIPPED], 8);
    double *o = static_cast<double *>(dst);
    for (int k = 0; k < 5; ++k)
      o[k] = blk[k];
    o[5] = (double)clipped;
    return ALEPPO_OK;
  }
  default:
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_batch: unknown field");
  }
}
