// api_refresh.hip - C ABI (include/aleppo.h), per-epoch advantage recomputation: aleppo_refresh_advantages,
// aleppo_refresh_read.  Between two aleppo_train calls on one rollout batch the critic has moved; the refresh forwards the
// batch's observation slots and the post-rollout observation in place (net_forward with train_map / slot_map, on any
// parameter set), keeps the value head's output in a second time-major plane (value_refresh_kernel, refresh.hip) and runs
// aleppo_finish_rollout's GAE scan - launch_gae in its "rewards as given, no log-probs" form - and advantage normalisation
// on it.  values_tm, the rewards, the old log-probs, the actions, the reward-scale state, the parameters and the moments
// are only read, and everything goes onto the context's main stream only.
#include "api_internal.hpp"

using namespace aleppo;

// what both calls refuse in the batch the context holds: only a rollout batch has a time axis, and only until the next
// rollout's first act carries slot T into slot 0
static int refresh_check_batch(aleppo_ctx *c, const char *who) {
  if (c->caller_batch)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   std::string(who) + ": the batch came from aleppo_set_batch and has no time axis to scan");
  if (c->batch_n != c->N || c->batch_n <= 0)
    return set_err(c, ALEPPO_ERR_RUNTIME, std::string(who) + ": no rollout batch: call aleppo_finish_rollout first");
  if (c->t != 0 || !c->need_carry)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   std::string(who) + ": the next rollout has begun (valid between aleppo_finish_rollout and the first "
                                      "aleppo_act / aleppo_step / aleppo_env_rollout after it)");
  return ALEPPO_OK;
}

extern "C" int aleppo_refresh_advantages(aleppo_ctx *c, int set, double *stats, size_t stat_count) {
  CHECK_CTX(c);
  if (stats ? stat_count != ALEPPO_REFRESH_STATS_COUNT : stat_count != 0)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "refresh_advantages: stat_count must be ALEPPO_REFRESH_STATS_COUNT, or 0 with NULL stats");
  ParamView view{};
  if (int rc = set_view(c, set, &view))
    return rc;
  if (int rc = refresh_check_batch(c, "refresh_advantages"))
    return rc;
  if (c->batch_refused)
    return set_err(c, ALEPPO_ERR_RUNTIME, "refresh_advantages: aleppo_finish_rollout refused this rollout's flags");
  if (c->world > 1 && !c->nccl_comm)
    return set_err(c, ALEPPO_ERR_RUNTIME, "world_size > 1 but aleppo_comm_init was not called");
  const int E = c->E, T = c->T, A = c->A, H = c->H;
  const int nblk = bstat_blocks(c->N);
  if (!c->fresh_tm)
    HIPCHK(c, dalloc(c, &c->fresh_tm, (size_t)(T + 1) * E * c->rsz));
  if (stats && !c->rf_scratch)
    HIPCHK(c, dalloc(c, &c->rf_scratch, (32 + (size_t)nblk * RSTAT_SUMS) * sizeof(double)));
  SampleSource src; // the whole batch (refresh_check_batch: batch_n == N), in place
  if (int rc = source_open(c, nullptr, 0, 0, &src))
    return rc;
  c->fresh_valid = false;
  const float *wv = Pf(c, view, P_WH) + (size_t)A * H, *bv = Pf(c, view, P_BH) + A;
  // the batch in logical order, then the post-rollout observation of every environment (slot T)
  source_walk(c, src, [&](const SampleMap &map, long n0, long ns) {
    net_forward(c, view, src.obs, map, ns);
    prof_begin(c, ALEPPO_K_ACT_STATS); // (the class of the read-only passes over the activations)
    launch_value_refresh(c->stream, c->h, wv, bv, c->fresh_tm, n0, ns, H, E, T, false, c->rt16);
    prof_end(c, ALEPPO_K_ACT_STATS);
    return ALEPPO_OK;
  });
  net_forward(c, view, c->obs, slot_map(c, T), E);
  prof_begin(c, ALEPPO_K_ACT_STATS);
  launch_value_refresh(c->stream, c->h, wv, bv, c->fresh_tm, 0, E, H, E, T, true, c->rt16);
  if (stats) { // before the scan overwrites the returns and advantages the last epoch trained on
    double *result = c->rf_scratch, *part = result + 32;
    launch_rstat_partial(c->stream, c->fresh_tm, c->values_tm, c->ret_n, c->adv_n, c->mask_n, c->N, E, T, part, c->rt16);
    launch_rstat_reduce(c->stream, part, nblk, result);
  }
  prof_end(c, ALEPPO_K_ACT_STATS);
  prof_begin(c, ALEPPO_K_GAE); // (the flags passed aleppo_finish_rollout's check: the scan leaves d_err alone)
  launch_gae(c->stream, c->step_rec, c->step_rec_bytes, c->fresh_tm, nullptr, nullptr, c->adv_n, c->ret_n, nullptr, nullptr,
             c->mask_n, c->d_err, E, T, A, c->cfg.gamma, c->cfg.lambda, false, c->rt16);
  prof_end(c, ALEPPO_K_GAE);
  if (c->cfg.advantage_norm) {
    launch_adv_norm(c->stream, c->adv_n, c->mask_n, c->adv_stats, c->N, 0, c->rt16);
    if ((c->world > 1 || c->force_comm) && c->nccl_comm)
      NCCLCHK(c, ncclAllReduce(c->adv_stats, c->adv_stats, 3, ncclFloat, ncclSum, static_cast<ncclComm_t>(c->nccl_comm),
                               c->stream));
    launch_adv_norm(c->stream, c->adv_n, c->mask_n, c->adv_stats, c->N, 1, c->rt16);
  }
  HIPCHK(c, hipGetLastError());
  double st[ALEPPO_REFRESH_STATS_COUNT]; // (through a host temporary: a failed call writes nothing)
  if (stats)
    HIPCHK(c, hipMemcpyAsync(st, c->rf_scratch, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  c->fresh_valid = true;
  if (stats)
    std::memcpy(stats, st, sizeof(st));
  return ALEPPO_OK;
}

// a plane stored as RT, time-major [T][E] (tm) or flat -> the caller's float array in reference layout, the way
// aleppo_read_batch returns its planes (the same two scratch buffers); complete when it returns
static int read_plane(aleppo_ctx *c, const void *src, size_t count, bool tm, float *dst) {
  HIPCHK(c, grow(c, &c->rb_tmp[0], &c->rb_cap[0], count * 4, ALLOC_RAW));
  if (tm) {
    HIPCHK(c, grow(c, &c->rb_tmp[1], &c->rb_cap[1], count * c->rsz, ALLOC_RAW));
    launch_transpose_tm_pitched(c->stream, src, (size_t)c->E * c->rsz, c->rb_tmp[1], c->E, c->T, 1, (int)c->rsz);
    src = c->rb_tmp[1];
  }
  launch_plane_to_float(c->stream, src, static_cast<float *>(c->rb_tmp[0]), (long)count, c->rt16);
  HIPCHK(c, copy_sync(c, dst, c->rb_tmp[0], count * 4, hipMemcpyDeviceToHost));
  return ALEPPO_OK;
}

extern "C" int aleppo_refresh_read(aleppo_ctx *c, float *values, size_t value_count, float *next_values,
                                   size_t next_count) {
  CHECK_CTX(c);
  if (!values && !next_values)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "refresh_read: null arguments");
  if ((values ? value_count != (size_t)c->N : value_count != 0) ||
      (next_values ? next_count != (size_t)c->E : next_count != 0))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "refresh_read: value_count must be E * horizon and next_count E (0 with a NULL pointer)");
  if (!c->fresh_valid || c->caller_batch || c->batch_n != c->N)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   "refresh_read: the batch the context holds has not been refreshed: call aleppo_refresh_advantages");
  const size_t N = (size_t)c->N, E = (size_t)c->E;
  if (values) // [T][E] as stored -> [E][T] float, through aleppo_read_batch's two scratch buffers
    if (int rc = read_plane(c, c->fresh_tm, N, true, values))
      return rc;
  if (next_values)
    if (int rc = read_plane(c, rp(c, c->fresh_tm, (size_t)c->T * E), E, false, next_values))
      return rc;
  return ALEPPO_OK;
}
