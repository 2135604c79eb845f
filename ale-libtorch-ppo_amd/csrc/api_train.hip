// api_train.hip - C ABI (include/aleppo.h), the PPO update: aleppo_train as a plan plus named phases, and the read-backs
// of what the last update left (aleppo_read_train_metric, aleppo_read_sample_order).
#include "api_internal.hpp"

using namespace aleppo;

// ------------------------------------------------------------------ update
int aleppo::ensure_metric_storage(aleppo_ctx *c, int epochs, int M, long B) {
  const size_t need = (size_t)epochs * M * B;
  HIPCHK(c, grow(c, &c->metric_ps, &c->metric_cap, need, need * 7 * 4, ALLOC_ZEROED)); // aleppo_metric_field 0-6
  const size_t nm = (size_t)epochs * M;
  if (nm > c->metric_red_cap) {
    c->metric_red_cap = 0; // (the group grows together: until all of it has, the capacity claims nothing)
    c->last_advn = false;  // (its statistics went with the old buffer)
    c->last_kl = false;   // (and so did the KL means)
    HIPCHK(c, dalloc(c, &c->metric_red, nm * METRIC_REC * 4));
    HIPCHK(c, dalloc(c, &c->grad_norms, nm * 4));
    HIPCHK(c, dalloc(c, &c->adam_sched, nm * 2 * 4));
    HIPCHK(c, dalloc(c, &c->advn_part, nm * 4 * 8));  // ALEPPO_OPT_ADV_NORM_MINIBATCH (n, S, Q, 0) per minibatch
    HIPCHK(c, dalloc(c, &c->advn_stats, nm * 4 * 4)); // ... and (mean_f, inv_f, std, 0)
    HIPCHK(c, halloc(c, &c->h_metric_red, nm * (METRIC_REC + 1) * 4,
                            hipHostMallocDefault)); // records, then the grad norms
    HIPCHK(c, halloc(c, &c->h_adam_sched, nm * 2 * 4, hipHostMallocDefault));
    HIPCHK(c, halloc(c, &c->h_advn_stats, nm * 4 * 4, hipHostMallocDefault));
    c->metric_red_cap = nm;
  }
  return ALEPPO_OK;
}

// ALEPPO_OPT_MINIBATCH_SHUFFLE: order + gathered planes for epochs x N samples, mask counts and round keys per epoch / minibatch
// (grown together, like the metric storage)
static int ensure_shuffle_storage(aleppo_ctx *c, int epochs, long N) {
  const size_t ns = (size_t)epochs * N;
  if (ns > c->shuf_cap || epochs > c->shuf_epochs_cap) {
    c->shuf_cap = 0;
    c->shuf_epochs_cap = 0;
    HIPCHK(c, dalloc(c, &c->order, ns * 4));
    HIPCHK(c, dalloc(c, &c->act_p, ns * 4));
    HIPCHK(c, dalloc(c, &c->oldlp_p, ns * c->A * c->rsz));
    HIPCHK(c, dalloc(c, &c->adv_p, ns * c->rsz));
    HIPCHK(c, dalloc(c, &c->ret_p, ns * c->rsz));
    HIPCHK(c, dalloc(c, &c->val_p, ns * c->rsz));
    HIPCHK(c, dalloc(c, &c->mask_p, ns));
    HIPCHK(c, dalloc(c, &c->mask_counts_ep, ns * 4)); // (epochs * M <= epochs * N counts)
    HIPCHK(c, dalloc(c, &c->shuf_keys, (size_t)epochs * 16));
    HIPCHK(c, halloc(c, &c->h_shuf_keys, (size_t)epochs * 16, hipHostMallocDefault));
    c->shuf_cap = ns;
    c->shuf_epochs_cap = epochs;
  }
  return ALEPPO_OK;
}

// ALEPPO_OPT_KL_PENALTY: beta's device word (allocated once, never moved: graphs bake it) and the per-sample exact-KL
// plane, as large as one field of metric_ps (regrown with it; the graph key holds its address)
static int ensure_kl_storage(aleppo_ctx *c) {
  if (!c->kl_beta) {
    HIPCHK(c, dalloc(c, &c->kl_beta, 16));
    HIPCHK(c, halloc(c, &c->h_kl_beta, 16, hipHostMallocDefault));
  }
  if (c->kl_cap < c->metric_cap) {
    c->last_kl = false;
    HIPCHK(c, grow(c, &c->kl_ps, &c->kl_cap, c->metric_cap, c->metric_cap * 4, ALLOC_ZEROED));
  }
  return ALEPPO_OK;
}

// ALEPPO_OPT_VALUE_CLIP: the env-major old-values plane, RT [E*T] (allocated on first use, never moved: graphs bake it)
int aleppo::ensure_val_storage(aleppo_ctx *c) {
  if (!c->val_n)
    HIPCHK(c, dalloc(c, &c->val_n, (size_t)c->N * c->rsz));
  return ALEPPO_OK;
}

// half width h of the Feistel network over [0, 2^(2h)) for N samples: 2h = ceil(log2 N), at least 2, rounded up to even
static int feistel_half_width(long N) {
  int w = 0;
  while ((1L << w) < N)
    ++w;
  w = std::max(w, 2);
  return (w + 1) / 2;
}

// Which record of a per-minibatch array (mask counts, advantage statistics) belongs to minibatch i = ep * M + mb: an
// update over gathered planes keeps one per (epoch, minibatch); a contiguous one reads the same `period` = M slices every
// epoch and keeps M.  (aleppo_read_sample_order: the same rule over samples, period = N.)
static inline size_t record_index(bool per_epoch, size_t period, size_t i) { return per_epoch ? i : i % period; }

// The per-sample planes one update reads: the batch's contiguous env-major planes, or - ALEPPO_OPT_MINIBATCH_SHUFFLE - the
// planes gathered into every epoch's order ([epochs][N]).  Decided once, in plan_update; the enqueue functions and the
// read-back only ask where minibatch (ep, mb) lies.
struct Planes {
  const int *act;
  void *oldlp, *adv, *ret, *vold; // RT planes; vold: nullptr unless ALEPPO_OPT_VALUE_CLIP
  const uint8_t *mask;
  const int32_t *order; // [epochs][N] sample order (SampleMap::idx), or nullptr: contiguous
  float *counts;        // [ncounts] global unmasked count per record
  int ncounts;          // records of the per-minibatch arrays: epochs * M gathered, M contiguous
  size_t epoch_stride;  // samples between two epochs' planes: N gathered, 0 contiguous
  long B;
  int M;
  // position of minibatch (ep, mb)'s first sample in the planes
  size_t offset(int ep, int mb) const { return (size_t)ep * epoch_stride + (size_t)mb * B; }
  // its record in counts / advn_stats
  size_t record(int ep, int mb) const { return record_index(order != nullptr, (size_t)M, (size_t)ep * M + mb); }
  // the order of epoch ep's samples (nullptr: contiguous)
  const int32_t *idx(int ep) const { return order ? order + (size_t)ep * epoch_stride : nullptr; }
};

// Everything one aleppo_train call decides before it enqueues anything: built once by plan_update, read by every phase.
struct UpdatePlan {
  int epochs, M, nm; // nm = epochs * M optimizer steps
  long N, B;
  bool shuffle, vclip, val_transpose, advn, klpen, dp, two, bwd_fused;
  bool reg;            // ALEPPO_OPT_WEIGHT_DECAY / ALEPPO_OPT_ANCHOR_COEF: either is non-zero - reg_step_kernel, not adam_kernel
  const float *anchor; // ... the anchor it reads (nullptr: none, and then the anchor coefficient is zero)
  hipStream_t s, sw; // main stream; stream of the weight-gradient kernels (== s unless two)
  ncclComm_t comm;
  // The hyper-parameters of this call (ALEPPO_OPT_CLIP_PARAM and its kin), and the device block they are uploaded to:
  // the head and Adam kernels read them there, so a captured update follows them
  Hyper hp;
  const float *hpd;
  int shuf_h, nblk_head, nblk_sq;
  size_t fs; // field stride of the per-sample metric arrays
  // What the head kernel writes and reads per minibatch: the per-sample metric planes, the advantage statistics, beta and
  // the exact-KL plane - the context's for aleppo_train, private ones for aleppo_grad_probe - and the batch sample the
  // first minibatch starts at (0 for aleppo_train)
  float *metric_ps, *kl_ps;
  const float *advn_stats, *kl_beta;
  long n0;
  float *sW1, *sB1, *sW2, *sB2, *sW3, *sB3, *sWfc, *sBfc, *sWh, *sBh; // split-K gradient slabs
  Planes pl;
};

// The kernel routes of a minibatch of p.B samples: the slabs, the grids of the head and the norm pass, one stream or two, the
// fused or the split tail of the conv backward.  whole_cus: nothing else (an all-reduce) shares the CUs with the backward
static void plan_routes(aleppo_ctx *c, UpdatePlan &p, bool whole_cus) {
  const long B = p.B;
  p.sW1 = c->slab + c->slab_off[0], p.sB1 = c->slab + c->slab_off[1], p.sW2 = c->slab + c->slab_off[2];
  p.sB2 = c->slab + c->slab_off[3], p.sW3 = c->slab + c->slab_off[4], p.sB3 = c->slab + c->slab_off[5];
  p.sWfc = c->slab + c->slab_off[6], p.sBfc = c->slab + c->slab_off[7], p.sWh = c->slab + c->slab_off[8];
  p.sBh = c->slab + c->slab_off[9];
  p.nblk_head = (int)std::min<long>(MAXS_HEAD, (B + 15) / 16);
  p.nblk_sq = (int)std::min<size_t>(800, (c->L.off[P_W1] + 4095) / 4096); // + 129 conv1 chunks <= 1024 partials

  // The three weight-gradient kernels (and the slab reduce of bucket 0) run on their own stream
  // next to the dgrad chain (fc wgrad || fc dgrad, conv3 wgrad || conv3 dgrad, conv2 wgrad || conv2 dgrad -> conv1
  // wgrad).  Every kernel is a latency-bound full-GPU persistent grid: co-scheduling fills the drain / ramp bubbles
  // between dependent launches (everything on one stream measured 8.80 ms per update).
  p.two = !c->serial_update; // (ALEPPO_OPT_SERIAL_UPDATE: profiling brackets every kernel on the stream it runs on)
  // (Not with data parallelism: the fused kernel's 512-register workgroups need whole CUs, and bucket 0's all-reduce - whose
  // RCCL kernels are resident on some of them by the time the dgrad chain gets there - is what the conv backward is meant to
  // run BESIDE; the three launches share CUs with it, the fused kernel's workgroups on those CUs would start when it ends.)
  p.bwd_fused = (c->tune.fused_bwd == 2 || (c->tune.fused_bwd == 1 && B >= 2048)) && c->prec == ALEPPO_BF16 &&
                use_patch_kernels() && whole_cus;
  p.sw = p.two ? c->wg_stream : p.s; // stream of the weight-gradient kernels
}

// Argument checks, storage, lazy stream creation and every flag decision of one call.
static int plan_update(aleppo_ctx *c, int epochs, int M, UpdatePlan *plan) {
  UpdatePlan &p = *plan;
  if (epochs <= 0 || M <= 0)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "epochs and num_mini_batches must be positive");
  const long N = c->batch_n;
  if (N <= 0)
    return set_err(c, ALEPPO_ERR_RUNTIME, "no batch: call aleppo_finish_rollout or aleppo_set_batch first");
  if (c->anchor_coef_bits != 0 && !c->anchor.on)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   "ALEPPO_OPT_ANCHOR_COEF > 0 needs an anchor: call aleppo_anchor_take or aleppo_anchor_import first");
  c->pre_acted = -1; // the update's activations overwrite the acting scratch, and the weights change
  c->bwd.B = 0;      // (aleppo_export_backward: valid again once this update has run)
  acted_clear(c);    // (aleppo_export_acting: nothing to read until the next acting forward)
  if (N % M != 0)
    return set_err(c, ALEPPO_ERR_RUNTIME, "Batch size must be divisible by num_mini_batches"); // train.h:140-143
  const long B = N / M;
  if (B > c->maxB)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "minibatch larger than config.max_minibatch");
  if (M > 4096)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "num_mini_batches > 4096");
  if (c->world > 1 && !c->nccl_comm)
    return set_err(c, ALEPPO_ERR_RUNTIME, "world_size > 1 but aleppo_comm_init was not called");
  p.epochs = epochs;
  p.M = M;
  p.nm = epochs * M;
  p.N = N;
  p.B = B;
  p.vclip = c->value_clip;
  if (p.vclip && c->val_src == Ctx::VAL_NONE)
    return set_err(c, ALEPPO_ERR_RUNTIME,
                   "ALEPPO_OPT_VALUE_CLIP needs the batch's old values: call aleppo_set_batch_values after aleppo_set_batch");
  int rc = ensure_metric_storage(c, epochs, M, B);
  if (rc)
    return rc;
  p.shuffle = c->shuffle;
  p.advn = c->adv_norm_mb; // ALEPPO_OPT_ADV_NORM_MINIBATCH (statistics in advn_stats, grown with the metrics)
  p.klpen = c->kl_pen;     // ALEPPO_OPT_KL_PENALTY (the exact-KL plane kl_ps, beta in kl_beta)
  p.reg = c->wd_bits != 0 || c->anchor_coef_bits != 0; // (valid patterns are >= +0.0f: non-zero bits are a value > 0)
  p.anchor = p.reg && c->anchor.on ? c->anchor.P : nullptr;
  if (p.klpen && (rc = ensure_kl_storage(c)))
    return rc;
  if (p.shuffle && (rc = ensure_shuffle_storage(c, epochs, N)))
    return rc;
  if (p.vclip && (rc = ensure_val_storage(c)))
    return rc;
  // a rollout batch's old values are slots 0..T-1 of values_tm ([T+1][E], time-major): transposed inside the update
  p.val_transpose = p.vclip && c->val_src == Ctx::VAL_ROLLOUT;
  p.comm = static_cast<ncclComm_t>(c->nccl_comm);
  p.dp = c->world > 1 || (c->nccl_comm && c->force_comm); // force_comm: 1-rank communicator (tests)
  // side streams, created on first use (see aleppo_create): the weight-gradient stream, and - only with data parallelism -
  // the communication stream
  if (!c->wg_stream)
    HIPCHK(c, hipStreamCreateWithFlags(&c->wg_stream, hipStreamNonBlocking));
  if (p.dp && !c->comm_stream)
    HIPCHK(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
  p.s = c->stream;
  p.hp = c->hyper;
  p.hpd = c->hyper_blk;
  p.shuf_h = feistel_half_width(N);

  p.fs = c->metric_cap;
  p.metric_ps = c->metric_ps, p.kl_ps = c->kl_ps, p.advn_stats = c->advn_stats, p.kl_beta = c->kl_beta;
  p.n0 = 0;
  plan_routes(c, p, !p.dp);

  // the per-sample planes: position n0 + b of the batch, or of epoch ep's gathered planes (the storage above is final)
  Planes &pl = p.pl;
  pl.B = B;
  pl.M = M;
  if (p.shuffle) {
    pl.act = c->act_p, pl.oldlp = c->oldlp_p, pl.adv = c->adv_p, pl.ret = c->ret_p, pl.vold = c->val_p;
    pl.mask = c->mask_p, pl.order = c->order, pl.counts = c->mask_counts_ep;
    pl.ncounts = p.nm;
    pl.epoch_stride = (size_t)N;
  } else {
    pl.act = c->act_n, pl.oldlp = c->oldlp_n, pl.adv = c->adv_n, pl.ret = c->ret_n, pl.vold = c->val_n;
    pl.mask = c->mask_n, pl.order = nullptr, pl.counts = c->mask_counts;
    pl.ncounts = M;
    pl.epoch_stride = 0;
  }
  if (!p.vclip)
    pl.vold = nullptr;
  return ALEPPO_OK;
}

// The call's device-side scalars, uploaded once on the main stream in front of the update.
static int upload_call_scalars(aleppo_ctx *c, const UpdatePlan &p, double lr) {
  hipStream_t s = p.s;
  // Adam's per-step scalars for the whole call, uploaded once: step size lr / (1 - beta1^t) and sqrt(1 - beta2^t) are
  // DEVICE values the Adam kernel reads (kernel arguments would be baked into a captured graph)
  for (int i = 0; i < p.nm; ++i) {
    const double b1 = c->cfg.adam_beta1, b2 = c->cfg.adam_beta2, t = (double)(c->adam_step + i + 1);
    c->h_adam_sched[2 * i] = (float)(lr / (1.0 - std::pow(b1, t)));
    c->h_adam_sched[2 * i + 1] = (float)std::sqrt(1.0 - std::pow(b2, t));
  }
  HIPCHK(c, hipMemcpyAsync(c->adam_sched, c->h_adam_sched, (size_t)p.nm * 8, hipMemcpyHostToDevice, s));
  // ... and the hyper-parameter block, for the same reason
  float *b = c->h_hyper_blk;
  std::memset(b, 0, HYPER_BLOCK * 4);
  b[HYPER_CLIP] = p.hp.clip;
  b[HYPER_VCLIP] = c->vclip_range_set ? c->value_clip_range : p.hp.clip;
  b[HYPER_CV] = p.hp.c_v;
  b[HYPER_CE] = p.hp.c_e;
  b[HYPER_MAX_NORM] = p.hp.max_norm;
  // the decoupled terms' factors f_wd = lr * wd and f_an = lr * la, formed in double and rounded once (aleppo.h); both are
  // uploaded by every call, and only reg_step_kernel reads them
  float wd, la;
  std::memcpy(&wd, &c->wd_bits, 4);
  std::memcpy(&la, &c->anchor_coef_bits, 4);
  b[HYPER_WD] = (float)(lr * (double)wd);
  b[HYPER_ANCHOR] = (float)(lr * (double)la);
  HIPCHK(c, hipMemcpyAsync(c->hyper_blk, c->h_hyper_blk, HYPER_BLOCK * 4, hipMemcpyHostToDevice, s));
  // ... and, with ALEPPO_OPT_KL_PENALTY, beta: the head kernel reads it from device memory for the same reason
  if (p.klpen) {
    std::memcpy(c->h_kl_beta, &c->kl_coef_bits, 4);
    HIPCHK(c, hipMemcpyAsync(c->kl_beta, c->h_kl_beta, 4, hipMemcpyHostToDevice, s));
  }
  // ... and, with ALEPPO_OPT_MINIBATCH_SHUFFLE, the round keys of every epoch's permutation (aleppo.h): keyed by the Adam
  // step the epoch starts at, so a graph replay reads this call's keys and a resumed run replays the same orders
  if (p.shuffle) {
    for (int e = 0; e < p.epochs; ++e) {
      const uint64_t step0 = (uint64_t)(c->adam_step + (int64_t)e * p.M);
      const uint64_t key = splitmix64(c->cfg.seed ^ splitmix64(((uint64_t)(uint32_t)c->rank << 40) ^ step0));
      for (int r = 0; r < 4; ++r)
        c->h_shuf_keys[4 * e + r] = (uint32_t)splitmix64(key + (uint64_t)r);
    }
    HIPCHK(c, hipMemcpyAsync(c->shuf_keys, c->h_shuf_keys, (size_t)p.epochs * 16, hipMemcpyHostToDevice, s));
  }
  return ALEPPO_OK;
}

// (Tried in round 3, tests/tools/forkbench.hip: in isolation an event record + wait costs the pair of streams ~12 us
// per dependency, a one-wave signal kernel + a one-wave gate kernel on a device word ~3 us.  In the update it changes
// nothing or loses: with signal kernels the weight-gradient kernel is released BEFORE the dgrad kernel beside it has its
// workgroups on the CUs and the dgrad chain slows down (485 vs 458 us per minibatch); with the dgrad kernel itself
// announcing its start the main stream runs without gaps - and the minibatch takes 445 vs 444 us: the two streams
// together keep the GPU saturated, so a gap on one is filled by the other.  DESIGN.md 4a.)
static hipError_t fork_wgrad_stream(const UpdatePlan &p, hipEvent_t ev) { // sw continues after everything enqueued on s so far
  if (!p.two)
    return hipSuccess;
  const hipError_t e = hipEventRecord(ev, p.s);
  return e != hipSuccess ? e : hipStreamWaitEvent(p.sw, ev, 0);
}

// What comes before the minibatches: value transpose, shuffle gather, mask counts, advantage statistics.
static int enqueue_prologue(aleppo_ctx *c, const UpdatePlan &p) {
  hipStream_t s = p.s;
  const Planes &pl = p.pl;
  if (p.val_transpose) // (ALEPPO_OPT_VALUE_CLIP on a rollout batch) values_tm [T][E] -> val_n [E][T]
    launch_transpose_tm_pitched(s, c->values_tm, (size_t)c->E * c->rsz, c->val_n, c->E, c->T, 1, (int)c->rsz);
  // Shuffled: the order of every epoch and the per-sample planes in that order ([epochs][N]); the minibatches then read
  // them like the contiguous planes, and find their observations through SampleMap::idx.  Mask counts per (epoch, minibatch).
  if (p.shuffle)
    launch_shuffle_gather(s, c->shuf_keys, p.shuf_h, p.N, p.epochs, c->A, c->order, c->act_n, c->oldlp_n, c->adv_n,
                          c->ret_n, p.vclip ? c->val_n : nullptr, c->mask_n, c->act_p, c->oldlp_p, c->adv_p, c->ret_p,
                          c->val_p, c->mask_p, c->rt16);
  launch_mask_count(s, pl.mask, pl.counts, p.B, pl.ncounts);
  if (p.dp) // N_m of the masked mean is the GLOBAL count
    NCCLCHK(c, ncclAllReduce(pl.counts, pl.counts, pl.ncounts, ncclFloat, ncclSum, p.comm, s));
  // ALEPPO_OPT_ADV_NORM_MINIBATCH: the statistics of the same (epoch, minibatch) sample sets as the counts - over the
  // global minibatch with data parallelism (double sums all-reduced, then finalised)
  if (p.advn) {
    launch_advn_stats(s, pl.adv, pl.mask, p.B, pl.ncounts, p.dp ? c->advn_part : nullptr, c->advn_stats, c->rt16);
    if (p.dp) {
      NCCLCHK(c, ncclAllReduce(c->advn_part, c->advn_part, (size_t)pl.ncounts * 4, ncclDouble, ncclSum, p.comm, s));
      launch_advn_finalise(s, c->advn_part, c->advn_stats, pl.ncounts);
    }
  }
  return ALEPPO_OK;
}

// The loss / head-backward kernel of minibatch (ep, mb), over the hparts slabs of h that net_forward left.
static void enqueue_head(aleppo_ctx *c, const UpdatePlan &p, int ep, int mb, int hparts) {
  prof_begin(c, ALEPPO_K_HEAD);
  const Planes &pl = p.pl;
  const int mi = ep * p.M + mb, A = c->A;
  const size_t p0 = pl.offset(ep, mb), fs = p.fs;
  float *const mps = p.metric_ps + (size_t)mi * p.B; // this minibatch's slice of every per-sample metric plane
  HeadTrainArgs ha{};
  ha.h = c->h;
  ha.Wh = Pf(c, P_WH);
  ha.bh = Pf(c, P_BH);
  ha.act = pl.act + p0;
  ha.oldlp = rp(c, pl.oldlp, p0 * A);
  ha.adv = rp(c, pl.adv, p0);
  ha.ret = rp(c, pl.ret, p0);
  ha.vold = pl.vold ? rp(c, pl.vold, p0) : nullptr;
  ha.mask = pl.mask + p0;
  ha.mask_count = pl.counts + pl.record(ep, mb);
  ha.dh = c->dh;
  ha.prec = c->prec;
  ha.ps_total = mps + 0 * fs, ha.ps_clipped = mps + 1 * fs, ha.ps_value = mps + 2 * fs, ha.ps_entropy = mps + 3 * fs;
  ha.ps_ratio = mps + 4 * fs, ha.ps_kl = mps + 5 * fs, ha.ps_cf = mps + 6 * fs;
  ha.slab_w = p.sWh;
  ha.slab_b = p.sBh;
  ha.nblk = p.nblk_head;
  ha.B = p.B;
  ha.H = c->H;
  ha.A = A;
  ha.hparts = hparts;
  ha.rt16 = c->rt16;
  ha.advs = p.advn ? p.advn_stats + pl.record(ep, mb) * 4 : nullptr;
  ha.klb = p.klpen ? p.kl_beta : nullptr;
  ha.ps_kle = p.klpen ? p.kl_ps + (size_t)mi * p.B : nullptr;
  launch_head_train(p.s, ha, p.hpd);
  prof_end(c, ALEPPO_K_HEAD);
}

// The slab groups of one minibatch that wait for their reduce into the gradient tensor
struct SegList {
  ReduceSeg seg[10];
  int n = 0;
  void add(const ReduceSeg &r) { seg[n++] = r; }
  void add(const SegList &o) {
    for (int i = 0; i < o.n; ++i)
      seg[n++] = o.seg[i];
  }
};
// With two streams the weight-gradient stream reduces every slab group that is complete while the main stream runs the
// last link of the dgrad chain; on one stream they stay listed for the reduce after it.
static void reduce_beside(aleppo_ctx *c, const UpdatePlan &p, SegList &segs, float *dst) {
  if (!p.two)
    return;
  prof_begin(c, ALEPPO_K_REDUCE, p.sw);
  launch_reduce_slabs(p.sw, segs.seg, segs.n, dst);
  prof_end(c, ALEPPO_K_REDUCE, p.sw);
  segs.n = 0;
}

// The two tails of the conv backward, after conv3's dgrad and wgrad (S3 slices).  late0: bucket 0's slab groups where
// they were not reduced early (empty with data parallelism).  Both leave in segs what is still to be reduced on the main
// stream and return conv1's slice count in *S1.  dst: the gradient vector the slab groups are reduced into.
static int enqueue_conv_bwd_fused(aleppo_ctx *c, const UpdatePlan &p, const SampleMap &map, int S3,
                                  const SegList &late0, SegList &segs, int *S1, float *dst) {
  const ParamLayout &L = c->L;
  // conv2 dgrad + conv2 wgrad + conv1 wgrad in ONE launch on the main stream (conv_bwd_fused.hpp: dz1 never leaves the
  // CU).  Meanwhile the weight-gradient stream reduces the slab groups that are complete (conv3, heads + fc).
  segs.add(ReduceSeg{p.sW3, S3, 64 * 576, (long)L.off[P_W3]});
  segs.add(ReduceSeg{p.sB3, S3, 64, (long)L.off[P_B3]});
  segs.add(late0);
  reduce_beside(c, p, segs, dst);
  prof_begin(c, ALEPPO_K_CONV_BWD);
  const int S2 = *S1 = patch_conv_bwd_fused(p.s, c->dz2, c->a1, c->obs, map, c->W2d, p.sW2, p.sB2, p.sW1, p.sB1, p.B);
  prof_end(c, ALEPPO_K_CONV_BWD);
  segs.add(ReduceSeg{p.sW2, S2, 64 * 512, (long)L.off[P_W2]});
  segs.add(ReduceSeg{p.sB2, S2, 64, (long)L.off[P_B2]});
  return ALEPPO_OK;
}
static int enqueue_conv_bwd_split(aleppo_ctx *c, const UpdatePlan &p, const SampleMap &map, int S3,
                                  const SegList &late0, SegList &segs, int *S1, float *dst) {
  const ParamLayout &L = c->L;
  const int prec = c->prec;
  HIPCHK(c, fork_wgrad_stream(p, c->ev_dz2)); // dz2 is ready
  prof_begin(c, ALEPPO_K_CONV2_DGRAD);
  conv2_dgrad(p.s, prec, c->dz2, c->W2d, c->a1, c->dz1, p.B);
  prof_end(c, ALEPPO_K_CONV2_DGRAD);
  prof_begin(c, ALEPPO_K_CONV2_WGRAD, p.sw);
  const int S2 = conv2_wgrad(p.sw, prec, c->dz2, c->a1, p.sW2, p.sB2, p.B);
  prof_end(c, ALEPPO_K_CONV2_WGRAD, p.sw);
  // conv1 wgrad is the last link of the dgrad chain and runs alone on s: meanwhile the wgrad stream reduces every
  // slab group that is already complete (reducing them AFTER conv1 wgrad on the main stream instead measured slower:
  // 7.89-7.96 vs 7.77 ms per update) (conv3, conv2 and - on one GPU - heads + fc); only conv1's slabs are left
  // for the reduce after the join.
  segs.add(ReduceSeg{p.sW3, S3, 64 * 576, (long)L.off[P_W3]});
  segs.add(ReduceSeg{p.sB3, S3, 64, (long)L.off[P_B3]});
  segs.add(ReduceSeg{p.sW2, S2, 64 * 512, (long)L.off[P_W2]});
  segs.add(ReduceSeg{p.sB2, S2, 64, (long)L.off[P_B2]});
  segs.add(late0);
  reduce_beside(c, p, segs, dst);
  prof_begin(c, ALEPPO_K_CONV1_WGRAD);
  *S1 = conv1_wgrad(p.s, prec, c->dz1, c->obs, map, p.sW1, p.sB1, p.B);
  prof_end(c, ALEPPO_K_CONV1_WGRAD);
  return ALEPPO_OK;
}

// The gradient half of one optimizer step: forward, head, fork, fc dgrad || fc wgrad, bucket 0, conv3, the conv backward's
// tail, join, tail reduce.  dst: the gradient vector (internal layout) it lands in - c->G for aleppo_train, a gradient slot
// for aleppo_grad_probe.  tail: conv1's two slab groups, which are NOT reduced yet unless their slab comes back nullptr
// (data parallelism: the all-reduce needs the whole gradient) - the norm pass, or the probe's own reduce, sums them.
static int enqueue_gradient(aleppo_ctx *c, const UpdatePlan &p, int ep, int mb, float *dst, ReduceSeg tail[2]) {
  const int H = c->H, A = c->A, prec = c->prec;
  const ParamLayout &L = c->L;
  const long B = p.B;
  hipStream_t s = p.s, sw = p.sw;
  // contiguous env-major slices unless shuffling (the reference's randperm is unused, Q1)
  SampleMap map = train_map(c, p.n0 + (long)mb * B);
  map.idx = p.pl.idx(ep);
  const int hparts = net_forward(c, c->obs, map, B, FC_FWD_MAX_PARTS);
  c->bwd_enq = Ctx::BwdMark{B, hparts, !p.bwd_fused}; // (aleppo_export_backward: what this minibatch leaves; host only)
  enqueue_head(c, p, ep, mb, hparts);
  HIPCHK(c, fork_wgrad_stream(p, c->ev_head)); // dh is ready
  prof_begin(c, ALEPPO_K_FC_DGRAD);
  fc_dgrad(s, prec, c->dh, c->WfcT, c->a3, c->dz3, B, H);
  prof_end(c, ALEPPO_K_FC_DGRAD);
  prof_begin(c, ALEPPO_K_FC_WGRAD, sw);
  // split-K slabs (or, with one slice, straight into the gradient tensor)
  const bool fc_direct = fc_wgrad_slices(prec, B) == 1;
  const int Sfc = fc_wgrad(sw, prec, c->dh, c->a3, fc_direct ? dst + L.off[P_WFC] : p.sWfc,
                           fc_direct ? dst + L.off[P_BFC] : p.sBfc, B, H);
  prof_end(c, ALEPPO_K_FC_WGRAD, sw);
  // bucket 0 = heads + fc.  With data parallelism it is reduced now so that its all-reduce overlaps the conv
  // backward; on one GPU all ten slab groups are reduced by ONE launch after the conv wgrads.
  SegList segs0;
  segs0.add(ReduceSeg{p.sWh, p.nblk_head, (long)(A + 1) * H, (long)L.off[P_WH]});
  segs0.add(ReduceSeg{p.sBh, p.nblk_head, (long)A + 1, (long)L.off[P_BH]});
  if (!fc_direct) {
    segs0.add(ReduceSeg{p.sWfc, Sfc, (long)H * FC_IN, (long)L.off[P_WFC]});
    segs0.add(ReduceSeg{p.sBfc, Sfc, (long)H, (long)L.off[P_BFC]});
  }
  // bucket 0 is reduced early only for the all-reduce overlap: on one GPU an early reduce next to the conv dgrads
  // measured slower (8.60 vs 8.38 ms per update) than one reduce of all ten slab groups at the end
  if (p.dp) { // bucket 0 (heads + fc = 95% of the bytes) travels while the conv backward runs.  Its slab reduce runs on
              // the communication stream too, in front of the all-reduce: on the weight-gradient stream it sat between
              // the fc and the conv weight gradients and that stream, not the dgrad chain, ended the minibatch (trace
              // with a 1-rank communicator: conv1 wgrad done at 419 us, conv2 wgrad at 453 us).
    HIPCHK(c, hipEventRecord(c->ev_bucket0, sw));
    HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->ev_bucket0, 0));
    prof_begin(c, ALEPPO_K_REDUCE, c->comm_stream);
    launch_reduce_slabs(c->comm_stream, segs0.seg, segs0.n, dst);
    prof_end(c, ALEPPO_K_REDUCE, c->comm_stream);
    NCCLCHK(c, ncclAllReduce(dst, dst, L.bucket0_end, ncclFloat, ncclSum, p.comm, c->comm_stream));
    HIPCHK(c, hipEventRecord(c->ev_comm0, c->comm_stream));
    segs0.n = 0; // (reduced: nothing of bucket 0 is left for the late reduce)
  }
  HIPCHK(c, fork_wgrad_stream(p, c->ev_dz3)); // dz3 is ready
  prof_begin(c, ALEPPO_K_CONV3_DGRAD);
  conv3_dgrad(s, prec, c->dz3, c->W3d, c->a2, c->dz2, B);
  prof_end(c, ALEPPO_K_CONV3_DGRAD);
  prof_begin(c, ALEPPO_K_CONV3_WGRAD, sw);
  const int S3 = conv3_wgrad(sw, prec, c->dz3, c->a2, p.sW3, p.sB3, B);
  prof_end(c, ALEPPO_K_CONV3_WGRAD, sw);
  int S1 = 0;
  SegList segs;
  if (int rc = p.bwd_fused ? enqueue_conv_bwd_fused(c, p, map, S3, segs0, segs, &S1, dst)
                           : enqueue_conv_bwd_split(c, p, map, S3, segs0, segs, &S1, dst))
    return rc;
  if (p.two) { // join: sumsq / Adam read the whole gradient
    HIPCHK(c, hipEventRecord(c->ev_wg, sw));
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_wg, 0));
  }
  // conv1's slabs: with data parallelism they are reduced now (the all-reduce needs the whole gradient); on one GPU
  // the sum-of-squares pass below sums them on the fly - one launch less on the serial tail of the minibatch.
  tail[0] = ReduceSeg{p.sW1, S1, 32 * 256, (long)L.off[P_W1]};
  tail[1] = ReduceSeg{p.sB1, S1, 32, (long)L.off[P_B1]};
  if (p.dp) {
    segs.add(tail[0]);
    segs.add(tail[1]);
    tail[0].slab = tail[1].slab = nullptr;
  }
  if (segs.n) {
    prof_begin(c, ALEPPO_K_REDUCE);
    launch_reduce_slabs(s, segs.seg, segs.n, dst);
    prof_end(c, ALEPPO_K_REDUCE);
  }
  return ALEPPO_OK;
}

// One optimizer step: the gradient into c->G, bucket 1, sum of squares and Adam.
static int enqueue_minibatch(aleppo_ctx *c, const UpdatePlan &p, int ep, int mb) {
  const int prec = c->prec, mi = ep * p.M + mb;
  const ParamLayout &L = c->L;
  hipStream_t s = p.s;
  ReduceSeg tail[2];
  if (int rc = enqueue_gradient(c, p, ep, mb, c->G, tail))
    return rc;
  if (p.dp) {
    // Bucket 1 (the conv tensors, 0.35 MB) is on the critical path whatever stream carries it - nothing is left to
    // overlap it with - so it runs on the MAIN stream: a round trip through the communication stream cost two more
    // cross-stream dependencies (~12 us each, forkbench) in the serial tail of every minibatch (update with a 1-rank
    // communicator: +31 -> +16 us per minibatch over the single-GPU schedule).  The wait for bucket 0's event comes
    // first: two collectives of one communicator must never be in flight together.
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_comm0, 0));
    NCCLCHK(c, ncclAllReduce(c->G + L.bucket0_end, c->G + L.bucket0_end, L.total() - L.bucket0_end, ncclFloat, ncclSum,
                             p.comm, s));
  }
  prof_begin(c, ALEPPO_K_ADAM);
  // (pads between tensors are zero: only [0, off[P_W1]) and the two conv1 tensors contribute)
  const int nblk_norm = launch_sumsq(s, c->G, (long)L.off[P_W1], c->sumsq_part, p.nblk_sq, tail);
  // (the Adam kernel also writes the bf16 compute copy and the dgrad-side transposed layouts W2d / W3d / WfcT)
  launch_adam(s, c->P, c->G, c->M1, c->M2, c->prec == ALEPPO_BF16 ? c->Pc : nullptr, c->WfcT, c->W3d, c->W2d, L,
              prec, c->sumsq_part, nblk_norm, p.hpd, c->adam_sched + 2 * mi, c->cfg.adam_beta1, c->cfg.adam_beta2,
              c->cfg.adam_eps, c->grad_norms + mi, p.reg, p.anchor);
  prof_end(c, ALEPPO_K_ADAM);
  return ALEPPO_OK;
}

// aleppo_grad_probe's front (api_internal.hpp): a plan of one epoch and one minibatch whose planes start at sample `first`
// and whose head reads and writes the probe's private storage, the prologue's launches for that slice, enqueue_gradient
// into dst, and conv1's slabs by the narrow path of the slab reduce - slab_column_sum, the norm pass's own sum.
int aleppo::grad_probe_enqueue(aleppo_ctx *c, long first, long n, bool policy, float *blk, float *ps, float *dst) {
  UpdatePlan p{};
  p.epochs = p.M = p.nm = 1;
  p.N = c->batch_n;
  p.B = n;
  p.vclip = c->value_clip;
  if (p.vclip)
    if (int rc = ensure_val_storage(c))
      return rc;
  p.val_transpose = p.vclip && c->val_src == Ctx::VAL_ROLLOUT;
  p.advn = !policy || c->adv_norm_mb; // (!policy: the record is (0, 0) and every advantage becomes a * 0)
  p.klpen = c->kl_pen;
  if (!c->wg_stream)
    HIPCHK(c, hipStreamCreateWithFlags(&c->wg_stream, hipStreamNonBlocking));
  p.s = c->stream;
  p.hp = c->hyper;
  p.hpd = blk + GP_HYPER;
  p.fs = (size_t)c->maxB;
  p.metric_ps = ps, p.kl_ps = ps + 7 * p.fs, p.advn_stats = blk + GP_ADVS, p.kl_beta = blk + GP_BETA;
  p.n0 = first;
  // (the routes of the context's own minibatches: under data parallelism aleppo_train keeps the split tail)
  plan_routes(c, p, !(c->world > 1 || (c->nccl_comm && c->force_comm)));
  Planes &pl = p.pl;
  pl.B = n;
  pl.M = 1;
  pl.act = c->act_n + first, pl.oldlp = rp(c, c->oldlp_n, (size_t)first * c->A), pl.adv = rp(c, c->adv_n, first);
  pl.ret = rp(c, c->ret_n, first), pl.vold = p.vclip ? rp(c, c->val_n, first) : nullptr;
  pl.mask = c->mask_n + first, pl.order = nullptr, pl.counts = blk + GP_COUNT;
  pl.ncounts = 1;
  pl.epoch_stride = 0;
  hipStream_t s = p.s;
  if (p.val_transpose)
    launch_transpose_tm_pitched(s, c->values_tm, (size_t)c->E * c->rsz, c->val_n, c->E, c->T, 1, (int)c->rsz);
  launch_mask_count(s, pl.mask, pl.counts, n, 1);
  if (policy && c->adv_norm_mb)
    launch_advn_stats(s, pl.adv, pl.mask, n, 1, nullptr, blk + GP_ADVS, c->rt16);
  ReduceSeg tail[2];
  if (int rc = enqueue_gradient(c, p, 0, 0, dst, tail))
    return rc;
  prof_begin(c, ALEPPO_K_REDUCE);
  launch_reduce_slabs(s, tail, 2, dst);
  prof_end(c, ALEPPO_K_REDUCE);
  return ALEPPO_OK;
}

// What comes after the minibatches: the per-minibatch metric records and their all-reduce.
static int enqueue_epilogue(aleppo_ctx *c, const UpdatePlan &p) {
  const Planes &pl = p.pl;
  // (gathered planes: epoch ep's masks in its order, minibatch mi's are the mi-th B of the plane - nm slices, one "epoch";
  // contiguous: the same M slices every epoch)
  launch_metrics_reduce(p.s, c->metric_ps, p.fs, pl.mask, p.B, pl.ncounts, p.nm / pl.ncounts, c->metric_red,
                        p.klpen ? c->kl_ps : nullptr);
  if (p.dp)
    NCCLCHK(c, ncclAllReduce(c->metric_red, c->metric_red, (size_t)p.nm * METRIC_REC, ncclFloat, ncclSum, p.comm, p.s));
  return ALEPPO_OK;
}

// Everything the update enqueues - mask counts, epochs x minibatches of forward / loss / backward / [all-reduce] /
// clip / Adam, the metric reduction - as one function: run eagerly, or recorded once into a hipGraph and replayed.
static int enqueue_update(aleppo_ctx *c, const UpdatePlan &p) {
  if (int rc = enqueue_prologue(c, p))
    return rc;
  for (int ep = 0; ep < p.epochs; ++ep)
    for (int mb = 0; mb < p.M; ++mb)
      if (int rc = enqueue_minibatch(c, p, ep, mb))
        return rc;
  return enqueue_epilogue(c, p);
}

// The ONLY place a GraphKey is made.  The rule: every pointer or flag that the enqueue_* functions read and that can
// differ between two aleppo_train calls of one context belongs here - a captured graph bakes all of them in, and a
// replay under a key that misses one computes on stale addresses or the wrong kernels without any error.  (Device
// VALUES the kernels read - the Adam schedule, the hyper block, beta, the round keys - are uploaded per call and are
// not part of it; storage that is allocated once and never moves is not either.)
static Ctx::GraphKey graph_key(const UpdatePlan &p, const aleppo_ctx *c) {
  Ctx::GraphKey key;
  key.epochs = p.epochs;
  key.M = p.M;
  key.two = p.two ? 1 : 0;
  key.N = p.N;
  key.metric_ps = c->metric_ps;
  key.metric_red = c->metric_red;
  key.order = p.pl.order;
  key.vclip = p.vclip ? 1 + c->val_src : 0;
  key.advn = p.advn ? c->advn_stats : nullptr;
  key.klpen = p.klpen ? 1 : 0;
  key.kl_ps = p.klpen ? c->kl_ps : nullptr;
  key.reg = p.reg ? 1 : 0;
  key.anchor = p.anchor;
  return key;
}

// ALEPPO_OPT_UPDATE_GRAPH (capture_train_cuda_graph, train.h:163-195): the first call of a shape runs eagerly (it also
// performs the kernels' one-time attribute set-up), the second records the same enqueue into a graph, later calls
// replay it.  Not with data parallelism (the collectives stay eager) and not while per-kernel profiling brackets launches.
static int run_update(aleppo_ctx *c, const UpdatePlan &p) {
  hipStream_t s = p.s;
  const Ctx::GraphKey key = graph_key(p, c);
  const bool want_graph = c->update_graph && !p.dp && !c->prof_on;
  if (want_graph && c->graph_exec && c->graph_key == key) {
    HIPCHK(c, hipGraphLaunch(c->graph_exec, s));
    c->graph_replays++;
    c->bwd_enq = c->bwd_graph;
  } else if (want_graph && c->warm_key == key) {
    if (c->graph_exec)
      HIPCHK(c, hipGraphExecDestroy(c->graph_exec));
    if (c->graph)
      HIPCHK(c, hipGraphDestroy(c->graph));
    c->graph_exec = nullptr;
    c->graph = nullptr;
    HIPCHK(c, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_update(c, p);
    hipGraph_t g = nullptr;
    hipError_t ee = hipStreamEndCapture(s, &g); // (also ends a capture that failed half way)
    if (rc == ALEPPO_OK && ee == hipSuccess)
      ee = hipGraphInstantiate(&c->graph_exec, g, nullptr, nullptr, 0);
    if (rc || ee != hipSuccess) {
      // Nothing has run yet (a capture only records).  Drop the half-built graph and its keys so that the next call
      // starts from the eager path again instead of re-capturing for ever, and report.
      if (g)
        hipGraphDestroy(g);
      c->graph_exec = nullptr;
      c->graph_key = Ctx::GraphKey();
      c->warm_key = Ctx::GraphKey();
      if (rc)
        return rc;
      HIPCHK(c, ee);
    }
    c->graph = g;
    c->graph_key = key;
    c->bwd_graph = c->bwd_enq;
    HIPCHK(c, hipGraphLaunch(c->graph_exec, s));
    c->graph_replays++;
  } else {
    const int rc = enqueue_update(c, p);
    if (rc) // some optimizer steps may already be on the stream: parameters / Adam state are no longer what the caller
            // thinks they are, and adam_step cannot say how far the device got
      return fail_ctx(c, rc, "aleppo_train failed while enqueuing the update (" + c->err + ")");
    c->warm_key = key;
  }
  return ALEPPO_OK;
}

// Wait for the update, bring back what the read-backs serve from host memory, remember the call's shape, fill out.
static int read_back_metrics(aleppo_ctx *c, const UpdatePlan &p, aleppo_minibatch_metrics *out) {
  hipStream_t s = p.s;
  const int nm = p.nm;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_metric_red, c->metric_red, (size_t)nm * METRIC_REC * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(c->h_metric_red + (size_t)nm * METRIC_REC, c->grad_norms, (size_t)nm * 4,
                           hipMemcpyDeviceToHost, s));
  if (p.advn) // (contiguous: M records, the same slices every epoch)
    HIPCHK(c, hipMemcpyAsync(c->h_advn_stats, c->advn_stats, (size_t)p.pl.ncounts * 16, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  CHECK_ASYNC(c);
  c->last_epochs = p.epochs;
  c->last_M = p.M;
  c->last_B = p.B;
  c->last_shuffled = p.shuffle;
  c->last_advn = p.advn;
  c->last_kl = p.klpen;
  c->last_max_norm = p.hp.max_norm;
  c->ts_sched[0] = c->h_adam_sched[2 * (nm - 1)]; // (aleppo_tensor_stats recomputes the last step from these)
  c->ts_sched[1] = c->h_adam_sched[2 * (nm - 1) + 1];
  c->ts_step_valid = true;
  c->bwd = c->bwd_enq; // the last minibatch's stored tensors are there to be read until something else runs the network
  if (out)
    for (int i = 0; i < nm; ++i) {
      const float *r = c->h_metric_red + (size_t)i * METRIC_REC;
      const float cnt = r[5];
      out[i].loss = r[0] / cnt;
      out[i].clipped_loss = r[1] / cnt;
      out[i].value_loss = r[2] / cnt;
      out[i].entropy = r[3] / cnt;
      out[i].ratio = r[4] / cnt;
      out[i].mask_count = cnt;
      out[i].grad_norm = c->h_metric_red[(size_t)nm * METRIC_REC + i];
    }
  return ALEPPO_OK;
}

extern "C" int aleppo_train(aleppo_ctx *c, double lr, int epochs, int M, aleppo_minibatch_metrics *out) {
  CHECK_CTX(c);
  UpdatePlan plan{};
  int rc = plan_update(c, epochs, M, &plan);
  if (rc == ALEPPO_OK)
    rc = upload_call_scalars(c, plan, lr);
  if (rc == ALEPPO_OK) {
    c->ts_step_valid = false; // (until this update's last step is known to have run: read_back_metrics)
    rc = run_update(c, plan);
  }
  if (rc)
    return rc;
  c->adam_step += plan.nm;
  return read_back_metrics(c, plan, out);
}

extern "C" int aleppo_read_train_metric(aleppo_ctx *c, int field, float *dst, size_t count) {
  CHECK_CTX(c);
  if (field == ALEPPO_M_MEAN_APPROX_KL || field == ALEPPO_M_MEAN_CLIP_FRACTION) {
    // masked means [epochs, M] from the reduced records aleppo_train brought back (slots 6 / 7 over the count, slot 5)
    const size_t nm = (size_t)c->last_epochs * c->last_M;
    if (!dst || count != nm || nm == 0)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_train_metric: count must be epochs * M of the last aleppo_train");
    const int slot = field == ALEPPO_M_MEAN_APPROX_KL ? 6 : 7;
    for (size_t i = 0; i < nm; ++i) {
      const float *r = c->h_metric_red + i * METRIC_REC;
      dst[i] = r[slot] / r[5];
    }
    return ALEPPO_OK;
  }
  if (field == ALEPPO_M_KL || field == ALEPPO_M_MEAN_KL) {
    // ALEPPO_OPT_KL_PENALTY's exact KL: the per-sample plane, or the masked means (slot 8 over the count, slot 5)
    const size_t nm = (size_t)c->last_epochs * c->last_M, n = nm * c->last_B;
    if (!c->last_kl || nm == 0)
      return set_err(c, ALEPPO_ERR_RUNTIME, "read_train_metric: the last aleppo_train ran without ALEPPO_OPT_KL_PENALTY");
    if (field == ALEPPO_M_MEAN_KL) {
      if (!dst || count != nm)
        return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                       "read_train_metric: count must be epochs * M of the last aleppo_train");
      for (size_t i = 0; i < nm; ++i) {
        const float *r = c->h_metric_red + i * METRIC_REC;
        dst[i] = r[8] / r[5];
      }
      return ALEPPO_OK;
    }
    if (!dst || count != n)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_train_metric: bad field or count");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, copy_sync(c, dst, c->kl_ps, n * 4, hipMemcpyDeviceToHost));
    return ALEPPO_OK;
  }
  if (field == ALEPPO_M_ADV_MEAN || field == ALEPPO_M_ADV_STD) {
    // the ALEPPO_OPT_ADV_NORM_MINIBATCH statistics [epochs, M] of the last aleppo_train (brought back by it)
    const size_t nm = (size_t)c->last_epochs * c->last_M;
    if (!c->last_advn || nm == 0)
      return set_err(c, ALEPPO_ERR_RUNTIME,
                     "read_train_metric: the last aleppo_train ran without ALEPPO_OPT_ADV_NORM_MINIBATCH");
    if (!dst || count != nm)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_train_metric: count must be epochs * M of the last aleppo_train");
    const int slot = field == ALEPPO_M_ADV_MEAN ? 0 : 2;
    for (size_t i = 0; i < nm; ++i)
      dst[i] = c->h_advn_stats[record_index(c->last_shuffled, (size_t)c->last_M, i) * 4 + slot];
    return ALEPPO_OK;
  }
  const size_t n = (size_t)c->last_epochs * c->last_M * c->last_B;
  if (!dst || field < 0 || field > ALEPPO_M_CLIP_FRACTION || count != n || n == 0)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_train_metric: bad field or count");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, copy_sync(c, dst, c->metric_ps + (size_t)field * c->metric_cap, n * 4, hipMemcpyDeviceToHost));
  return ALEPPO_OK;
}

extern "C" int aleppo_read_sample_order(aleppo_ctx *c, int32_t *dst, size_t count) {
  CHECK_CTX(c);
  const size_t N = (size_t)c->last_M * c->last_B, n = (size_t)c->last_epochs * N;
  if (n == 0)
    return set_err(c, ALEPPO_ERR_RUNTIME, "read_sample_order: no update has run yet");
  if (!dst || count != n)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "read_sample_order: count must be epochs * N of the last aleppo_train");
  if (!c->last_shuffled) { // (contiguous: every epoch reads the batch in its stored order)
    for (size_t i = 0; i < n; ++i)
      dst[i] = (int32_t)record_index(false, N, i);
    return ALEPPO_OK;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, copy_sync(c, dst, c->order, n * 4, hipMemcpyDeviceToHost));
  return ALEPPO_OK;
}
