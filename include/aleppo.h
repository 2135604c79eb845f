/* aleppo.h - C ABI of the MI355X-native PPO-over-ALE hot path (libaleppo.so).
 *
 * Drop-in boundary for the ONE data-parallel path of cemlyn007/ale-libtorch-ppo: vectorised
 * rollout pipeline (preprocess, 4-frame stack, rollout buffer, reward clamp + GAE + returns) and
 * the Nature-CNN actor-critic forward / backward with the PPO loss, global-norm clip and Adam.
 * The reference has no FFI; it reaches this path through ordinary C++ calls from main()
 * (src/bin/train.cc:320-465).  Each entry point below names the reference interface it replaces.
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions: C linkage, opaque context, plain pointers and sizes, no C++ / torch types.
 * Every call returns ALEPPO_OK (0) or a negative aleppo_status; aleppo_last_error() gives the
 * message (the reference throws std::invalid_argument / std::runtime_error at the same places).
 * One owner thread per context; several contexts of one process may be driven from different threads at the same time.
 * After aleppo_create a context only ever touches its own HIP streams: no entry point but aleppo_destroy (and
 * aleppo_host_free) calls hipFree / hipHostFree / hipDeviceSynchronize or uses the null stream - those wait for every
 * stream of the device, another context's stream parked behind its release word included (aleppo_arm_step).  The same
 * rule binds the caller: while a step is armed, its owner thread must be the one that releases it, and no OTHER call of
 * that thread may wait for the device.  Host pointers are caller-owned and may be reused as soon as the
 * call returns, unless stated.  Tensors crossing the boundary use the REFERENCE's layouts
 * (env-major [E,T,...], NCHW uint8 observations, libtorch parameters() order); internal HBM
 * layouts are private.
 */
#ifndef ALEPPO_H
#define ALEPPO_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ALEPPO_ABI_VERSION 2

typedef enum {
  ALEPPO_OK = 0,
  ALEPPO_ERR_INVALID_ARGUMENT = -1, /* std::invalid_argument in the reference */
  ALEPPO_ERR_RUNTIME = -2,          /* std::runtime_error in the reference */
  ALEPPO_ERR_HIP = -3,              /* a HIP / RCCL runtime call failed */
  ALEPPO_ERR_NO_DEVICE = -4         /* no usable gfx950 device: there is NO CPU fallback */
} aleppo_status;

typedef enum { ALEPPO_FP32 = 0, ALEPPO_BF16 = 1 } aleppo_precision;
/* Storage type of the rollout buffer's float planes (values, logits, advantages, returns, old log-probs:
 * Buffer's f32 tensors, src/ai/buffer.cc:12-38).  FP16 = BASELINE configs[4] "fp16 rollout buffer": the planes are
 * rounded to IEEE half when stored; reward clamp / GAE / returns / log-softmax arithmetic stays fp32 on the rounded
 * inputs; aleppo_read_batch still returns float.  The reference has only FP32. */
typedef enum { ALEPPO_ROLLOUT_FP32 = 0, ALEPPO_ROLLOUT_FP16 = 1 } aleppo_rollout_precision;
/* ALEPPO_HOST: ordinary or page-locked host memory, staged and copied by the call.  ALEPPO_DEVICE: device memory.
 * ALEPPO_HOST_MAPPED: page-locked host memory the GPU can address (hipHostMalloc / hipHostRegister'ed, e.g. the ring
 * the emulator threads write their frames into, src/ai/rollout.cc:325-326): the ingest kernel reads it in place over
 * the bus - no staging copy, no separate copy command on the slot's critical path. */
typedef enum { ALEPPO_HOST = 0, ALEPPO_DEVICE = 1, ALEPPO_HOST_MAPPED = 2 } aleppo_location;

/* What aleppo_push_frames receives per environment step. */
typedef enum {
  ALEPPO_FRAMES_84 = 0,      /* uint8 [E,84,84]: already gray + resized + max-pooled on the env threads
                                (what Rollout::step memcpy's into screen_buffers_, src/ai/rollout.cc:325-326) */
  ALEPPO_FRAMES_RAW_PAIR = 1 /* uint8 [E,2,210,160]: the last two emulator frames of the skip window as ALE
                                palette / gray bytes; the device applies the 256-entry LUT, the 84x84 area
                                resize and the 2-frame max (environment.cc:48-55, vision.cc:8-32,
                                max_and_skip.cc:33-42) */
} aleppo_frame_kind;

typedef struct aleppo_ctx aleppo_ctx;

/* Mirrors the hot-path part of Config (src/bin/train.cc:33-63) + Rollout ctor arguments
 * (src/ai/rollout.h:39-49).  New fields default (0) to reference behaviour. */
typedef struct {
  int32_t abi_version;    /* ALEPPO_ABI_VERSION */
  int32_t device_ordinal; /* HIP device; one process per GPU */
  int32_t world_size;     /* data-parallel ranks (1 = reference behaviour) */
  int32_t rank;
  int32_t num_envs;       /* E_local: environments owned by THIS rank (total_environments / world_size) */
  int32_t horizon;        /* T */
  int32_t num_actions;    /* A (the reference hard-codes 4, train.cc:36) */
  int32_t hidden_size;    /* H */
  int32_t frame_stack;    /* must be 4 (conv1 in-channels are hard-coded, train.cc:233) */
  int32_t precision;      /* aleppo_precision of the conv/linear stack */
  int32_t advantage_norm; /* 0 = none (the reference has none); 1 = normalise over masked samples */
  int32_t max_minibatch;  /* largest minibatch (samples per rank) aleppo_train will be asked for; 0 = E*T */
  int32_t rollout_precision; /* aleppo_rollout_precision; 0 = float planes like the reference */
  float gamma, lambda;    /* gae_discount, gae_lambda */
  float clip_param, value_loss_coef, entropy_coef, max_gradient_norm;
  float adam_beta1, adam_beta2, adam_eps; /* 0 -> 0.9 / 0.999 / 1e-5 (train.cc:360-362) */
  uint64_t seed;          /* counter-based sampling RNG when no external noise is supplied */
} aleppo_config;

/* Per-minibatch scalars = ai::ppo::train::Metrics reduced the way log_data() reduces them
 * (src/bin/train.cc:163-210): loss is the masked-mean loss tensor, the others masked means. */
typedef struct {
  float loss;          /* Metrics.loss[e][m] */
  float grad_norm;     /* Metrics.clipped_gradients[e][m] = PRE-clip total norm (train.cc:32-45) */
  float clipped_loss;  /* masked mean of clipped surrogate objective */
  float value_loss;    /* masked mean of 0.5 (v-R)^2 */
  float entropy;       /* masked mean entropy */
  float ratio;         /* masked mean probability ratio */
  float mask_count;    /* number of unmasked samples (global over ranks) */
} aleppo_minibatch_metrics;

/* Fields of the rollout batch (ai::buffer::Batch, src/ai/buffer.h:5-25, after prepare_batch,
 * src/bin/train.cc:272-283) readable with aleppo_read_batch, all in reference layout. */
typedef enum {
  ALEPPO_F_OBSERVATIONS = 0, /* uint8  [E,T,4,84,84] */
  ALEPPO_F_ACTIONS = 1,      /* int64  [E,T] */
  ALEPPO_F_REWARDS = 2,      /* float  [E,T] (clamped after finish_rollout; scaled and clipped with ALEPPO_OPT_REWARD_SCALE) */
  ALEPPO_F_MASKS = 3,        /* uint8  [E,T] = !episode_starts */
  ALEPPO_F_LOGITS = 4,       /* float  [E,T,A] */
  ALEPPO_F_VALUES = 5,       /* float  [E,T] */
  ALEPPO_F_ADVANTAGES = 6,   /* float  [E,T] */
  ALEPPO_F_RETURNS = 7,      /* float  [E,T] */
  ALEPPO_F_LOG_PROBS = 8,    /* float  [E,T,A] = normalize_logits(logits) */
  ALEPPO_F_TERMINALS = 9,    /* uint8  [E,T] */
  ALEPPO_F_TRUNCATIONS = 10, /* uint8  [E,T] */
  ALEPPO_F_CURRENT_OBS = 11, /* uint8  [E,4,84,84]: Rollout::observations_ right now */
  ALEPPO_F_NEXT_VALUES = 12, /* float  [E]: bootstrap values of the last finish_rollout */
  ALEPPO_F_BATCH_STATS = 13, /* double [ALEPPO_BATCH_STATS_COUNT]: explained variance and batch statistics, see below */
  ALEPPO_F_REWARD_SCALE = 14 /* double [ALEPPO_REWARD_SCALE_COUNT]: the state of ALEPPO_OPT_REWARD_SCALE, see below */
} aleppo_field;

/* ALEPPO_F_REWARD_SCALE: the running statistics of ALEPPO_OPT_REWARD_SCALE and what the last scaled rollout did, six
 * doubles indexed by aleppo_reward_scale_stat.  Readable at any time after aleppo_create (whether the option is on or
 * not, with or without a batch): before any scaled rollout it is the initial state (1e-4, 0, 1, 1, 0, 0).  Errors as for
 * the other fields: a wrong byte count is ALEPPO_ERR_INVALID_ARGUMENT, a read while a step is armed ALEPPO_ERR_RUNTIME.
 * Never a collective: the all-reduce happens inside aleppo_finish_rollout. */
#define ALEPPO_REWARD_SCALE_COUNT 6
typedef enum {
  ALEPPO_RS_COUNT = 0,       /* count of the running statistics (1e-4 + every sample merged so far) */
  ALEPPO_RS_MEAN = 1,        /* running mean of the discounted return */
  ALEPPO_RS_VAR = 2,         /* running (population) variance of the discounted return */
  ALEPPO_RS_SCALE = 3,       /* the float s the last scaled rollout's rewards were multiplied with, widened; 1 before any */
  ALEPPO_RS_BATCH_COUNT = 4, /* n of the last scaled rollout (global under data parallelism) */
  ALEPPO_RS_CLIPPED = 5      /* how many of THIS RANK's E*T rewards the clip changed (|r * s| > c) in that rollout */
} aleppo_reward_scale_stat;

/* ALEPPO_F_BATCH_STATS: the critic diagnostics CleanRL / Stable-Baselines3 log on every update (the reference has none),
 * reduced on the device where the planes are.  aleppo_read_batch(ctx, ALEPPO_F_BATCH_STATS, dst, ALEPPO_BATCH_STATS_COUNT
 * * sizeof(double)) writes the ten doubles indexed by aleppo_batch_stat.
 * Sample set: the unmasked samples (mask = !episode_start, the loss's mask) of the batch the context holds: the rollout
 *   batch after aleppo_finish_rollout (E*T samples), or the caller batch of aleppo_set_batch (its n samples: this field
 *   uses the batch's own sample count, what aleppo_train uses, while the other fields read E*T elements whatever the
 *   batch).  With a communicator (world_size > 1, or ALEPPO_OPT_FORCE_COMM) it is the union over the ranks, and the call
 *   is then a COLLECTIVE like aleppo_train: every rank makes it at the same point.
 * Planes: v, R, a are the values, returns and advantages AS STORED, widened to float and then to double: with
 *   ALEPPO_ROLLOUT_FP16 the rounded values aleppo_read_batch returns.  v is what ALEPPO_OPT_VALUE_CLIP calls v_old: the
 *   values plane of a rollout batch, or what aleppo_set_batch_values stored for a caller batch (a caller batch without
 *   them: ALEPPO_ERR_RUNTIME, as for value clipping).  a is the advantage plane as it stands: with config.advantage_norm
 *   = 1 the normalised one.  d = (double)R - (double)v.
 * Arithmetic: n and the sum S and sum of squares Q of v, R, a and d, in double (nine numbers per rank; under data
 *   parallelism all-reduced as ncclDouble / ncclSum).  Then on the device, in double: mean = S / n, var = max(0, Q / n -
 *   mean^2), std = sqrt(var), explained_variance = 1 - var(d) / var(R).  This is the POPULATION variance (numpy.var's
 *   default, what CleanRL's and SB3's explained_variance use), not the unbiased one of ALEPPO_OPT_ADV_NORM_MINIBATCH.
 *   explained_variance is NaN when n == 0 or var(R) == 0 (as CleanRL / SB3 return NaN); with n == 0 every mean and std
 *   is 0.  var(R) == 0 is decided on the variance as computed above: exact for R == 0 everywhere, or whenever the sums are
 *   exact; a constant R whose sum of squares rounds can leave a variance of a few ulp of mean^2 instead.
 * Deterministic: each rank sums in a fixed order that depends on the batch's sample count only (chunks of 4096 samples,
 *   256 strided accumulators per chunk folded by a fixed tree, chunks added in index order), not on the device or on
 *   timing: two reads of one batch are bit-identical.  The read refers to the batch in logical order, so it is
 *   bit-identical before and after aleppo_train whatever options that update ran with.
 * It is computed WHEN IT IS READ, on the context's stream, followed by that stream's synchronise like the other fields:
 *   aleppo_finish_rollout, aleppo_set_batch and aleppo_train enqueue nothing for it, and a context that never reads the
 *   field runs exactly the commands it ran before the field existed.
 * Errors: a wrong byte count is ALEPPO_ERR_INVALID_ARGUMENT like the other fields; ALEPPO_ERR_RUNTIME while a step is
 *   armed (every field), when the context holds no batch yet (neither aleppo_finish_rollout nor aleppo_set_batch has
 *   succeeded), when a caller batch has no values, and when world_size > 1 but aleppo_comm_init was not called. */
#define ALEPPO_BATCH_STATS_COUNT 10
typedef enum {
  ALEPPO_BS_COUNT = 0,              /* n: the number of unmasked samples */
  ALEPPO_BS_EXPLAINED_VARIANCE = 1, /* 1 - var(d) / var(R) */
  ALEPPO_BS_VALUE_MEAN = 2,
  ALEPPO_BS_VALUE_STD = 3,
  ALEPPO_BS_RETURN_MEAN = 4,
  ALEPPO_BS_RETURN_STD = 5,
  ALEPPO_BS_ADVANTAGE_MEAN = 6,
  ALEPPO_BS_ADVANTAGE_STD = 7,
  ALEPPO_BS_RESIDUAL_MEAN = 8,      /* of d = R - v */
  ALEPPO_BS_RESIDUAL_STD = 9
} aleppo_batch_stat;

/* Per-sample training metrics (ai::ppo::train::Metrics, src/ai/ppo/train.h:64-109), [epochs,M,B], read with
 * aleppo_read_train_metric; fields 5-12 are extensions (the reference has none).  With logr = logp(a) - old_logp(a) and
 * rho = exp(logr) per sample, computed on every update whatever ALEPPO_OPT_VALUE_CLIP is:
 *   approx_kl     = (rho - 1) - logr                  (the "k3" estimator CleanRL logs as approx_kl)
 *   clip_fraction = |rho - 1| > clip_param ? 1 : 0     (strict)
 * The two MEAN fields are the masked means of those planes per minibatch, float [epochs,M] (count = epochs * M), with the
 * denominator of aleppo_minibatch_metrics: the global unmasked count (under data parallelism they are global means).
 * Fields 9-10 are the statistics ALEPPO_OPT_ADV_NORM_MINIBATCH normalised each minibatch's advantages with in the last
 * aleppo_train, float [epochs,M] (count = epochs * M; with contiguous minibatches every epoch's row is the same): mean_f
 * and (float)std as defined there.  Reading them after an update that ran with the option off is ALEPPO_ERR_RUNTIME.
 * Fields 11-12 are the exact KL(pi_old || pi) of ALEPPO_OPT_KL_PENALTY: per sample [epochs,M,B] (unmasked, like field 5)
 * and its masked means [epochs,M] (like field 7: global means under data parallelism).  Reading them after an update
 * that ran with the option off is ALEPPO_ERR_RUNTIME, as for fields 9-10. */
typedef enum {
  ALEPPO_M_TOTAL_LOSSES = 0,
  ALEPPO_M_CLIPPED_LOSSES = 1,
  ALEPPO_M_VALUE_LOSSES = 2,
  ALEPPO_M_ENTROPIES = 3,
  ALEPPO_M_RATIO = 4,
  ALEPPO_M_APPROX_KL = 5,          /* [epochs,M,B] per sample, unmasked, in aleppo_read_sample_order order */
  ALEPPO_M_CLIP_FRACTION = 6,      /* [epochs,M,B] per sample (0 / 1), same conventions */
  ALEPPO_M_MEAN_APPROX_KL = 7,     /* [epochs,M] masked means */
  ALEPPO_M_MEAN_CLIP_FRACTION = 8, /* [epochs,M] masked means */
  ALEPPO_M_ADV_MEAN = 9,           /* [epochs,M] mean_f of ALEPPO_OPT_ADV_NORM_MINIBATCH */
  ALEPPO_M_ADV_STD = 10,           /* [epochs,M] (float)std of ALEPPO_OPT_ADV_NORM_MINIBATCH */
  ALEPPO_M_KL = 11,                /* [epochs,M,B] per-sample exact KL of ALEPPO_OPT_KL_PENALTY, unmasked */
  ALEPPO_M_MEAN_KL = 12            /* [epochs,M] masked means of ALEPPO_M_KL */
} aleppo_metric_field;

/* ------------------------------------------------------------------ lifetime */
int aleppo_abi_version(void);
/* ALEPPO_OK if HIP device `device_ordinal` exists and is a gfx950; ALEPPO_ERR_NO_DEVICE / _INVALID_ARGUMENT otherwise
 * (the check aleppo_create makes, on its own: what main() learns from torch::cuda::is_available(), train.cc:336-345). */
int aleppo_device_check(int device_ordinal);
/* Replaces the construction done in main(): Network + Adam + Rollout(+Buffer) (train.cc:358-387). */
int aleppo_create(const aleppo_config *cfg, aleppo_ctx **out);
void aleppo_destroy(aleppo_ctx *ctx);
/* Message of the last failed call on ctx (ctx may be NULL for aleppo_create failures). */
const char *aleppo_last_error(const aleppo_ctx *ctx);

/* ------------------------------------------------------------------ parameters
 * Flat float32 in libtorch parameters() order of NetworkImpl (train.cc:230-253):
 * sequential.{0,2,4,7}.{weight,bias}, action_head.{weight,bias}, value_head.{weight,bias}. */
int aleppo_param_count(const aleppo_ctx *ctx, size_t *count);
int aleppo_load_params(aleppo_ctx *ctx, const float *flat, size_t count);   /* also resets Adam state */
int aleppo_export_params(aleppo_ctx *ctx, float *flat, size_t count);
/* Gradient of the LAST minibatch as clip_grad_norm_ left it (scaled), same order. Parity dumps. */
int aleppo_export_grads(aleppo_ctx *ctx, float *flat, size_t count);

/* Checkpoint / resume (the reference has none): Adam moments in the same order as the
 * parameters plus the step count; together with aleppo_export_params this is the whole learner state. */
int aleppo_export_optimizer(aleppo_ctx *ctx, float *exp_avg, float *exp_avg_sq, int64_t *step, size_t count);
int aleppo_import_optimizer(aleppo_ctx *ctx, const float *exp_avg, const float *exp_avg_sq, int64_t step,
                            size_t count);
/* The state of ALEPPO_OPT_REWARD_SCALE: stats = (count, mean, var) of the running statistics, returns = the running
 * discounted return G[e] of this rank's environments, double [num_envs].  With the two pairs above this is the whole
 * learner state again: a fresh context that imports all three continues bit for bit.  The scale, batch count and clip
 * counter of ALEPPO_F_REWARD_SCALE describe the last scaled rollout and are not part of it (an import leaves them).
 * ALEPPO_ERR_INVALID_ARGUMENT: num_envs != config.num_envs, a null pointer, and for the import a non-finite entry,
 * count <= 0 or var < 0 (nothing is changed then).  Both work whether the option is on or not, synchronise the
 * context's own stream only, and are ALEPPO_ERR_RUNTIME while a step is armed. */
int aleppo_export_reward_scale(aleppo_ctx *ctx, double stats[3], double *returns, size_t num_envs);
int aleppo_import_reward_scale(aleppo_ctx *ctx, const double stats[3], const double *returns, size_t num_envs);
/* The rollout side of a checkpoint - what the three pairs above do not carry across a process boundary: the current
 * frame stacks and the counter of the acting generator.  With it a fresh context continues the RUN bit for bit, not only
 * the learner: the rollout that follows an import is the one the exporting context would have run - actions, logits,
 * values and every plane.
 * observations: uint8 [num_envs,4,84,84] in reference layout, the observation the next aleppo_act will act on (the bytes
 *   of ALEPPO_F_CURRENT_OBS).  words[0]: the counter of aleppo_act's built-in generator (every aleppo_act and the
 *   bootstrap forward of aleppo_finish_rollout advance it by one); words[1..3] are reserved: the export writes 0, the
 *   import refuses anything else.
 * Both calls are valid BETWEEN ROLLOUTS only: the next slot to fill is 0, which holds after aleppo_create and after
 *   aleppo_finish_rollout, with or without the aleppo_train that follows; at any other time ALEPPO_ERR_RUNTIME, as while a
 *   step is armed.  A null pointer, num_envs != config.num_envs and a non-zero reserved word are
 *   ALEPPO_ERR_INVALID_ARGUMENT.  A call that fails changes nothing.
 * The import puts the stacks where a finished rollout leaves its last observation (the next aleppo_act carries them into
 *   the first slot, as it does after aleppo_finish_rollout), drops the acting scratch aleppo_step pre-computed and sets the
 *   counter.  The batch (a rollout that was finished but not trained on yet included), the metrics, the options and the
 *   evaluation lanes are not part of the state and are left alone.
 * Both synchronise the context's own stream only and are never a collective; staging is grown on demand and kept until
 *   aleppo_destroy like the other boundary buffers. */
#define ALEPPO_ROLLOUT_STATE_WORDS 4
int aleppo_export_rollout_state(aleppo_ctx *ctx, uint8_t *observations, uint64_t words[ALEPPO_ROLLOUT_STATE_WORDS],
                                size_t num_envs);
int aleppo_import_rollout_state(aleppo_ctx *ctx, const uint8_t *observations,
                                const uint64_t words[ALEPPO_ROLLOUT_STATE_WORDS], size_t num_envs);
/* A digest of the whole run state, computed on the device where the state is: four 64-bit words, one per section, that
 * any host can recompute from the exported state.  Two contexts whose words agree hold the same run state (up to a
 * 64-bit hash collision): a resumed run proves that it continues the run that was saved, and two data-parallel ranks -
 * which must hold the same parameters and Adam state, and drift apart when they are given different options - can be
 * compared from their logs, without moving 20 MB to the host per check.
 * With splitmix64 as specified at aleppo_read_sample_order, u64 arithmetic that wraps, and w a sequence of 32-bit words:
 *   D(tag, w[0..n)) = sum_i splitmix64( splitmix64(tag) ^ (((uint64)i << 32) | w_i) )
 *   ALEPPO_DG_PARAMS        D(1, the bits of the flat fp32 parameters of aleppo_export_params, in that order)
 *   ALEPPO_DG_OPTIMIZER     D(2, bits of exp_avg) + D(3, bits of exp_avg_sq) + splitmix64(splitmix64(4) ^ (uint64)step)
 *                           (aleppo_export_optimizer)
 *   ALEPPO_DG_ROLLOUT       D(5, s) + splitmix64(splitmix64(6) ^ words[0]) of aleppo_export_rollout_state, with
 *                           s[e * 7056 + p] = obs[e,0,p] | obs[e,1,p] << 8 | obs[e,2,p] << 16 | obs[e,3,p] << 24
 *   ALEPPO_DG_REWARD_SCALE  D(7, w), w = the doubles (count, mean, var, G[0 .. num_envs)) of aleppo_export_reward_scale,
 *                           each as its low and then its high 32-bit word; before ALEPPO_OPT_REWARD_SCALE was ever used
 *                           that is the initial state (1e-4, 0, 1) and G = 0
 * The sums commute, so the words do not depend on how the device walks its private layouts.  Computed WHEN CALLED, on the
 * context's stream (one pass that only reads the state), followed by that stream's synchronise; never a collective; a
 * context that never calls it enqueues nothing for it.  ALEPPO_ERR_RUNTIME while a step is armed and, because the rollout
 * section is defined between rollouts only (see above), while a rollout is in progress; a null pointer is
 * ALEPPO_ERR_INVALID_ARGUMENT. */
#define ALEPPO_DIGEST_COUNT 4
typedef enum {
  ALEPPO_DG_PARAMS = 0,
  ALEPPO_DG_OPTIMIZER = 1,
  ALEPPO_DG_ROLLOUT = 2,
  ALEPPO_DG_REWARD_SCALE = 3
} aleppo_digest_section;
int aleppo_state_digest(aleppo_ctx *ctx, uint64_t out[ALEPPO_DIGEST_COUNT]);

/* Per-tensor parameter, gradient and update norms (what wandb.watch or a few lines of torch give a CleanRL / SB3 user; the
 * reference has none), reduced on the device where P, the gradient and the Adam moments are: which layer's gradient
 * vanished or exploded, how large the last step was relative to the weights, which tensor went non-finite first.
 * out: double [ALEPPO_TENSOR_STATS_ROWS][ALEPPO_TENSOR_STATS_COLS], row-major; count must be 130.  Rows 0-11 are the twelve
 *   tensors in the libtorch parameters() order of aleppo_export_params (conv1.w, conv1.b, conv2.w, conv2.b, conv3.w,
 *   conv3.b, fc.w, fc.b, action.w, action.b, value.w, value.b), row 12 is the whole model.  Columns: aleppo_tensor_stat.
 * Elements, per exported element i (the alignment pads of the private layout are not elements):
 *   p_i  the fp32 master parameter (bf16 contexts have one too; the bf16 copies are not read)
 *   g_i  = float32(raw_i * coef): exactly the element aleppo_export_grads returns - the gradient of the last minibatch,
 *        coef formed as that function forms it from the stored pre-clip norm and the limit the last update ran with
 *   u_i  = s * (m_i / (sqrtf(v_i) / c + eps)) in fp32: what the last optimizer step subtracted from p_i.  m, v are the
 *        moments as they stand (the step subtracts this expression of the very m, v it then stores); s = float32(lr /
 *        (1 - beta1^t)) and c = float32(sqrt(1 - beta2^t)) are the two schedule scalars of the last optimizer step the
 *        context ran, t the step count aleppo_export_optimizer returns
 * Arithmetic: every element is widened to double and squared (exact); the sums are in double, in an order that is a
 *   function of (H, A) only - per tensor of the private layout chunks of 4096 elements, inside a chunk each of 256
 *   threads adds its 16 elements in index order and the threads are folded by a fixed tree, the chunks are added in index
 *   order; no atomics, and the grid does not depend on the device.  A norm is sqrt of its sum, max-abs is exact.  A
 *   non-finite element is counted and left out of every sum and maximum of its column group: p for columns 1-3 (count:
 *   PARAM_NONFINITE), (g, m, v, u) for columns 4-9 (an element whose g, m, v or u is NaN / Inf counts once in
 *   STEP_NONFINITE and enters neither GRAD_ nor UPDATE_ columns), so the norms stay informative when one element is
 *   poisoned.  Row 12: SIZE and the counts are the sums of the rows, a norm is sqrt of the twelve sums of squares added
 *   in row order, max-abs the maximum, the ratio formed from its own two norms.  Two reads without an update in between
 *   are bit-identical.
 * sections: a non-empty set of aleppo_tensor_stats_section bits.  Columns 0-3 belong to ALEPPO_TS_SEC_PARAMS and are valid
 *   any time after aleppo_create (with that section alone only P is read).  Columns 4-9 belong to ALEPPO_TS_SEC_STEP and
 *   need an aleppo_train to have succeeded on this context with no aleppo_load_params / aleppo_import_optimizer since
 *   (those replace the state the step is recomputed from): otherwise ALEPPO_ERR_RUNTIME, and nothing is written.
 *   UPDATE_RATIO needs PARAM_NORM, so STEP computes it whether or not PARAMS was requested.  The columns of a section
 *   that was not requested are written as 0; SIZE is always written.
 * Computed WHEN CALLED, on the context's stream (one pass that only reads, then one small launch), followed by that
 *   stream's synchronise and one copy of 1040 bytes; the scratch is allocated on first use and kept until aleppo_destroy.
 *   Never a collective: under data parallelism the parameters and the all-reduced gradient are the same on every rank, so
 *   one rank reading suffices.  aleppo_train, a captured update (ALEPPO_OPT_UPDATE_GRAPH) and every other entry point
 *   enqueue nothing for it; reading it neither re-arms a capture nor changes a bit of the run.
 * Errors: sections 0 or with other bits, a null pointer or a wrong count are ALEPPO_ERR_INVALID_ARGUMENT (nothing is
 *   written); ALEPPO_ERR_RUNTIME while a step is armed. */
#define ALEPPO_TENSOR_STATS_ROWS 13   /* the 12 tensors in libtorch parameters() order, then the whole model */
#define ALEPPO_TENSOR_STATS_COLS 10
typedef enum { ALEPPO_TS_SEC_PARAMS = 1, ALEPPO_TS_SEC_STEP = 2 } aleppo_tensor_stats_section;
typedef enum {
  ALEPPO_TS_SIZE = 0,            /* elements of the tensor (alignment pads are not elements) */
  ALEPPO_TS_PARAM_NORM = 1,      /* sqrt(sum p^2) */
  ALEPPO_TS_PARAM_MAXABS = 2,
  ALEPPO_TS_PARAM_NONFINITE = 3, /* how many p are NaN / Inf */
  ALEPPO_TS_GRAD_NORM = 4,       /* of g: the elements aleppo_export_grads returns (last minibatch, clipped) */
  ALEPPO_TS_GRAD_MAXABS = 5,
  ALEPPO_TS_UPDATE_NORM = 6,     /* of u: what the last optimizer step subtracted from p */
  ALEPPO_TS_UPDATE_MAXABS = 7,
  ALEPPO_TS_UPDATE_RATIO = 8,    /* UPDATE_NORM / PARAM_NORM, IEEE double division (0 / 0 = NaN) */
  ALEPPO_TS_STEP_NONFINITE = 9   /* elements whose g, m, v or u is NaN / Inf */
} aleppo_tensor_stat;
int aleppo_tensor_stats(aleppo_ctx *ctx, int sections, double *out, size_t count);

/* ------------------------------------------------------------------ rollout (Rollout::rollout, rollout.cc:198-278)
 * Per slot t = 0..T-1 the caller does  act -> (step its emulators) -> push_frames -> record_step,
 * then finish_rollout.  aleppo_step = push_frames + record_step in one upload. */

/* Action selector (train.cc:367-379): eval forward on the current stack, softmax,
 * multinomial(1, replacement) = argmax(p/q).  noise: float [E,A] of Exp(1) draws (host) to reproduce a
 * captured stream bit-exactly, or NULL for the built-in counter-based generator.
 * *actions_pinned: int64 [E] in page-locked host memory owned by ctx, valid when the call returns and
 * until the next aleppo_act; env worker threads may read it concurrently (replaces the per-env
 * actions[i].item<int64_t>() of rollout.cc:312-313).  Stores logits/values for slot t.
 * Built-in generator (noise == NULL): Philox4x32-10 under the key config.seed itself (key words seed lo, seed hi; the
 *   evaluation lanes' key differs, see aleppo_eval_act).  Counter words { n lo, n hi, e, k / 4 } for environment e and
 *   action k, output words c[0..3]: q_k = -logf(U(c[k % 4])), U(x) = ((x >> 8) + 0.5) / 2^24 in fp32.
 *   n is the acting counter: 0 at aleppo_create, + 1 for EVERY acting head that is enqueued, whether it draws or takes the
 *   caller's noise - each aleppo_act (also the one aleppo_arm_step enqueues ahead, and each slot of aleppo_replay_rollout
 *   and aleppo_env_rollout) and aleppo_finish_rollout's bootstrap call, whose draw is discarded.  A rollout of T slots
 *   therefore uses n0 .. n0 + T - 1 for its slots and n0 + T for the bootstrap, and the next rollout starts at n0 + T + 1.
 *   The counter is words[0] of aleppo_export_rollout_state. */
int aleppo_act(aleppo_ctx *ctx, const float *noise, const int64_t **actions_pinned);

/* Rollout::update_observations (rollout.cc:184-196) fused with Buffer::add's observation copy
 * (buffer.cc:47) and, for ALEPPO_FRAMES_RAW_PAIR, the preprocessing the reference does on env threads.
 * episode_start: uint8 [E] = is_episode_start_cpu_ at ENTRY of this slot (rollout.cc:190). */
int aleppo_push_frames(aleppo_ctx *ctx, const uint8_t *frames, int frame_kind, int location,
                       const uint8_t *episode_start);
/* Page-locked host memory the GPU can address, for the buffers the emulator worker threads write their frames into
 * (replaces Rollout::screen_buffers_, src/ai/rollout.cc:325-326): pass it to aleppo_step / aleppo_push_frames with
 * ALEPPO_HOST_MAPPED and the ingest kernel reads the frames in place - no staging copy on the slot's critical path.
 * The caller must not rewrite a buffer before the aleppo_act / aleppo_finish_rollout that follows its aleppo_step has
 * returned (the emulators are stepped after aleppo_act, so the natural loop satisfies this with ONE buffer). */
int aleppo_host_alloc(aleppo_ctx *ctx, size_t bytes, void **ptr);
int aleppo_host_free(aleppo_ctx *ctx, void *ptr);
/* 256-entry palette -> gray LUT used by ALEPPO_FRAMES_RAW_PAIR (default: identity). */
int aleppo_set_gray_lut(aleppo_ctx *ctx, const uint8_t *lut256);

/* The per-env scalar writes of rollout.cc:212-227 + Buffer::add (buffer.cc:48-54) for slot t, as ONE
 * upload; advances t.  All arrays are host [E]; rewards of envs in an episode-start slot are whatever the
 * caller kept (the reference keeps the stale value, rollout.cc:214). */
int aleppo_record_step(aleppo_ctx *ctx, const float *rewards, const uint8_t *terminated,
                       const uint8_t *truncated, const uint8_t *episode_start);
int aleppo_step(aleppo_ctx *ctx, const uint8_t *frames, int frame_kind, int location, const float *rewards,
                const uint8_t *terminated, const uint8_t *truncated, const uint8_t *episode_start);

/* The same step with the stream running ONE SLOT AHEAD of the emulator (replaces the launch latency between
 * rollout.cc:312-313, the actions reaching the workers, and rollout.cc:204-208, the next forward pass).
 * aleppo_arm_step - called right after aleppo_act returned slot t's actions, BEFORE the emulators are stepped - enqueues
 * the ingest of the frames the emulators are about to write into `frames` and of the episode-start flags they are about
 * to write into `episode_start_mapped` (uint8 [E]; both in mapped page-locked memory from aleppo_host_alloc), plus slot
 * t+1's acting kernels (noise_next: that slot's sampling noise or NULL), all behind a one-wave gate kernel that polls a
 * release word in mapped host memory.  aleppo_release_step - called when the emulators are done - releases the
 * stream and records slot t's scalars (the per-env writes of rollout.cc:212-227; episode starts are read from
 * episode_start_mapped); it advances t.  The next aleppo_act only waits for the actions (its noise argument is ignored:
 * that head is already on the stream with noise_next).  Between the two calls every
 * other stateful entry point fails with ALEPPO_ERR_RUNTIME.  Results are bit-identical to aleppo_act / aleppo_step.
 * The gate has an exit condition: if it is not released within ALEPPO_OPT_GATE_TIMEOUT_MS (default 120 000) it gives
 * up, the stream drains, and the release (or the next aleppo_act / aleppo_finish_rollout) fails the context: from then
 * on every call returns ALEPPO_ERR_RUNTIME with that message until aleppo_destroy; the frame buffers must stay
 * allocated until then.  A null argument to aleppo_release_step is reported while the step is still armed (repeat the
 * call). */
int aleppo_arm_step(aleppo_ctx *ctx, const uint8_t *frames, int frame_kind, const uint8_t *episode_start_mapped,
                    const float *noise_next);
int aleppo_release_step(aleppo_ctx *ctx, const float *rewards, const uint8_t *terminated, const uint8_t *truncated);

/* Rollout::rollout()'s slot loop (rollout.cc:198-278) over a PRE-RECORDED environment trace: for t in [0, T):
 * aleppo_act (built-in RNG) then aleppo_step with slot t of the trace.  frames: DEVICE memory, slot t at
 * frames + t * slot_stride_bytes (16-byte aligned); rewards [T][E] f32 and terminated / truncated / episode_start
 * [T][E] u8 are HOST arrays.  frame_location: ALEPPO_DEVICE or ALEPPO_HOST_MAPPED (the whole trace in mapped
 * page-locked host memory: what a ring filled by emulator threads looks like to the device).  noise: float
 * [T][E][A] Exp(1) draws (host) for a reproducible action stream, or NULL for the built-in generator.  The sampled
 * actions do not influence a recorded trace, so this entry point only serves replay / throughput measurement with
 * the whole host loop native (like the reference's C++ loop); a live emulator calls aleppo_act / aleppo_step itself.
 * Leaves the context ready for aleppo_finish_rollout. */
int aleppo_replay_rollout(aleppo_ctx *ctx, const uint8_t *frames, int frame_kind, int frame_location,
                          size_t slot_stride_bytes, const float *rewards, const uint8_t *terminated,
                          const uint8_t *truncated, const uint8_t *episode_start, const float *noise);

/* Tail of Rollout::rollout (rollout.cc:268-270) + Buffer::get (buffer.cc:58-77) + prepare_batch
 * (train.cc:272-283): bootstrap forward (draws and discards one sample like the reference), reward
 * clamp, GAE, returns, masks, old log-probs.  ALEPPO_ERR_RUNTIME if the buffer is not full
 * (buffer.cc:64-65); ALEPPO_ERR_INVALID_ARGUMENT if flags overlap (gae.cc:49-53). */
int aleppo_finish_rollout(aleppo_ctx *ctx, const float *noise);

/* ------------------------------------------------------------------ update (ai::ppo::train::train, train.h:133-157)
 * epochs x num_mini_batches contiguous env-major slices (ALEPPO_OPT_MINIBATCH_SHUFFLE = 1: a fresh permutation per epoch,
 * see aleppo_read_sample_order); per minibatch forward, loss, backward,
 * [RCCL all-reduce when world_size>1], clip_grad_norm_, Adam.  lr is this rollout's annealed rate
 * (train.cc:424-428).  out_metrics: [epochs*num_mini_batches], may be NULL.
 * ALEPPO_ERR_RUNTIME if E*T % num_mini_batches != 0 (train.h:140-143). */
int aleppo_train(aleppo_ctx *ctx, double lr, int epochs, int num_mini_batches,
                 aleppo_minibatch_metrics *out_metrics);
/* Per-sample metric tensors of the last aleppo_train, float [epochs,M,B], in the order of aleppo_read_sample_order:
 * element [e][m][b] belongs to logical sample order[e][m*B + b].  Fields 7-10 and 12: float [epochs,M], count =
 * epochs * M. */
int aleppo_read_train_metric(aleppo_ctx *ctx, int metric_field, float *dst, size_t count);
/* Sample order of the last aleppo_train, int32 [epochs][N] (count = epochs * N, N = the batch's sample count): row e,
 * position m*B + b is the logical sample (n = e_env*T + t of the rollout, or row n of aleppo_set_batch) that sat at
 * position b of minibatch m in epoch e.  Identity rows after a contiguous update; ALEPPO_ERR_RUNTIME before any update.
 *
 * With ALEPPO_OPT_MINIBATCH_SHUFFLE = 1 row e is the keyed bijection below, which any host can recompute (stateless,
 * each position on its own; u32 / u64 arithmetic wraps):
 *   splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                  z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 *   fmix32(h):     h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16; return h
 *   w = ceil(log2 N), at least 2, rounded up to an even number; h = w / 2; mask = 2^h - 1
 *   step0 = the Adam step count when epoch e starts (the context's step at the call, + e * num_mini_batches; it is what
 *           aleppo_export_optimizer / aleppo_import_optimizer carry, so a resumed run replays the same orders)
 *   key = splitmix64(config.seed ^ splitmix64(((uint64)config.rank << 40) ^ step0))
 *   k_r = (uint32) splitmix64(key + r), r = 0..3
 *   P(x): L = x >> h, R = x & mask; for r = 0..3: (L, R) <- (R, L ^ (fmix32(R ^ k_r) & mask)); return (L << h) | R
 *   order[e][i]: y = P(i); while (y >= N) y = P(y)      (cycle-walking on [0, 2^w))
 * Each rank permutes its own N local samples (rank is in the key); a global minibatch is the union of the ranks'
 * shuffled local minibatches. */
int aleppo_read_sample_order(aleppo_ctx *ctx, int32_t *dst, size_t count);

/* Same update on a caller-supplied batch (what ai::ppo::train::train takes: train.h:34-57, 133-137):
 * observations uint8 [N,4,84,84], actions int64 [N], old log-probs float [N,A], advantages, returns
 * float [N], masks uint8 [N] (host).  N <= E*T. Used by the parity tests. */
int aleppo_set_batch(aleppo_ctx *ctx, const uint8_t *observations, const int64_t *actions,
                     const float *log_probabilities, const float *advantages, const float *returns,
                     const uint8_t *masks, int64_t n);
/* The values v_old the caller batch was collected with, float [n], for ALEPPO_OPT_VALUE_CLIP: called after
 * aleppo_set_batch with the same n (ALEPPO_ERR_INVALID_ARGUMENT otherwise; ALEPPO_ERR_RUNTIME without a caller batch).
 * Stored like the other planes of that call (rounded to the rollout plane type).  The next aleppo_set_batch or
 * aleppo_finish_rollout forgets them. */
int aleppo_set_batch_values(aleppo_ctx *ctx, const float *values, int64_t n);

int aleppo_read_batch(aleppo_ctx *ctx, int field, void *dst, size_t bytes);
/* Network forward only (NetworkImpl::forward, train.cc:255-265) on host observations uint8
 * [n,4,84,84] -> logits float [n,A], values float [n].  n <= max(E, max_minibatch). */
int aleppo_forward(aleppo_ctx *ctx, const uint8_t *observations, int64_t n, float *logits, float *values);

/* The hidden activations of that forward pass (what a forward hook gives a CleanRL / SB3 user; the reference has none):
 * for linear probes, embedding plots, a feature rank of one's own (aleppo_feature_rank has the usual ones), and as the
 * ground truth of aleppo_activation_stats.
 * observations and n as aleppo_forward: host uint8 [n,4,84,84], 1 <= n <= max(E, max_minibatch).  Each output may be NULL
 * (that layer is neither converted nor copied); at least one must be given.  Outputs, host float, in the reference's
 * tensor order (NCHW; the channel index is the reference's output-channel index):
 *   conv1 [n,32,20,20]   conv2 [n,64,9,9]   conv3 [n,64,7,7]   after the ReLU
 *   fc    [n,H]          the 3136 -> H linear layer's output, bias included; it has NO ReLU, so fc is signed
 * The values are the stored activations widened exactly: a bf16 context's conv activations are bf16 values in a float; fc
 * is fp32 on both precisions.  Like aleppo_forward it runs the network in the shared activation scratch, so what
 * aleppo_step pre-computed for the next aleppo_act is dropped (the act recomputes it: same bits).  The conversion runs on
 * the context's stream into staging the context keeps until aleppo_destroy.  It changes nothing the rollout or the update
 * can observe.  Errors: a NULL observations, no output, n out of range: ALEPPO_ERR_INVALID_ARGUMENT; ALEPPO_ERR_RUNTIME
 * while a step is armed. */
int aleppo_forward_activations(aleppo_ctx *ctx, const uint8_t *observations, int64_t n, float *conv1, float *conv2,
                               float *conv3, float *fc);

/* The stored tensors of both passes as the LAST minibatch of the last aleppo_train left them: what a per-layer check of the
 * backward pass starts from (tests/backward_ref.py).  It runs nothing of the network and writes nothing the update reads:
 * conversion kernels and copies on the context's stream into the staging aleppo_forward_activations uses.  aleppo_train
 * enqueues what it enqueued before; it only notes on the host that, and with how many samples B = N / num_mini_batches, its
 * last minibatch ran.  A context that never calls this runs what it ran before.
 * Outputs, host float, `capacity` samples each (>= B; B samples are written), each may be NULL, at least one must be given;
 * tensor order and widening as aleppo_forward_activations:
 *   conv1 [B,32,20,20]  conv2 [B,64,9,9]  conv3 [B,64,7,7]   the activations a1, a2, a3
 *   fc [B,H]            h as the head kernel read it: its split-K slabs added in the head kernel's order
 *   dfc [B,H]           dL/dh as the head kernel stored it (bf16 on a bf16 context)
 *   dconv3 [B,64,7,7]  dconv2 [B,64,9,9]  dconv1 [B,32,20,20]   dL/d(pre-activation) of conv3, conv2, conv1 as stored
 * Sample b is the b-th sample of that minibatch: sample (M - 1) B + b of the batch, or, after a shuffled update, of the last
 * epoch's order (aleppo_read_sample_order).  *n = B; *stored = the aleppo_bwd_tensor bits of what the route stored: all but
 * ALEPPO_BWD_DCONV1 on the fused backward tail (ALEPPO_OPT_FUSED_BWD), which keeps dz1 on the CU - dconv1 is then left
 * untouched.  n and stored may be NULL.
 * Errors: no output, capacity < B: ALEPPO_ERR_INVALID_ARGUMENT; before any aleppo_train, after anything else has run the
 * network since (aleppo_act / aleppo_step, aleppo_forward and every call that forwards as it does) or while a step is
 * armed: ALEPPO_ERR_RUNTIME. */
typedef enum {
  ALEPPO_BWD_CONV1 = 1,
  ALEPPO_BWD_CONV2 = 2,
  ALEPPO_BWD_CONV3 = 4,
  ALEPPO_BWD_FC = 8,
  ALEPPO_BWD_DFC = 16,
  ALEPPO_BWD_DCONV3 = 32,
  ALEPPO_BWD_DCONV2 = 64,
  ALEPPO_BWD_DCONV1 = 128
} aleppo_bwd_tensor;
int aleppo_export_backward(aleppo_ctx *ctx, int64_t capacity, float *conv1, float *conv2, float *conv3, float *fc,
                           float *dfc, float *dconv3, float *dconv2, float *dconv1, int64_t *n, uint32_t *stored);

/* What the LAST ACTING FORWARD of the rollout left in the context's scratch: what a per-link check of the acting path starts
 * from (tests/acting_ref.py).  That forward is aleppo_act's, the one aleppo_step pre-computed for the coming slot (fused
 * ingest: an export between aleppo_step and aleppo_act returns the coming slot's), or aleppo_finish_rollout's bootstrap;
 * aleppo_env_rollout's slots are aleppo_act's.  A test hook like aleppo_export_backward: it runs nothing but conversion
 * kernels and copies, into the staging aleppo_forward_activations uses, and writes nothing the rollout or the update reads.
 * The acting calls enqueue what they enqueued before and only note on the host that, and with how many samples, they ran.
 * Outputs, host float, each may be NULL, at least one must be given; n = num_envs samples are written, `capacity` (>= n) is
 * the samples the conv outputs have room for; tensor order and widening as aleppo_forward_activations:
 *   conv1 [n,32,20,20]  conv2 [n,64,9,9]   where the route stored them: the generic and fp32 routes, and the fused bf16
 *                                          launch under ALEPPO_OPT_ACT_STORE = 1; otherwise left untouched
 *   conv3 [n,64,7,7]
 *   fc_parts [ALEPPO_FC_SPLITS,n,H]        the split-K slices of the fc layer, fp32, no bias: slice z is the product of
 *                                          columns [448 z, 448 (z + 1)) of conv3 in its stored order (pixel-major, channel
 *                                          last: row z of the 7x7 map) with the matching fc weights.  The acting head adds
 *                                          them to the fc bias one after the other, z = 0 .. 6, in fp32, and never stores
 *                                          the sum.  Packed with n (not capacity); room for ALEPPO_FC_SPLITS * n * H floats
 * *n = num_envs; *stored = the aleppo_acting_tensor bits of what was there to read.  n and stored may be NULL.
 * The evaluation lanes have scratch of their own and are not exported (their bits equal aleppo_act's).
 * Errors: no output, capacity < n: ALEPPO_ERR_INVALID_ARGUMENT; before any acting forward, after anything else has run the
 * network in the scratch or replaced the parameters since (aleppo_train, aleppo_forward and every call that forwards as it
 * does - the diagnostics, aleppo_refresh_advantages -, aleppo_load_params, a recycle, aleppo_shrink_perturb) or while a step
 * is armed: ALEPPO_ERR_RUNTIME.  A refused call changes nothing. */
#define ALEPPO_FC_SPLITS 7
typedef enum {
  ALEPPO_ACTING_CONV1 = 1,
  ALEPPO_ACTING_CONV2 = 2,
  ALEPPO_ACTING_CONV3 = 4,
  ALEPPO_ACTING_FC_PARTS = 8
} aleppo_acting_tensor;
int aleppo_export_acting(aleppo_ctx *ctx, int64_t capacity, float *conv1, float *conv2, float *conv3, float *fc_parts,
                         int64_t *n, uint32_t *stored);

/* Per-unit and per-layer activation statistics, reduced on the device where the activations are: dormant units (Sokar et
 * al. 2023, "The Dormant Neuron Phenomenon in Deep RL"), dead units and firing rates (Moalla et al. 2024, "No
 * Representation, No Trust").  The activations (about 45 KB per sample in bf16 at H = 512) never leave the device.
 * Samples: observations != NULL: the caller's n observations, as aleppo_forward_activations.  observations == NULL and
 *   n == 0: THE BATCH THE CONTEXT HOLDS - every sample aleppo_train would train on now (a rollout batch or an
 *   aleppo_set_batch batch, masked samples included), read in place from the observation slots in logical order, in
 *   forward chunks of at most max(E, max_minibatch) samples; no observation crosses PCIe.  Never a collective: under data
 *   parallelism it describes this rank's samples.
 * units: double [160 + H][ALEPPO_ACT_UNIT_COLS], row-major; unit_count must be (160 + H) * 5.  Rows: conv1 channels 0-31,
 *   conv2 0-63, conv3 0-63, fc 0..H-1 (the reference's output-channel index, as aleppo_forward_activations exports it).
 *   A unit of a layer has K = samples * PIX positions, PIX = 400, 81, 49, 1.  Over its finite elements a (a NaN / Inf is
 *   counted in NONFINITE and left out of everything else): S = sum |a|, P = #{a > 0}, X = max |a|.  Columns:
 *   aleppo_act_unit_stat.  Because fc is signed, everything is defined with |a|, and POSITIVE_FRACTION of an fc unit is the
 *   share of samples on which the feature is positive (on conv1-3 it is the ReLU's firing rate).
 * layers: double [ALEPPO_ACT_LAYER_ROWS][ALEPPO_ACT_LAYER_COLS]; layer_count must be 40.  Rows: conv1, conv2, conv3, fc,
 *   total.  Columns: aleppo_act_layer_stat.  The total row adds the four rows in row order (UNITS, ELEMENTS, the sums behind
 *   MEAN_ABS and POSITIVE_FRACTION, DEAD, DORMANT, NONFINITE); its MAX_ABS is the maximum.
 * tau: the dormancy threshold, finite and >= 0 (Sokar et al. use 0, 0.025 and 0.1).
 * Arithmetic: every element is widened exactly; S is a double sum whose order is a function of (layer, sample count,
 *   max(E, max_minibatch), precision) only - per forward chunk a layer [rows][C] is cut into row chunks of 16384 16-byte
 *   loads (fc: 256 rows), inside a chunk a thread adds its rows in order and the threads of a channel are folded by a fixed
 *   tree, the chunks are added in index order, then the units of a layer in unit order.  No floating-point atomics; the grid
 *   does not depend on the device.  Counts, maxima and P / K are exact.  Two calls with nothing in between are bit-identical,
 *   and with at most max(E, max_minibatch) samples the batch source equals the caller source on the same observations.
 * Computed WHEN CALLED, on the context's stream: per chunk the forward pass and one launch that only reads, then one small
 *   finalising launch, the stream's synchronise and two small copies.  Scratch is allocated on first use and kept until
 *   aleppo_destroy.  Allowed wherever aleppo_forward is - in the middle of a rollout too: the next aleppo_act then
 *   recomputes what aleppo_step had pre-computed (same bits).  aleppo_train, a captured update (ALEPPO_OPT_UPDATE_GRAPH) and
 *   every other entry point enqueue nothing for it; calling it neither re-arms a capture nor changes a bit of the run.
 * Errors: tau negative or not finite, a NULL output, a wrong count, n out of range, NULL observations with n != 0:
 *   ALEPPO_ERR_INVALID_ARGUMENT.  The batch source without a batch, or any call while a step is armed: ALEPPO_ERR_RUNTIME.
 *   A failed call writes nothing. */
#define ALEPPO_ACT_UNIT_COLS 5
#define ALEPPO_ACT_LAYER_ROWS 5   /* conv1, conv2, conv3, fc, total */
#define ALEPPO_ACT_LAYER_COLS 8
typedef enum {
  ALEPPO_ACT_MEAN_ABS = 0,          /* S / K */
  ALEPPO_ACT_POSITIVE_FRACTION = 1, /* P / K */
  ALEPPO_ACT_MAX_ABS = 2,           /* X */
  ALEPPO_ACT_SCORE = 3,             /* MEAN_ABS_i / ((sum of the layer's MEAN_ABS, in unit order) / units): Sokar et al. eq. 1;
                                       0 where the layer mean is 0 */
  ALEPPO_ACT_NONFINITE = 4
} aleppo_act_unit_stat;
typedef enum {
  ALEPPO_ACT_L_UNITS = 0,
  ALEPPO_ACT_L_ELEMENTS = 1,          /* units * K; total: the sum */
  ALEPPO_ACT_L_MEAN_ABS = 2,          /* (sum of S, in unit order) / ELEMENTS */
  ALEPPO_ACT_L_POSITIVE_FRACTION = 3, /* (sum of P) / ELEMENTS */
  ALEPPO_ACT_L_MAX_ABS = 4,
  ALEPPO_ACT_L_DEAD = 5,              /* units with X == 0: every finite activation is zero (a ReLU unit that never fired) */
  ALEPPO_ACT_L_DORMANT = 6,           /* units with SCORE <= tau */
  ALEPPO_ACT_L_NONFINITE = 7
} aleppo_act_layer_stat;
int aleppo_activation_stats(aleppo_ctx *ctx, const uint8_t *observations, int64_t n, double tau, double *units,
                            size_t unit_count, double *layers, size_t layer_count);

/* Recycling units (ReDo, the second half of Sokar et al. 2023; the reference has none): re-initialise the incoming
 * weights of every masked unit, zero its outgoing weights and reset the Adam moments of both, in place on the device - the
 * master parameters, both moments and every derived copy (the bf16 compute copy, the data-gradient layouts) follow.
 * mask / mask_out: uint8 [160 + H] in the unit order of aleppo_activation_stats (conv1 0-31, conv2 0-63, conv3 0-63,
 *   fc 0..H-1); unit_count must be 160 + H; every mask byte must be 0 or 1.  Let m1, m2, m3, m4 be the four layers' masks.
 * What a recycle does, in the reference's tensor terms:
 *   conv1.w[o,c,kh,kw]        re-initialised if m1[o]
 *   conv2.w[o,c,kh,kw]        zero if m1[c], otherwise re-initialised if m2[o]
 *   conv3.w[o,c,kh,kw]        zero if m2[c], otherwise re-initialised if m3[o]
 *   fc.w[o, c*49 + p]         zero if m3[c], otherwise re-initialised if m4[o]
 *   conv1.b conv2.b conv3.b fc.b [o]   zero if unit o is masked
 *   action.w[a,j] value.w[0,j]         zero if m4[j]
 *   action.b value.b          never touched
 *   ZERO WINS: a weight that is both an outgoing weight of a masked unit and an incoming weight of another masked unit
 *   becomes zero (the order of ReDo's own implementation).  exp_avg and exp_avg_sq of every element a rule selects become
 *   +0.0f unless ALEPPO_RECYCLE_KEEP_MOMENTS is set; the Adam step count is unchanged.  The exported gradient, every
 *   element no rule selects and every alignment pad are not written at all.
 * The re-initialised value of element i, i its index in the flat aleppo_export_params vector, with splitmix64 as
 * specified at aleppo_read_sample_order:
 *   r = splitmix64(splitmix64(key) ^ (uint64)i)
 *   k = (int32)(r >> 40) - 8388608                       in [-2^23, 2^23)
 *   w = a_l * ((float)k * 0x1p-23f)                      fp32; the inner product is exact, so one rounding
 *   a_l = (float)sqrt(6.0 / fan_in), fan_in = 256, 512, 576, 3136 (conv1, conv2, conv3, fc)
 *   This is He-uniform on [-a_l, a_l): its per-element variance a_l^2 / 3 = 2 / fan_in is the variance of an element of
 *   the trainer's orthogonal initialisation with gain sqrt 2 (trainer/init.hpp).  It is stateless and every element is
 *   computed on its own, so any host recomputes it bit for bit, and two ranks given the same mask and key stay identical:
 *   the key must not contain the rank.
 * Afterwards aleppo_tensor_stats refuses ALEPPO_TS_SEC_STEP until the next aleppo_train (as after
 *   aleppo_import_optimizer), and what aleppo_step pre-computed for the next aleppo_act is dropped.  A captured update
 *   (ALEPPO_OPT_UPDATE_GRAPH) stays valid: no pointer changes.  counts: the masked units of conv1, conv2, conv3, fc and their
 *   sum.  An all-zero mask runs the pass and changes no bit.
 * aleppo_recycle_units takes the mask from the caller.  It is deterministic given (mask, key), so it is allowed under data
 *   parallelism: give every rank the same mask and key.
 * aleppo_recycle_dormant runs exactly the measurement of aleppo_activation_stats (observations, n and tau as there;
 *   observations == NULL and n == 0: the batch the context holds), then one small launch forms the mask from the device-side
 *   unit table - mask[u] = (the layer of u is in layers) && SCORE_u <= tau, the rule ALEPPO_ACT_L_DORMANT counts by - and the
 *   pass follows; no table crosses to the host in between.  All layers are scored on the parameters as they stood at entry
 *   and recycled together.  layers: a non-empty set of ALEPPO_RECYCLE_CONV1 ... ALEPPO_RECYCLE_FC bits.  mask_out (may be
 *   NULL) receives the mask.  Under world_size > 1 the scores describe one rank's samples and the ranks would pick different
 *   units, so it returns ALEPPO_ERR_RUNTIME there; a collective score is out of scope.
 * Both run on the context's stream, synchronise that stream only and are never a collective.  A context that never calls
 *   them enqueues and allocates exactly what it did before.
 * Errors: a NULL mask or counts, a wrong unit_count, a mask byte above 1, unknown flag bits, layers zero or with other
 *   bits: ALEPPO_ERR_INVALID_ARGUMENT; what aleppo_activation_stats refuses in tau, observations and n: the code it gives;
 *   a step is armed: ALEPPO_ERR_RUNTIME.  A failed call changes nothing. */
#define ALEPPO_RECYCLE_COUNTS 5 /* conv1, conv2, conv3, fc, total */
enum { ALEPPO_RECYCLE_CONV1 = 1, ALEPPO_RECYCLE_CONV2 = 2, ALEPPO_RECYCLE_CONV3 = 4, ALEPPO_RECYCLE_FC = 8,
       ALEPPO_RECYCLE_ALL = 15 };
enum { ALEPPO_RECYCLE_KEEP_MOMENTS = 1 }; /* flags */
int aleppo_recycle_units(aleppo_ctx *ctx, const uint8_t *mask, size_t unit_count, uint64_t key, int flags,
                         int64_t counts[ALEPPO_RECYCLE_COUNTS]);
int aleppo_recycle_dormant(aleppo_ctx *ctx, const uint8_t *observations, int64_t n, double tau, int layers,
                           uint64_t key, int flags, uint8_t *mask_out, size_t unit_count,
                           int64_t counts[ALEPPO_RECYCLE_COUNTS]);

/* The anchor of ALEPPO_OPT_ANCHOR_COEF: the parameters the optimizer step pulls toward (L2 Init: the initial ones).  A
 * fourth parameter set in the private layout, fp32 only, never forwarded, allocated on the first take or import through
 * the context's memory registry and never again; only these calls write it.  It is NOT a set aleppo_policy_diff or
 * aleppo_snapshot_take accept: their ALEPPO_SET_* stay the three they were.
 * aleppo_anchor_take(source_set): anchor = ALEPPO_SET_LIVE, ALEPPO_SET_AVERAGED or ALEPPO_SET_SNAPSHOT as it stands, one
 *   device-to-device copy on the context's main stream; the call enqueues only.
 * aleppo_anchor_import / aleppo_anchor_export move it in the order and with the count checks of aleppo_snapshot_import /
 *   aleppo_snapshot_export (aleppo_load_params / aleppo_export_params).
 * Interactions: aleppo_load_params, aleppo_recycle_units / aleppo_recycle_dormant, aleppo_shrink_perturb, the aleppo_ema_*
 *   and aleppo_snapshot_* calls never touch the anchor; aleppo_train only reads it.  aleppo_state_digest does not cover it:
 *   a checkpoint stores it with aleppo_anchor_export.  No call is a collective; under data parallelism every rank gives
 *   itself the same anchor.
 * Errors: an unknown source set, a NULL flat or a wrong count: ALEPPO_ERR_INVALID_ARGUMENT; a source set that does not
 *   exist yet, aleppo_anchor_export before any take or import, any call while a step is armed: ALEPPO_ERR_RUNTIME.  A failed
 *   call changes nothing. */
int aleppo_anchor_take(aleppo_ctx *ctx, int source_set);
int aleppo_anchor_import(aleppo_ctx *ctx, const float *flat, size_t count);
int aleppo_anchor_export(aleppo_ctx *ctx, float *flat, size_t count);

/* Shrink and perturb (Ash & Adams 2020), one shot, outside the update: every parameter is scaled and a fraction of a fresh
 * initialisation is added, in place on the device; every derived copy (the bf16 compute copy, the data-gradient layouts)
 * follows, as after aleppo_recycle_units.  Per element, lam = (float)shrink, sg = (float)sigma:
 *     p' = fl(fl(lam * p) + fl(sg * xi))             three fp32 operations, no fused multiply-add
 *   xi = the draw of aleppo_recycle_units at the same place: a_l * ((float)k * 0x1p-23f) with
 *     r = splitmix64(splitmix64(key) ^ (uint64)i), k = (int32)(r >> 40) - 8388608, i the element's index in the flat
 *     aleppo_export_params vector, a_l = (float)sqrt(6.0 / fan_in): fan_in = 256, 512, 576, 3136 for the conv1, conv2, conv3
 *     and fc weights, H for the action and the value weight rows.  xi = 0 for every bias: biases only shrink.
 *   Any host recomputes it bit for bit.  Alignment pads are not written.
 * flags: ALEPPO_SP_RESET_MOMENTS sets exp_avg and exp_avg_sq of every element to +0.0f; without it they are kept.  The Adam
 *   step count, the gradient, the averaged set, the snapshot and the anchor are never touched.
 * Afterwards aleppo_tensor_stats refuses ALEPPO_TS_SEC_STEP until the next aleppo_train and what aleppo_step pre-computed
 *   for the next aleppo_act is dropped, as after a recycle.  A captured update stays valid: no pointer changes.
 *   shrink = 1, sigma = 0 runs the pass and changes no bit.
 * It is deterministic in (key, i), so it is allowed under data parallelism: every rank passes the same arguments (the key
 *   must not contain the rank).  It runs on the context's stream, synchronises that stream only and is never a collective.
 * Errors: shrink not finite or outside [0, 1], sigma not finite, negative or beyond a float, unknown flag bits:
 *   ALEPPO_ERR_INVALID_ARGUMENT; a step is armed: ALEPPO_ERR_RUNTIME.  A failed call changes nothing. */
enum { ALEPPO_SP_RESET_MOMENTS = 1 }; /* flags */
int aleppo_shrink_perturb(aleppo_ctx *ctx, double shrink, double sigma, uint64_t key, int flags);

/* Exponentially averaged parameters (an EMA of the weights: torch.optim.swa_utils.AveragedModel / torch_ema, the "EWMA
 * policy" of Hilton, Cobbe and Schulman 2021; the reference has none): a second copy of the parameters on the device that
 * follows the live ones by e' = decay * e + (1 - decay) * p after every update the caller chooses, and that the
 * evaluation lanes can act on (ALEPPO_OPT_EVAL_PARAMS).  It stays out of aleppo_train entirely: the update's launch
 * sequence and a captured update (ALEPPO_OPT_UPDATE_GRAPH) are what they were, and the learner's state - parameters,
 * moments, step count, gradients, metrics, aleppo_state_digest - is bit-identical with and without these calls.
 * aleppo_ema_open allocates, on first use and never later, the averaged set in the private layout (fp32, and in bf16
 *   contexts its bf16 compute copy) and a small statistics block, then sets the average to the live parameters and
 *   updates = 0 by device copies on the context's stream.  Called again it re-initialises the same storage the same way
 *   (the average restarts) and allocates nothing.
 * aleppo_ema_update(decay): decay finite and 0 <= decay < 1.  With d = (float)decay and w = (float)(1.0 - decay) (the
 *   subtraction in double), each computed once on the host, every element of the padded vector becomes
 *     a = d * e;  b = w * p;  e' = a + b          three fp32 operations, each rounded, no fused multiply-add
 *   so the result is defined bit for bit: any host recomputes it from aleppo_export_params and the previous
 *   aleppo_ema_export, decay = 0 gives exactly p, and the alignment pads stay zero.  In bf16 contexts the same pass stores
 *   the compute copy (bf16)e', the conversion the live compute copy is made with.  updates is incremented.  One launch and
 *   one small finalising launch on the context's main stream; the call enqueues only and never waits for the host.
 * Statistics, accumulated in double by the same pass (one partial per workgroup, added in index order by the finalising
 *   launch: deterministic, no atomics), ALEPPO_EMA_STATS_COUNT doubles in device memory, read by aleppo_ema_read (which
 *   waits for the context's own stream only):
 *     ALEPPO_EMA_UPDATES            updates since the last open / load / import (the count given to an import)
 *     ALEPPO_EMA_DECAY              d of the last update, widened (0 before any update and after an import)
 *     ALEPPO_EMA_NORM               sqrt(sum e'^2)
 *     ALEPPO_EMA_PARAM_NORM         sqrt(sum p^2)
 *     ALEPPO_EMA_DISTANCE           sqrt(sum ((double)p - (double)e')^2)
 *     ALEPPO_EMA_RELATIVE_DISTANCE  sqrt(sum (p - e')^2 / sum p^2), 0 where sum p^2 = 0
 *   After open and before any update they are (0, 0, |P|, |P|, 0, 0).  The sums describe the sets as they stood when the
 *   last open / update / import was enqueued, not a later aleppo_train.
 * aleppo_ema_export / aleppo_ema_import move the averaged set in the order and with the count checks of
 *   aleppo_export_params / aleppo_load_params, plus the update count (import: updates >= 0); an import rebuilds the compute
 *   copy and the statistics block.  A checkpoint that stores what export returned and imports it resumes the average bit
 *   for bit.  aleppo_state_digest does not cover the average.
 * Interactions: aleppo_load_params on a context with the average open re-initialises it (average = the loaded parameters,
 *   updates 0), as it resets Adam.  aleppo_recycle_units / aleppo_recycle_dormant leave the average alone: the recycled
 *   weights enter it like any other change, and it converges to them at the rate of decay.  Under data parallelism the
 *   parameters are replicated bit for bit, so every rank that makes the same calls holds the same average: no call is a
 *   collective.  aleppo_forward, the saliency maps and the activation statistics always run on the live parameters.  A
 *   context that never calls aleppo_ema_open allocates and enqueues exactly what it did before.
 * Errors: update / read / export / import before aleppo_ema_open: ALEPPO_ERR_RUNTIME (nothing is allocated); a decay that
 *   is NaN, infinite, negative or >= 1, a NULL pointer, a wrong count, negative updates: ALEPPO_ERR_INVALID_ARGUMENT; a
 *   step is armed: ALEPPO_ERR_RUNTIME.  A failed call changes nothing. */
#define ALEPPO_EMA_STATS_COUNT 6
enum { ALEPPO_EMA_UPDATES = 0, ALEPPO_EMA_DECAY = 1, ALEPPO_EMA_NORM = 2, ALEPPO_EMA_PARAM_NORM = 3,
       ALEPPO_EMA_DISTANCE = 4, ALEPPO_EMA_RELATIVE_DISTANCE = 5 };
int aleppo_ema_open(aleppo_ctx *ctx);
int aleppo_ema_update(aleppo_ctx *ctx, double decay);
int aleppo_ema_read(aleppo_ctx *ctx, double out[ALEPPO_EMA_STATS_COUNT]);
int aleppo_ema_export(aleppo_ctx *ctx, float *flat, size_t count, int64_t *updates);
int aleppo_ema_import(aleppo_ctx *ctx, const float *flat, size_t count, int64_t updates);

/* Perturbation saliency maps of the policy and the value (Greydanus et al. 2018, "Visualizing and Understanding Atari
 * Agents"; the reference has none): blur the observation locally around each point of a grid, run the network on every
 * perturbed copy and score the point by how far the logits and the value move.  It needs only the forward pass the
 * context already has; the n * P perturbed stacks (28 KB each) are formed on the device and never cross PCIe.
 * Parameters (aleppo_saliency_config; a NULL pointer means the defaults): stride d in [2, 84], default 5; sigma_mask sM in
 *   [0.5, 16], default 5; sigma_blur sA in [0.5, 10], default 3; planes, a bit mask in [1, 15], default 15 - bit k is
 *   channel k of the NCHW observation, which is byte k of the packed stack.  Anything else (a NaN too):
 *   ALEPPO_ERR_INVALID_ARGUMENT.
 * Grid: G = ceil(84 / d) points per axis; point (gy, gx) has its centre at pixel (gy * d, gx * d); P = G * G; the
 *   position index is p = gy * G + gx.
 * Tables, built on the host in double by aleppo_saliency_tables (no context, no device); the engine uses exactly these:
 *   mask profile  g[k] = rint(4096 * exp(-k^2 / (2 sM^2))), k = 0 .. 83; g[0] = 4096
 *   blur taps     R = (int)(4 sA + 0.5); e_j = exp(-j^2 / (2 sA^2)); w[j] = rint(4096 * e_j / sum), sum = the e_j added in the
 *                 order j = -R .. R; then w[0] += 4096 - (sum of the w[j], j = -R .. R), so that the taps add up to 4096 exactly.
 *                 blur_w[j] holds w[j] for j = 0 .. R (w[-j] = w[j]) and is zero beyond R.
 * All pixel arithmetic is integer arithmetic, so the perturbed observations are defined bit for bit.
 * Blur B of one plane I (uint8, 84 x 84), separable, the horizontal pass first; an index outside [0, 83] is reflected,
 *   i < 0 -> -1 - i, i > 83 -> 167 - i (scipy's `reflect`):
 *   Hh[y][x] = sum_j w[j] * I[y][x + j]     V[y][x] = sum_j w[j] * Hh[y + j][x]     B = (V + 2^23) >> 24
 *   Everything fits unsigned 32 bits (V <= 255 * 2^24).  A constant plane blurs to itself.
 * Perturbed plane for the point with centre (cy, cx):
 *   m = (g[|y - cy|] * g[|x - cx|] + 2^15) >> 16, in [0, 256]       I' = (I * (256 - m) + B * m + 128) >> 8
 *   Where m = 0 the pixel is unchanged; a plane `planes` does not name is copied unchanged.
 * Scores: z, v are the logits and value of the unperturbed observation, z', v' those of the perturbed one, all from the
 *   context's own forward pass in its precision (fp32 outputs).  S_policy = 0.5 * sum_a (z_a - z'_a)^2, each difference,
 *   square and sum rounded to fp32, added in the order a = 0 .. A-1; S_value = 0.5 * (v - v')^2 likewise.  No softmax variant:
 *   Greydanus scores the logits, and `outputs` returns the raw numbers for any other metric.
 * Samples, as for aleppo_activation_stats: observations != NULL: the caller's host uint8 [n,4,84,84], first must be 0,
 *   1 <= n <= max(E, max_minibatch).  observations == NULL: samples [first, first + n) of THE BATCH THE CONTEXT HOLDS, in
 *   the env-major order n = e * T + t of aleppo_read_batch, read in place from the observation slots.
 * aleppo_saliency: policy and value are float [n][G][G]; outputs (may be NULL) is float [n][P + 1][A + 1]: row 0 the
 *   unperturbed logits and value, row 1 + p those of position p.  Per call: the forward pass and the head on the n samples,
 *   kept in a buffer of their own; then per chunk of at most max(E, max_minibatch) pairs i = sample * P + p (a chunk
 *   boundary may fall inside a sample's positions) one blur launch where the chunk touches a sample not blurred yet (the
 *   blur runs up to 128 samples ahead), one blend launch into a staging buffer, the forward pass, the head and one scoring
 *   launch (one thread per pair, a fixed order, no atomics).  Two calls with nothing in between return identical bits.
 * aleppo_saliency_perturbed: out is uint8 [n][position_count][4][84][84], the stacks the forward pass would see for the
 *   positions [position_first, position_first + position_count) of each sample - for tests, and to look at the perturbation.
 * Both run on the context's stream only, synchronise it where aleppo_activation_stats does, and are never a collective
 *   (they work under world_size > 1 and describe this rank's samples).  Staging is allocated on first use, grown on demand
 *   and kept until aleppo_destroy.  Like aleppo_forward they run the network in the shared activation scratch: what
 *   aleppo_step pre-computed for the next aleppo_act is dropped (the act recomputes it: same bits).  aleppo_train, a
 *   captured update (ALEPPO_OPT_UPDATE_GRAPH) and every other entry point enqueue nothing for them; a context that never
 *   calls them allocates and enqueues exactly what it did before, and calling them changes no bit of the run.
 * Errors: a parameter out of range, a NULL output, n or [first, first + n) or the positions out of range, first != 0 with
 *   observations: ALEPPO_ERR_INVALID_ARGUMENT.  The batch source without a batch, or any call while a step is armed:
 *   ALEPPO_ERR_RUNTIME.  A failed call writes nothing (the results pass through host temporaries). */
typedef struct {
  int32_t stride;
  int32_t planes;
  double sigma_mask;
  double sigma_blur;
} aleppo_saliency_config;
int aleppo_saliency_tables(const aleppo_saliency_config *cfg, uint16_t mask_g[84], uint16_t blur_w[84], int32_t *radius);
int aleppo_saliency(aleppo_ctx *ctx, const uint8_t *observations, int64_t first, int64_t n,
                    const aleppo_saliency_config *cfg, float *policy, float *value, float *outputs);
int aleppo_saliency_perturbed(aleppo_ctx *ctx, const uint8_t *observations, int64_t first, int64_t n,
                              const aleppo_saliency_config *cfg, int64_t position_first, int64_t position_count,
                              uint8_t *out);

/* Feature rank: the spectrum of the penultimate features from a Gram matrix formed on the device (Kumar et al. 2021,
 * "Implicit Under-Parameterization"; Lyle et al. 2022, "Understanding and Preventing Capacity Loss"; Moalla et al. 2024,
 * whose feature-rank collapse precedes PPO's; the reference has none).  Phi is the fc output [rows, H] as stored: fp32 on
 * both precisions, bias included, no ReLU - what aleppo_forward_activations exports as fc.  Neither an observation of the
 * batch nor a feature leaves the device: only G = Phi^T Phi (H x H doubles) and the H column sums do.
 * Samples: exactly those of aleppo_activation_stats.  observations == NULL and n == 0: the batch the context holds,
 *   masked samples included, read in place in logical order in forward chunks of at most maxB = max(E, max_minibatch);
 *   otherwise the caller's n <= maxB observations.  Never a collective: under data parallelism it describes this rank's
 *   samples.
 * On the device: a row with any non-finite feature is counted (NONFINITE_ROWS) and left out; it contributes nothing to
 *   G, to the column sums or to n.  Over the n rows that remain
 *     G[i][j] = sum_r (double)Phi[r][i] * (double)Phi[r][j]        s[i] = sum_r (double)Phi[r][i]
 *   A product of two widened fp32 values is exact in double, so only the order of the additions matters, and that order
 *   is a function of (row count, maxB, H) only:
 *     - per forward chunk of ns rows: S = min(16, ceil(ns / 256)) row splits of R = 4 * ceil(ceil(ns / S) / 4) rows each
 *       (the last may be shorter);
 *     - inside a split the rows enter four at a time, in row order, through v_mfma_f64_16x16x4_f64 (D = A B + C: the four
 *       products of one instruction are added to the accumulator by the hardware in its fixed order); a left-out row
 *       and a row past the split's end enter as zeros and are never read.  s: thread q of four adds rows q, q + 4, ...
 *       of the split in order, then the four are added as ((0 + 1) + 2) + 3;
 *     - a reduce launch adds the S partial results of the chunk in split order, t = ((p0 + p1) + p2) + ..., and carries
 *       the total across the forward chunks in chunk order: G = t for the first chunk, G = G + t for every later one.
 *   Only 64 x 64 blocks with i-block <= j-block are computed (and of a diagonal block only the 32 x 32 quarters on or
 *   above the diagonal); every G[i][j] with i > j is a copy of G[j][i]: the same bits.  No floating-point atomics; the
 *   grid does not depend on the device.  Two calls with nothing in between are bit-identical, and with at most maxB
 *   samples the batch source equals the caller source on the same observations, bit for bit.
 * On the host, inside the library (plain C++ in double, single-threaded, no LAPACK; csrc/feature_rank_host.hpp):
 *   centered != 0: Gc[i][j] = G[i][j] - (s[i] * s[j]) / n, in this order of operations - PCA of the features.  The
 *   eigenvalues lambda_1 >= ... >= lambda_H of G (or Gc) come from Householder tridiagonalisation and implicit-shift QL
 *   (values only), on the matrix scaled by an exact power of two; deterministic.  sigma_i = sqrt(max(lambda_i, 0)) are the
 *   singular values of Phi (of the centred Phi).  With S1 = sum sigma_i and S2 = sum sigma_i * sigma_i, both in index
 *   order, the stats are those of aleppo_feature_rank_stat.  With n == 0 or S1 == 0 every rank is 0 and every other stat
 *   but ROWS and NONFINITE_ROWS is 0.
 * Accuracy: the Gram route squares the condition number - an eigenvalue carries an absolute error of about
 *   H * 2^-53 * lambda_1, so singular values below about sqrt(H * 2^-53) * sigma_1 (2.4e-7 sigma_1 at H = 512) are rounding
 *   noise.  That is below the 2^-24 relative precision fp32 features carry, and far below every threshold above.
 * cfg: NULL means delta = 0.01, eps = 0.01, centered = 0.  stats: double [ALEPPO_FR_COUNT].  sigma: NULL or double [H],
 *   descending.  gram: NULL or double [H * H], row-major, the full symmetric matrix G (never Gc).  colsum: NULL or double
 *   [H], s.
 * Computed WHEN CALLED, on the context's stream: the stream's synchronise; per forward chunk the forward pass, one launch
 *   that flags the non-finite rows, one Gram launch and one reduce launch; one copy of G and s; the host solve.  Like
 *   aleppo_forward it runs the network in the shared activation scratch, so what aleppo_step pre-computed for the next
 *   aleppo_act is dropped (the act recomputes it: same bits).  Scratch (20.1 MB at H = 512, 0.6 MB at H = 32) is allocated on first use and kept
 *   until aleppo_destroy.  aleppo_train, a captured update (ALEPPO_OPT_UPDATE_GRAPH) and every other entry point enqueue
 *   nothing for it; a context that never calls it allocates and enqueues exactly what it did before, and calling it
 *   changes no bit of the run.
 * Errors: a NULL stats or stat_count != ALEPPO_FR_COUNT, a non-NULL output with a wrong count, delta not in (0, 1), eps
 *   negative or not finite, centered not 0 or 1, reserved != 0, and what aleppo_activation_stats refuses in observations and
 *   n: ALEPPO_ERR_INVALID_ARGUMENT.  The batch source without a batch, or any call while a step is armed:
 *   ALEPPO_ERR_RUNTIME.  A failed call writes nothing. */
typedef struct {
  float delta;      /* the share of the spectrum SRANK and PCA_RANK may leave out, in (0, 1) */
  float eps;        /* THRESHOLD_RANK's threshold on sigma_i / sqrt(n), finite and >= 0 */
  int32_t centered; /* 0: the spectrum of G; 1: of Gc */
  int32_t reserved; /* must be 0 */
} aleppo_feature_rank_config; /* 16 bytes */
typedef enum {
  ALEPPO_FR_ROWS = 0,           /* n: the rows that entered */
  ALEPPO_FR_NONFINITE_ROWS = 1, /* rows left out */
  ALEPPO_FR_SIGMA_MAX = 2,      /* sigma_1 */
  ALEPPO_FR_SIGMA_MIN = 3,      /* sigma_H */
  ALEPPO_FR_MEAN_SQ_NORM = 4,   /* (sum of G's diagonal, in index order) / n: the mean squared feature norm (Moalla et al.) */
  ALEPPO_FR_EFFECTIVE_RANK = 5, /* exp(-sum p_i ln p_i), p_i = sigma_i / S1, 0 ln 0 = 0 (Roy & Vetterli 2007) */
  ALEPPO_FR_SRANK = 6,          /* smallest k with sum_{i<=k} sigma_i >= (1 - delta) S1 (Kumar et al. 2021) */
  ALEPPO_FR_PCA_RANK = 7,       /* smallest k with sum_{i<=k} sigma_i^2 >= (1 - delta) S2 (Yang et al. 2020) */
  ALEPPO_FR_THRESHOLD_RANK = 8, /* #{i : sigma_i / sqrt(n) > eps} (Lyle et al. 2022) */
  ALEPPO_FR_STABLE_RANK = 9,    /* S2 / sigma_1^2 */
  ALEPPO_FR_NUMERICAL_RANK = 10 /* #{i : sigma_i > max(n, H) * 2^-23 * sigma_1} (numpy.linalg.matrix_rank on float32) */
} aleppo_feature_rank_stat;
#define ALEPPO_FR_COUNT 11
int aleppo_feature_rank(aleppo_ctx *ctx, const uint8_t *observations, int64_t n, const aleppo_feature_rank_config *cfg,
                        double *stats, size_t stat_count, double *sigma, size_t sigma_count, double *gram,
                        size_t gram_count, double *colsum, size_t colsum_count);

/* Policy churn: how far one parameter set's policy, value and fc features are from another's on the same states
 * (Schaul et al. 2022, "The Phenomenon of Policy Churn": the share of states whose greedy action an update changes;
 * Sokar et al. 2023 claim a recycle moves the outputs by almost nothing; Hilton, Cobbe & Schulman 2021 reason about the
 * distance of the averaged policy from the live one; the reference has none of it).  Both forward passes and the
 * comparison run on the device; only the ALEPPO_PD_COUNT doubles - and what the caller asks for - leave it.
 * Parameter sets: ALEPPO_SET_LIVE, the parameters aleppo_train updates; ALEPPO_SET_AVERAGED, the set of aleppo_ema_open;
 *   ALEPPO_SET_SNAPSHOT, a third set only the three calls below write.  It lives in the private layout like the averaged set
 *   (fp32, and in bf16 contexts its bf16 compute copy), is allocated on the first take or import and never again.
 * aleppo_snapshot_take(source_set): snapshot = the live or the averaged set, two device-to-device copies on the context's
 *   main stream, so the compute copy is the source's bit for bit; the call enqueues only.
 * aleppo_snapshot_import / aleppo_snapshot_export move the snapshot in the order and with the count checks of
 *   aleppo_load_params / aleppo_export_params (an import rebuilds the compute copy with the conversion the live one is
 *   made with): a checkpoint from disk can be compared with the running policy.
 * Interactions: aleppo_load_params, aleppo_train, aleppo_recycle_units / aleppo_recycle_dormant and the aleppo_ema_* calls
 *   never touch the snapshot - that is the point of it.  aleppo_state_digest does not cover it.  No call is a collective.
 *   While a step is armed every call is refused.  A failed call changes nothing.
 * aleppo_policy_diff(set_a, set_b): samples exactly as for aleppo_feature_rank - observations == NULL and n == 0: the
 *   batch the context holds, in forward chunks of at most maxB = max(E, max_minibatch); otherwise the caller's n <= maxB
 *   observations.  Per chunk: the forward pass and the heads on set a (the forward pass of aleppo_forward, reading that
 *   set), one device copy that keeps its fc rows, the forward pass and the heads on set b, then the comparison launch and
 *   a small finalising launch.  set_a == set_b is allowed.
 * Per row, all in double, from the fp32 logits l, value v and fc row h of each set, widened:
 *     m = max l;  z = l - m;  lse = log(sum exp z);  logp = z - lse;  p = exp(logp)
 *     g = the lowest index of the maximum of l (the ALEPPO_EVAL_GREEDY rule)
 *   A row in which any logit, value or fc element of either set is not finite is counted (NONFINITE_ROWS) and left out of
 *   everything else.  per_sample: double [rows][ALEPPO_PD_ROW], a left-out row all NaN -
 *     0 kl_ab = sum p_a (logp_a - logp_b)     1 kl_ba = sum p_b (logp_b - logp_a)     2 tv = 0.5 sum |p_a - p_b|
 *     3 dv = v_b - v_a     4 cos = <h_a,h_b> / sqrt(|h_a|^2 |h_b|^2), 1 where either norm is 0     5 dh2 = |h_b - h_a|^2
 *     6 g_a     7 g_b
 * stats: double [ALEPPO_PD_COUNT], aleppo_policy_diff_stat; a mean is the sum over the rows that entered divided by ROWS.
 *   With ROWS == 0 every stat but ROWS and NONFINITE_ROWS is 0.
 * transitions: NULL or int64 [A][A], [i][j] = the rows with g_a = i and g_b = j.  outputs: NULL or float [2][rows][A + 1],
 *   the logits then the value of every row, set a's block first - left-out rows included, as computed.
 * Order: one wave per row adds the H products across its lanes in a fixed tree; the sums go to one double record per
 *   workgroup (the grid is a function of the chunk's row count alone), a finalising launch adds the records in index order
 *   and the chunks are accumulated in order; extrema are order-free and the transition counts are integer adds.  No
 *   floating-point atomics: two calls on the same state return the same bits.
 * Computed WHEN CALLED, on the context's stream, like aleppo_feature_rank: the stream's synchronise, the launches above,
 *   one copy of the results.  It runs the network in the shared activation scratch, so what aleppo_step pre-computed for
 *   the next aleppo_act is dropped (the act recomputes it: same bits).  Scratch (set a's fc rows of one chunk, the logits,
 *   values and per-sample table of max(E * horizon, maxB) rows) is allocated on first use and kept until aleppo_destroy.
 *   It only reads the parameter sets: aleppo_train, a captured update (ALEPPO_OPT_UPDATE_GRAPH) and every other entry point
 *   enqueue nothing for it; a context that never calls it allocates and enqueues exactly what it did before, and calling
 *   it changes no bit of the run.
 * Errors: a set that is none of the three, ALEPPO_SET_SNAPSHOT as the source of a take, a NULL stats or flat, a wrong
 *   count (stat_count != ALEPPO_PD_COUNT, a non-NULL output whose count is not rows * ALEPPO_PD_ROW, A * A,
 *   2 * rows * (A + 1)), and what aleppo_activation_stats refuses in observations and n: ALEPPO_ERR_INVALID_ARGUMENT.
 *   ALEPPO_SET_AVERAGED before aleppo_ema_open, ALEPPO_SET_SNAPSHOT (and aleppo_snapshot_export) before any take or import,
 *   the batch source without a batch, any call while a step is armed: ALEPPO_ERR_RUNTIME.  A failed call writes nothing. */
enum { ALEPPO_SET_LIVE = 0, ALEPPO_SET_AVERAGED = 1, ALEPPO_SET_SNAPSHOT = 2 };
typedef enum {
  ALEPPO_PD_ROWS = 0,               /* the rows that entered */
  ALEPPO_PD_NONFINITE_ROWS = 1,     /* rows left out */
  ALEPPO_PD_CHURN = 2,              /* the share of rows with g_a != g_b */
  ALEPPO_PD_MEAN_KL_AB = 3,
  ALEPPO_PD_MAX_KL_AB = 4,
  ALEPPO_PD_MEAN_KL_BA = 5,
  ALEPPO_PD_MEAN_TV = 6,
  ALEPPO_PD_MAX_TV = 7,
  ALEPPO_PD_MEAN_ABS_DV = 8,
  ALEPPO_PD_MAX_ABS_DV = 9,
  ALEPPO_PD_RMS_DV = 10,            /* sqrt(mean dv^2) */
  ALEPPO_PD_MEAN_ENTROPY_A = 11,    /* mean of -sum p_a logp_a */
  ALEPPO_PD_MEAN_ENTROPY_B = 12,
  ALEPPO_PD_MEAN_FEATURE_COS = 13,
  ALEPPO_PD_MIN_FEATURE_COS = 14,
  ALEPPO_PD_FEATURE_REL_CHANGE = 15 /* sqrt(sum dh2 / sum |h_a|^2), 0 where the denominator is 0 */
} aleppo_policy_diff_stat;
#define ALEPPO_PD_COUNT 16
#define ALEPPO_PD_ROW 8
int aleppo_snapshot_take(aleppo_ctx *ctx, int source_set);
int aleppo_snapshot_export(aleppo_ctx *ctx, float *flat, size_t count);
int aleppo_snapshot_import(aleppo_ctx *ctx, const float *flat, size_t count);
int aleppo_policy_diff(aleppo_ctx *ctx, const uint8_t *observations, int64_t n, int set_a, int set_b, double *stats,
                       size_t stat_count, double *per_sample, size_t per_sample_count, int64_t *transitions,
                       size_t transition_count, float *outputs, size_t output_count);

/* Gradient probes: the gradient as a DIRECTION, on the device.  aleppo_tensor_stats gives the norm of the last minibatch's
 * gradient; these calls compute the gradient of any slice of the batch the context holds WITHOUT an optimizer step, keep a
 * few of them next to G, and reduce their inner products per tensor.  What they answer: the gradient noise scale
 * (McCandlish et al. 2018, "An Empirical Model of Large-Batch Training", B_simple from the norms at two batch sizes);
 * whether the critic fights the actor in the shared trunk (the per-tensor cosine of the policy term's and the value term's
 * gradient - the motivation of Phasic Policy Gradient, Cobbe et al. 2021); how much minibatches interfere (Lyle et al.
 * 2023); whether Adam's momentum still points where a fresh gradient points.  The reference has none of it; the route
 * without these calls is aleppo_train(lr = 0), which still advances Adam's moments and step count and overwrites the
 * per-sample metric planes, then aleppo_export_grads over PCIe, per question - and it cannot separate the loss terms.
 * Slots: ALEPPO_GRAD_SLOTS vectors in the private padded layout of G (fp32, zero-filled, pads stay zero), allocated
 *   together through the context's memory registry by the first call that writes one and kept until aleppo_destroy.
 *   aleppo_state_digest does not cover them, no checkpoint holds them, aleppo_train never reads them.
 * aleppo_grad_probe(slot, first, n, cfg, unmasked_out): slot = the gradient the optimizer step of aleppo_train would have
 *   been given for the minibatch of samples [first, first + n) of the batch, in logical (env-major, contiguous) order, at
 *   the live parameters; no clip, no Adam.  1 <= n <= maxB = max(E, max_minibatch).
 *   cfg: NULL = { 1, the current ALEPPO_OPT_VALUE_LOSS_COEF, the current ALEPPO_OPT_ENTROPY_COEF, 0 }; policy_term 0 or
 *     1, the two coefficients finite and >= 0, reserved 0.  Everything else is as aleppo_train would do it for a
 *     contiguous minibatch of n samples: the clip range and the value-clip range, ALEPPO_OPT_VALUE_CLIP (with the rollout
 *     batch's value transpose), ALEPPO_OPT_ADV_NORM_MINIBATCH with the statistics of THIS slice, ALEPPO_OPT_KL_PENALTY
 *     with the current beta, the masked mean over this slice's unmasked count, the kernel routes a minibatch of n
 *     samples takes (fused forward; the fused or split backward tail by the ALEPPO_OPT_FUSED_BWD rule; the pipelined or
 *     small-tile fc; the two streams), the same slab reduction with conv1's slabs summed as the norm pass sums them.
 *     ALEPPO_OPT_MINIBATCH_SHUFFLE is not consulted: a probe names its samples itself.
 *   The head: with policy_term = 1 the entry point and arguments of aleppo_train; with policy_term = 0 the
 *     advantage-record entry point with a private record (mean_f, inv_f) = (+0.0f, +0.0f), so every advantage is a * 0 and
 *     the policy term's gradient is exactly zero - no kernel knows about probes.  The head reads a private hyper block
 *     (clip ranges from the context, c_v / c_e from cfg) and writes its per-sample planes to private scratch.  With
 *     (n = N / M, first = mb * n) and cfg = NULL the slot is bit for bit the G that aleppo_train(M) leaves for minibatch mb.
 *   Linear combinations: in exact arithmetic g(1, c_v, c_e) = g_pi + c_v g_v + c_e g_e with the three pure probes
 *     g_pi = g(1, 0, 0), g_v = g(0, 1, 0), g_e = g(0, 0, 1), and the Gram is bilinear: a host forms the inner product of
 *     ANY two combinations from the 3 x 3 Gram of the pure probes.  That is why there is no per-term slot arithmetic on
 *     the device.  (In fp32 / bf16 the identity holds to rounding, not bit for bit.)
 *   Afterwards aleppo_export_grads, aleppo_tensor_stats, aleppo_read_train_metric, aleppo_state_digest, the parameters,
 *     both moments and the step count are bit for bit what they were; a captured update (ALEPPO_OPT_UPDATE_GRAPH) replays
 *     without a re-capture; the next aleppo_train gives the bits of a context that never probed.  It does run the network
 *     in the shared activation scratch: like aleppo_policy_diff it drops what aleppo_step pre-computed, and
 *     aleppo_export_backward / aleppo_export_acting refuse afterwards.
 *   Data parallelism: NEVER a collective.  The slot is THIS rank's slice with THIS rank's unmasked count (and this rank's
 *     advantage statistics), unlike aleppo_train's all-reduced G: ranks may probe different slices, or only one may probe.
 *   Computed WHEN CALLED: the stream's synchronise, the launches, one synchronise.  *unmasked_out (NULL: not wanted)
 *     receives the slice's unmasked count.
 * aleppo_grad_take(slot, source, set): ALEPPO_GRAD_SRC_EXP_AVG - the slot becomes Adam's first moment as it stands (set
 *   must be 0); ALEPPO_GRAD_SRC_PARAM_DELTA - the slot becomes fl(p_live - p_set), one fp32 subtraction per element that
 *   a host recomputes bit for bit from the two exports, set = ALEPPO_SET_AVERAGED or ALEPPO_SET_SNAPSHOT.  Enqueues only.
 * aleppo_grad_export / aleppo_grad_import move a slot in the order and with the count checks of aleppo_export_params /
 *   aleppo_load_params: a stored direction (a checkpointed gradient, another run's update) becomes comparable.
 * aleppo_grad_gram(slots, k): slots names 1 <= k <= ALEPPO_GRAD_SLOTS written slots x_0 .. x_{k-1}, repeats allowed.
 *   gram: double [ALEPPO_TENSOR_STATS_ROWS][k][k], the rows of aleppo_tensor_stats (the 12 tensors in libtorch
 *   parameters() order, then the whole model); [r][i][j] = the sum over the elements e of tensor r of
 *   (double)x_i[e] * (double)x_j[e].  The products are exact in double; the additions are in an order that is a function
 *   of (H, A, k) only - aleppo_tensor_stats' chunks, thread order and fixed tree, the chunks in index order, row 12 the
 *   twelve rows in row order - so two calls return the same bits, and [r][i][j] and [r][j][i] are the same bits.  An
 *   element index at which ANY of the k named slots is NaN / Inf is left out of every entry and counted once in
 *   nonfinite[r] (NULL, or int64 [ALEPPO_TENSOR_STATS_ROWS], row 12 the total).  No atomics; it only reads the slots.
 *   Under aleppo_profile_enable its two launches are one bracket of class ALEPPO_K_ACT_STATS (the class the read-only
 *   diagnostic passes share); a probe's launches fall into the update's classes, as aleppo_train's do.
 * Errors: a slot outside [0, ALEPPO_GRAD_SLOTS), n < 1, n > maxB, first < 0, first + n past the batch, bad cfg values, a
 *   source or set the call does not take, a NULL or a wrong count: ALEPPO_ERR_INVALID_ARGUMENT.  No batch, a caller batch
 *   without values under ALEPPO_OPT_VALUE_CLIP, a set that does not exist yet, exporting or naming in a Gram a slot that
 *   nothing has written, any call while a step is armed: ALEPPO_ERR_RUNTIME.  A failed call changes nothing. */
#define ALEPPO_GRAD_SLOTS 4
enum { ALEPPO_GRAD_SRC_EXP_AVG = 0, ALEPPO_GRAD_SRC_PARAM_DELTA = 1 };
typedef struct {
  int32_t policy_term;   /* 1: the policy term is part of the loss; 0: it is switched off exactly */
  float value_loss_coef; /* c_v, finite and >= 0 */
  float entropy_coef;    /* c_e, finite and >= 0 */
  int32_t reserved;      /* 0 */
} aleppo_grad_probe_config;
int aleppo_grad_probe(aleppo_ctx *ctx, int slot, int64_t first, int64_t n, const aleppo_grad_probe_config *cfg,
                      int64_t *unmasked_out);
int aleppo_grad_take(aleppo_ctx *ctx, int slot, int source, int set);
int aleppo_grad_export(aleppo_ctx *ctx, int slot, float *flat, size_t count);
int aleppo_grad_import(aleppo_ctx *ctx, int slot, const float *flat, size_t count);
int aleppo_grad_gram(aleppo_ctx *ctx, const int32_t *slots, int k, double *gram, size_t gram_count, int64_t *nonfinite,
                     size_t nonfinite_count);

/* Per-epoch advantage recomputation (Andrychowicz et al. 2021, "What Matters in On-Policy RL", choice C.5: recompute the
 * advantages before every pass over the data; what a CleanRL / SB3 user writes as "re-run compute_gae inside the epoch
 * loop"; the reference has none of it).  After the first epoch of an update the critic has moved, so the advantages and
 * returns aleppo_finish_rollout left are stale.  aleppo_refresh_advantages is a call BETWEEN two aleppo_train calls on one
 * rollout batch: it forwards the batch on the device, scans again and overwrites the two planes; aleppo_train, its
 * schedules and a captured update (ALEPPO_OPT_UPDATE_GRAPH) are what they were and simply read the new planes.
 * Valid when the context holds a ROLLOUT batch: aleppo_finish_rollout has succeeded, and neither an aleppo_set_batch nor
 *   the first aleppo_act / aleppo_step / aleppo_env_rollout of the next rollout has come since (that act carries the
 *   post-rollout observation into slot 0 and the time axis is gone).  A caller batch has no time axis and is refused.
 * Fresh values: for every sample (e, t) of the batch, and for the post-rollout observation of every environment (the bytes
 *   of ALEPPO_F_CURRENT_OBS), the value head's output under `set` (ALEPPO_SET_LIVE / _AVERAGED / _SNAPSHOT) - the forward
 *   pass of aleppo_forward over the observation slots in place, in chunks of at most maxB = max(E, max_minibatch) samples
 *   in logical order, then the E post-rollout observations as one chunk.  The fp32 value is bit for bit what
 *   aleppo_forward returns for those observations in the same chunks (one wave per row sums the H products lane-strided,
 *   then the fixed butterfly, then + bias, as the forward-only head does).  Each is rounded to the rollout plane type (IEEE
 *   half under ALEPPO_ROLLOUT_FP16) and stored in a SECOND plane [T+1][E], allocated on first use and kept until
 *   aleppo_destroy.  The collected plane is not written: ALEPPO_F_VALUES, ALEPPO_F_NEXT_VALUES, the v of
 *   ALEPPO_F_BATCH_STATS and the v_old of ALEPPO_OPT_VALUE_CLIP keep meaning "as collected".
 * Advantages and returns: the GAE scan of aleppo_finish_rollout (the same kernel) on the stored rewards AS THEY STAND -
 *   already clamped, or scaled and clipped by ALEPPO_OPT_REWARD_SCALE, in place; they are not transformed again and the
 *   reward-scale state is neither read nor written - the stored flags, config.gamma / lambda and the fresh plane.  It
 *   overwrites ALEPPO_F_ADVANTAGES and ALEPPO_F_RETURNS (= a + v_fresh) and rewrites the same ALEPPO_F_MASKS.  With
 *   config.advantage_norm = 1 the normalisation of aleppo_finish_rollout follows, with its all-reduce under a communicator
 *   (world_size > 1, or ALEPPO_OPT_FORCE_COMM): the call is then a COLLECTIVE like aleppo_finish_rollout, and never one
 *   otherwise.  Old log-probs, actions, logits, rewards, observations, the frame stacks, the sampling counter, parameters
 *   and moments are untouched; aleppo_state_digest is the same before and after.
 * stats: NULL (stat_count 0) or double [ALEPPO_REFRESH_STATS_COUNT], THIS RANK's samples, never all-reduced, computed
 *   before the scan overwrites anything, in double over the unmasked samples with ALEPPO_F_BATCH_STATS's arithmetic and
 *   order (chunks of 4096 logical samples, 256 strided accumulators, a fixed tree, chunks in index order):
 *     [0..9]  the aleppo_batch_stat layout with v := the fresh values as stored, and R and a := the returns and
 *             advantages AS THEY STOOD AT ENTRY: how well the updated critic explains the targets the last epoch trained on
 *     [10]    mean of d' = v_fresh - v_collected      [11] population std of d'      [12] max |d'| (exact)
 * aleppo_refresh_read: the fresh plane in reference layout, float [E,T] and float [E] (either pointer may be NULL with a
 *   count of 0, not both).  A function and not two more aleppo_field values: a field is readable straight after
 *   aleppo_finish_rollout, this plane only once the batch the context holds has been refreshed.
 * Computed WHEN CALLED, on the context's stream: the stream's synchronise, the forward chunks (their own profiling
 *   classes) each followed by the value launch, the statistics' two launches (ALEPPO_K_ACT_STATS, the class
 *   of the read-only passes over the activations: one bracket per chunk), the scan (ALEPPO_K_GAE),
 *   the normalisation, one synchronise.  It runs the network in the shared activation scratch: what aleppo_step
 *   pre-computed for the next aleppo_act is dropped (the act recomputes it: same bits) and aleppo_export_backward refuses
 *   afterwards.  A context that never makes the calls allocates and enqueues exactly what it did before.
 * Errors: a set that is none of the three, a stat_count that is neither 0 with NULL nor ALEPPO_REFRESH_STATS_COUNT, wrong
 *   counts or two NULLs in aleppo_refresh_read: ALEPPO_ERR_INVALID_ARGUMENT.  No rollout batch (none yet, a caller batch,
 *   a rollout whose flags aleppo_finish_rollout refused, the next rollout begun), a set that does not exist yet, a step
 *   armed, world_size > 1 without aleppo_comm_init, aleppo_refresh_read before the batch the context holds was refreshed:
 *   ALEPPO_ERR_RUNTIME.  A failed call changes nothing. */
#define ALEPPO_REFRESH_STATS_COUNT 13
typedef enum {
  ALEPPO_REFRESH_VALUE_CHANGE_MEAN = 10,  /* [0..9]: aleppo_batch_stat */
  ALEPPO_REFRESH_VALUE_CHANGE_STD = 11,
  ALEPPO_REFRESH_VALUE_CHANGE_MAXABS = 12
} aleppo_refresh_stat;
int aleppo_refresh_advantages(aleppo_ctx *ctx, int set, double *stats, size_t stat_count); /* stats may be NULL (count 0) */
int aleppo_refresh_read(aleppo_ctx *ctx, float *values, size_t value_count, float *next_values, size_t next_count);

/* ------------------------------------------------------------------ evaluation lanes (the reference has no evaluation
 * loop: SB3's predict(deterministic=True) / EvalCallback, the epsilon-greedy scores of the DQN / PPO papers)
 * L frame stacks of their own, next to the rollout, on which the network acts under one of three rules - so that a
 * trained (or half-trained) agent can be scored on OTHER emulator instances without touching the batch being collected.
 * Per evaluation step the caller does  eval_act -> (step its L evaluation emulators) -> eval_push_frames; returns and
 * episode lengths are the caller's bookkeeping, as they are for training.
 * Isolation: the four calls change nothing the rollout or the update can observe - not the rollout's stacks and planes,
 * t, the acting generator's counter, the pre-computed acting scratch of aleppo_step, aleppo_act's pinned buffer and
 * ticket, Adam state, metrics or a captured update.  A training run with evaluation calls inserted at any point where no
 * step is armed (between an aleppo_step and the aleppo_act that follows it included) is bit-identical to the run without
 * them.  While a step is armed all four fail with ALEPPO_ERR_RUNTIME like every other stateful entry point; before
 * aleppo_eval_open the other three are ALEPPO_ERR_RUNTIME.  The lanes are local to a rank: nothing is exchanged under
 * data parallelism and no call is a collective. */
typedef enum { ALEPPO_EVAL_GREEDY = 0, ALEPPO_EVAL_SAMPLE = 1, ALEPPO_EVAL_EPSILON_GREEDY = 2 } aleppo_eval_rule;
typedef enum {
  ALEPPO_EF_OBSERVATIONS = 0, /* uint8 [L,4,84,84] the lanes' stacks right now */
  ALEPPO_EF_LOGITS = 1,       /* float [L,A] of the last aleppo_eval_act (always fp32, whatever rollout_precision is) */
  ALEPPO_EF_VALUES = 2,       /* float [L] */
  ALEPPO_EF_ACTIONS = 3       /* int64 [L] */
} aleppo_eval_field;
/* Allocates, in this call and never later, everything the lanes need: the packed stacks (zeroed), the pinned action
 * buffer, upload staging for frames / start flags / noise, and the lanes' OWN acting scratch (the conv3 output and the
 * split-K fc partials; the conv1 / conv2 outputs too where the context's acting convolutions are separate launches: fp32,
 * or ALEPPO_OPT_GENERIC_CONV set BEFORE this call - a bf16 context that switches to the generic convolutions afterwards
 * gets ALEPPO_ERR_RUNTIME from aleppo_eval_act).  1 <= num_lanes <= 4096 (ALEPPO_ERR_INVALID_ARGUMENT otherwise).
 * Called again with the same num_lanes it zeroes the stacks, restarts the evaluation counter at 0 and forgets the last
 * aleppo_eval_act; with another num_lanes it is ALEPPO_ERR_RUNTIME.  Nothing is freed before aleppo_destroy. */
int aleppo_eval_open(aleppo_ctx *ctx, int32_t num_lanes);
/* aleppo_push_frames for the L lanes: same arguments and meaning (both frame kinds, all three locations, the gray LUT of
 * aleppo_set_gray_lut), through the same ingest kernel, in place on the evaluation stacks.  A lane whose episode_start
 * flag is set gets its new frame in all four positions. */
int aleppo_eval_push_frames(aleppo_ctx *ctx, const uint8_t *frames, int frame_kind, int location,
                            const uint8_t *episode_start);
/* Eval forward on the lanes' stacks with the parameters as they stand (after the last aleppo_train / aleppo_load_params) -
 * or, under ALEPPO_OPT_EVAL_PARAMS = 1, with the averaged parameters of aleppo_ema_open as they stand, which is then what
 * aleppo_eval_read returns and what an ALEPPO_REC_EVAL recorder records:
 * aleppo_act's acting kernels, then the evaluation head.  With z the fp32 logits:
 *   ALEPPO_EVAL_GREEDY          the lowest index of the maximum of z.  param must be 0 and noise NULL; nothing is drawn.
 *   ALEPPO_EVAL_SAMPLE          param = the temperature tau, finite and > 0 (and 1 / tau finite in fp32).  With inv = 1 / tau
 *                               computed once in fp32: e_k = expf((z_k - max z) * inv), p_k = e_k / sum e, action =
 *                               argmax_k p_k / q_k, first maximum wins.  noise: float [L,A] of Exp(1) draws q, or NULL.
 *                               At tau = 1 the multiplication is exact and the rule is aleppo_act's, instruction for
 *                               instruction.
 *   ALEPPO_EVAL_EPSILON_GREEDY  param = epsilon in [0, 1].  noise: float [L,2] of uniforms (u, w) in [0, 1), or NULL.  A
 *                               lane explores iff u < epsilon; its action is then min((int)(w * A), A - 1), w * A rounded
 *                               once in fp32; otherwise the greedy action.
 * Anything else (an unknown rule, a NaN / Inf / out-of-range param, noise given to GREEDY) is
 * ALEPPO_ERR_INVALID_ARGUMENT, and such a call changes nothing.
 * Built-in generator (noise == NULL): Philox4x32-10, the block function of aleppo_act's generator, under the key
 *   K = config.seed ^ 0x4556414C4C414E45 ("EVALLANE"; key words K lo, K hi) - another stream than aleppo_act's, whose key
 *   is config.seed.  n = the evaluation counter: 0 at aleppo_eval_open, + 1 per successful aleppo_eval_act whatever the
 *   rule (GREEDY included).  Counter words { n lo, n hi, lane, block }, output words c[0..3]:
 *     SAMPLE          block = k / 4, q_k = -logf(U(c[k % 4]))
 *     EPSILON_GREEDY  block = 0, u = U(c[0]), w = U(c[1])
 *   with U(x) = ((x >> 8) + 0.5) / 2^24 in fp32, as aleppo_act draws its uniforms.
 * *actions_pinned (may be NULL): int64 [L] in page-locked host memory owned by ctx - a buffer of its own, not aleppo_act's -
 * valid when the call returns and until the next aleppo_eval_act. */
int aleppo_eval_act(aleppo_ctx *ctx, int rule, float param, const float *noise, const int64_t **actions_pinned);
/* Read an aleppo_eval_field; synchronises the context's stream like aleppo_read_batch.  A wrong byte count is
 * ALEPPO_ERR_INVALID_ARGUMENT; fields 1-3 before the first aleppo_eval_act (since aleppo_eval_open) are
 * ALEPPO_ERR_RUNTIME. */
int aleppo_eval_read(aleppo_ctx *ctx, int field, void *dst, size_t bytes);
/* Sets the evaluation counter n of the built-in generator (what aleppo_eval_open sets to 0 and every aleppo_eval_act
 * advances by one) and nothing else: the next act draws block n.  For a caller that evaluates in chunks
 * (aleppo_eval_env_run) and wants its NEXT evaluation to draw what a step-by-step caller, which stops at the step its last
 * episode ends in, would draw.  ALEPPO_ERR_RUNTIME before aleppo_eval_open and while a step is armed. */
int aleppo_eval_set_counter(aleppo_ctx *ctx, uint64_t counter);

/* ------------------------------------------------------------------ device-resident environments (no reference
 * counterpart: the reference's emulators are host threads, rollout.cc:280-328)
 * E environments that live in device memory and are stepped by a kernel, so that a whole rollout of T slots is ONE burst
 * of enqueued kernels - per slot the acting head, the environment step and render, the ingest and acting convolutions -
 * with nothing returning to the host in between.  The only kind is ALEPPO_ENV_SYNTHETIC: the trainer's SyntheticAtari
 * (trainer/emulator.hpp, which IS the specification: reset, step, the xorshift64 generator and both renderers, read
 * literally), stepped the way the trainer's EnvSet::step and collect() step it: an episode-start slot resets and keeps
 * the stale reward, any other slot steps with the action the acting head just sampled; terminal / truncated are 0 in a
 * start slot; `start` is set after a terminal or a truncation and cleared after the reset slot.  Integer arithmetic and
 * float additions of small integers only: a device rollout is the rollout the host loop aleppo_act -> emulator ->
 * aleppo_step would have collected, byte for byte - every plane of aleppo_read_batch, the episode log, the environment
 * state and aleppo_state_digest - so the two can be mixed rollout by rollout and a checkpoint written with one resumes
 * with the other.
 * Shared rules: the context's own stream only, no hipFree, no device-wide synchronise; never a collective (under data
 * parallelism each rank owns its environments); ALEPPO_ERR_RUNTIME while a step is armed; nothing the evaluation lanes
 * can observe changes, and the evaluation calls change nothing here.  A context that never calls aleppo_env_open
 * allocates and enqueues nothing for any of this. */
typedef enum { ALEPPO_ENV_SYNTHETIC = 0 } aleppo_env_kind;
typedef struct {
  int32_t kind;       /* ALEPPO_ENV_SYNTHETIC */
  int32_t frame_kind; /* ALEPPO_FRAMES_84 | ALEPPO_FRAMES_RAW_PAIR: what the environments render and the ingest reads */
  uint64_t seed_base; /* environment e is SyntheticAtari(seed_base + e, max_steps, max_return, A, raw) */
  uint64_t max_steps; /* truncation by emulator-frame budget (4 frames per agent step) */
  float max_return;   /* truncation by emulator episode return, compared in float; <= 0: off */
  int32_t reserved;   /* 0 */
} aleppo_env_config; /* 32 bytes */
/* One environment between two rollouts, 88 bytes, no padding: the twelve fields SyntheticAtari::visit lists (the
 * trainer's checkpoint order), then the trainer-side bookkeeping of collect() (TrainerState). */
typedef struct {
  uint64_t rng;          /* offset 0: xorshift64 state */
  uint64_t steps;        /*  8: emulator frames of the current game */
  uint64_t ep_len;       /* 16: agent steps of the current episode / game (trainer side) */
  uint64_t game_len;     /* 24 */
  int32_t lives;         /* 32: 0..5 */
  int32_t paddle;        /* 36: 4..79 */
  int32_t ball_x, ball_y, prev_x, prev_y; /* 40, 44, 48, 52: 0..83 */
  int32_t dx, dy;        /* 56, 60: +1 / -1 */
  int32_t bricks;        /* 64: >= 0 */
  float episode_return;  /* 68: the emulator's return of the current game (what max_return is compared with) */
  float reward;          /* 72: the last recorded reward (a start slot records it again) */
  float ep_ret, game_ret;/* 76, 80: returns of the current episode / game (trainer side) */
  uint8_t start;         /* 84: the next slot is an episode-start slot */
  uint8_t game_over;     /* 85: the last step ended the game */
  uint8_t reserved[2];   /* 86: 0 */
} aleppo_env_state;
typedef enum {
  ALEPPO_ENV_F_FRAMES = 0,          /* uint8 [E,84,84] or [E,2,210,160]: the frame buffer right now */
  ALEPPO_ENV_F_EPISODE_RETURNS = 1, /* float  [T,E] time-major: the return of the episode that ended in slot (t, e) */
  ALEPPO_ENV_F_EPISODE_LENGTHS = 2, /* uint32 [T,E]: its length in agent steps; 0 = no episode ended in that slot */
  ALEPPO_ENV_F_GAME_RETURNS = 3,    /* float  [T,E]: the same for games (an episode that ended with game over) */
  ALEPPO_ENV_F_GAME_LENGTHS = 4,    /* uint32 [T,E] */
  ALEPPO_ENV_F_STEP_MS = 5          /* double [2]: mean device time in ms of the environment kernel and the number of
                                       launches timed, over the aleppo_env_rollout calls made while aleppo_profile_enable
                                       was on since the last aleppo_profile_reset (HIP events around each launch) */
} aleppo_env_field;
/* Allocates - in this call and never later - the environments' state, the frame buffer ([E,84,84] or [E,2,210,160],
 * 16-byte aligned; the per-environment strides 7056 and 67200 are multiples of 16) and the four episode-log planes, and
 * puts every environment into the constructor's state with start = 1 and reward 0.  Called again with the same config
 * it resets the environments to that state; with another config it is ALEPPO_ERR_RUNTIME.  An unknown kind or frame
 * kind, a non-zero reserved field or a null pointer is ALEPPO_ERR_INVALID_ARGUMENT.  Nothing is freed before
 * aleppo_destroy. */
int aleppo_env_open(aleppo_ctx *ctx, const aleppo_env_config *cfg);
/* One whole rollout: for t in [0, T) aleppo_act's kernels with the built-in generator (the head publishes the actions and
 * the ticket as always), the environment kernel - it reads slot t's int32 actions where the head wrote them, steps and
 * renders every environment, and writes slot t's step record (rewards, terminal, truncated and start-at-entry bytes)
 * straight into the device record - and aleppo_step's kernels on the frame buffer with the record's start bytes.
 * Returns once the work is enqueued; no host wait in between.  Leaves the context ready for aleppo_finish_rollout, which
 * uses the device-written records as they are, as do ALEPPO_OPT_REWARD_SCALE, advantage_norm and ALEPPO_ROLLOUT_FP16.
 * The acting generator's counter advances as T aleppo_act calls advance it, and the ticket and the pinned action buffer
 * stay consistent: a host-driven rollout may follow a device one and vice versa.
 * ALEPPO_ERR_RUNTIME before aleppo_env_open, and unless the rollout buffer is empty (the next slot to fill is 0). */
int aleppo_env_rollout(aleppo_ctx *ctx);
/* The environments' part of a checkpoint, states [num_envs].  Valid between rollouts only, like
 * aleppo_export_rollout_state (ALEPPO_ERR_RUNTIME otherwise, and before aleppo_env_open); a null pointer or num_envs !=
 * config.num_envs is ALEPPO_ERR_INVALID_ARGUMENT.  The import refuses (ALEPPO_ERR_INVALID_ARGUMENT) what a run cannot
 * reach - lives outside 0..5, paddle outside 4..79, a ball coordinate outside 0..83, dx / dy not +-1, negative bricks,
 * a flag that is not 0 / 1, a non-zero reserved byte, a non-finite float - and a refused import changes nothing. */
int aleppo_env_export_state(aleppo_ctx *ctx, aleppo_env_state *states, size_t num_envs);
int aleppo_env_import_state(aleppo_ctx *ctx, const aleppo_env_state *states, size_t num_envs);
/* Read an aleppo_env_field; synchronises the context's stream like aleppo_read_batch.  The log planes are those of the
 * last aleppo_env_rollout (zero before any); compacted in slot-then-environment order they are the trainer's episode log
 * in the order collect() appends.  A wrong byte count or an unknown field is ALEPPO_ERR_INVALID_ARGUMENT; before
 * aleppo_env_open ALEPPO_ERR_RUNTIME. */
int aleppo_env_read(aleppo_ctx *ctx, int field, void *dst, size_t bytes);

/* ------------------------------------------------------------------ device-resident evaluation environments (no
 * reference counterpart)
 * L device-resident SyntheticAtari instances, one per evaluation lane, behind the lanes of aleppo_eval_open: one call
 * enqueues `steps` whole evaluation steps - per step the lanes' acting forward, the evaluation head, the environment
 * step and render, and the ingest - with nothing returning to the host in between.  The run is byte for byte the run the
 * host loop aleppo_eval_act -> emulator -> aleppo_eval_push_frames would have produced (the environments are stepped as
 * aleppo_env_rollout steps its own: a start lane resets and ignores its action), so the two can be mixed step by step.
 * Isolation: the five calls change nothing the rollout or the update can observe - not the rollout's stacks and planes,
 * t, the acting generator's counter, the pre-computed acting scratch of aleppo_step, aleppo_act's pinned buffer and
 * ticket, Adam state, metrics or a captured update.  A training run with these calls inserted at any point where no
 * step is armed (between an aleppo_step and the aleppo_act that follows it included) is bit-identical to the run without
 * them.  While a step is armed all five fail with ALEPPO_ERR_RUNTIME like every other stateful entry point; before
 * aleppo_eval_env_open the other four are ALEPPO_ERR_RUNTIME.  The environments are local to a rank: nothing is
 * exchanged under data parallelism and no call is a collective.  Nothing the device-resident TRAINING environments can
 * observe changes - not their state, frames, log or aleppo_state_digest - and their calls change nothing here.  The
 * context's own stream only, no hipFree, no device-wide synchronise.  A context that never calls aleppo_eval_env_open
 * allocates and enqueues nothing for any of this. */
typedef enum {
  ALEPPO_EEF_FRAMES = 0,          /* uint8 [L,84,84] or [L,2,210,160]: the frame buffer right now */
  ALEPPO_EEF_EPISODE_RETURNS = 1, /* float  [S,L] step-major: return of the episode that ended in (step, lane) of the LAST run */
  ALEPPO_EEF_EPISODE_LENGTHS = 2, /* uint32 [S,L]: its length in agent steps; 0 = none ended there */
  ALEPPO_EEF_GAME_RETURNS = 3,    /* float  [S,L]: the same for games (an episode that ended with game over) */
  ALEPPO_EEF_GAME_LENGTHS = 4     /* uint32 [S,L] */
} aleppo_eval_env_field;
/* Needs aleppo_eval_open first (ALEPPO_ERR_RUNTIME otherwise); L is that call's lane count.  Lane l becomes
 * SyntheticAtari(cfg->seed_base + l, max_steps, max_return, A, raw) in the constructor's state with start = 1 and reward
 * 0.  Allocates - in this call and never later, in one block kept until aleppo_destroy - the frame buffer, two alternating
 * state arrays and the four [S,L] log planes (zeroed), S = max_run_steps in [1, 1024].  Called again with the same kind,
 * frame kind, max_steps, max_return and S and ANY seed_base it re-seeds every lane to the constructor's state of the new
 * seed and zeroes the log, and touches neither the lanes' stacks nor the evaluation counter nor the ticket (every lane
 * then starts with a start step, which overwrites all four stack positions); with another kind, frame kind, budget or S
 * it is ALEPPO_ERR_RUNTIME.  A null config, an unknown kind or frame kind, a non-zero reserved field or S out of range is
 * ALEPPO_ERR_INVALID_ARGUMENT. */
int aleppo_eval_env_open(aleppo_ctx *ctx, const aleppo_env_config *cfg, int32_t max_run_steps);
/* `steps` evaluation steps, 1 <= steps <= S, with the built-in generator (there is no noise argument); rule and param
 * are aleppo_eval_act's and are checked by the same code.  For s in [0, steps), on the context's stream and with no host
 * wait: aleppo_eval_act's kernels (the head publishes the actions and the ticket to the lanes' pinned buffer as always;
 * the evaluation counter and the ticket advance by one), the environment kernel - it reads the int32 actions the head
 * just wrote, steps and renders every lane's environment and writes the start-at-entry bytes and row s of the log - and
 * aleppo_eval_push_frames' ingest on the frame buffer with those start bytes and the gray LUT of aleppo_set_gray_lut.
 * Returns once everything is enqueued.  Afterwards the lanes are where `steps` host-driven steps would have left them -
 * stacks, the ALEPPO_EF_* fields of the last step, evaluation counter, ticket and pinned buffer - so an aleppo_eval_act or
 * aleppo_eval_push_frames may follow and a host-driven step may precede.  Log rows [0, steps) hold this run's records,
 * rows [steps, S) are zero.  A launch that fails after part of the run is on the stream fails the context, as in
 * aleppo_env_rollout; a refused call changes nothing. */
int aleppo_eval_env_run(aleppo_ctx *ctx, int rule, float param, int32_t steps);
/* As aleppo_env_export_state / aleppo_env_import_state with num_lanes == L and the same refusals (one validator; a
 * refused import changes nothing), but valid whenever no step is armed: there is no "between rollouts" condition.  Both
 * synchronise the context's stream. */
int aleppo_eval_env_export_state(aleppo_ctx *ctx, aleppo_env_state *states, size_t num_lanes);
int aleppo_eval_env_import_state(aleppo_ctx *ctx, const aleppo_env_state *states, size_t num_lanes);
/* Read an aleppo_eval_env_field; synchronises the context's stream like aleppo_eval_read.  Compacted in
 * step-then-lane order the log planes are the episodes in the order the host loop would have met them.  A wrong byte
 * count or an unknown field is ALEPPO_ERR_INVALID_ARGUMENT; before aleppo_eval_env_open ALEPPO_ERR_RUNTIME. */
int aleppo_eval_env_read(aleppo_ctx *ctx, int field, void *dst, size_t bytes);

/* ------------------------------------------------------------------ episode recorders of the device-resident environments
 * (the reference's EpisodeRecorder / EpisodeObservationRecorder around environment 0, rollout.cc:149-158)
 * One recorder per source - ALEPPO_REC_ROLLOUT: environment `index` of aleppo_env_rollout; ALEPPO_REC_EVAL: lane `index` of
 * aleppo_eval_env_run - each an append log of `capacity` rows in device memory.  Every step of the source that those two
 * calls run takes row `rows` and increments it: ONE more kernel on the context's stream, directly behind the step's
 * ingest, writes the row's part of up to four planes:
 *   steps         one aleppo_rec_step;
 *   logits        float [A]: the logits of the step's acting decision as the source stores them (ALEPPO_ROLLOUT_FP16: the
 *                 half values widened, what aleppo_read_batch returns; evaluation lanes store fp32);
 *   frames        (ALEPPO_REC_FRAMES) the index's part of the frame buffer as the environment kernel left it:
 *                 uint8 [84,84] or [2,210,160];
 *   observations  (ALEPPO_REC_OBSERVATION) uint8 [84,84]: the newest plane of the index's stack after the ingest - for raw
 *                 pairs the frame after the gray LUT, the area resize and the two-frame maximum.
 * A plane that is not part of `content` is not allocated and not written.  With the log full a step is not captured: no
 * launch is made and `dropped` is incremented.  `ordinal` advances for every step of the source, captured or not -
 * host-driven ones included: wherever aleppo_step / aleppo_record_step / aleppo_release_step advance the rollout's slot
 * (aleppo_replay_rollout: by T), and for every aleppo_eval_push_frames - so a gap in the ordinals of consecutive rows is a
 * visible discontinuity.
 * Isolation: the calls change nothing the rollout, the update, the evaluation lanes or either set of environments can
 * observe: a training run with a recorder open gives bit-identical aleppo_read_batch planes, episode logs, environment
 * states, aleppo_state_digest and parameters.  The recorder is not part of any checkpoint, is local to a rank and never a
 * collective, and uses the context's own stream only, no hipFree, no device-wide synchronise.  While a step is armed all
 * calls but aleppo_rec_count fail with ALEPPO_ERR_RUNTIME.  A context that never calls aleppo_rec_open allocates nothing
 * and enqueues nothing more. */
typedef enum { ALEPPO_REC_ROLLOUT = 0, ALEPPO_REC_EVAL = 1 } aleppo_rec_source;
enum { ALEPPO_REC_FRAMES = 1, ALEPPO_REC_OBSERVATION = 2 }; /* content bits */
typedef struct {
  int32_t source;      /* aleppo_rec_source */
  int32_t index;       /* the environment in [0, E) / the lane in [0, L) that is recorded */
  int32_t content;     /* ALEPPO_REC_FRAMES | ALEPPO_REC_OBSERVATION, at least one */
  int32_t capacity;    /* rows, 1..65536 */
  int32_t reserved[4]; /* 0 */
} aleppo_rec_config; /* 32 bytes */
typedef struct {       /* 32 bytes, no padding */
  uint64_t ordinal;    /*  0: steps the source had taken since aleppo_rec_open, before this one */
  int32_t action;      /*  8: the head's action (a start step's environment ignores it) */
  float reward;        /* 12: as recorded, unclamped and unscaled; a start step: the stale one */
  float value;         /* 16: taken like the logits */
  uint8_t start, terminated, truncated, game_over; /* 20: start = the flag at entry; game_over = an episode ended here AND
                                                      the game with it */
  int32_t lives;       /* 24: after the step */
  int32_t reserved;    /* 28: 0 */
} aleppo_rec_step;
typedef struct {
  uint64_t rows, dropped, next_ordinal;
  int32_t capacity;
  int32_t frame_bytes;       /* bytes of a frames row (7056 or 67200); 0: not part of content */
  int32_t observation_bytes; /* 7056; 0: not part of content */
  int32_t actions;           /* A: a logits row is float [A] */
} aleppo_rec_counts; /* 40 bytes */
typedef enum {
  ALEPPO_REC_F_STEPS = 0,       /* aleppo_rec_step [rows] */
  ALEPPO_REC_F_LOGITS = 1,      /* float [rows, A] */
  ALEPPO_REC_F_FRAMES = 2,      /* uint8 [rows, 84, 84] or [rows, 2, 210, 160] */
  ALEPPO_REC_F_OBSERVATIONS = 3 /* uint8 [rows, 84, 84] */
} aleppo_rec_field;
/* Needs aleppo_env_open (ALEPPO_REC_ROLLOUT) or aleppo_eval_env_open (ALEPPO_REC_EVAL) first, ALEPPO_ERR_RUNTIME
 * otherwise: their frame kind fixes the row size.  Allocates one block - in this call and never later - and keeps it until
 * aleppo_destroy.  Called again with the same config it empties the log and sets the ordinal to 0; with another config for
 * an open source it is ALEPPO_ERR_RUNTIME.  A null pointer, an unknown source, an index outside the source's range, a
 * content of 0 or with unknown bits, a capacity outside [1, 65536] or a non-zero reserved word is
 * ALEPPO_ERR_INVALID_ARGUMENT; a refused call changes nothing. */
int aleppo_rec_open(aleppo_ctx *ctx, const aleppo_rec_config *cfg);
/* Host state only: no synchronise, and valid while a step is armed.  A source that was never opened reports zeros.  A
 * null pointer or an unknown source is ALEPPO_ERR_INVALID_ARGUMENT. */
int aleppo_rec_count(aleppo_ctx *ctx, int source, aleppo_rec_counts *out);
/* Copies rows [first_row, first_row + rows) of one aleppo_rec_field to dst; synchronises the context's stream like
 * aleppo_env_read.  A range outside [0, rows of the log], bytes != rows x the field's row size, an unknown field or source,
 * a field that is not part of content or a null dst is ALEPPO_ERR_INVALID_ARGUMENT; a source that is not open
 * ALEPPO_ERR_RUNTIME. */
int aleppo_rec_read(aleppo_ctx *ctx, int source, int field, uint64_t first_row, uint64_t rows, void *dst, size_t bytes);
/* rows = dropped = 0; the ordinal stays.  ALEPPO_ERR_RUNTIME for a source that is not open. */
int aleppo_rec_clear(aleppo_ctx *ctx, int source);

/* ------------------------------------------------------------------ multi-GPU (no reference counterpart)
 * One process per GPU.  Rank 0 creates the id, the launcher broadcasts its bytes, every rank calls
 * aleppo_comm_init.  Gradients (+ mask counts) are all-reduced with RCCL inside aleppo_train. */
#define ALEPPO_UNIQUE_ID_BYTES 128
int aleppo_comm_unique_id(uint8_t id[ALEPPO_UNIQUE_ID_BYTES]);
int aleppo_comm_init(aleppo_ctx *ctx, const uint8_t id[ALEPPO_UNIQUE_ID_BYTES]);

/* ------------------------------------------------------------------ stateless operators (host in / host out)
 * The reference's free functions, for parity tests that read like the reference's own tests.  Each one converts
 * its host tensors to the hot path's device layout and launches the SAME kernel the rollout / update launches
 * (gae_kernel, ingest_kernel, head_train_kernel, infer_head_kernel): there is no second implementation. */
/* ai::gae::gae (src/ai/gae.h:4-7): env-major [E,T]; same validation errors (gae.cc:8-53). */
int aleppo_gae(int device_ordinal, float *advantages, const float *rewards, const float *values,
               const float *next_values, const uint8_t *terminals, const uint8_t *truncations,
               const uint8_t *episode_starts, int64_t num_envs, int64_t num_steps, float gamma, float lambda);
/* ALEPPO_OPT_REWARD_SCALE on host tensors (no reference counterpart): steps 1-5 of the option on one rollout, through
 * the kernels aleppo_finish_rollout launches (rs_scan_kernel, rs_reduce_kernel, gae_scaled_kernel).  rewards: float [E,T]
 * env-major, raw in, scaled and clipped out; the flags uint8 [E,T]; stats_inout = (count, mean, var) and returns_inout =
 * G, double [E], before / after; *scale_out = s and *clipped_out = the clip count (either may be NULL).  Validation as
 * aleppo_gae (null tensors, E or T <= 0, overlapping flags: ALEPPO_ERR_INVALID_ARGUMENT), plus clip finite and > 0 and a
 * state aleppo_import_reward_scale would accept.  Nothing is written back when the call fails. */
int aleppo_reward_scale(int device_ordinal, float *rewards, const uint8_t *terminals, const uint8_t *truncations,
                        const uint8_t *episode_starts, int64_t num_envs, int64_t num_steps, float gamma, float clip,
                        double stats_inout[3], double *returns_inout, float *scale_out, int64_t *clipped_out);
/* ai::vision::resize_frame_stacked_grayscale_images (vision.cc:22-32): float [n,210,160] -> [n,84,84] */
int aleppo_vision_resize_area(int device_ordinal, const float *images, float *out, int64_t n);
/* ai::vision::rgb_to_grayscale_frame_stacked_images (vision.cc:71-84): float [n,3,84,84] -> [n,84,84] */
int aleppo_vision_rgb_to_gray(int device_ordinal, const float *images, float *out, int64_t n);
/* The fused device preprocessing on its own: uint8 [n,2,210,160] (+lut or NULL) -> uint8 [n,84,84] */
int aleppo_preprocess(int device_ordinal, const uint8_t *raw_pairs, const uint8_t *lut256, uint8_t *out, int64_t n);
/* Rollout::update_observations (rollout.cc:184-196) on host tensors: obs uint8 [E,4,84,84] in/out */
int aleppo_update_observations(int device_ordinal, uint8_t *observations, const uint8_t *frames,
                               const uint8_t *episode_start, int64_t num_envs);
/* ai::ppo::losses::compute (+ normalize_logits) forward and gradients (losses.cc:4-47):
 * logits float [B,A] RAW (un-normalised); outputs per-sample [B]; dlogits [B,A]; any output may be NULL. */
int aleppo_ppo_loss(int device_ordinal, const float *logits, const float *old_log_probabilities,
                    const int64_t *actions, const float *advantages, const float *values, const float *returns,
                    const uint8_t *masks, int64_t batch, int64_t num_actions, float clip_param,
                    float value_loss_coef, float entropy_coef, float *loss, float *clipped, float *value_losses,
                    float *entropies, float *total_losses, float *ratio, float *dlogits, float *dvalues);
/* multinomial(probs,1,true) given its exponential noise (train.cc:374-375): probs,q float [E,A] */
int aleppo_sample(int device_ordinal, const float *probs, const float *q, int64_t *actions, int64_t num_envs,
                  int64_t num_actions);

/* ------------------------------------------------------------------ measurement hooks (bench.py)
 * Average device time in ms of the named kernel class over the calls since the last reset, measured
 * with HIP events on the stream the kernels run on; *launches gets the number of timed launches. */
typedef enum {
  ALEPPO_K_INGEST = 0,      /* preprocess + frame stack + rollout-slot write */
  ALEPPO_K_GAE = 1,         /* reward clamp (or ALEPPO_OPT_REWARD_SCALE's scan and merge) + GAE + returns + old log-probs */
  ALEPPO_K_HEAD = 2,        /* heads + PPO loss forward/backward */
  ALEPPO_K_ADAM = 3,        /* sum of squares + clip + Adam (with ALEPPO_OPT_WEIGHT_DECAY / _ANCHOR_COEF: its regularised form) + dgrad weight repack */
  ALEPPO_K_CONV1_FWD = 4,
  ALEPPO_K_CONV2_FWD = 5,
  ALEPPO_K_CONV3_FWD = 6,
  ALEPPO_K_FC_FWD = 7,
  ALEPPO_K_FC_DGRAD = 8,
  ALEPPO_K_FC_WGRAD = 9,
  ALEPPO_K_CONV3_DGRAD = 10,
  ALEPPO_K_CONV3_WGRAD = 11,
  ALEPPO_K_CONV2_DGRAD = 12,
  ALEPPO_K_CONV2_WGRAD = 13,
  ALEPPO_K_CONV1_WGRAD = 14,
  ALEPPO_K_REDUCE = 15,     /* split-K slab reduction */
  ALEPPO_K_INFER_HEAD = 16, /* action head + sampling */
  ALEPPO_K_ACT_FUSED = 17,  /* frame ingest + conv1-3 of the acting batch in one launch (aleppo_step, bf16) */
  ALEPPO_K_CONV_FWD = 18,   /* conv1 -> conv2 -> conv3 of the update's forward pass in one launch (bf16) */
  ALEPPO_K_CONV_BWD = 19,   /* conv2 dgrad + conv2 wgrad + conv1 wgrad of the update's backward pass in one launch (bf16) */
  ALEPPO_K_REC_CAPTURE = 20, /* the episode recorders' capture kernel (aleppo_rec_open), one launch per recorded step */
  ALEPPO_K_ACT_STATS = 21,  /* the read-only passes over the activations, one bracket per forward chunk: aleppo_activation_stats' launch,
                               aleppo_feature_rank's three (flags, Gram, reduce), aleppo_refresh_advantages' value launch (the last
                               bracket of a call also holds its two statistics launches); and the read-only diagnostic passes
                               that have no class of their own: aleppo_policy_diff's comparison, one bracket per chunk, and
                               aleppo_grad_gram's two launches, one bracket per call */
  ALEPPO_K_RECYCLE = 22,    /* the masked pass of aleppo_recycle_units / aleppo_recycle_dormant over P / M1 / M2, one launch per call */
  ALEPPO_K_SAL_BLUR = 23,    /* aleppo_saliency's blur of the samples a forward chunk touches */
  ALEPPO_K_SAL_PERTURB = 24, /* ... its blend of one chunk's perturbed stacks into the staging buffer */
  ALEPPO_K_SAL_SCORE = 25,   /* ... its scoring launch, one per forward chunk */
  ALEPPO_K_EMA = 26,         /* aleppo_ema_update's streaming pass over P / the averaged set, one launch per call */
  ALEPPO_K_COUNT = 27
} aleppo_kernel_class;
int aleppo_profile_enable(aleppo_ctx *ctx, int on);
int aleppo_profile_read(aleppo_ctx *ctx, int kernel_class, double *avg_ms, int64_t *launches);
int aleppo_profile_reset(aleppo_ctx *ctx);
/* Per-context tuning / A-B switches.  ALEPPO_OPT_GENERIC_CONV = 1: run the bf16 convolutions on the generic
 * gather-GEMM kernels instead of the sample-stationary ones (same math, used by the parity tests). */
typedef enum {
  ALEPPO_OPT_GENERIC_CONV = 0,
  ALEPPO_OPT_DEBUG_NO_PUBLISH = 1, /* diagnosis only: the head kernel skips the pinned-memory hand-off */
  ALEPPO_OPT_FORCE_COMM = 2,       /* tests: run the RCCL all-reduce path even with a 1-rank communicator */
  ALEPPO_OPT_SERIAL_UPDATE = 3,    /* measurement: run the weight-gradient kernels on the main stream too (isolated
                                      per-kernel timings; default 0 = co-scheduled on a second stream) */
  ALEPPO_OPT_FC_PIPE = 4,          /* 0: small-tile fc GEMMs instead of the pipelined LDS-DMA ones (A/B, parity tests) */
  /* 5 and 8 were the opt-in pipelined fc weight gradient and the fused conv2-dgrad + conv1-wgrad launch: both measured
     slower than the defaults in rounds 1-3 and were deleted */
  ALEPPO_OPT_FUSED_ACT = 6,        /* frame ingest fused in front of the acting convolutions (bf16): 0 never, 1 where it
                                      is faster (default: given 84x84 frames, raw pairs in mapped host memory), 2 always */
  ALEPPO_OPT_GATE_TIMEOUT_MS = 9,  /* exit condition of the slot-ahead gate in milliseconds (default 120 000; also the
                                      environment variable ALEPPO_GATE_TIMEOUT_MS at aleppo_create) */
  ALEPPO_OPT_FUSED_FWD = 10,       /* 0: the update's forward convolutions as three launches instead of the fused
                                      conv1 -> conv2 -> conv3 kernel (bf16; same bits either way: A/B, parity tests; also
                                      the environment variable ALEPPO_FWD_FUSED at aleppo_create) */
  ALEPPO_OPT_FUSED_BWD = 11,       /* conv2's data gradient, conv2's weight gradient and conv1's weight gradient as ONE launch that
                                      keeps dz1 on the CU (bf16): 0 never (three launches on two streams: A/B, parity
                                      tests), 1 at minibatches of >= 2048 samples (default), 2 always; environment:
                                      ALEPPO_BWD_FUSED */
  ALEPPO_OPT_UPDATE_GRAPH = 7,     /* 1: capture the epochs x minibatches loop of aleppo_train in a hipGraph and replay it
                                      (capture_train_cuda_graph, src/ai/ppo/train.h:163-195); lr and the Adam bias
                                      corrections are device scalars, so a replay follows the annealed rate */
  ALEPPO_OPT_MINIBATCH_SHUFFLE = 12, /* 0 (default): minibatch m of every epoch is the contiguous slice [m*B, (m+1)*B) of the
                                      batch, like the reference (which draws randperm and never uses it, train.h:146).
                                      1: every epoch of every aleppo_train uses a fresh permutation of the N local samples
                                      (the keyed bijection documented at aleppo_read_sample_order), on every schedule -
                                      eager or ALEPPO_OPT_UPDATE_GRAPH, fp32 or bf16, one GPU or data parallel */
  ALEPPO_OPT_VALUE_CLIP = 13,      /* value-function clipping (CleanRL clip_vloss, baselines ppo2).  0 (default): the
                                      reference's value loss 0.5 (v - R)^2.  1: clipped at c = config.clip_param; any other
                                      value is ALEPPO_ERR_INVALID_ARGUMENT.  Per sample, v = the value head's output, R = the
                                      return, v_old = the value stored when the sample was collected:
                                        d   = v - v_old
                                        v_c = |d| <= c ? v : v_old + copysign(c, d)   (a select: inside the range v_c IS v)
                                        l_u = (v - R)^2,  l_c = (v_c - R)^2
                                        value loss = 0.5 max(l_u, l_c)   (ALEPPO_M_VALUE_LOSSES and the value_loss mean)
                                        dL/dv = l_u >= l_c ? v - R : 0   (ties: the unclipped branch)
                                      and only that term of the total loss changes (same coefficients, masked mean and
                                      global count).  v_old of a rollout batch (aleppo_finish_rollout) is the values plane
                                      as stored - with ALEPPO_ROLLOUT_FP16 the fp16-rounded values, what aleppo_read_batch
                                      (ALEPPO_F_VALUES) returns; of a caller batch, what aleppo_set_batch_values stored:
                                      aleppo_train on a caller batch without them is ALEPPO_ERR_RUNTIME.  The same on every
                                      schedule, like ALEPPO_OPT_MINIBATCH_SHUFFLE */
  ALEPPO_OPT_ADV_NORM_MINIBATCH = 14, /* per-minibatch advantage normalisation (CleanRL norm_adv, SB3 normalize_advantage).
                                      0 (default): the advantages as stored.  1: normalised per minibatch; any other value
                                      is ALEPPO_ERR_INVALID_ARGUMENT.  Read at each aleppo_train.  For every (epoch e,
                                      minibatch m) of the call:
                                        sample set: the minibatch's unmasked samples (mask = !episode_start, the loss's
                                          mask) in the call's order, contiguous or shuffled; with data parallelism the
                                          global minibatch, the union over ranks (like the masked-mean count)
                                        sums, in double: n = count, S = sum a, Q = sum a^2, a = the advantage as stored
                                          widened to fp32 and then to double; each rank sums in a fixed order and the
                                          ranks' (n, S, Q) are all-reduced in double
                                        mean = S / n,  var = max(0, (Q - S*S/n) / max(n - 1, 1))  (unbiased, like
                                          torch.std),  std = sqrt(var),  mean_f = (float)mean,
                                          inv_f = (float)(1 / (std + 1e-8))  (computed in double)
                                        n = 0: mean_f = 0, inv_f = 1 (and std = 0); such a minibatch contributes nothing
                                        every sample of the minibatch, masked or not, uses a^ = (a - mean_f) * inv_f in fp32
                                          in place of a wherever the loss uses the advantage: the surrogate, the clip
                                          activity test and the gradient.  a^ is never stored (with ALEPPO_ROLLOUT_FP16
                                          planes it is not rounded to half)
                                      It composes with config.advantage_norm = 1 (the whole-batch normalisation of
                                      aleppo_finish_rollout runs first, this one on top of it in the update) and works with
                                      ALEPPO_OPT_MINIBATCH_SHUFFLE, ALEPPO_OPT_VALUE_CLIP, ALEPPO_OPT_UPDATE_GRAPH, fp32 and
                                      bf16, rollout and aleppo_set_batch batches, one GPU or data parallel.  The statistics
                                      depend only on a minibatch's sample set, so one call of E epochs equals E one-epoch
                                      calls bit for bit.  Read back: ALEPPO_M_ADV_MEAN / ALEPPO_M_ADV_STD */
  ALEPPO_OPT_KL_PENALTY = 15,      /* the adaptive-KL-penalty objective of the PPO paper (section 4; RLlib's kl_coeff), on
                                      top of the clipped one.  0 (default): nothing changes.  1: the exact KL is computed
                                      for every sample and beta KL is added to the loss, beta = ALEPPO_OPT_KL_COEF; any
                                      other value is ALEPPO_ERR_INVALID_ARGUMENT.  Read at each aleppo_train.  Per sample,
                                      masked or not, with olp = the stored old log-probs widened to fp32 (with
                                      ALEPPO_ROLLOUT_FP16 planes: the fp16 values as stored) and lp = the log-softmax of
                                      the logits the loss computes, p = exp(lp):
                                        q_a = exp(olp_a),  S = sum_a q_a,  KL = sum_a q_a (olp_a - lp_a)
                                        total loss += beta KL   (ALEPPO_M_TOTAL_LOSSES, aleppo_minibatch_metrics.loss)
                                        dL/dz_j += (mask / mask_count) beta (p_j S - q_j)   (z: the logits; the value
                                          output's gradient is untouched)
                                      S stands where 1 would with exact old probabilities: with fp16 planes sum q is not
                                      exactly 1, and the gradient is the exact derivative of the loss reported.  With
                                      beta = 0 the per-sample KL is still computed and read back, and every other number
                                      (parameters, Adam state, every other plane and metric) is bit-identical to option 0.
                                      A very large config.clip_param makes the clipped surrogate the plain ratio times the
                                      advantage, which turns the update into pure PPO-penalty.  Works with
                                      ALEPPO_OPT_MINIBATCH_SHUFFLE, ALEPPO_OPT_VALUE_CLIP, ALEPPO_OPT_ADV_NORM_MINIBATCH,
                                      config.advantage_norm, ALEPPO_OPT_UPDATE_GRAPH, fp32 and bf16, fp32 and fp16 rollout
                                      planes, rollout and aleppo_set_batch batches, one GPU or data parallel; one call of
                                      E epochs equals E one-epoch calls bit for bit.  Read back: ALEPPO_M_KL /
                                      ALEPPO_M_MEAN_KL.  Adapting beta between updates (the paper's rule) is the caller's
                                      part: the trainer's kl_target does it */
  ALEPPO_OPT_KL_COEF = 16,         /* beta of ALEPPO_OPT_KL_PENALTY as the IEEE-754 binary32 BIT PATTERN in `value`
                                      (default 0 = +0.0f).  Valid: exactly the finite non-negative floats, value in
                                      [0, 0x7F800000); -0.0, negative values, Inf and NaN are ALEPPO_ERR_INVALID_ARGUMENT.
                                      aleppo_get_option returns the bits.  A device value, uploaded at each aleppo_train:
                                      a captured update (ALEPPO_OPT_UPDATE_GRAPH) follows a beta changed between calls,
                                      and unlike the other options setting it does not re-arm the capture */
  /* 17-21: the clip range, the loss coefficients and the gradient-norm limit PER UPDATE (baselines ppo2's annealed
     cliprange, SB3's clip_range / clip_range_vf schedules, RLlib's entropy_coeff_schedule).  Each carries the IEEE-754
     binary32 BIT PATTERN of its float in `value`, like ALEPPO_OPT_KL_COEF, and replaces one aleppo_config value from the
     next aleppo_train on.  An invalid pattern (-0.0, a negative value, Inf, NaN, and zero where > 0 is required) is
     ALEPPO_ERR_INVALID_ARGUMENT and leaves the old value in place.  Until an option is set aleppo_get_option returns the
     bits of the config value it stands for; there is no "unset", and setting the config's own value is allowed.
     The values are read at each aleppo_train and hold for the whole call (no schedule inside a call).  They are device
     values uploaded at the start of the call, next to Adam's step scalars: a captured update (ALEPPO_OPT_UPDATE_GRAPH)
     follows values changed between calls, and setting one does not re-arm the capture.  Every context works this way,
     whether one of the five was ever set or not: the head and Adam kernels read the numbers from device memory, and a
     context created with values X and one created with other values and set to X give bit-identical parameters, Adam
     state, metrics, per-sample planes and gradients.  They work on every schedule the other options
     work on: eager or captured, fp32 or bf16, fp32 or fp16 rollout planes, rollout and aleppo_set_batch batches, with
     ALEPPO_OPT_MINIBATCH_SHUFFLE, ALEPPO_OPT_VALUE_CLIP, ALEPPO_OPT_ADV_NORM_MINIBATCH and ALEPPO_OPT_KL_PENALTY in any
     combination, one GPU or data parallel.  With data parallelism EVERY RANK MUST SET THE SAME VALUES before the same
     update (they are not exchanged: ranks that clip or weigh differently apply different steps and drift apart). */
  ALEPPO_OPT_CLIP_PARAM = 17,      /* replaces config.clip_param: the range of the clipped surrogate, of the clip-fraction
                                      metric (ALEPPO_M_CLIP_FRACTION), and of ALEPPO_OPT_VALUE_CLIP's c unless
                                      ALEPPO_OPT_VALUE_CLIP_RANGE was set.  Valid: finite and > 0 */
  ALEPPO_OPT_VALUE_CLIP_RANGE = 18, /* the c of ALEPPO_OPT_VALUE_CLIP only (SB3's clip_range_vf); nothing else reads it.
                                      Until it is set it IS the current clip parameter, and follows ALEPPO_OPT_CLIP_PARAM
                                      (aleppo_get_option returns those bits); once set it stays what it was set to.
                                      Valid: finite and > 0 */
  ALEPPO_OPT_VALUE_LOSS_COEF = 19, /* replaces config.value_loss_coef.  Valid: finite and >= 0 (+0.0: no value gradient) */
  ALEPPO_OPT_ENTROPY_COEF = 20,    /* replaces config.entropy_coef.  Valid: finite and >= 0 */
  ALEPPO_OPT_MAX_GRAD_NORM = 21,   /* replaces config.max_gradient_norm, the limit of the global-norm clip in front of
                                      Adam.  The reported grad_norm is the norm before clipping and does not depend on
                                      it; aleppo_export_grads scales by the limit the last aleppo_train ran with.
                                      Valid: finite and > 0 */
  /* 22 stays unassigned: tests/test_hyper_schedule.py holds it as its example of an option that does not exist */
  ALEPPO_OPT_REWARD_SCALE = 23,    /* return-based reward scaling (gym's NormalizeReward, SB3's VecNormalize(norm_reward),
                                      the "reward scaling" of Engstrom et al. 2020) in place of the reward clamp.
                                      0 (default): the reference's clamp to [-1, 1] (buffer.cc:67).  1: scaling; any other
                                      value is ALEPPO_ERR_INVALID_ARGUMENT.  Read at each aleppo_finish_rollout, which then,
                                      before GAE, on the records as the caller recorded them (raw fp32 rewards r[t][e] and
                                      the three flags; whichever of aleppo_record_step / aleppo_step, aleppo_arm_step /
                                      aleppo_release_step and aleppo_replay_rollout filled them):
                                        1 running return.  G[e], a double per environment of this rank, 0 at aleppo_create,
                                          carried from rollout to rollout.  For t = 0 .. T-1, in a slot that is NOT an
                                          episode-start slot: G[e] = G[e] * (double)gamma + (double)r[t][e] (two roundings),
                                          and this G[e] is one sample x; then G[e] = 0 if the slot is terminal or truncated.
                                          An episode-start slot (whose reward is the stale one, rollout.cc:214) gives no
                                          sample and leaves G[e] alone.
                                        2 batch moments, in double: n, S = sum x, Q = sum x^2 over the rollout's samples.
                                          The order is fixed and a function of (E, T) only: each environment in slot
                                          order, 64 consecutive environments folded by a fixed tree, the groups of 64 added
                                          in index order - two runs give the same bits.  With a communicator (world_size > 1
                                          or ALEPPO_OPT_FORCE_COMM) the ranks' (n, S, Q) are all-reduced as ncclDouble /
                                          ncclSum, and the call is a COLLECTIVE (as it is with advantage_norm = 1).
                                          mean_b = S / n, var_b = max(0, Q / n - mean_b^2).
                                        3 running statistics (count, mean, var), gym's / SB3's RunningMeanStd in double,
                                          (1e-4, 0, 1) at aleppo_create.  If n > 0: d = mean_b - mean, tot = count + n,
                                          mean += d * n / tot, var = (var * count + var_b * n + d * d * count * n / tot) /
                                          tot, count = tot (left to right, no fused multiply-add; the same code with and
                                          without the all-reduce, so a 1-rank communicator gives the single-GPU bits).
                                        4 s = (float)(1 / sqrt(var + 1e-8)), computed in double and rounded once.
                                        5 every reward of the rollout, start slots included, becomes
                                          min(max(r * s, -c), c) in fp32, in place, c = ALEPPO_OPT_REWARD_SCALE_CLIP.  These
                                          are the rewards GAE uses and ALEPPO_F_REWARDS returns; the clamp does not run.
                                      Unlike gym, which updates the statistics after every step and scales that step's
                                      reward with the statistics so far, all T slots of a rollout are scaled with the
                                      statistics AFTER the whole rollout was merged; the running state after the rollout
                                      is gym's (the merge is associative up to rounding).  The mean is never subtracted.
                                      With the option off the state is kept and not updated.  aleppo_set_batch batches and
                                      the evaluation lanes are untouched; ALEPPO_ROLLOUT_FP16 changes nothing here (the
                                      records hold fp32 rewards).  A rollout aleppo_finish_rollout refuses for overlapping
                                      flags leaves the state as it was.  With data parallelism every rank must set the same
                                      two options (they are not exchanged, as for 17-21).  Read back: ALEPPO_F_REWARD_SCALE;
                                      checkpoint: aleppo_export_reward_scale / aleppo_import_reward_scale */
  ALEPPO_OPT_REWARD_SCALE_CLIP = 24, /* the clip c of ALEPPO_OPT_REWARD_SCALE as the IEEE-754 binary32 BIT PATTERN, like
                                      ALEPPO_OPT_KL_COEF (default: the bits of 10.0f).  Valid: finite and > 0; anything else
                                      is ALEPPO_ERR_INVALID_ARGUMENT and leaves the old value in place.  Read at each
                                      aleppo_finish_rollout */
  ALEPPO_OPT_EVAL_PARAMS = 25,      /* which parameters the evaluation lanes act on.  0 (default): the live ones.  1: the
                                      averaged set of aleppo_ema_open - every weight and bias of aleppo_eval_act's and
                                      aleppo_eval_env_run's acting forward and of the evaluation head (the compute-type
                                      copy for the convolution and fc weights, the fp32 set for the biases and the heads).
                                      The rollout's acting (aleppo_act / aleppo_step / aleppo_env_rollout) and everything
                                      in aleppo_train keep the live parameters, and a captured update stays valid.  An
                                      ALEPPO_REC_EVAL recorder then records the AVERAGED policy's logits, values and
                                      actions.  1 before aleppo_ema_open: ALEPPO_ERR_RUNTIME; any other value:
                                      ALEPPO_ERR_INVALID_ARGUMENT; both leave the old value in place */
  /* 26-27: decoupled regularisation INSIDE the optimizer step.  Each carries the IEEE-754 binary32 BIT PATTERN of its float in
     `value`, like ALEPPO_OPT_KL_COEF: valid are exactly the finite non-negative floats, value in [0, 0x7F800000); anything else
     is ALEPPO_ERR_INVALID_ARGUMENT and leaves the old value in place; the default is 0 = +0.0f; aleppo_get_option returns the
     bits.  With wd the weight decay and la the anchor coefficient, every optimizer step of an aleppo_train(lr, ...) call uses
       f_wd = (float)((double)lr * (double)wd)        f_an = (float)((double)lr * (double)la)
     uploaded into two slots of the device hyper-parameter block at the start of the call, next to the five values of 17-21.
     For every element of the parameters (all 12 tensors), p0 the parameter before the step and a the anchor's element:
       q = the parameter Adam's step produces from p0, exactly as without the options (moments, clip factor, step size)
       r = fma(f_wd, p0, fl(f_an * fl(p0 - a)))       fp32: one fused multiply-add, written out
       p = fl(q - r)
     and p is what the master parameters, the bf16 compute copy and the data-gradient layouts receive, in the same launch.
     The terms are DECOUPLED: they never pass through the gradient-norm clip or Adam's moments, so the moments, the reported
     grad_norm, aleppo_export_grads and every metric are what they are without the options.  With la = 0 this is
     torch.optim.AdamW (Loshchilov & Hutter 2019): p0 (1 - lr wd) - step.  With wd = 0 it is the decoupled form of L2 Init /
     regenerative regularisation (Kumar, Marklund & Van Roy 2023).  The coupled form (the gradient grows by wd * p before the
     norm) and a per-tensor selection (no decay on biases) are out of scope.
     The anchor a is a fourth parameter set: aleppo_anchor_take / aleppo_anchor_import below.  aleppo_train with la > 0 and no
     anchor is ALEPPO_ERR_RUNTIME and changes nothing; weight decay alone needs no anchor and allocates nothing (a reads as
     +0.0f, f_an is 0).
     A context whose two coefficients are both zero launches the Adam kernel it always launched and nothing else: it is
     bit-identical and equally fast whether the options were never set or set back to zero.  Otherwise a second entry point
     over the same step is launched in its place, which also reads the anchor: one more fp32 stream.  Every schedule works -
     eager or ALEPPO_OPT_UPDATE_GRAPH, fp32 or bf16, ALEPPO_OPT_MINIBATCH_SHUFFLE, ALEPPO_OPT_VALUE_CLIP,
     ALEPPO_OPT_ADV_NORM_MINIBATCH, ALEPPO_OPT_KL_PENALTY, one GPU or data parallel.  A captured update follows coefficients
     changed between calls and equals the eager update bit for bit; only a change of WHICH kernel runs (both zero <-> not, or
     the first anchor) re-arms the capture.  aleppo_tensor_stats' STEP section keeps recomputing Adam's term from the moments
     and does not include r.  With data parallelism EVERY RANK MUST SET THE SAME VALUES AND THE SAME ANCHOR before the same
     update (they are not exchanged: ranks that decay differently apply different steps and drift apart). */
  ALEPPO_OPT_WEIGHT_DECAY = 26,    /* wd, torch.optim.AdamW's weight_decay.  Valid: finite and >= 0 */
  ALEPPO_OPT_ANCHOR_COEF = 27,     /* la, the strength of the pull toward the anchor.  Valid: finite and >= 0 */
  ALEPPO_OPT_ACT_STORE = 28        /* test hook of aleppo_export_acting.  0 (default): the fused acting launch of a bf16
                                      context keeps conv1 / conv2 in LDS.  1: a storing instantiation of the same kernel
                                      also writes them to the activation scratch, in the training layout; conv3, the fc
                                      slices, logits, values and actions keep their bits.  Any other value is
                                      ALEPPO_ERR_INVALID_ARGUMENT; like every option it is refused while a step is armed.
                                      The generic and fp32 routes store conv1 / conv2 anyway and do not read it */
} aleppo_option;
int aleppo_set_option(aleppo_ctx *ctx, int option, int value);
/* Current value of an option; for ALEPPO_OPT_UPDATE_GRAPH the number of graph launches so far (0 = every update ran
 * eagerly), for the others the value last set / the default. */
int aleppo_get_option(aleppo_ctx *ctx, int option, int64_t *value);
/* Block until everything enqueued on ctx's streams has finished. */
int aleppo_synchronize(aleppo_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
