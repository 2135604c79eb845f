// train - C++ trainer shell over libaleppo.so (C ABI only; no libtorch, no HIP headers).
//
// Keeps the command line and the configs/*.yaml keys of the reference trainer
//   train <rom> <log path> <video dir> <group> <config.yaml> [profile]          (src/bin/train.cc:323-335)
// and re-hosts what main() and Rollout's HOST half do around the hot path:
//   * Config / load_config with the reference's keys and defaults           (src/bin/train.cc:33-63,108-136)
//   * worker threads stepping environments, fed by an index queue           (src/ai/rollout.cc:280-328, queue.h)
//     - actions are read from the pinned buffer aleppo_act returns instead of tensor.item()  (rollout.cc:312-313)
//   * the slot protocol: episode-start slots, stale rewards, flag bookkeeping, episode / game statistics,
//     total_steps counting only non-start slots                              (src/ai/rollout.cc:204-267)
//   * warm rollout before the loop, linear lr anneal, "Rollout i of N", scalar logging
//                                                                            (src/bin/train.cc:391-458,163-210)
//   * orthogonal init with gains sqrt(2) / 0.01 / 1, zero biases            (src/bin/train.cc:212-253)
//   * a TensorBoard event file (TFRecord + hand-encoded protobuf): every scalar and histogram of log_data
//     (src/bin/train.cc:163-210) and the hparams session record of logger.add_hparams (:72-105, :389)
//   * the optional 6th argument [profile] (src/bin/train.cc:409-419, 459-462 save a Kineto trace there): a
//     chrome://tracing / Perfetto JSON of every C-ABI call (host spans) plus the per-kernel-class device times the
//     library measures with HIP events; the same spans are roctx ranges (rocprofv3 --marker-trace) when libroctx64.so
//     is loadable
//   * the emulator threads write their frames into ONE page-locked, GPU-mapped buffer (aleppo_host_alloc) that the
//     ingest kernel reads in place (ALEPPO_HOST_MAPPED) - no per-slot staging copy (rollout.cc:325-326 memcpy's into
//     per-env host vectors that update_observations then stacks and uploads)
// ALE is not available in this build environment (no headers, no ROMs): the emulator behind the
// VirtualEnvironment-like interface is a deterministic synthetic Atari-shaped game (84x84 gray frames,
// 5 lives, reward on "brick hits", terminal on life loss like EpisodeLife, truncation at max_steps /
// max_return).  The rom argument is accepted and recorded but not opened.
// New OPTIONAL yaml keys (defaults reproduce the reference): precision: fp32|bf16, rollout_precision: fp32|fp16,
// device_preprocess: false (true: the emulators hand over RAW 210x160 frame pairs and the device does gray LUT + resize +
// max), advantage_norm: false, action_size (honoured here; the reference hard-codes 4, Q4), seed,
// slot_ahead: true (the next slot's ingest + acting kernels are enqueued BEFORE the emulator threads run, behind a stream
// wait that aleppo_release_step lifts when they are done: aleppo_arm_step in include/aleppo.h; false: aleppo_step),
// shuffle_minibatches: false, clip_value_loss: false (ALEPPO_OPT_VALUE_CLIP: CleanRL's clip_vloss), target_kl (absent or
// <= 0: off; else the update runs one epoch per aleppo_train call and stops after the epoch whose LAST minibatch's
// approx-KL exceeds it, CleanRL's rule; exact, because E one-epoch calls equal one call of E epochs),
// minibatch_advantage_norm: false (ALEPPO_OPT_ADV_NORM_MINIBATCH: CleanRL's norm_adv; logs mean_advantage_std),
// kl_coef (absent or 0: off; > 0: ALEPPO_OPT_KL_PENALTY with this initial beta, the PPO paper's KL penalty on top of
// clipping) and kl_target (absent or 0: beta stays put; > 0, which needs kl_coef > 0: after each rollout's update, with
// d = the mean exact KL over the minibatches of the last epoch that ran, beta /= 2 if d < kl_target / 1.5 and beta *= 2
// if d > 1.5 kl_target, the paper's section 4 rule; halving stops at KL_BETA_MIN, so that beta can always grow again;
// every rank computes the same beta, since the means are global).  Negative values are refused.  With kl_coef > 0 the
// trainer logs kl_coef (the beta of the rollout's update) and mean_kl (d).  log_batch_stats: false (true: after every
// rollout that is trained on, ALEPPO_F_BATCH_STATS is read - a collective under data parallelism, so every rank reads -
// and explained_variance, mean_value / std_value, mean_return / std_return, mean_advantage / std_advantage are logged;
// a NaN explained variance is logged as NaN).  log_tensor_stats: false (true: after each rollout's update rank 0 - the call
// is not a collective, and every rank holds the same parameters and all-reduced gradient - reads both sections of
// aleppo_tensor_stats and logs tensor_stats/<tensor>/grad_norm, /param_norm and /update_ratio for the twelve tensors
// (conv1.w ... value.b) and total, and tensor_stats/nonfinite, the two non-finite counts of the whole model added; a
// library without the entry point refuses the key at start-up).  log_activation_stats: false (true: after the update of
// every activation_stats_interval-th rollout - default 1 - rank 0 calls aleppo_activation_stats on the batch the context
// holds, with the dormancy threshold dormant_tau - default 0.025 - and logs, for conv1, conv2, conv3, fc and total,
// activation_stats/<layer>/dormant_fraction, /dead_fraction, /positive_fraction and /mean_abs, and
// activation_stats/nonfinite; never a collective: the figures describe rank 0's samples; a library without the entry point
// refuses the key at start-up, and a dormant_tau that is negative or not a finite number, or an interval below 1, is
// refused when the config is loaded).  recycle_dormant: false (true: ReDo, Sokar et al. 2023 - after the update of every
// recycle_interval-th rollout - default 64: ReDo's 1000 gradient steps at the 16 minibatch steps per rollout of the benched
// configuration - the trainer calls aleppo_recycle_dormant on the batch the context holds, with the threshold recycle_tau -
// default 0.025 - on the layers of recycle_layers - a list of conv1 / conv2 / conv3 / fc, default all - and the key
// splitmix64(seed ^ rollout index), so that a resumed run replays the same recycles; this comes after the statistics above
// are read, before the iteration's checkpoint is written and before any digest is taken; it logs recycle/<layer>/units and
// recycle/total; the three other keys without recycle_dormant, a bad tau, interval or layer name, a library without the
// entry point and WORLD_SIZE > 1 - the scores describe one rank's samples - are refused at start-up).  record_saliency: false
// (true: after the update of every saliency_interval-th rollout - default 1 - rank 0 calls aleppo_saliency on environment 0's
// horizon samples of the batch the context holds, with the grid stride saliency_stride - default 5 - and saliency_sigma_mask /
// saliency_sigma_blur - defaults 5 and 3 -, and writes <video dir>/saliency_<rollout>.y4m, the rollout counted from 1:
// trainer/saliency.hpp has the format - the newest frame as luma, the actor's saliency in blue, the critic's in red; it comes
// after the statistics above and before a recycle, so it shows the network the update left; never a collective; the four
// other keys without record_saliency, values aleppo_saliency would refuse and a library without the entry point are refused
// at start-up).  log_feature_rank: false (true: after the update of every feature_rank_interval-th rollout - default 1 - rank 0
// calls aleppo_feature_rank on the batch the context holds, with feature_rank_delta - default 0.01 -, feature_rank_eps -
// default 0.01 - and feature_rank_centered - default false -, and logs feature_rank/effective, /srank, /pca, /threshold,
// /stable, /numerical, /sigma_max, /sigma_min, /mean_sq_norm and /nonfinite_rows; it comes after the activation statistics
// and before a recycle, which changes the weights; never a collective: the figures describe rank 0's samples; the four other
// keys without log_feature_rank, values aleppo_feature_rank would refuse and a library without the entry point are refused
// at start-up).  log_policy_churn: false (true: on every policy_churn_interval-th rollout - default 1 - rank 0 calls
// aleppo_snapshot_take(ALEPPO_SET_LIVE) before the update and aleppo_policy_diff(ALEPPO_SET_SNAPSHOT, ALEPPO_SET_LIVE) after
// it, on the batch it trained on, and logs policy_churn/churn - the share of states whose greedy action the update changed,
// Schaul et al. 2022 -, /kl, /kl_reverse, /tv, /value_change - RMS -, /feature_cos and /feature_change;
// policy_churn_averaged: true, needs ema_decay, also logs policy_churn/ema_churn and /ema_kl from (ALEPPO_SET_AVERAGED,
// ALEPPO_SET_LIVE) after the EMA update; never a collective; the two other keys without log_policy_churn, a non-positive
// interval, policy_churn_averaged without ema_decay and a library without the entry points are refused at start-up).
// log_gradient_stats: false (true: BEFORE the update of every gradient_stats_interval-th rollout - default 1 - rank 0 probes
// the gradient of the first minibatch's samples without a step: aleppo_grad_probe with the loss as it stands at
// gradient_stats_small_batch samples - default a quarter of the minibatch - and at the whole minibatch, the policy term alone
// and the value term alone at the minibatch, aleppo_grad_take of Adam's first moment, and two aleppo_grad_gram calls; logs
// gradients/noise_scale - B_simple of McCandlish et al. 2018 with the unmasked counts as the batch sizes -,
// gradients/policy_value_cosine/conv1, /conv2, /conv3, /fc - the weight tensors - and /all, and gradients/momentum_cosine
// - not on the first update, where the moment is zero; likewise no noise scale where the two slices have the same unmasked
// count or the estimate of |G|^2 is not positive, and no cosine of a tensor whose gradient is zero; the probes change nothing the update reads, so the run is
// bit-identical to the run without the key; never a collective: rank 0's samples; the two other keys without
// log_gradient_stats, a non-positive interval, a small batch that is not smaller than the minibatch and a library without
// the entry points are refused at start-up).
// clip_param_final, value_loss_coef_final, entropy_coef_final,
// max_gradient_norm_final (absent: the value stays what the config says and no option is set; given: rollout i of
// num_rollouts updates with v0 + (v_final - v0) * i / num_rollouts, computed in double and rounded to float once - the
// shape of the learning-rate anneal, which never reaches its end value either - set through ALEPPO_OPT_CLIP_PARAM /
// _VALUE_LOSS_COEF / _ENTROPY_COEF / _MAX_GRAD_NORM before the update, logged under the key's own name (clip_param, ...)
// and recorded in the hparams; every rank computes the same values) and value_clip_range (a constant:
// ALEPPO_OPT_VALUE_CLIP_RANGE, SB3's clip_range_vf; needs clip_value_loss).  Values the options would refuse are
// refused when the config is loaded.  eval_interval (absent or 0: off; n: after the update of every n-th rollout, before the
// next rollout, the agent plays eval_episodes - default 10 - full episodes, life loss to life loss like the training
// episodes, on eval_environments - default 8 - SyntheticAtari instances of its own, seeded past every training
// environment of every rank, through the evaluation lanes: aleppo_eval_open / aleppo_eval_push_frames / aleppo_eval_act,
// stepped by the same worker pool) with eval_rule: greedy|sample|epsilon (default greedy), eval_temperature (default 1)
// and eval_epsilon (default 0.05); logs eval/episode_return_mean, eval/episode_return_max, eval/episode_length_mean and
// eval/episodes on the training scalars' step axis.  Each evaluation starts from freshly reset emulators and stacks, and
// the lanes change nothing the rollout or the update can observe: the training run is bit-identical to the run without
// the keys.  Under data parallelism every rank evaluates its own lanes and rank 0's are logged.
// reward_scaling: false (true: ALEPPO_OPT_REWARD_SCALE - every rollout's rewards are divided by the running standard
// deviation of the per-environment discounted return and clipped at +-reward_scale_clip, default 10, instead of being
// clamped to +-1, so 1 and 4 points per brick stay 1 : 4; logs reward_scale, return_rms_std and rewards_clipped per
// rollout).  A reward_scale_clip that is not finite and positive, or given without reward_scaling, is refused when the
// config is loaded; a build whose library lacks the entry points refuses reward_scaling: true at start-up.
// checkpoint_path: <file> (absent: the run is unchanged), checkpoint_interval: n (needs checkpoint_path; n > 0: the whole run
// state - parameters, Adam state, reward-scale state, the rollout's frame stacks and sampling counter, and this trainer's
// own bookkeeping down to every emulator's fields - is written after the update of every n-th rollout and after the last
// one, to <file>.tmp and then renamed; the four words of aleppo_state_digest are stored in the file and logged as hex) and
// resume: <file> (the run continues at the rollout the file was written before, bit for bit: the warm rollout is not
// repeated, and after the import the digest is computed again and compared with the file's, a mismatch being fatal).
// Under data parallelism every rank writes and reads <file>.rank<r>.  A resume file that is missing, truncated, of another
// format version or written for another shape (environments, horizon, actions, hidden size, precision, world size, rank)
// is refused before anything is created; a library without the entry points refuses the three keys at start-up.
// device_environments: false (true: the training environments are the library's device-resident SyntheticAtari instances,
// seeded like this trainer's own - environment i of the run is seed i - and a rollout is aleppo_env_rollout +
// aleppo_finish_rollout: nothing comes back to the host between slots, slot_ahead and the worker pool are not used for
// training, and the episode log and the step / episode counters come from the library's log planes and the exported
// environment state.  The run is the run with host environments, bit for bit, and so is the checkpoint file: save exports
// the device state into the fields the host emulators are saved in, resume imports them, and a file written in one mode
// resumes in the other.  Evaluation keeps its host emulators and lanes unless device_evaluation is set.  A library without
// the entry points refuses the key at start-up).
// device_evaluation: false (true, needs eval_interval: each evaluation's environments are the library's device-resident
// ones behind the lanes - aleppo_eval_env_open with the seed base the host path uses, then aleppo_eval_env_run in chunks of
// device_evaluation_steps, default 32, in [1, 1024], until eval_episodes are in hand, taken from the log planes in
// step-then-lane order: the first eval_episodes to finish, as the host path takes them.  No host emulators, no worker-pool
// pass and no mapped frame buffer exist for evaluation then.  The device runs up to device_evaluation_steps - 1 steps past
// the step the host path stops at, on environments that are thrown away; the evaluation counter is set back to where the
// host path would have left it - aleppo_eval_set_counter - so that every later evaluation draws what it draws there and
// the eval/* scalars are the host path's bit for bit.  A library without the entry points refuses the key at start-up).
// record_video: true with device_environments: true (without it the key is only noted, as before: the host emulators are
// not recorded): environment 0 of rank 0 is followed by the library's episode recorder (aleppo_rec_open, capacity =
// horizon, drained and cleared after every aleppo_env_rollout) and every episode is written into <video dir> as
// episode_<n>.y4m (uncompressed YUV4MPEG2, no ffmpeg) and episode_<n>.tsv (one line per step), n counting from 1 and, in a
// resumed run, on from the highest n in the directory; record_observation: true records the 84x84 observation the network
// sees instead of the frames the emulator renders (the reference's choice, rollout.cc:150-157).  record_evaluation: false
// (true, needs device_evaluation: the same for lane 0 of every evaluation, files eval_<step>_episode_<n>, the unfinished
// episode at an evaluation's end discarded).  record_interval: 1 (N: only episodes 1, N + 1, 2 N + 1, ... are written; every
// step's 32-byte record is read, the frames of the other episodes never leave the device).  recorder.hpp has the formats.
// The recorders change nothing the run computes; a library without the entry points refuses the keys at start-up.
// ema_decay: <d> (absent: off; 0 <= d < 1: an exponentially averaged copy of the parameters - aleppo_ema_open once the
// parameters are loaded or resumed, one aleppo_ema_update after the update of every trained rollout, never after the warm
// rollout; ema_warmup: true runs update n, n the updates so far, with min(ema_decay, (1 + n) / (10 + n)), the TensorFlow /
// timm rule; eval_averaged: true, needs eval_interval, evaluates the averaged policy - ALEPPO_OPT_EVAL_PARAMS = 1 - host-driven
// or device_evaluation alike; logs ema_decay, ema_distance and ema_relative_distance per rollout; with checkpoint_path the
// averaged parameters and their update count go into the optional section 7, which a resume with the key imports and proves
// by exporting it again, and without which the average starts at the resumed parameters; never a collective; the two other
// keys without ema_decay, a decay outside [0, 1) and a library without the entry points are refused at start-up).
// weight_decay: <wd> (absent or 0: off; ALEPPO_OPT_WEIGHT_DECAY, torch.optim.AdamW's decoupled decay inside every optimizer
// step).  l2_init_coef: <la> (absent or 0: off; L2 Init, Kumar et al. 2023 - ALEPPO_OPT_ANCHOR_COEF with the INITIAL parameters
// as the anchor: aleppo_anchor_take(live) once, right after the initial parameters are loaded and before the first update;
// with checkpoint_path the anchor goes into the optional section 8, which a resume with the key REQUIRES, imports and proves
// by exporting it again, and which a run without the key ignores).  shrink_perturb_interval: <n> (absent: off; Ash & Adams
// 2020 - after the update of every n-th rollout, after a recycle, aleppo_shrink_perturb with shrink_perturb_shrink - default
// 1 - and shrink_perturb_sigma - default 0 - and the key splitmix64(seed ^ rollout index), the way recycle_dormant derives
// its key, so a resumed run replays the same perturbations; the moments are kept).  Under data parallelism every rank
// computes the same values, anchor and keys; none of the calls is a collective.  Negative or non-finite values, the two
// other shrink_perturb keys without the interval and a library without the entry points are refused at start-up.
// recompute_advantages: false (true: Andrychowicz et al. 2021, choice C.5 - the update runs one epoch per aleppo_train call,
// as with target_kl, and every rank calls aleppo_refresh_advantages on the live parameters before every epoch but the first,
// so each later epoch trains on advantages and returns recomputed from the current critic; an early target_kl stop leaves no
// trailing refresh; rank 0 logs its last refresh of the update as refresh/explained_variance, refresh/value_change_std and
// refresh/value_change_maxabs; a library without the entry point refuses the key at start-up).
// Data parallelism (no reference counterpart): start one process per GPU with RANK / WORLD_SIZE / LOCAL_RANK
// in the environment (torchrun / mpirun style).  Rank r owns the contiguous environment block
// [r * E / W, (r + 1) * E / W) and GPU LOCAL_RANK; rank 0 creates the RCCL id, hands it to the others through the file
// <log path>.rcclid, and is the only rank that writes the event file (its own environments' episode statistics, the
// global - all-reduced - update metrics).  Everything else is unchanged: aleppo_train all-reduces the gradients.
// The pieces: config.hpp (keys, defaults and what follows from them), emulator.hpp (the synthetic game and the environment
// set the workers step), pool.hpp, events.hpp, profile.hpp, init.hpp, checkpoint.hpp (the file and what it holds).  This
// file is the run itself: its state, its phases, and main() putting them in order.
#include "../include/aleppo.h"
#include "checkpoint.hpp"
#include "config.hpp"
#include "events.hpp"
#include "init.hpp"
#include "pool.hpp"
#include "profile.hpp"
#include "recorder.hpp"
#include "saliency.hpp"
#include <cstdio>
#include <iostream>
#include <numeric>
#include <optional>
#include <thread>

// These entry points are weak: a build linked against a library without them (the host-only stand-in of the
// ThreadSanitizer build) still links, and a config that asks for them is then refused at start-up.  The evaluation lanes
// (eval_interval) ...
#pragma weak aleppo_eval_open
#pragma weak aleppo_eval_push_frames
#pragma weak aleppo_eval_act
#pragma weak aleppo_eval_read
// ... the reward-scaling state (reward_scaling: true) ...
#pragma weak aleppo_export_reward_scale
#pragma weak aleppo_import_reward_scale
// ... and what a checkpoint needs (checkpoint_path / checkpoint_interval / resume)
#pragma weak aleppo_export_optimizer
#pragma weak aleppo_import_optimizer
#pragma weak aleppo_export_rollout_state
#pragma weak aleppo_import_rollout_state
#pragma weak aleppo_state_digest
// ... and the device-resident environments (device_environments: true)
#pragma weak aleppo_env_open
#pragma weak aleppo_env_rollout
#pragma weak aleppo_env_export_state
#pragma weak aleppo_env_import_state
#pragma weak aleppo_env_read
// ... and the per-tensor statistics (log_tensor_stats: true)
#pragma weak aleppo_tensor_stats
// ... and the per-unit activation statistics (log_activation_stats: true)
#pragma weak aleppo_activation_stats
// ... and the recycling of dormant units (recycle_dormant: true)
#pragma weak aleppo_recycle_dormant
// ... and the feature rank (log_feature_rank: true)
#pragma weak aleppo_feature_rank
// ... and the policy churn (log_policy_churn: true)
#pragma weak aleppo_refresh_advantages
#pragma weak aleppo_snapshot_take
#pragma weak aleppo_policy_diff
// ... and the gradient probes (log_gradient_stats: true)
#pragma weak aleppo_grad_probe
#pragma weak aleppo_grad_take
#pragma weak aleppo_grad_gram
// (record_saliency: true - aleppo_saliency is declared weak in saliency.hpp)
// ... and the exponentially averaged parameters (ema_decay)
#pragma weak aleppo_ema_open
#pragma weak aleppo_ema_update
#pragma weak aleppo_ema_read
#pragma weak aleppo_ema_export
#pragma weak aleppo_ema_import
// ... and the anchor and shrink and perturb (l2_init_coef, shrink_perturb_interval)
#pragma weak aleppo_anchor_take
#pragma weak aleppo_anchor_import
#pragma weak aleppo_anchor_export
#pragma weak aleppo_shrink_perturb
// ... and the device-resident evaluation environments (device_evaluation: true)
#pragma weak aleppo_eval_env_open
#pragma weak aleppo_eval_env_run
#pragma weak aleppo_eval_env_export_state
#pragma weak aleppo_eval_env_import_state
#pragma weak aleppo_eval_env_read
#pragma weak aleppo_eval_set_counter

static void check(aleppo_ctx *ctx, int rc) { // the reference throws at the same places
  if (rc == ALEPPO_OK)
    return;
  const char *m = aleppo_last_error(ctx);
  if (rc == ALEPPO_ERR_INVALID_ARGUMENT)
    throw std::invalid_argument(m ? m : "invalid argument");
  throw std::runtime_error(m ? m : "aleppo error");
}
template <class T> static float meanf(const std::vector<T> &v) {
  return v.empty() ? 0.f : (float)(std::accumulate(v.begin(), v.end(), 0.0) / (double)v.size());
}

static void set_float_option(aleppo_ctx *ctx, int option, float v) { // (the options take the binary32 bit pattern)
  int32_t bits;
  std::memcpy(&bits, &v, 4);
  check(ctx, aleppo_set_option(ctx, option, bits));
}
static int env_int(const char *k, int dflt) {
  const char *v = std::getenv(k);
  return v ? std::atoi(v) : dflt;
}

// ------------------------------------------------------------------ the run's state: what every phase below works on
struct Run {
  const int64_t start_time = std::chrono::system_clock::now().time_since_epoch().count();
  const std::string rom_path, log_arg, video_dir, group;
  Profile prof; // the optional 6th argument (train.cc:328-335)
  const Config cfg;
  std::string log_path;
  const int world = std::max(1, env_int("WORLD_SIZE", 1)), rank = env_int("RANK", 0),
            local_rank = env_int("LOCAL_RANK", rank);
  size_t E = 0, T = 0, A = 0, env0 = 0; // E: THIS rank's environments, env0: its first one
  std::string ckpt_file, resume_file;   // (per rank under data parallelism)
  CkptShape shape{};
  Checkpoint resumed;
  aleppo_ctx *ctx = nullptr;
  std::optional<EventWriter> logger;
  TrainerState st{0}; // counters, kl_beta, the training environment set and its slot bookkeeping: what a checkpoint keeps
  uint8_t *start_mapped = nullptr; // episode-start flags at slot entry, where the armed ingest kernel reads them
  bool slot_ahead = false;
  std::vector<HyperSchedule> schedules;
  EnvSet eval_set; // the evaluation lanes' environments (empty without eval_interval, and with device_evaluation)
  uint8_t lut[256]; // the gray table the library was given (device_preprocess), for the recorded raw pairs
  std::optional<EpisodeWriter> video; // record_video with device_environments: environment 0 of rank 0
  bool record_training() const { return cfg.record_video && cfg.device_environments && rank == 0; }
  bool record_evaluation() const { return cfg.record_evaluation && rank == 0; }
  int record_field() const { return cfg.record_observation ? ALEPPO_REC_F_OBSERVATIONS : ALEPPO_REC_F_FRAMES; }
  uint64_t eval_counter = 0; // device_evaluation: the evaluation counter where the host path would have left it
  uint64_t ema_updates = 0;  // ema_decay: the average's updates so far (ema_warmup's n; resumed from the checkpoint)
  size_t first_rollout = 0, rollouts_done = 0;
  std::optional<WorkerPool> pool; // (last: its threads are joined before anything they touch goes away)

  // load and validate: the arguments, the config, the launch (RANK / WORLD_SIZE) and the shapes that follow
  Run(int argc, char **argv)
      : rom_path(argv[1]), log_arg(argv[2]), video_dir(argv[3]), group(argv[4]), prof(argc > 6 ? argv[6] : ""), cfg(load_config(argv[5])),
        log_path(argv[2]) {
    { // replace_extension("tfevents.<start-time>") like train.cc:324-325
      const size_t slash = log_path.find_last_of('/'), dot = log_path.find_last_of('.');
      if (dot != std::string::npos && (slash == std::string::npos || dot > slash))
        log_path = log_path.substr(0, dot);
      log_path += ".tfevents." + std::to_string(start_time);
    }
    { // train.cc:347-352: create the log (and video) directories
      const auto parent = std::filesystem::path(log_path).parent_path();
      if (!parent.empty() && !std::filesystem::exists(parent))
        std::filesystem::create_directories(parent);
    }
    if (rank < 0 || rank >= world)
      throw std::runtime_error("RANK must be in [0, WORLD_SIZE)");
    if (cfg.total_environments % (size_t)world)
      throw std::runtime_error("total_environments must be divisible by WORLD_SIZE");
    E = cfg.total_environments / (size_t)world, T = cfg.horizon, A = cfg.action_size;
    env0 = (size_t)rank * E;
    if ((E * T) % (size_t)cfg.num_mini_batches)
      throw std::runtime_error("Batch size must be divisible by num_mini_batches");
    if (E % cfg.worker_batch_size)
      std::cerr << "warning: total_environments % worker_batch_size != 0 would deadlock the reference's queue\n";
    if (cfg.log_gradient_stats) { // (the minibatch is this rank's: known only here)
      const size_t B = E * T / (size_t)cfg.num_mini_batches;
      if (cfg.gradient_stats_small_batch >= B || B < 2)
        throw std::runtime_error("gradient_stats_small_batch must be smaller than the minibatch (" + std::to_string(B) +
                                 " samples)");
    }
    if (cfg.recycle_dormant && world > 1) // (each rank would score its own samples and recycle its own units)
      throw std::runtime_error("recycle_dormant needs WORLD_SIZE 1: the dormancy scores describe one rank's samples");
    if (cfg.record_video && !cfg.device_environments)
      std::cerr << "note: record_video ignored (it needs device_environments: true; the host emulators are not recorded)\n";
    const std::string rank_suffix = world > 1 ? ".rank" + std::to_string(rank) : "";
    ckpt_file = cfg.checkpoint_path.empty() ? "" : cfg.checkpoint_path + rank_suffix;
    resume_file = cfg.resume.empty() ? "" : cfg.resume + rank_suffix;
    shape = CkptShape{(uint32_t)E, (uint32_t)T, (uint32_t)A, (uint32_t)cfg.hidden_size, (uint32_t)precision_of(cfg),
                      (uint32_t)world, (uint32_t)rank, 0, (uint64_t)reference_param_count(cfg.hidden_size, A)};
    slot_ahead = cfg.slot_ahead && !prof.on(); // (per-kernel device profiling brackets every launch)
    schedules = hyper_schedules_of(cfg);
    st = TrainerState(E);
    st.kl_beta = cfg.kl_coef > 0 ? (float)cfg.kl_coef : 0.0f; // set before every update, adapted after it (kl_target)
  }
  bool kl_penalty() const { return cfg.kl_coef > 0; }
  size_t n_params() const { return (size_t)shape.param_count; }
  std::vector<float> initial_params() const {
    return init_params(cfg.hidden_size, A, cfg.deterministic ? 42 : (uint64_t)start_time);
  }
};

// ------------------------------------------------------------------ before anything is created: what cannot be served
// checkpoint / resume: refused here when the library or the file cannot serve it
static void open_checkpoint_files(Run &run) {
  const bool ckpt_keys = !run.cfg.checkpoint_path.empty() || !run.cfg.resume.empty();
  if (ckpt_keys && !(aleppo_export_rollout_state && aleppo_import_rollout_state && aleppo_state_digest &&
                     aleppo_export_optimizer && aleppo_import_optimizer && aleppo_export_reward_scale &&
                     aleppo_import_reward_scale))
    throw std::runtime_error("checkpoint_path / checkpoint_interval / resume are set but this build's library cannot "
                             "checkpoint a run (aleppo_export_rollout_state is missing)");
  if (!run.resume_file.empty()) {
    run.resumed = read_checkpoint_file(run.resume_file);
    check_checkpoint_shape(run.resume_file, run.resumed, run.shape);
  }
}
static bool dump_initial_params(const Run &run) { // test hook: the initial parameters, no GPU needed
  const char *dump = std::getenv("ALEPPO_TRAINER_DUMP_INIT");
  if (!dump)
    return false;
  const std::vector<float> p = run.initial_params();
  std::ofstream f(dump, std::ios::binary);
  f.write(reinterpret_cast<const char *>(p.data()), (std::streamsize)(p.size() * sizeof(float)));
  std::cout << "initial parameters written: " << p.size() << std::endl;
  return true;
}
static void refuse_missing_entry_points(const Config &cfg) {
  if (cfg.eval_interval > 0 && !(aleppo_eval_open && aleppo_eval_push_frames && aleppo_eval_act && aleppo_eval_read))
    throw std::runtime_error("eval_interval is set but this build's library has no evaluation lanes "
                             "(aleppo_eval_open is missing)");
  if (cfg.reward_scaling && !(aleppo_export_reward_scale && aleppo_import_reward_scale))
    throw std::runtime_error("reward_scaling is set but this build's library has no reward scaling "
                             "(aleppo_export_reward_scale is missing)");
  if (cfg.device_environments && !(aleppo_env_open && aleppo_env_rollout && aleppo_env_export_state &&
                                   aleppo_env_import_state && aleppo_env_read))
    throw std::runtime_error("device_environments is set but this build's library has no device-resident environments "
                             "(aleppo_env_open is missing)");
  if (cfg.device_evaluation && !(aleppo_eval_env_open && aleppo_eval_env_run && aleppo_eval_env_export_state &&
                                 aleppo_eval_env_import_state && aleppo_eval_env_read && aleppo_eval_set_counter))
    throw std::runtime_error("device_evaluation is set but this build's library has no device-resident evaluation "
                             "environments (aleppo_eval_env_open is missing)");
  if (((cfg.record_video && cfg.device_environments) || cfg.record_evaluation) &&
      !(aleppo_rec_open && aleppo_rec_count && aleppo_rec_read && aleppo_rec_clear))
    throw std::runtime_error("record_video / record_evaluation are set but this build's library has no episode recorders "
                             "(aleppo_rec_open is missing)");
  if (cfg.log_tensor_stats && !aleppo_tensor_stats)
    throw std::runtime_error("log_tensor_stats is set but this build's library has no per-tensor statistics "
                             "(aleppo_tensor_stats is missing)");
  if (cfg.log_activation_stats && !aleppo_activation_stats)
    throw std::runtime_error("log_activation_stats is set but this build's library has no activation statistics "
                             "(aleppo_activation_stats is missing)");
  if (cfg.recycle_dormant && !aleppo_recycle_dormant)
    throw std::runtime_error("recycle_dormant is set but this build's library cannot recycle units "
                             "(aleppo_recycle_dormant is missing)");
  if (cfg.recompute_advantages && !aleppo_refresh_advantages)
    throw std::runtime_error("recompute_advantages is set but this build's library has no aleppo_refresh_advantages");
  if (cfg.ema_decay_set && !(aleppo_ema_open && aleppo_ema_update && aleppo_ema_read && aleppo_ema_export && aleppo_ema_import))
    throw std::runtime_error("ema_decay is set but this build's library has no averaged parameters "
                             "(aleppo_ema_open is missing)");
  if (cfg.l2_init_coef > 0 && !(aleppo_anchor_take && aleppo_anchor_import && aleppo_anchor_export))
    throw std::runtime_error("l2_init_coef is set but this build's library has no anchor (aleppo_anchor_take is missing)");
  if (cfg.shrink_perturb_interval && !aleppo_shrink_perturb)
    throw std::runtime_error("shrink_perturb_interval is set but this build's library cannot shrink and perturb "
                             "(aleppo_shrink_perturb is missing)");
  if (cfg.log_policy_churn && !(aleppo_snapshot_take && aleppo_policy_diff))
    throw std::runtime_error("log_policy_churn is set but this build's library has no policy churn "
                             "(aleppo_snapshot_take / aleppo_policy_diff are missing)");
  if (cfg.log_gradient_stats && !(aleppo_grad_probe && aleppo_grad_take && aleppo_grad_gram))
    throw std::runtime_error("log_gradient_stats is set but this build's library has no gradient probes "
                             "(aleppo_grad_probe / aleppo_grad_take / aleppo_grad_gram are missing)");
  if (cfg.log_feature_rank && !aleppo_feature_rank)
    throw std::runtime_error("log_feature_rank is set but this build's library has no feature rank "
                             "(aleppo_feature_rank is missing)");
  if (cfg.record_saliency && !aleppo_saliency)
    throw std::runtime_error("record_saliency is set but this build's library has no saliency maps "
                             "(aleppo_saliency is missing)");
}

// ------------------------------------------------------------------ start-up
static void create_context(Run &run) {
  const Config &cfg = run.cfg;
  aleppo_config ac{};
  ac.abi_version = ALEPPO_ABI_VERSION;
  ac.device_ordinal = run.local_rank;
  ac.world_size = run.world;
  ac.rank = run.rank;
  ac.num_envs = (int32_t)run.E;
  ac.horizon = (int32_t)run.T;
  ac.num_actions = (int32_t)run.A;
  ac.hidden_size = (int32_t)cfg.hidden_size;
  ac.frame_stack = (int32_t)cfg.frame_stack;
  ac.precision = precision_of(cfg);
  ac.rollout_precision = cfg.rollout_precision == "fp16" ? ALEPPO_ROLLOUT_FP16 : ALEPPO_ROLLOUT_FP32;
  ac.advantage_norm = cfg.advantage_norm;
  ac.gamma = cfg.gae_discount;
  ac.lambda = cfg.gae_lambda;
  ac.clip_param = cfg.clip_param;
  ac.value_loss_coef = cfg.value_loss_coef;
  ac.entropy_coef = cfg.entropy_coef;
  ac.max_gradient_norm = cfg.max_gradient_norm;
  ac.seed = cfg.seed;
  check(nullptr, aleppo_create(&ac, &run.ctx));
  std::cout << "MI355X is available! Training on GPU (rom argument '" << run.rom_path << "' -> synthetic emulator)."
            << std::endl;
}
// RCCL communicator: rank 0's 128-byte id travels through a file next to the log.  The file belongs to ONE launch: its name
// carries the launcher's MASTER_PORT (+ torchrun's run id when there is one), rank 0 removes whatever a crashed earlier
// launch left under that name BEFORE it creates the id and removes its own file once every rank has joined
// (aleppo_comm_init is collective), and the other ranks ignore a file older than their own start: a stale id would leave
// ncclCommInitRank waiting for ever on mismatched ids.
static void rendezvous(Run &run) {
  const int rank = run.rank, world = run.world;
  std::string nonce = std::getenv("MASTER_PORT") ? std::getenv("MASTER_PORT") : "0";
  if (const char *rid = std::getenv("TORCHELASTIC_RUN_ID"))
    nonce += std::string(".") + rid;
  const std::string idfile = run.log_arg + ".rcclid." + nonce;
  const auto proc_start = std::filesystem::file_time_type::clock::now();
  uint8_t id[ALEPPO_UNIQUE_ID_BYTES];
  if (rank == 0) {
    std::error_code ec;
    std::filesystem::remove(idfile, ec);
    for (int r = 1; r < world; ++r)
      std::filesystem::remove(idfile + ".ack." + std::to_string(r), ec);
    check(nullptr, aleppo_comm_unique_id(id));
    {
      std::ofstream f(idfile + ".tmp", std::ios::binary);
      f.write(reinterpret_cast<const char *>(id), sizeof(id));
      if (!f)
        throw std::runtime_error("cannot write " + idfile + ".tmp");
    }
    std::filesystem::rename(idfile + ".tmp", idfile); // atomic: a reader sees all 128 bytes or no file
  } else {
    const char *limit_s = std::getenv("ALEPPO_RENDEZVOUS_TIMEOUT_S");
    const double limit = limit_s ? std::atof(limit_s) : 300.0;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      std::error_code ec;
      const auto mt = std::filesystem::last_write_time(idfile, ec);
      // (ranks of one launch start within seconds of each other: anything written more than two minutes before this
      // process started is a leftover)
      if (!ec && mt + std::chrono::seconds(120) >= proc_start) {
        std::ifstream f(idfile, std::ios::binary);
        if (f && f.read(reinterpret_cast<char *>(id), sizeof(id))) {
          std::ofstream(idfile + ".ack." + std::to_string(rank)) << "read\n"; // rank 0 keeps the file until then
          break;
        }
      }
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit)
        throw std::runtime_error("rank " + std::to_string(rank) + " timed out after " + std::to_string((int)limit) +
                                 " s waiting for rank 0's communicator id in " + idfile +
                                 (ec ? " (no such file)" : " (only a stale file from an earlier launch)"));
      std::this_thread::sleep_for(std::chrono::milliseconds(50));
    }
  }
  check(run.ctx, aleppo_comm_init(run.ctx, id));
  if (rank == 0) { // remove the file once every rank has acknowledged reading it (bounded: a rank that died before
                   // it read the id has already failed the collective init above, or will fail the first all-reduce)
    const auto t0 = std::chrono::steady_clock::now();
    std::error_code ec;
    for (int r = 1; r < world; ++r) {
      const std::string ack = idfile + ".ack." + std::to_string(r);
      while (!std::filesystem::exists(ack, ec) && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(300))
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
      std::filesystem::remove(ack, ec);
    }
    std::filesystem::remove(idfile, ec);
  }
  std::cout << "rank " << rank << " of " << world << ": environments [" << run.env0 << ", " << run.env0 + run.E << ")"
            << std::endl;
}
static void load_initial_params(Run &run) {
  const std::vector<float> p = run.initial_params();
  size_t n = 0;
  check(run.ctx, aleppo_param_count(run.ctx, &n));
  if (n != p.size())
    throw std::runtime_error("parameter count mismatch");
  check(run.ctx, aleppo_load_params(run.ctx, p.data(), p.size()));
}
// every option the config switches on, once, before the first rollout (the scheduled ones are set per update)
static void apply_options(aleppo_ctx *ctx, const Config &cfg) {
  if (cfg.cuda_graph) // the reference's `cuda_graph: true`: replay the update loop as a captured graph
    check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_UPDATE_GRAPH, 1));
  if (cfg.shuffle_minibatches) // extension: minibatches of a fresh per-epoch permutation instead of contiguous slices
    check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_MINIBATCH_SHUFFLE, 1));
  if (cfg.clip_value_loss) // extension: the clipped value loss of ppo2 / CleanRL (clip range = clip_param)
    check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_VALUE_CLIP, 1));
  if (cfg.minibatch_advantage_norm) // extension: each minibatch's advantages normalised before the loss (norm_adv)
    check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_ADV_NORM_MINIBATCH, 1));
  if (cfg.kl_coef > 0) // extension: the KL penalty; beta is set before every update
    check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_KL_PENALTY, 1));
  if (cfg.value_clip_range_set) // extension: a value-clip range of its own (constant)
    set_float_option(ctx, ALEPPO_OPT_VALUE_CLIP_RANGE, (float)cfg.value_clip_range);
  if (cfg.reward_scaling) { // extension: rewards divided by the running return's std and clipped, not clamped to +-1
    set_float_option(ctx, ALEPPO_OPT_REWARD_SCALE_CLIP, (float)cfg.reward_scale_clip);
    check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_REWARD_SCALE, 1));
  }
}
// ---- Rollout host half (src/ai/rollout.cc): the emulators, their mapped buffers, the workers, the evaluation lanes
static void create_environments(Run &run) {
  const Config &cfg = run.cfg;
  const size_t E = run.E, fbytes = SyntheticAtari::frame_bytes(cfg.device_preprocess); // per environment
  EnvSet &set = run.st.set;
  for (size_t i = 0; i < E; ++i)
    set.envs.emplace_back(run.env0 + i + 0 /*seed arg of train.cc:380*/, cfg.max_steps, cfg.max_return, run.A,
                          cfg.device_preprocess);
  set.frame_bytes = run.eval_set.frame_bytes = fbytes;
  set.num_actions = run.eval_set.num_actions = run.A;
  // the workers' frame buffer: page-locked + GPU-mapped, read in place by the ingest kernel (see the file header)
  check(run.ctx, aleppo_host_alloc(run.ctx, E * fbytes, reinterpret_cast<void **>(&set.frames)));
  for (int i = 0; i < 256; ++i) // ALE's palette -> gray table would go here; the synthetic palette is its own gray value
    run.lut[i] = (uint8_t)i;
  if (cfg.device_preprocess)
    check(run.ctx, aleppo_set_gray_lut(run.ctx, run.lut));
  check(run.ctx, aleppo_host_alloc(run.ctx, E, reinterpret_cast<void **>(&run.start_mapped)));
  if (cfg.device_environments) { // the same E emulators on the device; the host instances above only hold checkpoint fields
    aleppo_env_config ec{};
    ec.kind = ALEPPO_ENV_SYNTHETIC;
    ec.frame_kind = frame_kind(cfg);
    ec.seed_base = run.env0;
    ec.max_steps = cfg.max_steps;
    ec.max_return = (float)cfg.max_return;
    check(run.ctx, aleppo_env_open(run.ctx, &ec));
    if (run.record_training()) { // environment 0's episodes: the reference's recorder choice (rollout.cc:150-157)
      aleppo_rec_config rc{};
      rc.source = ALEPPO_REC_ROLLOUT;
      rc.index = 0;
      rc.content = cfg.record_observation ? ALEPPO_REC_OBSERVATION : ALEPPO_REC_FRAMES;
      rc.capacity = (int32_t)run.T; // drained after every rollout: nothing is dropped
      check(run.ctx, aleppo_rec_open(run.ctx, &rc));
      run.video.emplace(run.video_dir, "episode_", ALEPPO_REC_ROLLOUT, run.record_field(),
                        cfg.device_preprocess && !cfg.record_observation, run.A, cfg.record_interval, run.lut, true);
    }
  }
  std::cout << "Creating " << cfg.num_workers << " worker threads." << std::endl;
  run.pool.emplace(cfg.num_workers);
  // evaluation (eval_interval): full episodes on emulators of its own through the evaluation lanes.  Nothing there touches
  // the training emulators, their flags or the rollout: the lanes have their own stacks, scratch and noise stream.
  if (const size_t L = cfg.eval_interval > 0 ? cfg.eval_environments : 0) {
    check(run.ctx, aleppo_eval_open(run.ctx, (int32_t)L));
    if (!cfg.device_evaluation) { // (device_evaluation: the lanes' environments are the library's, opened per evaluation)
      run.eval_set.start.assign(L, 1);
      run.eval_set.results.resize(L);
      run.eval_set.what = "evaluation environment";
      check(run.ctx, aleppo_host_alloc(run.ctx, L * fbytes, reinterpret_cast<void **>(&run.eval_set.frames)));
    }
  }
}

// ------------------------------------------------------------------ one rollout: collect
struct EpisodeLog {
  std::vector<float> episode_returns, game_returns;
  std::vector<size_t> episode_lengths, game_lengths;
};
// device_environments: the state of the library's environments <-> the fields a checkpoint keeps them in (TrainerState and
// its host SyntheticAtari instances, which are never stepped in that mode)
struct EnvFieldCopy {
  aleppo_env_state &s;
  bool to_host;
  template <class A, class B> void one(A &host, B &dev) {
    if (to_host)
      host = (A)dev;
    else
      dev = (B)host;
  }
  void operator()(uint64_t &rng, int &lives, int &paddle, int &ball_x, int &ball_y, int &prev_x, int &prev_y, int &dx, int &dy,
                  int &bricks, uint64_t &steps, float &episode_return) {
    one(rng, s.rng), one(lives, s.lives), one(paddle, s.paddle), one(ball_x, s.ball_x), one(ball_y, s.ball_y);
    one(prev_x, s.prev_x), one(prev_y, s.prev_y), one(dx, s.dx), one(dy, s.dy), one(bricks, s.bricks), one(steps, s.steps);
    one(episode_return, s.episode_return);
  }
};
static void copy_env_fields(TrainerState &st, std::vector<aleppo_env_state> &dev, bool to_host) {
  for (size_t i = 0; i < dev.size(); ++i) {
    EnvFieldCopy f{dev[i], to_host};
    st.set.envs[i].visit(f);
    f.one(st.set.start[i], dev[i].start), f.one(st.game_over[i], dev[i].game_over), f.one(st.rewards[i], dev[i].reward);
    f.one(st.ep_ret[i], dev[i].ep_ret), f.one(st.game_ret[i], dev[i].game_ret), f.one(st.ep_len[i], dev[i].ep_len);
    f.one(st.game_len[i], dev[i].game_len);
  }
}
static void pull_device_environments(Run &run) {
  std::vector<aleppo_env_state> dev(run.E);
  check(run.ctx, aleppo_env_export_state(run.ctx, dev.data(), dev.size()));
  copy_env_fields(run.st, dev, true);
}
static void push_device_environments(Run &run) {
  std::vector<aleppo_env_state> dev(run.E); // (zeroed: the reserved bytes)
  copy_env_fields(run.st, dev, false);
  check(run.ctx, aleppo_env_import_state(run.ctx, dev.data(), dev.size()));
}
// one rollout on the device's environments: the whole slot loop is one burst of enqueued kernels
static EpisodeLog collect_on_device(Run &run) {
  aleppo_ctx *ctx = run.ctx;
  TrainerState &st = run.st;
  const size_t n = run.E * run.T;
  {
    Profile::Span sp(&run.prof, "aleppo_env_rollout");
    check(ctx, aleppo_env_rollout(ctx));
  }
  {
    Profile::Span sp(&run.prof, "aleppo_finish_rollout");
    check(ctx, aleppo_finish_rollout(ctx, nullptr));
  }
  if (run.video) // this rollout's rows of environment 0 -> the episode files; the log is empty again afterwards
    run.video->drain(ctx, check);
  // the four [T][E] log planes in slot-then-environment order: the order the host loop appends in
  std::vector<float> ep_ret(n), game_ret(n);
  std::vector<uint32_t> ep_len(n), game_len(n);
  check(ctx, aleppo_env_read(ctx, ALEPPO_ENV_F_EPISODE_RETURNS, ep_ret.data(), n * 4));
  check(ctx, aleppo_env_read(ctx, ALEPPO_ENV_F_EPISODE_LENGTHS, ep_len.data(), n * 4));
  check(ctx, aleppo_env_read(ctx, ALEPPO_ENV_F_GAME_RETURNS, game_ret.data(), n * 4));
  check(ctx, aleppo_env_read(ctx, ALEPPO_ENV_F_GAME_LENGTHS, game_len.data(), n * 4));
  EpisodeLog log;
  // every non-start slot added one to its environment's episode length: the steps of this rollout are the lengths that
  // were logged plus what the running lengths grew by
  uint64_t steps = 0;
  for (uint64_t l : st.ep_len)
    steps -= l;
  for (size_t k = 0; k < n; ++k) {
    if (ep_len[k]) {
      st.episodes++;
      steps += ep_len[k];
      log.episode_returns.push_back(ep_ret[k]);
      log.episode_lengths.push_back(ep_len[k]);
    }
    if (game_len[k]) {
      log.game_returns.push_back(game_ret[k]);
      log.game_lengths.push_back(game_len[k]);
    }
  }
  pull_device_environments(run);
  for (uint64_t l : st.ep_len)
    steps += l;
  st.total_steps += steps;
  return log;
}
static EpisodeLog collect(Run &run) {
  if (run.cfg.device_environments)
    return collect_on_device(run);
  aleppo_ctx *ctx = run.ctx;
  TrainerState &st = run.st;
  EnvSet &set = st.set;
  const size_t E = run.E;
  const int fkind = frame_kind(run.cfg);
  EpisodeLog log;
  for (size_t t = 0; t < run.T; ++t) {
    {
      Profile::Span sp(&run.prof, "aleppo_act");
      check(ctx, aleppo_act(ctx, nullptr, &set.actions));
    }
    const std::vector<uint8_t> start_at_entry = set.start;
    if (run.slot_ahead) { // slot t + 1's kernels go onto the stream now; they start when release_step lifts the wait
      std::memcpy(run.start_mapped, start_at_entry.data(), E);
      check(ctx, aleppo_arm_step(ctx, set.frames, fkind, run.start_mapped, nullptr));
    }
    {
      Profile::Span sp(&run.prof, "step_all (emulator threads)");
      run.pool->run_all(E, [&set](size_t i) { set.step(i); });
    }
    for (size_t i = 0; i < E; ++i) {
      if (!set.start[i]) { // rollout.cc:214-226 (start slots keep the stale reward)
        const StepOut &o = set.results[i];
        st.rewards[i] = o.reward;
        st.term[i] = o.terminated;
        st.trunc[i] = o.truncated;
        st.game_over[i] = o.game_over;
        st.ep_ret[i] += o.reward;
        st.ep_len[i]++;
        st.game_ret[i] += o.reward;
        st.game_len[i]++;
        st.total_steps++;
      }
    }
    if (run.slot_ahead) {
      check(ctx, aleppo_release_step(ctx, st.rewards.data(), st.term.data(), st.trunc.data()));
    } else {
      Profile::Span sp(&run.prof, "aleppo_step");
      check(ctx, aleppo_step(ctx, set.frames, fkind, ALEPPO_HOST_MAPPED, st.rewards.data(), st.term.data(),
                             st.trunc.data(), start_at_entry.data()));
    }
    for (size_t i = 0; i < E; ++i) { // rollout.cc:239-265
      if (set.results[i].terminated || set.results[i].truncated) {
        set.start[i] = 1;
        st.term[i] = st.trunc[i] = 0;
        st.episodes++;
        log.episode_returns.push_back(st.ep_ret[i]);
        log.episode_lengths.push_back(st.ep_len[i]);
        st.ep_ret[i] = 0;
        st.ep_len[i] = 0;
        if (st.game_over[i]) {
          log.game_returns.push_back(st.game_ret[i]);
          log.game_lengths.push_back(st.game_len[i]);
          st.game_ret[i] = 0;
          st.game_len[i] = 0;
        }
      } else if (set.start[i]) {
        set.start[i] = 0;
      }
    }
  }
  {
    Profile::Span sp(&run.prof, "aleppo_finish_rollout");
    check(ctx, aleppo_finish_rollout(ctx, nullptr));
  }
  return log;
}

// ------------------------------------------------------------------ ... read its statistics
struct BatchStatistics {
  double reward_scale[ALEPPO_REWARD_SCALE_COUNT] = {}, return_rms[3] = {0.0, 0.0, 1.0};
  double batch[ALEPPO_BATCH_STATS_COUNT] = {};
};
static BatchStatistics read_statistics(Run &run) {
  BatchStatistics s;
  if (run.cfg.reward_scaling) { // what this rollout's finish_rollout did (the state is global under data parallelism)
    std::vector<double> running(run.E);
    check(run.ctx, aleppo_read_batch(run.ctx, ALEPPO_F_REWARD_SCALE, s.reward_scale, sizeof(s.reward_scale)));
    check(run.ctx, aleppo_export_reward_scale(run.ctx, s.return_rms, running.data(), running.size()));
  }
  if (run.cfg.log_batch_stats) { // of the rollout batch as the update will see it; every rank calls (collective)
    Profile::Span sp(&run.prof, "read_batch_stats");
    check(run.ctx, aleppo_read_batch(run.ctx, ALEPPO_F_BATCH_STATS, s.batch, sizeof(s.batch)));
  }
  return s;
}

// ------------------------------------------------------------------ ... update
static const std::pair<int, const char *> SAMPLE_FIELDS[5] = {{ALEPPO_M_TOTAL_LOSSES, "losses"},
                                                              {ALEPPO_M_CLIPPED_LOSSES, "clipped_losses"},
                                                              {ALEPPO_M_VALUE_LOSSES, "value_losses"},
                                                              {ALEPPO_M_ENTROPIES, "entropies"},
                                                              {ALEPPO_M_RATIO, "ratios"}};
// the rows of aleppo_tensor_stats: libtorch parameters() order, then the whole model
static const char *const TENSOR_STAT_NAMES[ALEPPO_TENSOR_STATS_ROWS] = {
    "conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc.w", "fc.b", "action.w", "action.b", "value.w",
    "value.b", "total"};
// the rows of aleppo_activation_stats' layer table
static const char *const ACT_LAYER_NAMES[ALEPPO_ACT_LAYER_ROWS] = {"conv1", "conv2", "conv3", "fc", "total"};
static uint64_t splitmix64(uint64_t x) { // the permutation of aleppo.h (aleppo_read_sample_order)
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// metrics of every epoch that ran: per minibatch, and the per-sample planes of log_data's histograms ([epochs][N])
struct Update {
  const size_t nmb, N, slots; // minibatches per epoch, samples per epoch, minibatch slots of num_epochs epochs
  std::vector<aleppo_minibatch_metrics> m;
  std::vector<float> kl, cf, adv_std, mean_kl;
  std::vector<std::vector<float>> planes;
  double lr = 0;
  std::vector<float> hyper_now; // this rollout's scheduled hyper-parameters, in run.schedules' order
  size_t epochs_run = 0;
  float kl_beta = 0;   // the beta this update ran with ...
  double last_kl = 0;  // ... and the mean exact KL over the minibatches of its last epoch
  double tensor_stats[ALEPPO_TENSOR_STATS_ROWS][ALEPPO_TENSOR_STATS_COLS] = {}; // log_tensor_stats, rank 0: after the update
  bool act_stats_read = false; // log_activation_stats, rank 0: this rollout is one of the interval's, act_layers is its table
  double act_layers[ALEPPO_ACT_LAYER_ROWS][ALEPPO_ACT_LAYER_COLS] = {};
  std::vector<double> act_units; // [(160 + H) * ALEPPO_ACT_UNIT_COLS] (the call fills it; only the layer table is logged)
  bool feature_rank_read = false; // log_feature_rank, rank 0: this rollout is one of the interval's, feature_rank holds it
  double feature_rank[ALEPPO_FR_COUNT] = {};
  bool churn_read = false; // log_policy_churn, rank 0: this rollout is one of the interval's, churn / ema_churn hold it
  double churn[ALEPPO_PD_COUNT] = {}, ema_churn[ALEPPO_PD_COUNT] = {};
  bool grad_read = false; // log_gradient_stats, rank 0: this rollout is one of the interval's, the fields below hold it
  double noise_scale = 0, pv_cosine[5] = {}, momentum_cosine = 0; // pv_cosine: conv1.w, conv2.w, conv3.w, fc.w, all
  // ... and which of them exist: the two counts differ and the estimate of |G|^2 is positive; neither norm of a tensor
  // is zero; the moment is not zero (a figure that does not exist is not logged)
  bool noise_read = false, pv_read[5] = {}, momentum_read = false;
  bool recycled = false; // recycle_dormant: this rollout is one of the interval's, recycle_counts is what it recycled
  int64_t recycle_counts[ALEPPO_RECYCLE_COUNTS] = {};
  bool refreshed = false; // recompute_advantages: a refresh ran in this update, refresh holds the last one's statistics
  double refresh[ALEPPO_REFRESH_STATS_COUNT] = {};
  double ema_decay_now = 0;                       // ema_decay: the decay this rollout's aleppo_ema_update ran with ...
  double ema_stats[ALEPPO_EMA_STATS_COUNT] = {};  // ... and the statistics it left
  explicit Update(const Run &run)
      : nmb((size_t)run.cfg.num_mini_batches), N(run.E * run.T), slots((size_t)run.cfg.num_epochs * nmb), m(slots),
        kl(slots), cf(slots), adv_std(run.cfg.minibatch_advantage_norm ? slots : 0), mean_kl(run.kl_penalty() ? slots : 0),
        planes(5, std::vector<float>((size_t)run.cfg.num_epochs * N)), hyper_now(run.schedules.size()) {}
  size_t nrun() const { return epochs_run * nmb; } // minibatches that ran
};
// log_gradient_stats: four probes of the first minibatch's samples, the moment, two Grams (the header's gradient probes);
// slots 0 .. 3 = the small slice (then the moment), the minibatch, the policy term alone, the value term alone
static void probe_gradients(Run &run, Update &u) {
  const Config &cfg = run.cfg;
  aleppo_ctx *ctx = run.ctx;
  Profile::Span sp(&run.prof, "aleppo_grad_probe");
  const int64_t B = (int64_t)(u.N / u.nmb);
  const int64_t small = cfg.gradient_stats_small_batch ? (int64_t)cfg.gradient_stats_small_batch : std::max<int64_t>(1, B / 4);
  int64_t b_small = 0, b_big = 0;
  check(ctx, aleppo_grad_probe(ctx, 0, 0, small, nullptr, &b_small));
  check(ctx, aleppo_grad_probe(ctx, 1, 0, B, nullptr, &b_big));
  const int32_t pair[2] = {0, 1}, all[4] = {0, 1, 2, 3};
  const size_t rows = ALEPPO_TENSOR_STATS_ROWS;
  double g2[ALEPPO_TENSOR_STATS_ROWS][2][2], g4[ALEPPO_TENSOR_STATS_ROWS][4][4];
  check(ctx, aleppo_grad_gram(ctx, pair, 2, &g2[0][0][0], rows * 4, nullptr, 0));
  // McCandlish et al. 2018, Appendix A, on the whole model: |G|^2 and S from the two squared norms, B_simple = S / |G|^2
  const double s2 = g2[rows - 1][0][0], l2 = g2[rows - 1][1][1], bs = (double)b_small, bl = (double)b_big;
  const double G2 = (bl * l2 - bs * s2) / (bl - bs), S = (s2 - l2) / (1.0 / bs - 1.0 / bl);
  u.noise_read = b_small > 0 && b_small < b_big && G2 > 0 && std::isfinite(S / G2);
  u.noise_scale = u.noise_read ? S / G2 : 0.0;
  const aleppo_grad_probe_config policy{1, 0.f, 0.f, 0}, value{0, 1.f, 0.f, 0};
  check(ctx, aleppo_grad_probe(ctx, 2, 0, B, &policy, nullptr));
  check(ctx, aleppo_grad_probe(ctx, 3, 0, B, &value, nullptr));
  check(ctx, aleppo_grad_take(ctx, 0, ALEPPO_GRAD_SRC_EXP_AVG, 0));
  check(ctx, aleppo_grad_gram(ctx, all, 4, &g4[0][0][0], rows * 16, nullptr, 0));
  static const int weight_rows[5] = {0, 2, 4, 6, ALEPPO_TENSOR_STATS_ROWS - 1};
  for (int k = 0; k < 5; ++k) {
    const auto &g = g4[weight_rows[k]];
    u.pv_read[k] = g[2][2] > 0 && g[3][3] > 0;
    u.pv_cosine[k] = u.pv_read[k] ? g[2][3] / std::sqrt(g[2][2] * g[3][3]) : 0.0;
  }
  const auto &g = g4[rows - 1];
  u.momentum_read = g[0][0] > 0 && g[1][1] > 0;
  u.momentum_cosine = u.momentum_read ? g[0][1] / std::sqrt(g[0][0] * g[1][1]) : 0.0;
}
static void update(Run &run, size_t r, Update &u) {
  const Config &cfg = run.cfg;
  aleppo_ctx *ctx = run.ctx;
  const size_t nmb = u.nmb, N = u.N;
  u.lr = cfg.learning_rate * (1.0 - r / static_cast<double>(cfg.num_rollouts)); // train.cc:424-428
  // one call of num_epochs epochs, or - with target_kl - one call per epoch until an epoch's last minibatch is over
  // the target (the Adam schedule and the shuffle keys follow the Adam step, so the calls add up to the same update)
  u.epochs_run = 0;
  // recompute_advantages: one call per epoch too, with aleppo_refresh_advantages on the live parameters in front of every
  // epoch but the first - on every rank (a collective under advantage_norm); an early stop leaves no trailing refresh
  const size_t per_call = (cfg.target_kl > 0 || cfg.recompute_advantages) ? 1 : (size_t)cfg.num_epochs;
  u.refreshed = false;
  for (size_t k = 0; k < run.schedules.size(); ++k) { // (a function of r alone: the same on every rank)
    u.hyper_now[k] = run.schedules[k].at(r, cfg.num_rollouts);
    set_float_option(ctx, run.schedules[k].option, u.hyper_now[k]);
  }
  u.kl_beta = run.st.kl_beta;
  if (run.kl_penalty())
    set_float_option(ctx, ALEPPO_OPT_KL_COEF, u.kl_beta);
  // the gradient as a direction, at the parameters this update starts from (not a collective: rank 0's samples; after the
  // options above, so that the probed loss is the one the update uses)
  u.grad_read = cfg.log_gradient_stats && run.rank == 0 && (r + 1) % cfg.gradient_stats_interval == 0;
  if (u.grad_read)
    probe_gradients(run, u);
  // policy churn: the parameters this update starts from, kept on the device (not a collective: rank 0's samples)
  u.churn_read = cfg.log_policy_churn && run.rank == 0 && (r + 1) % cfg.policy_churn_interval == 0;
  if (u.churn_read) {
    Profile::Span sp(&run.prof, "aleppo_snapshot_take");
    check(ctx, aleppo_snapshot_take(ctx, ALEPPO_SET_LIVE));
  }
  while (u.epochs_run < (size_t)cfg.num_epochs) {
    const size_t e0 = u.epochs_run;
    if (cfg.recompute_advantages && e0 > 0) {
      Profile::Span sp(&run.prof, "aleppo_refresh_advantages");
      check(ctx, aleppo_refresh_advantages(ctx, ALEPPO_SET_LIVE, u.refresh, ALEPPO_REFRESH_STATS_COUNT));
      u.refreshed = true;
    }
    {
      Profile::Span sp(&run.prof, "aleppo_train");
      check(ctx, aleppo_train(ctx, u.lr, (int)per_call, (int)nmb, u.m.data() + e0 * nmb));
    }
    Profile::Span sp_read(&run.prof, "read_train_metrics");
    check(ctx, aleppo_read_train_metric(ctx, ALEPPO_M_MEAN_APPROX_KL, u.kl.data() + e0 * nmb, per_call * nmb));
    check(ctx, aleppo_read_train_metric(ctx, ALEPPO_M_MEAN_CLIP_FRACTION, u.cf.data() + e0 * nmb, per_call * nmb));
    if (cfg.minibatch_advantage_norm)
      check(ctx, aleppo_read_train_metric(ctx, ALEPPO_M_ADV_STD, u.adv_std.data() + e0 * nmb, per_call * nmb));
    if (run.kl_penalty())
      check(ctx, aleppo_read_train_metric(ctx, ALEPPO_M_MEAN_KL, u.mean_kl.data() + e0 * nmb, per_call * nmb));
    for (size_t k = 0; k < 5; ++k)
      check(ctx, aleppo_read_train_metric(ctx, SAMPLE_FIELDS[k].first, u.planes[k].data() + e0 * N, per_call * N));
    u.epochs_run += per_call;
    if (cfg.target_kl > 0 && u.kl[u.epochs_run * nmb - 1] > cfg.target_kl)
      break;
  }
  if (run.kl_penalty()) { // the adaptive KL coefficient (PPO paper section 4) from the last epoch's mean exact KL
    double d = 0;
    for (size_t i = u.nrun() - nmb; i < u.nrun(); ++i)
      d += u.mean_kl[i];
    u.last_kl = d /= (double)nmb;
    float &beta = run.st.kl_beta;
    if (cfg.kl_target > 0) {
      if (d < cfg.kl_target / 1.5)
        beta = std::max(0.5f * beta, std::min(beta, KL_BETA_MIN));
      else if (d > 1.5 * cfg.kl_target && std::isfinite(2.0f * beta))
        beta *= 2.0f;
    }
  }
  // the averaged parameters follow every trained rollout's update (never a collective: the parameters are replicated bit for
  // bit, so every rank computes the same average); ema_warmup: the TensorFlow / timm rule on the updates so far
  if (cfg.ema_decay_set) {
    Profile::Span sp(&run.prof, "aleppo_ema_update");
    const double n = (double)run.ema_updates;
    u.ema_decay_now = cfg.ema_warmup ? std::min(cfg.ema_decay, (1.0 + n) / (10.0 + n)) : cfg.ema_decay;
    check(ctx, aleppo_ema_update(ctx, u.ema_decay_now));
    run.ema_updates++;
    check(ctx, aleppo_ema_read(ctx, u.ema_stats));
  }
  // ... and how far the update moved the policy, the value and the features on the batch it trained on
  if (u.churn_read) {
    Profile::Span sp(&run.prof, "aleppo_policy_diff");
    check(ctx, aleppo_policy_diff(ctx, nullptr, 0, ALEPPO_SET_SNAPSHOT, ALEPPO_SET_LIVE, u.churn, ALEPPO_PD_COUNT, nullptr, 0,
                                  nullptr, 0, nullptr, 0));
    if (cfg.policy_churn_averaged) // (after the EMA update above: the averaged policy against the live one)
      check(ctx, aleppo_policy_diff(ctx, nullptr, 0, ALEPPO_SET_AVERAGED, ALEPPO_SET_LIVE, u.ema_churn, ALEPPO_PD_COUNT,
                                    nullptr, 0, nullptr, 0, nullptr, 0));
  }
  if (cfg.log_tensor_stats && run.rank == 0) { // (not a collective: every rank's answer would be the same)
    Profile::Span sp(&run.prof, "aleppo_tensor_stats");
    check(ctx, aleppo_tensor_stats(ctx, ALEPPO_TS_SEC_PARAMS | ALEPPO_TS_SEC_STEP, &u.tensor_stats[0][0],
                                   (size_t)ALEPPO_TENSOR_STATS_ROWS * ALEPPO_TENSOR_STATS_COLS));
  }
  u.act_stats_read = cfg.log_activation_stats && run.rank == 0 && (r + 1) % cfg.activation_stats_interval == 0;
  if (u.act_stats_read) { // (not a collective: rank 0's samples, the batch this update trained on, under the new weights)
    Profile::Span sp(&run.prof, "aleppo_activation_stats");
    u.act_units.resize((size_t)(160 + cfg.hidden_size) * ALEPPO_ACT_UNIT_COLS);
    check(ctx, aleppo_activation_stats(ctx, nullptr, 0, cfg.dormant_tau, u.act_units.data(), u.act_units.size(),
                                       &u.act_layers[0][0], (size_t)ALEPPO_ACT_LAYER_ROWS * ALEPPO_ACT_LAYER_COLS));
  }
  // the feature rank of the batch this update trained on, under the new weights (not a collective: rank 0's samples)
  u.feature_rank_read = cfg.log_feature_rank && run.rank == 0 && (r + 1) % cfg.feature_rank_interval == 0;
  if (u.feature_rank_read) {
    Profile::Span sp(&run.prof, "aleppo_feature_rank");
    check(ctx, aleppo_feature_rank(ctx, nullptr, 0, &cfg.feature_rank, u.feature_rank, ALEPPO_FR_COUNT, nullptr, 0, nullptr,
                                   0, nullptr, 0));
  }
  // the saliency video of environment 0: the batch this update trained on, under the new weights (not a collective)
  if (cfg.record_saliency && run.rank == 0 && (r + 1) % cfg.saliency_interval == 0) {
    Profile::Span sp(&run.prof, "aleppo_saliency");
    write_saliency_y4m(ctx, check, run.video_dir, r + 1, run.E, run.T, cfg.saliency);
  }
  // ReDo: score the units on the batch this update trained on, under the new weights, and recycle the dormant ones - after
  // the statistics above have described the update that ran (aleppo_tensor_stats refuses the step section after a recycle)
  // and before this iteration's checkpoint and digest; the key is a function of the seed
  // and the rollout index alone, so a resumed run replays the same recycles
  u.recycled = cfg.recycle_dormant && (r + 1) % cfg.recycle_interval == 0;
  if (u.recycled) {
    Profile::Span sp(&run.prof, "aleppo_recycle_dormant");
    check(ctx, aleppo_recycle_dormant(ctx, nullptr, 0, cfg.recycle_tau, cfg.recycle_layers,
                                      splitmix64(cfg.seed ^ (uint64_t)r), 0, nullptr, (size_t)(160 + cfg.hidden_size),
                                      u.recycle_counts));
  }
  // shrink and perturb: after the statistics and a recycle, before this iteration's checkpoint and digest; the key as above
  if (cfg.shrink_perturb_interval && (r + 1) % cfg.shrink_perturb_interval == 0) {
    Profile::Span sp(&run.prof, "aleppo_shrink_perturb");
    check(ctx, aleppo_shrink_perturb(ctx, cfg.shrink_perturb_shrink, cfg.shrink_perturb_sigma,
                                     splitmix64(cfg.seed ^ (uint64_t)r), 0));
  }
}

// ------------------------------------------------------------------ ... log (log_data, train.cc:163-210)
static void log_scalars(Run &run, const EpisodeLog &log, const BatchStatistics &s, const Update &u, int64_t step) {
  const Config &cfg = run.cfg;
  EventWriter &logger = *run.logger;
  auto finished = [&](const std::string &kind, const std::vector<float> &returns, const std::vector<size_t> &lengths) {
    logger.add_scalar("mean_" + kind + "_return", step, meanf(returns));
    logger.add_scalar("mean_" + kind + "_length", step, meanf(lengths));
    logger.add_histogram(kind + "_returns", step, returns);
    logger.add_histogram(kind + "_lengths", step, std::vector<float>(lengths.begin(), lengths.end()));
  };
  if (!log.episode_returns.empty()) {
    finished("episode", log.episode_returns, log.episode_lengths);
    if (!log.game_returns.empty())
      finished("game", log.game_returns, log.game_lengths);
  }
  const size_t nrun = u.nrun();
  auto avg = [&](float aleppo_minibatch_metrics::*f) {
    double sum = 0;
    for (size_t i = 0; i < nrun; ++i)
      sum += u.m[i].*f;
    return (float)(sum / (double)nrun);
  };
  auto avgv = [&](const std::vector<float> &x) { // (computed like mean_ratio)
    double sum = 0;
    for (size_t i = 0; i < nrun; ++i)
      sum += x[i];
    return (float)(sum / (double)nrun);
  };
  logger.add_scalar("mean_clipped_gradient", step, avg(&aleppo_minibatch_metrics::grad_norm));
  logger.add_scalar("mean_loss", step, avg(&aleppo_minibatch_metrics::loss));
  logger.add_scalar("mean_clipped_loss", step, avg(&aleppo_minibatch_metrics::clipped_loss));
  logger.add_scalar("mean_value_loss", step, avg(&aleppo_minibatch_metrics::value_loss));
  logger.add_scalar("mean_entropy", step, avg(&aleppo_minibatch_metrics::entropy));
  logger.add_scalar("mean_ratio", step, avg(&aleppo_minibatch_metrics::ratio));
  logger.add_scalar("mean_approx_kl", step, avgv(u.kl));
  logger.add_scalar("mean_clip_fraction", step, avgv(u.cf));
  if (cfg.minibatch_advantage_norm) // (the std each minibatch's advantages were divided by, before the 1e-8)
    logger.add_scalar("mean_advantage_std", step, avgv(u.adv_std));
  if (cfg.target_kl > 0)
    logger.add_scalar("update_epochs", step, (float)u.epochs_run);
  if (run.kl_penalty()) {
    logger.add_scalar("kl_coef", step, u.kl_beta);
    logger.add_scalar("mean_kl", step, (float)u.last_kl);
  }
  if (cfg.reward_scaling) { // (rewards_clipped: rank 0's environments)
    logger.add_scalar("reward_scale", step, (float)s.reward_scale[ALEPPO_RS_SCALE]);
    logger.add_scalar("return_rms_std", step, (float)std::sqrt(s.return_rms[2]));
    logger.add_scalar("rewards_clipped", step, (float)s.reward_scale[ALEPPO_RS_CLIPPED]);
  }
  if (cfg.log_batch_stats) { // (global statistics under data parallelism; a NaN explained variance is logged as NaN)
    logger.add_scalar("explained_variance", step, (float)s.batch[ALEPPO_BS_EXPLAINED_VARIANCE]);
    logger.add_scalar("mean_value", step, (float)s.batch[ALEPPO_BS_VALUE_MEAN]);
    logger.add_scalar("std_value", step, (float)s.batch[ALEPPO_BS_VALUE_STD]);
    logger.add_scalar("mean_return", step, (float)s.batch[ALEPPO_BS_RETURN_MEAN]);
    logger.add_scalar("std_return", step, (float)s.batch[ALEPPO_BS_RETURN_STD]);
    logger.add_scalar("mean_advantage", step, (float)s.batch[ALEPPO_BS_ADVANTAGE_MEAN]);
    logger.add_scalar("std_advantage", step, (float)s.batch[ALEPPO_BS_ADVANTAGE_STD]);
  }
  if (u.refreshed && run.rank == 0) { // recompute_advantages: the last refresh of this update (rank 0's samples)
    logger.add_scalar("refresh/explained_variance", step, (float)u.refresh[ALEPPO_BS_EXPLAINED_VARIANCE]);
    logger.add_scalar("refresh/value_change_std", step, (float)u.refresh[ALEPPO_REFRESH_VALUE_CHANGE_STD]);
    logger.add_scalar("refresh/value_change_maxabs", step, (float)u.refresh[ALEPPO_REFRESH_VALUE_CHANGE_MAXABS]);
  }
  if (cfg.log_tensor_stats && run.rank == 0) { // (of the last minibatch's gradient and the last optimizer step)
    for (int k = 0; k < ALEPPO_TENSOR_STATS_ROWS; ++k) {
      const std::string tag = std::string("tensor_stats/") + TENSOR_STAT_NAMES[k];
      logger.add_scalar(tag + "/grad_norm", step, (float)u.tensor_stats[k][ALEPPO_TS_GRAD_NORM]);
      logger.add_scalar(tag + "/param_norm", step, (float)u.tensor_stats[k][ALEPPO_TS_PARAM_NORM]);
      logger.add_scalar(tag + "/update_ratio", step, (float)u.tensor_stats[k][ALEPPO_TS_UPDATE_RATIO]);
    }
    const double *total = u.tensor_stats[ALEPPO_TENSOR_STATS_ROWS - 1];
    logger.add_scalar("tensor_stats/nonfinite", step,
                      (float)(total[ALEPPO_TS_PARAM_NONFINITE] + total[ALEPPO_TS_STEP_NONFINITE]));
  }
  if (u.act_stats_read) { // (of the batch this update trained on; set on rank 0 only)
    for (int k = 0; k < ALEPPO_ACT_LAYER_ROWS; ++k) {
      const std::string tag = std::string("activation_stats/") + ACT_LAYER_NAMES[k];
      const double *row = u.act_layers[k];
      logger.add_scalar(tag + "/dormant_fraction", step, (float)(row[ALEPPO_ACT_L_DORMANT] / row[ALEPPO_ACT_L_UNITS]));
      logger.add_scalar(tag + "/dead_fraction", step, (float)(row[ALEPPO_ACT_L_DEAD] / row[ALEPPO_ACT_L_UNITS]));
      logger.add_scalar(tag + "/positive_fraction", step, (float)row[ALEPPO_ACT_L_POSITIVE_FRACTION]);
      logger.add_scalar(tag + "/mean_abs", step, (float)row[ALEPPO_ACT_L_MEAN_ABS]);
    }
    logger.add_scalar("activation_stats/nonfinite", step,
                      (float)u.act_layers[ALEPPO_ACT_LAYER_ROWS - 1][ALEPPO_ACT_L_NONFINITE]);
  }
  if (u.feature_rank_read) { // (of the batch this update trained on; set on rank 0 only)
    static const std::pair<const char *, int> tags[] = {
        {"effective", ALEPPO_FR_EFFECTIVE_RANK}, {"srank", ALEPPO_FR_SRANK}, {"pca", ALEPPO_FR_PCA_RANK},
        {"threshold", ALEPPO_FR_THRESHOLD_RANK}, {"stable", ALEPPO_FR_STABLE_RANK}, {"numerical", ALEPPO_FR_NUMERICAL_RANK},
        {"sigma_max", ALEPPO_FR_SIGMA_MAX}, {"sigma_min", ALEPPO_FR_SIGMA_MIN}, {"mean_sq_norm", ALEPPO_FR_MEAN_SQ_NORM},
        {"nonfinite_rows", ALEPPO_FR_NONFINITE_ROWS}};
    for (const auto &t : tags)
      logger.add_scalar(std::string("feature_rank/") + t.first, step, (float)u.feature_rank[t.second]);
  }
  if (u.churn_read) { // (of the batch this update trained on; set on rank 0 only)
    static const std::pair<const char *, int> tags[] = {
        {"churn", ALEPPO_PD_CHURN}, {"kl", ALEPPO_PD_MEAN_KL_AB}, {"kl_reverse", ALEPPO_PD_MEAN_KL_BA},
        {"tv", ALEPPO_PD_MEAN_TV}, {"value_change", ALEPPO_PD_RMS_DV}, {"feature_cos", ALEPPO_PD_MEAN_FEATURE_COS},
        {"feature_change", ALEPPO_PD_FEATURE_REL_CHANGE}};
    for (const auto &t : tags)
      logger.add_scalar(std::string("policy_churn/") + t.first, step, (float)u.churn[t.second]);
    if (cfg.policy_churn_averaged) {
      logger.add_scalar("policy_churn/ema_churn", step, (float)u.ema_churn[ALEPPO_PD_CHURN]);
      logger.add_scalar("policy_churn/ema_kl", step, (float)u.ema_churn[ALEPPO_PD_MEAN_KL_AB]);
    }
  }
  if (u.grad_read) { // (of the first minibatch's samples, before the update; set on rank 0 only)
    if (u.noise_read)
      logger.add_scalar("gradients/noise_scale", step, (float)u.noise_scale);
    static const char *const names[5] = {"conv1", "conv2", "conv3", "fc", "all"};
    for (int k = 0; k < 5; ++k)
      if (u.pv_read[k])
        logger.add_scalar(std::string("gradients/policy_value_cosine/") + names[k], step, (float)u.pv_cosine[k]);
    if (u.momentum_read)
      logger.add_scalar("gradients/momentum_cosine", step, (float)u.momentum_cosine);
  }
  if (u.recycled) {
    for (int k = 0; k < 4; ++k)
      logger.add_scalar(std::string("recycle/") + ACT_LAYER_NAMES[k] + "/units", step, (float)u.recycle_counts[k]);
    logger.add_scalar("recycle/total", step, (float)u.recycle_counts[4]);
  }
  if (cfg.ema_decay_set) { // (only with the key: the event files of existing configs stay byte-identical)
    logger.add_scalar("ema_decay", step, (float)u.ema_decay_now);
    logger.add_scalar("ema_distance", step, (float)u.ema_stats[ALEPPO_EMA_DISTANCE]);
    logger.add_scalar("ema_relative_distance", step, (float)u.ema_stats[ALEPPO_EMA_RELATIVE_DISTANCE]);
  }
  for (size_t k = 0; k < run.schedules.size(); ++k) // (the values this rollout's update ran with)
    logger.add_scalar(run.schedules[k].name, step, u.hyper_now[k]);
  logger.add_scalar("learning_rate", step, (float)u.lr);
}
static void log_histograms(Run &run, const Update &u, int64_t step) {
  EventWriter &logger = *run.logger;
  const size_t N = u.N;
  {
    std::vector<float> gn;
    for (size_t i = 0; i < u.nrun(); ++i)
      gn.push_back(u.m[i].grad_norm);
    if (gn.size() > 1)
      logger.add_histogram("clipped_gradients", step, gn);
  }
  // the per-sample histograms of log_data (train.cc:190-207): mask-selected values of the [epochs, M, B] planes
  std::vector<uint8_t> masks(N);
  std::vector<float> adv(N), ret(N), sel;
  check(run.ctx, aleppo_read_batch(run.ctx, ALEPPO_F_MASKS, masks.data(), N));
  auto gather = [&](const std::vector<float> &x, size_t reps) { // gather(t, masks): unmasked entries, every epoch
    sel.clear();
    for (size_t r = 0; r < reps; ++r)
      for (size_t i = 0; i < N; ++i)
        if (masks[i])
          sel.push_back(x[r * N + i]);
    return sel;
  };
  for (size_t k = 0; k < 5; ++k) // (every epoch that ran)
    logger.add_histogram(SAMPLE_FIELDS[k].second, step, gather(u.planes[k], u.epochs_run));
  check(run.ctx, aleppo_read_batch(run.ctx, ALEPPO_F_ADVANTAGES, adv.data(), N * 4));
  check(run.ctx, aleppo_read_batch(run.ctx, ALEPPO_F_RETURNS, ret.data(), N * 4));
  logger.add_histogram("advantages", step, gather(adv, 1));
  logger.add_histogram("returns", step, gather(ret, 1));
}

// ------------------------------------------------------------------ ... evaluate
static void log_evaluation(Run &run, int64_t step, const std::vector<float> &returns, const std::vector<size_t> &lengths) {
  run.logger->add_scalar("eval/episode_return_mean", step, meanf(returns));
  run.logger->add_scalar("eval/episode_return_max", step, *std::max_element(returns.begin(), returns.end()));
  run.logger->add_scalar("eval/episode_length_mean", step, meanf(lengths));
  run.logger->add_scalar("eval/episodes", step, (float)returns.size());
}
// device_evaluation: the same episodes from the library's log planes, a chunk of S steps at a time
static void evaluate_on_device(Run &run, uint64_t seed_base, int64_t step) {
  const Config &cfg = run.cfg;
  aleppo_ctx *ctx = run.ctx;
  const size_t L = cfg.eval_environments, S = cfg.device_evaluation_steps;
  aleppo_env_config ec{};
  ec.kind = ALEPPO_ENV_SYNTHETIC;
  ec.frame_kind = frame_kind(cfg);
  ec.seed_base = seed_base;
  ec.max_steps = cfg.max_steps;
  ec.max_return = (float)cfg.max_return;
  check(ctx, aleppo_eval_env_open(ctx, &ec, (int32_t)S)); // (again: fresh environments under this evaluation's seeds)
  check(ctx, aleppo_eval_set_counter(ctx, run.eval_counter));
  std::optional<EpisodeWriter> video; // record_evaluation: lane 0 of this evaluation, eval_<step>_episode_<n>
  if (run.record_evaluation()) {
    aleppo_rec_config rc{};
    rc.source = ALEPPO_REC_EVAL;
    rc.index = 0;
    rc.content = cfg.record_observation ? ALEPPO_REC_OBSERVATION : ALEPPO_REC_FRAMES;
    rc.capacity = (int32_t)S; // drained after every chunk
    check(ctx, aleppo_rec_open(ctx, &rc)); // (again with the same config: an empty log, ordinal 0)
    video.emplace(run.video_dir, "eval_" + std::to_string(step) + "_episode_", ALEPPO_REC_EVAL, run.record_field(),
                  cfg.device_preprocess && !cfg.record_observation, run.A, cfg.record_interval, run.lut, false);
  }
  std::vector<float> ret(S * L), returns;
  std::vector<uint32_t> len(S * L);
  std::vector<size_t> lengths;
  while (returns.size() < cfg.eval_episodes) {
    check(ctx, aleppo_eval_env_run(ctx, eval_rule(cfg), eval_param(cfg), (int32_t)S));
    check(ctx, aleppo_eval_env_read(ctx, ALEPPO_EEF_EPISODE_RETURNS, ret.data(), ret.size() * sizeof(float)));
    check(ctx, aleppo_eval_env_read(ctx, ALEPPO_EEF_EPISODE_LENGTHS, len.data(), len.size() * sizeof(uint32_t)));
    if (video)
      video->drain(ctx, check);
    for (size_t s = 0; s < S && returns.size() < cfg.eval_episodes; ++s) { // step, then lane: the host path's order
      run.eval_counter++; // (the host path acts once more only while episodes are missing)
      for (size_t i = 0; i < L && returns.size() < cfg.eval_episodes; ++i)
        if (len[s * L + i]) {
          returns.push_back(ret[s * L + i]);
          lengths.push_back(len[s * L + i]);
        }
    }
  }
  if (video) // the unfinished episode at the end of an evaluation is not kept
    video->discard();
  log_evaluation(run, step, returns, lengths);
}
static void evaluate(Run &run, size_t round, int64_t step) {
  Profile::Span sp(&run.prof, "evaluate");
  const Config &cfg = run.cfg;
  aleppo_ctx *ctx = run.ctx;
  EnvSet &set = run.eval_set;
  const size_t L = cfg.eval_environments;
  // fresh emulators per evaluation, seeded past every rank's training environments (env0 + i < total_environments)
  const size_t seed_base = cfg.total_environments + (round * (size_t)run.world + (size_t)run.rank) * L;
  if (cfg.device_evaluation)
    return evaluate_on_device(run, seed_base, step);
  set.envs.clear();
  for (size_t i = 0; i < L; ++i)
    set.envs.emplace_back(seed_base + i, cfg.max_steps, cfg.max_return, run.A, cfg.device_preprocess);
  std::fill(set.start.begin(), set.start.end(), 1);
  std::vector<float> ret(L, 0.f), returns;
  std::vector<size_t> len(L, 0), lengths;
  while (returns.size() < cfg.eval_episodes) {
    check(ctx, aleppo_eval_act(ctx, eval_rule(cfg), eval_param(cfg), nullptr, &set.actions));
    const std::vector<uint8_t> start_at_entry = set.start;
    run.pool->run_all(L, [&set](size_t i) { set.step(i); });
    check(ctx, aleppo_eval_push_frames(ctx, set.frames, frame_kind(cfg), ALEPPO_HOST_MAPPED, start_at_entry.data()));
    for (size_t i = 0; i < L; ++i) {
      if (!start_at_entry[i]) {
        ret[i] += set.results[i].reward;
        len[i]++;
      }
      if (set.results[i].terminated || set.results[i].truncated) {
        if (returns.size() < cfg.eval_episodes) { // (the first eval_episodes to finish, in lane order within a step)
          returns.push_back(ret[i]);
          lengths.push_back(len[i]);
        }
        ret[i] = 0;
        len[i] = 0;
        set.start[i] = 1;
      } else {
        set.start[i] = 0;
      }
    }
  }
  // the ingest of the last push reads the frames in place: it must have run before the next evaluation's workers (or
  // the teardown's host_free) touch the buffer (aleppo_eval_read synchronises the context's stream)
  std::vector<float> last_values(L);
  check(ctx, aleppo_eval_read(ctx, ALEPPO_EF_VALUES, last_values.data(), L * sizeof(float)));
  log_evaluation(run, step, returns, lengths);
}

// ------------------------------------------------------------------ ... checkpoint; and resume, its mirror
// the whole run state between two rollouts; visit_checkpoint (checkpoint.hpp) says what goes where
static void save_checkpoint(Run &run, size_t next_rollout) {
  Profile::Span sp(&run.prof, "checkpoint");
  aleppo_ctx *ctx = run.ctx;
  const size_t n = run.n_params(), E = run.E;
  DeviceState d(n, E);
  check(ctx, aleppo_export_params(ctx, d.params.data(), n));
  check(ctx, aleppo_export_optimizer(ctx, d.exp_avg.data(), d.exp_avg_sq.data(), &d.adam_step, n));
  check(ctx, aleppo_export_reward_scale(ctx, d.reward_scale.data(), d.reward_scale.data() + 3, E));
  check(ctx, aleppo_export_rollout_state(ctx, d.observations.data(), d.rollout_words, E));
  check(ctx, aleppo_state_digest(ctx, d.digest));
  run.st.next_rollout = run.st.schedule_position = next_rollout;
  Checkpoint ck;
  ck.shape = run.shape;
  CkptWriter out(ck.sections);
  visit_checkpoint(out, d, run.st);
  if (run.cfg.ema_decay_set) { // the optional section CK_EMA: the averaged parameters in reference order, then u64 updates
    std::vector<float> avg(n);
    int64_t updates = 0;
    check(ctx, aleppo_ema_export(ctx, avg.data(), n, &updates));
    ck.sections[CK_EMA] = ema_section(avg, (uint64_t)updates);
  }
  if (run.cfg.l2_init_coef > 0) { // the optional section CK_ANCHOR: the anchor in reference order
    std::vector<float> anchor(n);
    check(ctx, aleppo_anchor_export(ctx, anchor.data(), n));
    ck.sections[CK_ANCHOR] = anchor_section(anchor);
  }
  write_checkpoint_file(run.ckpt_file, ck);
  char line[256];
  std::snprintf(line, sizeof line, "checkpoint rollout %zu digest params=%016llx optimizer=%016llx rollout=%016llx "
                "reward_scale=%016llx", next_rollout, (unsigned long long)d.digest[0], (unsigned long long)d.digest[1],
                (unsigned long long)d.digest[2], (unsigned long long)d.digest[3]);
  std::cout << line << " -> " << run.ckpt_file << std::endl;
}
static void resume(Run &run) { // import everything, then prove it: the device's digest against the file's
  aleppo_ctx *ctx = run.ctx;
  const size_t n = run.n_params(), E = run.E;
  DeviceState d(n, E);
  CkptReader in(run.resumed.sections);
  visit_checkpoint(in, d, run.st);
  check(ctx, aleppo_load_params(ctx, d.params.data(), n)); // (resets the Adam state, restored next)
  check(ctx, aleppo_import_optimizer(ctx, d.exp_avg.data(), d.exp_avg_sq.data(), d.adam_step, n));
  check(ctx, aleppo_import_reward_scale(ctx, d.reward_scale.data(), d.reward_scale.data() + 3, E));
  check(ctx, aleppo_import_rollout_state(ctx, d.observations.data(), d.rollout_words, E));
  if (run.st.next_rollout > run.cfg.num_rollouts || run.st.schedule_position != run.st.next_rollout)
    throw std::runtime_error("resume: checkpoint " + run.resume_file + " continues at rollout " +
                             std::to_string(run.st.next_rollout) + ", this run has " +
                             std::to_string(run.cfg.num_rollouts));
  run.first_rollout = (size_t)run.st.next_rollout;
  if (run.cfg.device_environments) // (whichever mode wrote the file: the fields are the same)
    push_device_environments(run);
  uint64_t got[ALEPPO_DIGEST_COUNT];
  check(ctx, aleppo_state_digest(ctx, got));
  for (int k = 0; k < ALEPPO_DIGEST_COUNT; ++k)
    if (d.digest[k] != got[k]) {
      char b[160];
      std::snprintf(b, sizeof b, ": the %s digest after the import is %016llx, the file recorded %016llx", DIGEST_NAMES[k],
                    (unsigned long long)got[k], (unsigned long long)d.digest[k]);
      throw std::runtime_error("resume: checkpoint " + run.resume_file + b);
    }
  std::cout << "resumed from " << run.resume_file << " at rollout " << run.first_rollout << " of " << run.cfg.num_rollouts
            << ", state digest verified" << std::endl;
}

// ema_decay: open the averaged parameters once the live ones are loaded or resumed.  A resumed file's CK_EMA section is
// imported and proved by exporting it again (the state digest does not cover the average); without the section the average
// starts at the resumed parameters.  A section in a file resumed without the key is ignored.
static void open_average(Run &run) {
  aleppo_ctx *ctx = run.ctx;
  const size_t n = run.n_params();
  check(ctx, aleppo_ema_open(ctx));
  if (!run.resume_file.empty()) {
    const auto sec = run.resumed.sections.find(CK_EMA);
    if (sec == run.resumed.sections.end()) {
      std::cerr << "note: checkpoint " << run.resume_file << " has no averaged parameters (section " << CK_EMA
                << "): the average starts at the resumed parameters" << std::endl;
    } else {
      if (sec->second.size() != n * sizeof(float) + sizeof(uint64_t))
        throw std::runtime_error("resume: checkpoint " + run.resume_file + " is corrupt (section " + std::to_string(CK_EMA) +
                                 " has " + std::to_string(sec->second.size()) + " bytes, expected " +
                                 std::to_string(n * sizeof(float) + sizeof(uint64_t)) + ")");
      std::vector<float> avg(n);
      uint64_t updates = 0;
      std::memcpy(avg.data(), sec->second.data(), n * sizeof(float));
      std::memcpy(&updates, sec->second.data() + n * sizeof(float), sizeof updates);
      if (updates > (uint64_t)INT64_MAX)
        throw std::runtime_error("resume: checkpoint " + run.resume_file + " is corrupt (the average's update count)");
      check(ctx, aleppo_ema_import(ctx, avg.data(), n, (int64_t)updates));
      std::vector<float> back(n);
      int64_t got = 0;
      check(ctx, aleppo_ema_export(ctx, back.data(), n, &got));
      if (ema_section(back, (uint64_t)got) != sec->second)
        throw std::runtime_error("resume: checkpoint " + run.resume_file +
                                 ": the averaged parameters after the import differ from the file's");
      run.ema_updates = updates;
      std::cout << "resumed the averaged parameters at update " << updates << ", verified" << std::endl;
    }
  }
  if (run.cfg.eval_averaged) // (every evaluation, host-driven or device_evaluation, goes through the lanes' acting forward)
    check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_EVAL_PARAMS, 1));
}

// weight_decay / l2_init_coef: the two coefficients, and the anchor before the first update.  A fresh run anchors at the
// parameters it starts from (call this while they are still the initial ones); a resumed run REQUIRES the file's CK_ANCHOR
// section - the initial parameters are gone - imports it and proves it by exporting it again (the state digest does not
// cover the anchor).  A section in a file resumed without the key is ignored.
static void apply_regularization(Run &run) {
  aleppo_ctx *ctx = run.ctx;
  const Config &cfg = run.cfg;
  auto bits = [](double v) {
    const float f = (float)v;
    int32_t b;
    std::memcpy(&b, &f, 4);
    return b;
  };
  if (cfg.weight_decay > 0)
    check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_WEIGHT_DECAY, bits(cfg.weight_decay)));
  if (!(cfg.l2_init_coef > 0))
    return;
  const size_t n = run.n_params();
  if (run.resume_file.empty()) {
    check(ctx, aleppo_anchor_take(ctx, ALEPPO_SET_LIVE));
  } else {
    const auto sec = run.resumed.sections.find(CK_ANCHOR);
    if (sec == run.resumed.sections.end())
      throw std::runtime_error("resume: checkpoint " + run.resume_file + " has no anchor (section " +
                               std::to_string(CK_ANCHOR) + "): it was written by a run without l2_init_coef");
    if (sec->second.size() != n * sizeof(float))
      throw std::runtime_error("resume: checkpoint " + run.resume_file + " is corrupt (section " + std::to_string(CK_ANCHOR) +
                               " has " + std::to_string(sec->second.size()) + " bytes, expected " +
                               std::to_string(n * sizeof(float)) + ")");
    std::vector<float> anchor(n), back(n);
    std::memcpy(anchor.data(), sec->second.data(), n * sizeof(float));
    check(ctx, aleppo_anchor_import(ctx, anchor.data(), n));
    check(ctx, aleppo_anchor_export(ctx, back.data(), n));
    if (anchor_section(back) != sec->second)
      throw std::runtime_error("resume: checkpoint " + run.resume_file + ": the anchor after the import differs from the file's");
    std::cout << "resumed the anchor, verified" << std::endl;
  }
  check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_ANCHOR_COEF, bits(cfg.l2_init_coef)));
}

// ------------------------------------------------------------------ the rollout loop, the summary line, teardown
static void train_loop(Run &run) {
  const Config &cfg = run.cfg;
  // test hook: stop (cleanly) right after the checkpoint that continues at this rollout index, as an interruption would
  const long stop_after = std::getenv("ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT")
                              ? std::atol(std::getenv("ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT"))
                              : -1;
  run.rollouts_done = run.first_rollout;
  const auto t_begin = std::chrono::steady_clock::now();
  Update u(run);
  for (size_t r = run.first_rollout; r < cfg.num_rollouts; ++r) {
    std::cout << "Rollout " << r + 1 << " of " << cfg.num_rollouts << std::endl;
    const EpisodeLog log = collect(run);
    const BatchStatistics stats = read_statistics(run);
    update(run, r, u);
    Profile::Span sp_log(&run.prof, "log_data");
    const int64_t step = (int64_t)run.st.total_steps; // x axis = non-reset env steps
    log_scalars(run, log, stats, u, step);
    if (cfg.eval_interval > 0 && (r + 1) % cfg.eval_interval == 0) // between this update and the next rollout
      evaluate(run, r / cfg.eval_interval, step);
    log_histograms(run, u, step);
    run.logger->flush();
    run.rollouts_done = r + 1;
    if (!run.ckpt_file.empty() && (r + 1 == cfg.num_rollouts ||
                                   (cfg.checkpoint_interval > 0 && (r + 1) % (size_t)cfg.checkpoint_interval == 0))) {
      save_checkpoint(run, r + 1);
      if (stop_after == (long)(r + 1)) {
        std::cout << "stopped after the checkpoint of rollout " << r + 1 << std::endl;
        break;
      }
    }
  }
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
  size_t pending_starts = 0; // environments whose next slot is an episode-start slot
  for (uint8_t s : run.st.set.start)
    pending_starts += s;
  // total_steps counts only non-start slots (rollout.cc:225,266): slots = steps + start slots, and the start slots are
  // the E initial ones plus one per finished episode, minus those still pending
  const size_t ET = run.E * run.T;
  std::cout << "steps " << run.st.total_steps << " episodes " << run.st.episodes << " pending_starts " << pending_starts
            << " slots " << (run.rollouts_done + 1) * ET << " env-steps/s "
            << (double)((run.rollouts_done - run.first_rollout) * ET) / secs << std::endl;
}
static void teardown(Run &run) {
  aleppo_ctx *ctx = run.ctx;
  if (run.prof.on()) {
    run.prof.device_summary(ctx);
    run.prof.save();
  }
  if (const char *dump = std::getenv("ALEPPO_TRAINER_DUMP_FINAL")) { // test hook: the trained parameters
    size_t n = 0;
    check(ctx, aleppo_param_count(ctx, &n));
    std::vector<float> p(n);
    check(ctx, aleppo_export_params(ctx, p.data(), n));
    std::ofstream f(dump, std::ios::binary);
    f.write(reinterpret_cast<const char *>(p.data()), (std::streamsize)(n * sizeof(float)));
  }
  check(ctx, aleppo_host_free(ctx, run.st.set.frames));
  check(ctx, aleppo_host_free(ctx, run.start_mapped));
  if (run.eval_set.frames)
    check(ctx, aleppo_host_free(ctx, run.eval_set.frames));
  aleppo_destroy(ctx);
}

int main(int argc, char **argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s <rom> <tensorboard log path> <video dir> <group> <config.yaml> [profile]\n", argv[0]);
    return 2;
  }
  try {
    Run run(argc, argv); // load and validate
    // refuse what the linked library or the resume file cannot serve, before anything is created (in this order)
    open_checkpoint_files(run);
    if (dump_initial_params(run))
      return 0;
    refuse_missing_entry_points(run.cfg);
    create_context(run);
    if (run.world > 1)
      rendezvous(run);
    load_initial_params(run);
    run.logger.emplace(run.rank == 0 ? run.log_path : run.log_path + ".rank" + std::to_string(run.rank)); // rank 0: THE log
    apply_options(run.ctx, run.cfg);
    apply_regularization(run); // (the live parameters are still the initial ones: a fresh run's anchor)
    if (run.prof.on())
      check(run.ctx, aleppo_profile_enable(run.ctx, 1));
    const HParams hp = hparams_of(run.cfg);
    run.logger->add_hparams(hp.numbers, hp.flags, run.group, (double)run.start_time * 1e-9);
    create_environments(run);
    if (!run.resume_file.empty())
      resume(run);
    else
      collect(run); // the warm rollout before the loop (train.cc:391-396): collected, never trained on
    if (run.cfg.ema_decay_set)
      open_average(run);
    train_loop(run);
    teardown(run);
    std::cout << "Success" << std::endl;
    return 0;
  } catch (const std::exception &e) {
    std::cerr << "error: " << e.what() << std::endl;
    return 1;
  }
}
