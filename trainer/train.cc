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
// a NaN explained variance is logged as NaN).  clip_param_final, value_loss_coef_final, entropy_coef_final,
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
// Data parallelism (no reference counterpart): start one process per GPU with RANK / WORLD_SIZE / LOCAL_RANK
// in the environment (torchrun / mpirun style).  Rank r owns the contiguous environment block
// [r * E / W, (r + 1) * E / W) and GPU LOCAL_RANK; rank 0 creates the RCCL id, hands it to the others through the file
// <log path>.rcclid, and is the only rank that writes the event file (its own environments' episode statistics, the
// global - all-reduced - update metrics).  Everything else is unchanged: aleppo_train all-reduces the gradients.
#include "../include/aleppo.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <filesystem>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <mutex>
#include <numeric>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

// The evaluation lanes are declared weak: a build linked against a library without them (the host-only stand-in of the
// ThreadSanitizer build) still links, and a config that asks for evaluation is then refused at start-up.
extern "C" {
int aleppo_eval_open(aleppo_ctx *ctx, int32_t num_lanes) __attribute__((weak));
int aleppo_eval_push_frames(aleppo_ctx *ctx, const uint8_t *frames, int frame_kind, int location,
                            const uint8_t *episode_start) __attribute__((weak));
int aleppo_eval_act(aleppo_ctx *ctx, int rule, float param, const float *noise, const int64_t **actions_pinned)
    __attribute__((weak));
int aleppo_eval_read(aleppo_ctx *ctx, int field, void *dst, size_t bytes) __attribute__((weak));
// ... and so is the reward-scaling state (reward_scaling: true is refused without it)
int aleppo_export_reward_scale(aleppo_ctx *ctx, double stats[3], double *returns, size_t num_envs) __attribute__((weak));
int aleppo_import_reward_scale(aleppo_ctx *ctx, const double stats[3], const double *returns, size_t num_envs)
    __attribute__((weak));
// ... and what a checkpoint needs (checkpoint_path / checkpoint_interval / resume are refused without it)
int aleppo_export_optimizer(aleppo_ctx *ctx, float *exp_avg, float *exp_avg_sq, int64_t *step, size_t count)
    __attribute__((weak));
int aleppo_import_optimizer(aleppo_ctx *ctx, const float *exp_avg, const float *exp_avg_sq, int64_t step, size_t count)
    __attribute__((weak));
int aleppo_export_rollout_state(aleppo_ctx *ctx, uint8_t *observations, uint64_t words[4], size_t num_envs)
    __attribute__((weak));
int aleppo_import_rollout_state(aleppo_ctx *ctx, const uint8_t *observations, const uint64_t words[4], size_t num_envs)
    __attribute__((weak));
int aleppo_state_digest(aleppo_ctx *ctx, uint64_t out[4]) __attribute__((weak));
}

// ------------------------------------------------------------------ config
struct Config {
  size_t total_environments = 512, hidden_size = 512, action_size = 4, horizon = 128, max_steps = 108000,
         frame_stack = 4;
  double learning_rate = 2.5e-4;
  float clip_param = 0.1f, value_loss_coef = 0.5f, entropy_coef = 0.01f;
  long num_epochs = 1, mini_batch_size = 2048, num_mini_batches = 32;
  float gae_discount = 0.99f, gae_lambda = 0.95f, max_gradient_norm = 0.5f;
  size_t num_rollouts = 7000, num_workers = 16, worker_batch_size = 32, frame_skip = 4;
  float max_return = -1.0f;
  bool record_observation = false, record_video = false, cuda_graph = false, deterministic = false;
  bool shuffle_minibatches = false; // extension: a fresh sample permutation per epoch (ALEPPO_OPT_MINIBATCH_SHUFFLE)
  bool clip_value_loss = false;     // extension: value-function clipping (ALEPPO_OPT_VALUE_CLIP)
  bool minibatch_advantage_norm = false; // extension: per-minibatch advantage normalisation (ALEPPO_OPT_ADV_NORM_MINIBATCH)
  double target_kl = 0.0;           // extension: early stop of the update's epochs on approx-KL (<= 0: off)
  double kl_coef = 0.0, kl_target = 0.0; // extension: adaptive KL penalty (ALEPPO_OPT_KL_PENALTY; <= 0: off / fixed beta)
  bool kl_coef_set = false, kl_target_set = false; // (the keys were given: hparams entries)
  // extension: per-update hyper-parameters (ALEPPO_OPT_CLIP_PARAM and its kin).  *_final: the end of a linear schedule
  // from the value above; *_set: the key was given (absent keys set no option)
  double clip_param_final = 0, value_loss_coef_final = 0, entropy_coef_final = 0, max_gradient_norm_final = 0;
  bool clip_param_final_set = false, value_loss_coef_final_set = false, entropy_coef_final_set = false,
       max_gradient_norm_final_set = false;
  double value_clip_range = 0; // constant c of the clipped value loss (ALEPPO_OPT_VALUE_CLIP_RANGE)
  bool value_clip_range_set = false;
  // extension: periodic evaluation episodes through the evaluation lanes (aleppo_eval_*)
  size_t eval_interval = 0, eval_environments = 8, eval_episodes = 10;
  std::string eval_rule = "greedy";
  double eval_temperature = 1.0, eval_epsilon = 0.05;
  // extension: return-based reward scaling in place of the reward clamp (ALEPPO_OPT_REWARD_SCALE / _CLIP)
  bool reward_scaling = false;
  double reward_scale_clip = 10.0;
  // extension: checkpoint and resume (aleppo_export_rollout_state / aleppo_state_digest and the learner's export pairs)
  std::string checkpoint_path, resume;
  long checkpoint_interval = 0; // 0: only after the last rollout
  bool log_batch_stats = false; // extension: explained variance and value / return / advantage statistics (ALEPPO_F_BATCH_STATS)
  // extensions
  std::string precision = "fp32", rollout_precision = "fp32";
  bool device_preprocess = false; // emulators hand over raw frame pairs; gray LUT + resize + max run on the device (N2)
  bool slot_ahead = true;         // aleppo_arm_step / aleppo_release_step: the stream runs one slot ahead of the emulators
  bool advantage_norm = false;
  uint64_t seed = 42;
};

static std::string trim(const std::string &s) {
  const size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
  return a == std::string::npos ? "" : s.substr(a, b - a + 1);
}
// flat "key: value" YAML (what configs/*.yaml use): comments, blank lines, scalars
static std::map<std::string, std::string> parse_yaml(const std::string &path) {
  std::ifstream f(path);
  if (!f)
    throw std::runtime_error("cannot open config: " + path);
  std::map<std::string, std::string> kv;
  std::string line;
  while (std::getline(f, line)) {
    const size_t h = line.find('#');
    if (h != std::string::npos)
      line = line.substr(0, h);
    const size_t c = line.find(':');
    if (c == std::string::npos)
      continue;
    const std::string k = trim(line.substr(0, c)), v = trim(line.substr(c + 1));
    if (!k.empty() && !v.empty())
      kv[k] = v;
  }
  return kv;
}
template <class T> static T as(const std::map<std::string, std::string> &kv, const char *k, T dflt) {
  auto it = kv.find(k);
  if (it == kv.end())
    return dflt;
  std::istringstream ss(it->second);
  T v;
  ss >> v;
  if (ss.fail())
    throw std::runtime_error(std::string("bad value for ") + k);
  return v;
}
static bool as_bool(const std::map<std::string, std::string> &kv, const char *k, bool dflt) {
  auto it = kv.find(k);
  if (it == kv.end())
    return dflt;
  return it->second == "true" || it->second == "True" || it->second == "1" || it->second == "yes";
}
// kl_target's rule never halves beta below this (nor raises a smaller initial kl_coef to it): repeated halving would
// otherwise reach 0 through the subnormals, and 0 doubled stays 0
constexpr float KL_BETA_MIN = 1e-6f;
static Config load_config(const std::string &path) { // keys / defaults of src/bin/train.cc:108-136
  const auto kv = parse_yaml(path);
  Config c;
  c.total_environments = as<size_t>(kv, "total_environments", 512);
  c.hidden_size = as<size_t>(kv, "hidden_size", 512);
  c.action_size = as<size_t>(kv, "action_size", 4);
  c.horizon = as<size_t>(kv, "horizon", 128);
  c.max_steps = as<size_t>(kv, "max_steps", 108000);
  c.frame_stack = as<size_t>(kv, "frame_stack", 4);
  c.learning_rate = as<double>(kv, "learning_rate", 2.5e-4);
  c.clip_param = as<float>(kv, "clip_param", 0.1f);
  c.value_loss_coef = as<float>(kv, "value_loss_coef", 0.5f);
  c.entropy_coef = as<float>(kv, "entropy_coef", 0.01f);
  c.num_epochs = as<long>(kv, "num_epochs", 1);
  c.mini_batch_size = as<long>(kv, "mini_batch_size", 2048);
  c.num_mini_batches = as<long>(kv, "num_mini_batches", 32);
  c.gae_discount = as<float>(kv, "gae_discount", 0.99f);
  c.gae_lambda = as<float>(kv, "gae_lambda", 0.95f);
  c.max_gradient_norm = as<float>(kv, "max_gradient_norm", 0.5f);
  c.num_rollouts = as<size_t>(kv, "num_rollouts", 7000);
  c.num_workers = as<size_t>(kv, "num_workers", 16);
  c.worker_batch_size = as<size_t>(kv, "worker_batch_size", 32);
  c.frame_skip = as<size_t>(kv, "frame_skip", 4);
  c.max_return = as<float>(kv, "max_return", -1.0f);
  c.record_observation = as_bool(kv, "record_observation", false);
  c.record_video = as_bool(kv, "record_video", false);
  c.cuda_graph = as_bool(kv, "cuda_graph", false);
  c.shuffle_minibatches = as_bool(kv, "shuffle_minibatches", false);
  c.clip_value_loss = as_bool(kv, "clip_value_loss", false);
  c.minibatch_advantage_norm = as_bool(kv, "minibatch_advantage_norm", false);
  c.target_kl = as<double>(kv, "target_kl", 0.0);
  c.kl_coef = as<double>(kv, "kl_coef", 0.0);
  c.kl_target = as<double>(kv, "kl_target", 0.0);
  c.log_batch_stats = as_bool(kv, "log_batch_stats", false);
  c.kl_coef_set = kv.count("kl_coef") != 0;
  c.kl_target_set = kv.count("kl_target") != 0;
  if (!(c.kl_coef >= 0 && c.kl_coef < 3.0e38) || !(c.kl_target >= 0 && c.kl_target < 3.0e38)) // (beta is a float)
    throw std::runtime_error("kl_coef / kl_target must be finite and non-negative");
  if (c.kl_target > 0 && !(c.kl_coef > 0)) // (it would adapt a penalty that is off)
    throw std::runtime_error("kl_target needs kl_coef > 0");
  // the per-update hyper-parameters: what the options would refuse is refused here (they are floats: < 3e38 is finite)
  auto sched_key = [&](const char *key, double &v, bool &set, double v0, bool zero_ok) {
    set = kv.count(key) != 0;
    if (!set)
      return;
    v = as<double>(kv, key, 0.0);
    const bool ok = (zero_ok ? v >= 0 : v > 0) && v < 3.0e38 && (zero_ok ? v0 >= 0 : v0 > 0) && v0 < 3.0e38;
    if (!ok) // (the schedule's start is the config's own value: it has to be settable too)
      throw std::runtime_error(std::string(key) + (zero_ok ? " and the value it starts from must be finite and non-negative"
                                                           : " and the value it starts from must be finite and positive"));
  };
  sched_key("clip_param_final", c.clip_param_final, c.clip_param_final_set, c.clip_param, false);
  sched_key("value_loss_coef_final", c.value_loss_coef_final, c.value_loss_coef_final_set, c.value_loss_coef, true);
  sched_key("entropy_coef_final", c.entropy_coef_final, c.entropy_coef_final_set, c.entropy_coef, true);
  sched_key("max_gradient_norm_final", c.max_gradient_norm_final, c.max_gradient_norm_final_set, c.max_gradient_norm,
            false);
  c.value_clip_range_set = kv.count("value_clip_range") != 0;
  if (c.value_clip_range_set) {
    c.value_clip_range = as<double>(kv, "value_clip_range", 0.0);
    if (!(c.value_clip_range > 0 && c.value_clip_range < 3.0e38))
      throw std::runtime_error("value_clip_range must be finite and positive");
    if (!c.clip_value_loss) // (nothing else reads it)
      throw std::runtime_error("value_clip_range needs clip_value_loss: true");
  }
  c.reward_scaling = as_bool(kv, "reward_scaling", false);
  if (kv.count("reward_scale_clip")) { // what the option would refuse is refused here (a float: < 3e38 is finite)
    c.reward_scale_clip = as<double>(kv, "reward_scale_clip", 10.0);
    if (!(c.reward_scale_clip > 0 && c.reward_scale_clip < 3.0e38))
      throw std::runtime_error("reward_scale_clip must be finite and positive");
    if (!c.reward_scaling) // (nothing else reads it)
      throw std::runtime_error("reward_scale_clip needs reward_scaling: true");
  }
  { // evaluation: what aleppo_eval_open / aleppo_eval_act would refuse is refused here
    const long interval = as<long>(kv, "eval_interval", 0), envs = as<long>(kv, "eval_environments", 8),
               episodes = as<long>(kv, "eval_episodes", 10);
    if (interval < 0)
      throw std::runtime_error("eval_interval must be non-negative");
    for (const char *k : {"eval_environments", "eval_episodes", "eval_rule", "eval_temperature", "eval_epsilon"})
      if (kv.count(k) && interval == 0)
        throw std::runtime_error(std::string(k) + " needs eval_interval > 0");
    if (envs < 1 || envs > 4096)
      throw std::runtime_error("eval_environments must be in [1, 4096]");
    if (episodes < 1)
      throw std::runtime_error("eval_episodes must be positive");
    c.eval_interval = (size_t)interval;
    c.eval_environments = (size_t)envs;
    c.eval_episodes = (size_t)episodes;
    c.eval_rule = as<std::string>(kv, "eval_rule", "greedy");
    if (c.eval_rule != "greedy" && c.eval_rule != "sample" && c.eval_rule != "epsilon")
      throw std::runtime_error("eval_rule must be greedy, sample or epsilon");
    c.eval_temperature = as<double>(kv, "eval_temperature", 1.0);
    if (!(c.eval_temperature > 0 && c.eval_temperature < 3.0e38) || !std::isfinite(1.0f / (float)c.eval_temperature))
      throw std::runtime_error("eval_temperature must be finite and positive");
    c.eval_epsilon = as<double>(kv, "eval_epsilon", 0.05);
    if (!(c.eval_epsilon >= 0 && c.eval_epsilon <= 1))
      throw std::runtime_error("eval_epsilon must be in [0, 1]");
  }
  c.checkpoint_path = as<std::string>(kv, "checkpoint_path", "");
  c.resume = as<std::string>(kv, "resume", "");
  if (kv.count("checkpoint_interval")) {
    c.checkpoint_interval = as<long>(kv, "checkpoint_interval", 0);
    if (c.checkpoint_interval <= 0)
      throw std::runtime_error("checkpoint_interval must be positive");
    if (c.checkpoint_path.empty()) // (there would be nowhere to write to)
      throw std::runtime_error("checkpoint_interval needs checkpoint_path");
  }
  c.deterministic = as_bool(kv, "deterministic", false);
  c.precision = as<std::string>(kv, "precision", "fp32");
  c.rollout_precision = as<std::string>(kv, "rollout_precision", "fp32");
  c.device_preprocess = as_bool(kv, "device_preprocess", false);
  c.slot_ahead = as_bool(kv, "slot_ahead", true);
  c.advantage_norm = as_bool(kv, "advantage_norm", false);
  c.seed = as<uint64_t>(kv, "seed", 42);
  return c;
}

// ------------------------------------------------------------------ synthetic emulator (stands in for the ALE wrapper chain)
struct StepOut {
  float reward = 0.f;
  bool terminated = false, truncated = false, game_over = false;
};
class SyntheticAtari {
public:
  // raw = true: the emulator hands over what ALE itself produces - the last TWO 210x160 palette-code frames of the skip
  // window - and the gray LUT, the 84x84 resize and the 2-frame max (environment.cc:48-55, resize.cc:34-41,
  // max_and_skip.cc:33-42) run on the device (ALEPPO_FRAMES_RAW_PAIR); raw = false: one finished 84x84 gray frame.
  SyntheticAtari(uint64_t seed, size_t max_steps, float max_return, size_t actions, bool raw = false)
      : rng_(seed * 0x9E3779B97F4A7C15ull + 12345), max_steps_(max_steps), max_return_(max_return), actions_(actions),
        raw_(raw) {}
  static size_t frame_bytes(bool raw) { return raw ? 2 * 210 * 160 : 84 * 84; }
  // FireReset / EpisodeLife semantics: a full reset only after game over, otherwise continue with the next life
  void reset(uint8_t *frame) {
    if (lives_ == 0) {
      lives_ = 5;
      steps_ = 0;
      episode_return_ = 0.f;
      bricks_ = 0;
    }
    ball_x_ = 42;
    ball_y_ = 60;
    prev_x_ = ball_x_;
    prev_y_ = ball_y_;
    dx_ = (next() & 1) ? 1 : -1;
    dy_ = -1;
    render(frame);
  }
  StepOut step(int action, uint8_t *frame) {
    StepOut o;
    paddle_ += (action == 2 ? 3 : action == 3 ? -3 : 0); // NOOP FIRE RIGHT LEFT like Breakout's minimal set
    paddle_ = std::clamp(paddle_, 4, 79);
    for (int k = 0; k < 4; ++k) { // frame_skip emulator frames per agent step
      prev_x_ = ball_x_;
      prev_y_ = ball_y_;
      ball_x_ += dx_ * 2;
      ball_y_ += dy_ * 2;
      if (ball_x_ <= 1 || ball_x_ >= 82)
        dx_ = -dx_;
      if (ball_y_ <= 20) { // brick row
        dy_ = 1;
        o.reward += (float)(1 + 3 * (bricks_ % 3 == 2));
        ++bricks_;
      }
      if (ball_y_ >= 78) {
        if (std::abs(ball_x_ - paddle_) <= 8 || (next() % 3) == 0)
          dy_ = -1;
        else { // life lost -> EpisodeLife reports a terminal
          --lives_;
          o.terminated = true;
          break;
        }
      }
    }
    steps_ += 4;
    episode_return_ += o.reward;
    o.game_over = lives_ == 0;
    if (!o.terminated && (steps_ >= max_steps_ || (max_return_ > 0 && episode_return_ >= max_return_))) {
      o.truncated = true; // ALE max_num_frames_per_episode / TruncateOnEpisodeReturn
      lives_ = 0;
      o.game_over = true;
    }
    render(frame);
    (void)actions_;
    return o;
  }

  // every field that changes after construction, for a checkpoint (the constructor's arguments come from the config)
  static constexpr size_t state_bytes = 8 + 9 * 4 + 8 + 4;
  void save(std::string &out) const {
    const int32_t ints[9] = {lives_, paddle_, ball_x_, ball_y_, prev_x_, prev_y_, dx_, dy_, bricks_};
    const uint64_t steps = steps_;
    out.append(reinterpret_cast<const char *>(&rng_), 8);
    out.append(reinterpret_cast<const char *>(ints), sizeof(ints));
    out.append(reinterpret_cast<const char *>(&steps), 8);
    out.append(reinterpret_cast<const char *>(&episode_return_), 4);
  }
  void load(const uint8_t *in) { // state_bytes bytes that save() wrote
    int32_t ints[9];
    uint64_t steps;
    std::memcpy(&rng_, in, 8);
    std::memcpy(ints, in + 8, sizeof(ints));
    std::memcpy(&steps, in + 8 + sizeof(ints), 8);
    std::memcpy(&episode_return_, in + 16 + sizeof(ints), 4);
    lives_ = ints[0], paddle_ = ints[1], ball_x_ = ints[2], ball_y_ = ints[3], prev_x_ = ints[4], prev_y_ = ints[5];
    dx_ = ints[6], dy_ = ints[7], bricks_ = ints[8];
    steps_ = (size_t)steps;
  }

private:
  uint64_t next() {
    rng_ ^= rng_ << 13;
    rng_ ^= rng_ >> 7;
    rng_ ^= rng_ << 17;
    return rng_;
  }
  void render(uint8_t *f) const {
    if (raw_) { // two emulator frames (the ball at its previous and current position), ALE-style even palette codes
      for (int k = 0; k < 2; ++k) {
        uint8_t *g = f + (size_t)k * 210 * 160;
        std::memset(g, 0, 210 * 160);
        auto rect = [&](int x0, int x1, int y0, int y1, uint8_t c) { // [x0,x1) x [y0,y1) in 84-grid units
          for (int y = y0 * 210 / 84; y < y1 * 210 / 84; ++y)
            for (int x = x0 * 160 / 84; x < x1 * 160 / 84; ++x)
              if (x >= 0 && x < 160 && y >= 0 && y < 210)
                g[y * 160 + x] = c;
        };
        for (int y = 8; y < 20; y += 3)
          for (int x = 0; x < 84; x += 6)
            rect(x, x + 6, y, y + 3, (uint8_t)((((x / 6 + y / 3 + bricks_) % 4) * 50 + 60) & ~1));
        rect(paddle_ - 6, paddle_ + 7, 80, 82, 200);
        const int bx = k == 0 ? prev_x_ : ball_x_, by = k == 0 ? prev_y_ : ball_y_;
        rect(bx, bx + 2, by, by + 2, 236);
      }
      return;
    }
    std::memset(f, 0, 84 * 84);
    for (int y = 8; y < 20; ++y)
      for (int x = 0; x < 84; ++x)
        f[y * 84 + x] = (uint8_t)(((x / 6 + y / 3 + bricks_) % 4) * 50 + 60);
    for (int x = paddle_ - 6; x <= paddle_ + 6; ++x)
      if (x >= 0 && x < 84)
        f[80 * 84 + x] = f[81 * 84 + x] = 200;
    for (int y = ball_y_; y < ball_y_ + 2; ++y)
      for (int x = ball_x_; x < ball_x_ + 2; ++x)
        if (x >= 0 && x < 84 && y >= 0 && y < 84)
          f[y * 84 + x] = 236;
  }
  uint64_t rng_;
  size_t max_steps_;
  float max_return_;
  size_t actions_;
  bool raw_;
  int lives_ = 0, paddle_ = 42, ball_x_ = 42, ball_y_ = 60, prev_x_ = 42, prev_y_ = 60, dx_ = 1, dy_ = -1, bricks_ = 0;
  size_t steps_ = 0;
  float episode_return_ = 0.f;
};

// ------------------------------------------------------------------ worker pool (std::thread + index queue, rollout.cc:280-297)
class WorkerPool {
public:
  WorkerPool(size_t n, std::function<void(size_t)> fn) : fn_(std::move(fn)) {
    for (size_t i = 0; i < n; ++i)
      threads_.emplace_back([this] { loop(); });
  }
  ~WorkerPool() {
    {
      std::lock_guard<std::mutex> l(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : threads_)
      t.join();
  }
  void run_all(size_t count) { // push indices 0..count-1, wait until all are done (step_all)
    {
      std::lock_guard<std::mutex> l(m_);
      next_ = 0;
      end_ = count;
      done_ = 0;
    }
    cv_.notify_all();
    std::unique_lock<std::mutex> l(m_);
    done_cv_.wait(l, [&] { return done_ == end_; });
  }

private:
  void loop() {
    for (;;) {
      size_t i;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return stop_ || next_ < end_; });
        if (stop_)
          return;
        i = next_++;
      }
      fn_(i);
      {
        std::lock_guard<std::mutex> l(m_);
        if (++done_ == end_)
          done_cv_.notify_all();
      }
    }
  }
  std::function<void(size_t)> fn_;
  std::vector<std::thread> threads_;
  std::mutex m_;
  std::condition_variable cv_, done_cv_;
  size_t next_ = 0, end_ = 0, done_ = 0;
  bool stop_ = false;
};

// ------------------------------------------------------------------ TensorBoard event file (TFRecord + protobuf by hand)
static uint32_t crc32c(const uint8_t *p, size_t n) {
  static uint32_t table[256];
  static bool init = false;
  if (!init) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k)
        c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
      table[i] = c;
    }
    init = true;
  }
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i)
    c = table[(c ^ p[i]) & 255] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}
static uint32_t masked_crc(const uint8_t *p, size_t n) {
  const uint32_t c = crc32c(p, n);
  return ((c >> 15) | (c << 17)) + 0xa282ead8u;
}
struct Pb { // minimal protobuf encoder
  std::string b;
  void varint(uint64_t v) {
    while (v >= 128) {
      b.push_back((char)(v | 128));
      v >>= 7;
    }
    b.push_back((char)v);
  }
  void key(int field, int wire) { varint(((uint64_t)field << 3) | wire); }
  void f64(int field, double v) {
    key(field, 1);
    b.append(reinterpret_cast<const char *>(&v), 8);
  }
  void f32(int field, float v) {
    key(field, 5);
    b.append(reinterpret_cast<const char *>(&v), 4);
  }
  void i64(int field, int64_t v) {
    key(field, 0);
    varint((uint64_t)v);
  }
  void bytes(int field, const std::string &s) {
    key(field, 2);
    varint(s.size());
    b += s;
  }
  void packed_f64(int field, const std::vector<double> &v) {
    key(field, 2);
    varint(v.size() * 8);
    b.append(reinterpret_cast<const char *>(v.data()), v.size() * 8);
  }
};
class EventWriter {
public:
  explicit EventWriter(const std::string &path) : f_(path, std::ios::binary) {
    if (!f_)
      throw std::runtime_error("cannot open event file: " + path);
    Pb e;
    e.f64(1, now());
    e.bytes(3, "brain.Event:2"); // file_version
    record(e.b);
  }
  void add_scalar(const std::string &tag, int64_t step, float value) {
    Pb v;
    v.bytes(1, tag);
    v.f32(2, value);
    Pb s;
    s.bytes(1, v.b);
    Pb e;
    e.f64(1, now());
    e.i64(2, step);
    e.bytes(5, s.b);
    record(e.b);
  }
  void add_histogram(const std::string &tag, int64_t step, const std::vector<float> &x) {
    if (x.empty())
      return;
    double mn = x[0], mx = x[0], sum = 0, sq = 0;
    for (float v : x) {
      mn = std::min<double>(mn, v);
      mx = std::max<double>(mx, v);
      sum += v;
      sq += (double)v * v;
    }
    const int nb = 30;
    std::vector<double> limits(nb), counts(nb, 0.0);
    const double w = (mx - mn) / nb > 0 ? (mx - mn) / nb : 1.0;
    for (int i = 0; i < nb; ++i)
      limits[i] = mn + w * (i + 1);
    for (float v : x)
      counts[std::min(nb - 1, (int)((v - mn) / w))] += 1.0;
    Pb h; // HistogramProto: min=1 max=2 num=3 sum=4 sum_squares=5 bucket_limit=6 bucket=7
    h.f64(1, mn);
    h.f64(2, mx);
    h.f64(3, (double)x.size());
    h.f64(4, sum);
    h.f64(5, sq);
    h.packed_f64(6, limits);
    h.packed_f64(7, counts);
    Pb v;
    v.bytes(1, tag);
    v.bytes(5, h.b); // Summary.Value.histo
    Pb s;
    s.bytes(1, v.b);
    Pb e;
    e.f64(1, now());
    e.i64(2, step);
    e.bytes(5, s.b);
    record(e.b);
  }
  // logger.add_hparams(get_parameters(config), group_name, start_time) (src/bin/train.cc:72-105, :389): the HParams
  // plugin's session-start record.  Summary.Value{tag "_hparams_/session_start_info", metadata.plugin_data{plugin_name
  // "hparams", content = HParamsPluginData{version 0, session_start_info{hparams map<string, google.protobuf.Value>,
  // group_name, start_time_secs}}}}
  void add_hparams(const std::vector<std::pair<std::string, double>> &numbers,
                   const std::vector<std::pair<std::string, bool>> &flags, const std::string &group, double start_secs) {
    Pb ssi;
    auto entry = [&](const std::string &k, const Pb &val) {
      Pb kv; // map entry: key = 1, value = 2
      kv.bytes(1, k);
      kv.bytes(2, val.b);
      ssi.bytes(1, kv.b);
    };
    for (auto &n : numbers) {
      Pb v;
      v.f64(2, n.second); // google.protobuf.Value.number_value
      entry(n.first, v);
    }
    for (auto &b : flags) {
      Pb v;
      v.i64(4, b.second ? 1 : 0); // google.protobuf.Value.bool_value
      entry(b.first, v);
    }
    ssi.bytes(4, group);
    ssi.f64(5, start_secs);
    Pb plugin; // HParamsPluginData: version = 1, session_start_info = 3
    plugin.i64(1, 0);
    plugin.bytes(3, ssi.b);
    Pb pd; // SummaryMetadata.PluginData: plugin_name = 1, content = 2
    pd.bytes(1, "hparams");
    pd.bytes(2, plugin.b);
    Pb md; // SummaryMetadata: plugin_data = 1
    md.bytes(1, pd.b);
    Pb v; // Summary.Value: tag = 1, metadata = 9
    v.bytes(1, "_hparams_/session_start_info");
    v.bytes(9, md.b);
    Pb s;
    s.bytes(1, v.b);
    Pb e;
    e.f64(1, now());
    e.bytes(5, s.b);
    record(e.b);
  }
  void flush() { f_.flush(); }

private:
  static double now() { return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count(); }
  void record(const std::string &data) {
    const uint64_t len = data.size();
    const uint32_t c1 = masked_crc(reinterpret_cast<const uint8_t *>(&len), 8);
    const uint32_t c2 = masked_crc(reinterpret_cast<const uint8_t *>(data.data()), data.size());
    f_.write(reinterpret_cast<const char *>(&len), 8);
    f_.write(reinterpret_cast<const char *>(&c1), 4);
    f_.write(data.data(), (std::streamsize)data.size());
    f_.write(reinterpret_cast<const char *>(&c2), 4);
  }
  std::ofstream f_;
};

// ------------------------------------------------------------------ [profile] argument: host spans + roctx ranges
class Profile {
public:
  explicit Profile(const std::string &path) : path_(path), t0_(std::chrono::steady_clock::now()) {
    if (path_.empty())
      return;
    if (void *h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL)) { // optional: markers for rocprofv3 --marker-trace
      push_ = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
      pop_ = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    }
  }
  bool on() const { return !path_.empty(); }
  struct Span {
    Profile *p;
    const char *name;
    double t0;
    Span(Profile *p_, const char *n) : p(p_), name(n), t0(0) {
      if (!p->on())
        return;
      t0 = p->now_us();
      if (p->push_)
        p->push_(name);
    }
    ~Span() {
      if (!p->on())
        return;
      if (p->pop_)
        p->pop_();
      p->events_.push_back({name, t0, p->now_us() - t0});
    }
  };
  void device_summary(aleppo_ctx *ctx) { // per-kernel-class device time (HIP events on the kernels' streams)
    static const char *names[ALEPPO_K_COUNT] = {"ingest", "gae", "head", "adam", "conv1_fwd", "conv2_fwd", "conv3_fwd",
                                                "fc_fwd", "fc_dgrad", "fc_wgrad", "conv3_dgrad", "conv3_wgrad",
                                                "conv2_dgrad", "conv2_wgrad", "conv1_wgrad", "reduce", "infer_head",
                                                "act_fused", "conv_fwd", "conv_bwd"};
    for (int k = 0; k < ALEPPO_K_COUNT; ++k) {
      double ms = 0;
      int64_t n = 0;
      if (aleppo_profile_read(ctx, k, &ms, &n) == ALEPPO_OK && n > 0)
        device_.push_back({names[k], ms, n});
    }
  }
  void save() {
    if (!on())
      return;
    std::ofstream f(path_);
    f << "{\"traceEvents\": [\n";
    bool first = true;
    for (auto &e : events_) {
      f << (first ? "" : ",\n") << "{\"name\": \"" << e.name << "\", \"ph\": \"X\", \"pid\": 1, \"tid\": 1, \"ts\": "
        << e.ts << ", \"dur\": " << e.dur << "}";
      first = false;
    }
    f << "\n],\n\"device_kernel_classes\": [\n";
    first = true;
    for (auto &d : device_) {
      f << (first ? "" : ",\n") << "{\"kernel_class\": \"" << d.name << "\", \"avg_ms\": " << d.ms
        << ", \"launches\": " << d.n << "}";
      first = false;
    }
    f << "\n]}\n";
  }

private:
  friend struct Span;
  double now_us() const { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0_).count(); }
  struct Ev {
    const char *name;
    double ts, dur;
  };
  struct Dev {
    const char *name;
    double ms;
    int64_t n;
  };
  std::string path_;
  std::chrono::steady_clock::time_point t0_;
  int (*push_)(const char *) = nullptr;
  int (*pop_)() = nullptr;
  std::vector<Ev> events_;
  std::vector<Dev> device_;
};

// ------------------------------------------------------------------ orthogonal init (train.cc:212-228)
// rows x cols matrix of N(0,1), orthonormalised (modified Gram-Schmidt on the smaller dimension), times gain
static void orthogonal(float *w, size_t rows, size_t cols, double gain, std::mt19937_64 &g) {
  std::normal_distribution<double> nd(0.0, 1.0);
  const bool tr = rows < cols;
  const size_t R = tr ? cols : rows, C = tr ? rows : cols; // R >= C: orthonormal columns
  std::vector<double> a(R * C);
  for (auto &v : a)
    v = nd(g);
  for (size_t j = 0; j < C; ++j) {
    for (size_t k = 0; k < j; ++k) {
      double dot = 0;
      for (size_t i = 0; i < R; ++i)
        dot += a[i * C + j] * a[i * C + k];
      for (size_t i = 0; i < R; ++i)
        a[i * C + j] -= dot * a[i * C + k];
    }
    double n = 0;
    for (size_t i = 0; i < R; ++i)
      n += a[i * C + j] * a[i * C + j];
    n = std::sqrt(n);
    for (size_t i = 0; i < R; ++i)
      a[i * C + j] /= n;
  }
  for (size_t r = 0; r < rows; ++r)
    for (size_t c = 0; c < cols; ++c)
      w[r * cols + c] = (float)(gain * (tr ? a[c * C + r] : a[r * C + c]));
}
static std::vector<float> init_params(size_t H, size_t A, uint64_t seed) { // libtorch parameters() order
  std::mt19937_64 g(seed);
  const double s2 = std::sqrt(2.0);
  struct T {
    size_t rows, cols;
    double gain;
  };
  const T t[6] = {{32, 4 * 8 * 8, s2}, {64, 32 * 4 * 4, s2}, {64, 64 * 3 * 3, s2}, {H, 3136, s2}, {A, H, 0.01}, {1, H, 1.0}};
  std::vector<float> p;
  for (const T &x : t) {
    const size_t o = p.size();
    p.resize(o + x.rows * x.cols + x.rows, 0.0f); // weight then zero bias
    orthogonal(p.data() + o, x.rows, x.cols, x.gain, g);
  }
  return p;
}

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

// ------------------------------------------------------------------ checkpoint file (INTEGRATION.md has the format)
// little-endian: magic, version, the shape header, sections of (u32 id, u64 byte length, bytes), the end mark
constexpr char CKPT_MAGIC[8] = {'A', 'L', 'E', 'P', 'P', 'O', 'C', 'K'};
constexpr char CKPT_END[8] = {'A', 'L', 'E', 'P', 'P', 'O', 'E', 'N'};
constexpr uint32_t CKPT_VERSION = 1;
enum CkptSection : uint32_t { CK_PARAMS = 1, CK_OPTIMIZER = 2, CK_REWARD_SCALE = 3, CK_ROLLOUT = 4, CK_TRAINER = 5, CK_DIGEST = 6 };
static const char *const DIGEST_NAMES[ALEPPO_DIGEST_COUNT] = {"params", "optimizer", "rollout", "reward_scale"};
struct CkptShape {
  uint32_t E, T, A, H, precision, world, rank, reserved;
  uint64_t param_count;
};
struct Checkpoint {
  CkptShape shape{};
  std::map<uint32_t, std::string> sections;
};
template <class T> static void put(std::string &out, const T &v) { out.append(reinterpret_cast<const char *>(&v), sizeof(T)); }
template <class T> static void put_vec(std::string &out, const std::vector<T> &v) {
  out.append(reinterpret_cast<const char *>(v.data()), v.size() * sizeof(T));
}
static void write_checkpoint_file(const std::string &path, const Checkpoint &ck) {
  std::string out(CKPT_MAGIC, 8);
  put(out, CKPT_VERSION);
  put(out, ck.shape);
  for (const auto &sec : ck.sections) {
    put(out, sec.first);
    put(out, (uint64_t)sec.second.size());
    out += sec.second;
  }
  out.append(CKPT_END, 8);
  const std::string tmp = path + ".tmp";
  {
    std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
    f.write(out.data(), (std::streamsize)out.size());
    f.flush();
    if (!f)
      throw std::runtime_error("cannot write checkpoint " + tmp);
  }
  std::filesystem::rename(tmp, path); // atomic: a reader sees a whole checkpoint under the final name, or the old one
}
// reads and checks the framing: every failure names the file and what is wrong with it
static Checkpoint read_checkpoint_file(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f)
    throw std::runtime_error("resume: cannot open checkpoint " + path);
  const std::string in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  size_t pos = 0;
  auto need = [&](size_t n) {
    if (in.size() - pos < n)
      throw std::runtime_error("resume: checkpoint " + path + " is truncated");
  };
  auto get = [&](void *dst, size_t n) {
    need(n);
    std::memcpy(dst, in.data() + pos, n);
    pos += n;
  };
  char magic[8];
  get(magic, 8);
  if (std::memcmp(magic, CKPT_MAGIC, 8) != 0)
    throw std::runtime_error("resume: " + path + " is not a checkpoint (wrong magic)");
  uint32_t version = 0;
  get(&version, 4);
  if (version != CKPT_VERSION)
    throw std::runtime_error("resume: checkpoint " + path + " has format version " + std::to_string(version) +
                             ", this build reads version " + std::to_string(CKPT_VERSION));
  Checkpoint ck;
  get(&ck.shape, sizeof(ck.shape));
  for (;;) {
    need(8);
    if (std::memcmp(in.data() + pos, CKPT_END, 8) == 0 && in.size() - pos == 8)
      break;
    uint32_t id = 0;
    uint64_t len = 0;
    get(&id, 4);
    get(&len, 8);
    if (len > in.size() - pos)
      throw std::runtime_error("resume: checkpoint " + path + " is truncated");
    ck.sections[id] = in.substr(pos, (size_t)len);
    pos += (size_t)len;
  }
  for (uint32_t id : {CK_PARAMS, CK_OPTIMIZER, CK_REWARD_SCALE, CK_ROLLOUT, CK_TRAINER, CK_DIGEST})
    if (!ck.sections.count(id))
      throw std::runtime_error("resume: checkpoint " + path + " lacks section " + std::to_string(id));
  return ck;
}
// the shape the file was written for against this run's; the section sizes that follow from it
static void check_checkpoint_shape(const std::string &path, const Checkpoint &ck, const CkptShape &want) {
  const struct {
    const char *name;
    uint64_t file, run;
  } f[] = {{"total_environments / WORLD_SIZE", ck.shape.E, want.E}, {"horizon", ck.shape.T, want.T},
           {"action_size", ck.shape.A, want.A},                     {"hidden_size", ck.shape.H, want.H},
           {"precision", ck.shape.precision, want.precision},       {"WORLD_SIZE", ck.shape.world, want.world},
           {"RANK", ck.shape.rank, want.rank},                      {"parameter count", ck.shape.param_count, want.param_count}};
  for (const auto &x : f)
    if (x.file != x.run)
      throw std::runtime_error("resume: checkpoint " + path + " was written for " + x.name + " = " +
                               std::to_string(x.file) + ", this run has " + std::to_string(x.run));
  const size_t n = (size_t)want.param_count, E = want.E;
  const size_t trainer_bytes = 4 * 8 + 4 + 4 * E + 3 * 4 * E + 2 * 8 * E + E * SyntheticAtari::state_bytes;
  const std::pair<uint32_t, size_t> sizes[] = {{CK_PARAMS, n * 4},
                                               {CK_OPTIMIZER, 2 * n * 4 + 8},
                                               {CK_REWARD_SCALE, (3 + E) * 8},
                                               {CK_ROLLOUT, 4 * 8 + E * 4 * 84 * 84},
                                               {CK_TRAINER, trainer_bytes},
                                               {CK_DIGEST, ALEPPO_DIGEST_COUNT * 8}};
  for (const auto &sz : sizes)
    if (ck.sections.at(sz.first).size() != sz.second)
      throw std::runtime_error("resume: checkpoint " + path + " is corrupt (section " + std::to_string(sz.first) + " has " +
                               std::to_string(ck.sections.at(sz.first).size()) + " bytes, expected " +
                               std::to_string(sz.second) + ")");
}
static size_t reference_param_count(size_t H, size_t A) { // libtorch parameters() element count of the network
  return 32 * 256 + 32 + 64 * 512 + 64 + 64 * 576 + 64 + H * 3136 + H + A * H + A + H + 1;
}

int main(int argc, char **argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s <rom> <tensorboard log path> <video dir> <group> <config.yaml> [profile]\n", argv[0]);
    return 2;
  }
  try {
    const auto start_time = std::chrono::system_clock::now().time_since_epoch().count();
    const std::string rom_path = argv[1], group = argv[4];
    const std::string profile_path = argc > 6 ? argv[6] : ""; // train.cc:328-335
    Profile prof(profile_path);
    std::string log_path = argv[2];
    { // replace_extension("tfevents.<start-time>") like train.cc:324-325
      const size_t slash = log_path.find_last_of('/'), dot = log_path.find_last_of('.');
      if (dot != std::string::npos && (slash == std::string::npos || dot > slash))
        log_path = log_path.substr(0, dot);
      log_path += ".tfevents." + std::to_string(start_time);
    }
    const Config cfg = load_config(argv[5]);
    { // train.cc:347-352: create the log (and video) directories
      const auto parent = std::filesystem::path(log_path).parent_path();
      if (!parent.empty() && !std::filesystem::exists(parent))
        std::filesystem::create_directories(parent);
    }
    auto env_int = [](const char *k, int dflt) {
      const char *v = std::getenv(k);
      return v ? std::atoi(v) : dflt;
    };
    const int world = std::max(1, env_int("WORLD_SIZE", 1)), rank = env_int("RANK", 0), local_rank = env_int("LOCAL_RANK", rank);
    if (rank < 0 || rank >= world)
      throw std::runtime_error("RANK must be in [0, WORLD_SIZE)");
    if (cfg.total_environments % (size_t)world)
      throw std::runtime_error("total_environments must be divisible by WORLD_SIZE");
    const size_t E = cfg.total_environments / (size_t)world, T = cfg.horizon, A = cfg.action_size; // E: THIS rank's envs
    const size_t env0 = (size_t)rank * E;                                                           // its first environment
    if ((E * T) % (size_t)cfg.num_mini_batches)
      throw std::runtime_error("Batch size must be divisible by num_mini_batches");
    if (E % cfg.worker_batch_size)
      std::cerr << "warning: total_environments % worker_batch_size != 0 would deadlock the reference's queue\n";
    if (cfg.record_video)
      std::cerr << "note: record_video ignored (no ffmpeg / ALE in this build)\n";

    // checkpoint / resume: refused here, before anything is created, when the library or the file cannot serve it
    const bool ckpt_keys = !cfg.checkpoint_path.empty() || !cfg.resume.empty();
    if (ckpt_keys && !(aleppo_export_rollout_state && aleppo_import_rollout_state && aleppo_state_digest &&
                       aleppo_export_optimizer && aleppo_import_optimizer && aleppo_export_reward_scale &&
                       aleppo_import_reward_scale))
      throw std::runtime_error("checkpoint_path / checkpoint_interval / resume are set but this build's library cannot "
                               "checkpoint a run (aleppo_export_rollout_state is missing)");
    const std::string rank_suffix = world > 1 ? ".rank" + std::to_string(rank) : "";
    const std::string ckpt_file = cfg.checkpoint_path.empty() ? "" : cfg.checkpoint_path + rank_suffix;
    const std::string resume_file = cfg.resume.empty() ? "" : cfg.resume + rank_suffix;
    CkptShape ckpt_shape{(uint32_t)E, (uint32_t)T, (uint32_t)A, (uint32_t)cfg.hidden_size,
                         (uint32_t)(cfg.precision == "bf16" ? ALEPPO_BF16 : ALEPPO_FP32), (uint32_t)world, (uint32_t)rank, 0,
                         (uint64_t)reference_param_count(cfg.hidden_size, A)};
    Checkpoint resumed;
    if (!resume_file.empty()) {
      resumed = read_checkpoint_file(resume_file);
      check_checkpoint_shape(resume_file, resumed, ckpt_shape);
    }
    if (const char *dump = std::getenv("ALEPPO_TRAINER_DUMP_INIT")) { // test hook: the initial parameters, no GPU needed
      const std::vector<float> p = init_params(cfg.hidden_size, A, cfg.deterministic ? 42 : (uint64_t)start_time);
      std::ofstream f(dump, std::ios::binary);
      f.write(reinterpret_cast<const char *>(p.data()), (std::streamsize)(p.size() * sizeof(float)));
      std::cout << "initial parameters written: " << p.size() << std::endl;
      return 0;
    }
    if (cfg.eval_interval > 0 && !(aleppo_eval_open && aleppo_eval_push_frames && aleppo_eval_act && aleppo_eval_read))
      throw std::runtime_error("eval_interval is set but this build's library has no evaluation lanes "
                               "(aleppo_eval_open is missing)");
    if (cfg.reward_scaling && !(aleppo_export_reward_scale && aleppo_import_reward_scale))
      throw std::runtime_error("reward_scaling is set but this build's library has no reward scaling "
                               "(aleppo_export_reward_scale is missing)");
    aleppo_config ac{};
    ac.abi_version = ALEPPO_ABI_VERSION;
    ac.device_ordinal = local_rank;
    ac.world_size = world;
    ac.rank = rank;
    ac.num_envs = (int32_t)E;
    ac.horizon = (int32_t)T;
    ac.num_actions = (int32_t)A;
    ac.hidden_size = (int32_t)cfg.hidden_size;
    ac.frame_stack = (int32_t)cfg.frame_stack;
    ac.precision = cfg.precision == "bf16" ? ALEPPO_BF16 : ALEPPO_FP32;
    ac.rollout_precision = cfg.rollout_precision == "fp16" ? ALEPPO_ROLLOUT_FP16 : ALEPPO_ROLLOUT_FP32;
    ac.advantage_norm = cfg.advantage_norm;
    ac.gamma = cfg.gae_discount;
    ac.lambda = cfg.gae_lambda;
    ac.clip_param = cfg.clip_param;
    ac.value_loss_coef = cfg.value_loss_coef;
    ac.entropy_coef = cfg.entropy_coef;
    ac.max_gradient_norm = cfg.max_gradient_norm;
    ac.seed = cfg.seed;
    aleppo_ctx *ctx = nullptr;
    check(nullptr, aleppo_create(&ac, &ctx));
    std::cout << "MI355X is available! Training on GPU (rom argument '" << rom_path << "' -> synthetic emulator)."
              << std::endl;
    if (world > 1) {
      // RCCL communicator: rank 0's 128-byte id travels through a file next to the log.  The file belongs to ONE launch:
      // its name carries the launcher's MASTER_PORT (+ torchrun's run id when there is one), rank 0 removes whatever a
      // crashed earlier launch left under that name BEFORE it creates the id and removes its own file once every rank
      // has joined (aleppo_comm_init is collective), and the other ranks ignore a file older than their own start: a
      // stale id would leave ncclCommInitRank waiting for ever on mismatched ids.
      std::string nonce = std::getenv("MASTER_PORT") ? std::getenv("MASTER_PORT") : "0";
      if (const char *rid = std::getenv("TORCHELASTIC_RUN_ID"))
        nonce += std::string(".") + rid;
      const std::string idfile = std::string(argv[2]) + ".rcclid." + nonce;
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
        const double limit = std::getenv("ALEPPO_RENDEZVOUS_TIMEOUT_S") ? std::atof(std::getenv("ALEPPO_RENDEZVOUS_TIMEOUT_S")) : 300.0;
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
      check(ctx, aleppo_comm_init(ctx, id));
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
      std::cout << "rank " << rank << " of " << world << ": environments [" << env0 << ", " << env0 + E << ")" << std::endl;
    }
    {
      const std::vector<float> p = init_params(cfg.hidden_size, A, cfg.deterministic ? 42 : (uint64_t)start_time);
      size_t n = 0;
      check(ctx, aleppo_param_count(ctx, &n));
      if (n != p.size())
        throw std::runtime_error("parameter count mismatch");
      check(ctx, aleppo_load_params(ctx, p.data(), p.size()));
    }
    EventWriter logger(rank == 0 ? log_path : log_path + ".rank" + std::to_string(rank)); // rank 0's file is THE log
    if (cfg.cuda_graph) // the reference's `cuda_graph: true`: replay the update loop as a captured graph
      check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_UPDATE_GRAPH, 1));
    if (cfg.shuffle_minibatches) // extension: minibatches of a fresh per-epoch permutation instead of contiguous slices
      check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_MINIBATCH_SHUFFLE, 1));
    if (cfg.clip_value_loss) // extension: the clipped value loss of ppo2 / CleanRL (clip range = clip_param)
      check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_VALUE_CLIP, 1));
    if (cfg.minibatch_advantage_norm) // extension: each minibatch's advantages normalised before the loss (norm_adv)
      check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_ADV_NORM_MINIBATCH, 1));
    const bool kl_pen = cfg.kl_coef > 0; // extension: the KL penalty; beta is set before every update (adapted below)
    float kl_beta = kl_pen ? (float)cfg.kl_coef : 0.0f;
    if (kl_pen)
      check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_KL_PENALTY, 1));
    auto set_float_option = [&](int option, float v) { // (the options take the binary32 bit pattern)
      int32_t bits;
      std::memcpy(&bits, &v, 4);
      check(ctx, aleppo_set_option(ctx, option, bits));
    };
    if (cfg.value_clip_range_set) // extension: a value-clip range of its own (constant)
      set_float_option(ALEPPO_OPT_VALUE_CLIP_RANGE, (float)cfg.value_clip_range);
    if (cfg.reward_scaling) { // extension: rewards divided by the running return's std and clipped, not clamped to +-1
      set_float_option(ALEPPO_OPT_REWARD_SCALE_CLIP, (float)cfg.reward_scale_clip);
      check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_REWARD_SCALE, 1));
    }
    // extension: linear schedules of the clip range, the loss coefficients and the norm limit, one value per rollout
    struct HyperSchedule {
      const char *name; // the scalar's tag: the config key it schedules
      int option;
      double v0, v1;
    };
    std::vector<HyperSchedule> hyper_schedules;
    if (cfg.clip_param_final_set)
      hyper_schedules.push_back({"clip_param", ALEPPO_OPT_CLIP_PARAM, cfg.clip_param, cfg.clip_param_final});
    if (cfg.value_loss_coef_final_set)
      hyper_schedules.push_back({"value_loss_coef", ALEPPO_OPT_VALUE_LOSS_COEF, cfg.value_loss_coef,
                                 cfg.value_loss_coef_final});
    if (cfg.entropy_coef_final_set)
      hyper_schedules.push_back({"entropy_coef", ALEPPO_OPT_ENTROPY_COEF, cfg.entropy_coef, cfg.entropy_coef_final});
    if (cfg.max_gradient_norm_final_set)
      hyper_schedules.push_back({"max_gradient_norm", ALEPPO_OPT_MAX_GRAD_NORM, cfg.max_gradient_norm,
                                 cfg.max_gradient_norm_final});
    if (prof.on())
      check(ctx, aleppo_profile_enable(ctx, 1));
    std::vector<std::pair<std::string, double>> hparam_numbers_eval;
    std::vector<std::pair<std::string, bool>> hparam_flags{{"record_observation", cfg.record_observation},
                                                           {"record_video", cfg.record_video},
                                                           {"cuda_graph", cfg.cuda_graph},
                                                           {"deterministic", cfg.deterministic}};
    if (cfg.shuffle_minibatches) // (only when set: the records of existing configs stay byte-identical)
      hparam_flags.emplace_back("shuffle_minibatches", true);
    if (cfg.clip_value_loss)
      hparam_flags.emplace_back("clip_value_loss", true);
    if (cfg.minibatch_advantage_norm)
      hparam_flags.emplace_back("minibatch_advantage_norm", true);
    if (cfg.log_batch_stats)
      hparam_flags.emplace_back("log_batch_stats", true);
    if (cfg.reward_scaling)
      hparam_flags.emplace_back("reward_scaling", true);
    if (cfg.eval_interval > 0) { // (only when set, like the others)
      hparam_numbers_eval = {{"eval_interval", (double)cfg.eval_interval},
                             {"eval_environments", (double)cfg.eval_environments},
                             {"eval_episodes", (double)cfg.eval_episodes},
                             {"eval_rule", cfg.eval_rule == "greedy" ? 0.0 : cfg.eval_rule == "sample" ? 1.0 : 2.0},
                             {"eval_temperature", cfg.eval_temperature},
                             {"eval_epsilon", cfg.eval_epsilon}};
    }
    std::vector<std::pair<std::string, double>> hparam_numbers{ // get_parameters (train.cc:76-105), same keys
        {"total_environments", (double)cfg.total_environments}, {"hidden_size", (double)cfg.hidden_size},
        {"action_size", (double)cfg.action_size}, {"horizon", (double)cfg.horizon}, {"max_steps", (double)cfg.max_steps},
        {"frame_stack", (double)cfg.frame_stack}, {"learning_rate", cfg.learning_rate}, {"clip_param", cfg.clip_param},
        {"value_loss_coef", cfg.value_loss_coef}, {"entropy_coef", cfg.entropy_coef},
        {"num_epochs", (double)cfg.num_epochs}, {"mini_batch_size", (double)cfg.mini_batch_size},
        {"num_mini_batches", (double)cfg.num_mini_batches}, {"gae_discount", cfg.gae_discount},
        {"gae_lambda", cfg.gae_lambda}, {"max_gradient_norm", cfg.max_gradient_norm},
        {"num_rollouts", (double)cfg.num_rollouts}, {"num_workers", (double)cfg.num_workers},
        {"worker_batch_size", (double)cfg.worker_batch_size}, {"frame_skip", (double)cfg.frame_skip},
        {"max_return", cfg.max_return}};
    if (cfg.kl_coef_set) // (only when set, like the flags above)
      hparam_numbers.emplace_back("kl_coef", cfg.kl_coef);
    if (cfg.kl_target_set)
      hparam_numbers.emplace_back("kl_target", cfg.kl_target);
    if (cfg.clip_param_final_set)
      hparam_numbers.emplace_back("clip_param_final", cfg.clip_param_final);
    if (cfg.value_loss_coef_final_set)
      hparam_numbers.emplace_back("value_loss_coef_final", cfg.value_loss_coef_final);
    if (cfg.entropy_coef_final_set)
      hparam_numbers.emplace_back("entropy_coef_final", cfg.entropy_coef_final);
    if (cfg.max_gradient_norm_final_set)
      hparam_numbers.emplace_back("max_gradient_norm_final", cfg.max_gradient_norm_final);
    if (cfg.value_clip_range_set)
      hparam_numbers.emplace_back("value_clip_range", cfg.value_clip_range);
    hparam_numbers.insert(hparam_numbers.end(), hparam_numbers_eval.begin(), hparam_numbers_eval.end());
    logger.add_hparams(hparam_numbers, hparam_flags, group, (double)start_time * 1e-9);

    // ---- Rollout host half (src/ai/rollout.cc)
    std::vector<SyntheticAtari> envs;
    for (size_t i = 0; i < E; ++i)
      envs.emplace_back(env0 + i + 0 /*seed arg of train.cc:380*/, cfg.max_steps, cfg.max_return, A, cfg.device_preprocess);
    // the workers' frame buffer: page-locked + GPU-mapped, read in place by the ingest kernel (see the file header)
    uint8_t *frames = nullptr;
    const size_t fbytes = SyntheticAtari::frame_bytes(cfg.device_preprocess); // per environment
    check(ctx, aleppo_host_alloc(ctx, E * fbytes, reinterpret_cast<void **>(&frames)));
    if (cfg.device_preprocess) { // ALE's palette -> gray table would go here; the synthetic palette is its own gray value
      uint8_t lut[256];
      for (int i = 0; i < 256; ++i)
        lut[i] = (uint8_t)i;
      check(ctx, aleppo_set_gray_lut(ctx, lut));
    }
    // episode-start flags at slot entry, where the armed ingest kernel reads them (mapped like the frames)
    uint8_t *start_mapped = nullptr;
    check(ctx, aleppo_host_alloc(ctx, E, reinterpret_cast<void **>(&start_mapped)));
    const bool slot_ahead = cfg.slot_ahead && !prof.on(); // (per-kernel device profiling brackets every launch)
    std::vector<uint8_t> start_cpu(E, 1), term(E, 0), trunc(E, 0), game_over(E, 0);
    std::vector<float> rewards(E, 0.f), ep_ret(E, 0.f), game_ret(E, 0.f);
    std::vector<size_t> ep_len(E, 0), game_len(E, 0);
    std::vector<StepOut> results(E);
    const int64_t *actions = nullptr;
    size_t total_steps = 0, episodes = 0;
    std::cout << "Creating " << cfg.num_workers << " worker threads." << std::endl;
    std::atomic<bool> eval_mode{false}; // the pool steps the evaluation emulators instead (set around run_all only)
    std::function<void(size_t)> eval_step;
    WorkerPool pool(cfg.num_workers, [&](size_t i) { // Rollout::step (rollout.cc:299-328)
      if (eval_mode.load()) {
        eval_step(i);
        return;
      }
      if (start_cpu[i]) {
        envs[i].reset(&frames[i * fbytes]);
        results[i] = StepOut{};
      } else {
        const int64_t a = actions[i];
        if (a < 0 || (size_t)a >= A)
          throw std::out_of_range("Action index out of range for environment " + std::to_string(i));
        results[i] = envs[i].step((int)a, &frames[i * fbytes]);
      }
    });
    struct Log {
      std::vector<float> episode_returns, game_returns;
      std::vector<size_t> episode_lengths, game_lengths;
    };
    auto rollout = [&]() {
      Log log;
      for (size_t t = 0; t < T; ++t) {
        {
          Profile::Span sp(&prof, "aleppo_act");
          check(ctx, aleppo_act(ctx, nullptr, &actions));
        }
        std::vector<uint8_t> start_at_entry = start_cpu;
        const int fkind = cfg.device_preprocess ? ALEPPO_FRAMES_RAW_PAIR : ALEPPO_FRAMES_84;
        if (slot_ahead) { // slot t + 1's kernels go onto the stream now; they start when release_step lifts the wait
          std::memcpy(start_mapped, start_at_entry.data(), E);
          check(ctx, aleppo_arm_step(ctx, frames, fkind, start_mapped, nullptr));
        }
        {
          Profile::Span sp(&prof, "step_all (emulator threads)");
          pool.run_all(E);
        }
        for (size_t i = 0; i < E; ++i) {
          if (!start_cpu[i]) { // rollout.cc:214-226 (start slots keep the stale reward)
            rewards[i] = results[i].reward;
            term[i] = results[i].terminated;
            trunc[i] = results[i].truncated;
            game_over[i] = results[i].game_over;
            ep_ret[i] += results[i].reward;
            ep_len[i]++;
            game_ret[i] += results[i].reward;
            game_len[i]++;
            total_steps++;
          }
        }
        if (slot_ahead) {
          check(ctx, aleppo_release_step(ctx, rewards.data(), term.data(), trunc.data()));
        } else {
          Profile::Span sp(&prof, "aleppo_step");
          check(ctx, aleppo_step(ctx, frames, fkind, ALEPPO_HOST_MAPPED, rewards.data(), term.data(), trunc.data(),
                                 start_at_entry.data()));
        }
        for (size_t i = 0; i < E; ++i) { // rollout.cc:239-265
          if (results[i].terminated || results[i].truncated) {
            start_cpu[i] = 1;
            term[i] = trunc[i] = 0;
            episodes++;
            log.episode_returns.push_back(ep_ret[i]);
            log.episode_lengths.push_back(ep_len[i]);
            ep_ret[i] = 0;
            ep_len[i] = 0;
            if (game_over[i]) {
              log.game_returns.push_back(game_ret[i]);
              log.game_lengths.push_back(game_len[i]);
              game_ret[i] = 0;
              game_len[i] = 0;
            }
          } else if (start_cpu[i]) {
            start_cpu[i] = 0;
          }
        }
      }
      {
        Profile::Span sp(&prof, "aleppo_finish_rollout");
        check(ctx, aleppo_finish_rollout(ctx, nullptr));
      }
      return log;
    };

    // ---- evaluation (eval_interval): full episodes on emulators of its own through the evaluation lanes.  Nothing here
    // touches the training emulators, their flags or the rollout: the lanes have their own stacks, scratch and noise stream.
    const size_t L = cfg.eval_interval > 0 ? cfg.eval_environments : 0;
    std::vector<SyntheticAtari> eval_envs;
    uint8_t *eval_frames = nullptr;
    std::vector<uint8_t> eval_start(L, 1);
    std::vector<StepOut> eval_results(L);
    const int64_t *eval_actions = nullptr;
    if (L > 0) {
      check(ctx, aleppo_eval_open(ctx, (int32_t)L));
      check(ctx, aleppo_host_alloc(ctx, L * fbytes, reinterpret_cast<void **>(&eval_frames)));
    }
    eval_step = [&](size_t i) {
      if (eval_start[i]) {
        eval_envs[i].reset(&eval_frames[i * fbytes]);
        eval_results[i] = StepOut{};
      } else {
        const int64_t a = eval_actions[i];
        if (a < 0 || (size_t)a >= A)
          throw std::out_of_range("Action index out of range for evaluation environment " + std::to_string(i));
        eval_results[i] = eval_envs[i].step((int)a, &eval_frames[i * fbytes]);
      }
    };
    struct EvalLog {
      float return_mean = 0, return_max = 0, length_mean = 0;
      size_t episodes = 0;
    };
    auto evaluate = [&](size_t round) {
      // fresh emulators per evaluation, seeded past every rank's training environments (env0 + i < total_environments)
      eval_envs.clear();
      for (size_t i = 0; i < L; ++i)
        eval_envs.emplace_back(cfg.total_environments + (round * (size_t)world + (size_t)rank) * L + i, cfg.max_steps,
                               cfg.max_return, A, cfg.device_preprocess);
      std::fill(eval_start.begin(), eval_start.end(), 1);
      std::vector<float> ret(L, 0.f), returns;
      std::vector<size_t> len(L, 0), lengths;
      const int rule = cfg.eval_rule == "greedy" ? ALEPPO_EVAL_GREEDY
                                                 : cfg.eval_rule == "sample" ? ALEPPO_EVAL_SAMPLE : ALEPPO_EVAL_EPSILON_GREEDY;
      const float param = rule == ALEPPO_EVAL_SAMPLE ? (float)cfg.eval_temperature
                                                     : rule == ALEPPO_EVAL_EPSILON_GREEDY ? (float)cfg.eval_epsilon : 0.f;
      const int fkind = cfg.device_preprocess ? ALEPPO_FRAMES_RAW_PAIR : ALEPPO_FRAMES_84;
      while (returns.size() < cfg.eval_episodes) {
        check(ctx, aleppo_eval_act(ctx, rule, param, nullptr, &eval_actions));
        const std::vector<uint8_t> start_at_entry = eval_start;
        eval_mode.store(true);
        pool.run_all(L);
        eval_mode.store(false);
        check(ctx, aleppo_eval_push_frames(ctx, eval_frames, fkind, ALEPPO_HOST_MAPPED, start_at_entry.data()));
        for (size_t i = 0; i < L; ++i) {
          if (!start_at_entry[i]) {
            ret[i] += eval_results[i].reward;
            len[i]++;
          }
          if (eval_results[i].terminated || eval_results[i].truncated) {
            if (returns.size() < cfg.eval_episodes) { // (the first eval_episodes to finish, in lane order within a step)
              returns.push_back(ret[i]);
              lengths.push_back(len[i]);
            }
            ret[i] = 0;
            len[i] = 0;
            eval_start[i] = 1;
          } else {
            eval_start[i] = 0;
          }
        }
      }
      // the ingest of the last push reads eval_frames in place: it must have run before the next evaluation's workers
      // (or the training loop's host_free) touch the buffer
      // (aleppo_eval_read synchronises the context's stream)
      std::vector<float> last_values(L);
      check(ctx, aleppo_eval_read(ctx, ALEPPO_EF_VALUES, last_values.data(), L * sizeof(float)));
      EvalLog e;
      e.return_mean = meanf(returns);
      e.return_max = *std::max_element(returns.begin(), returns.end());
      e.length_mean = meanf(lengths);
      e.episodes = returns.size();
      return e;
    };

    // ---- checkpoint / resume: the whole run state between two rollouts
    const size_t n_params = (size_t)ckpt_shape.param_count;
    auto save_checkpoint = [&](size_t next_rollout) {
      Profile::Span sp(&prof, "checkpoint");
      Checkpoint ck;
      ck.shape = ckpt_shape;
      std::vector<float> p(n_params), m1(n_params), m2(n_params);
      int64_t adam_step = 0;
      check(ctx, aleppo_export_params(ctx, p.data(), n_params));
      check(ctx, aleppo_export_optimizer(ctx, m1.data(), m2.data(), &adam_step, n_params));
      std::string &so = ck.sections[CK_OPTIMIZER];
      put_vec(ck.sections[CK_PARAMS], p);
      put_vec(so, m1);
      put_vec(so, m2);
      put(so, adam_step);
      std::vector<double> rs(3 + E);
      check(ctx, aleppo_export_reward_scale(ctx, rs.data(), rs.data() + 3, E));
      put_vec(ck.sections[CK_REWARD_SCALE], rs);
      std::vector<uint8_t> obs(E * 4 * 84 * 84);
      uint64_t words[ALEPPO_ROLLOUT_STATE_WORDS];
      check(ctx, aleppo_export_rollout_state(ctx, obs.data(), words, E));
      std::string &sr = ck.sections[CK_ROLLOUT];
      put(sr, words);
      put_vec(sr, obs);
      std::string &st = ck.sections[CK_TRAINER];
      put(st, (uint64_t)next_rollout);
      put(st, (uint64_t)total_steps);
      put(st, (uint64_t)episodes);
      put(st, (uint64_t)next_rollout); // the schedule position: the rollout index the annealed values are functions of
      put(st, kl_beta);
      put_vec(st, start_cpu);
      put_vec(st, term);
      put_vec(st, trunc);
      put_vec(st, game_over);
      put_vec(st, rewards);
      put_vec(st, ep_ret);
      put_vec(st, game_ret);
      put_vec(st, std::vector<uint64_t>(ep_len.begin(), ep_len.end()));
      put_vec(st, std::vector<uint64_t>(game_len.begin(), game_len.end()));
      for (const SyntheticAtari &e : envs)
        e.save(st);
      uint64_t dg[ALEPPO_DIGEST_COUNT];
      check(ctx, aleppo_state_digest(ctx, dg));
      put(ck.sections[CK_DIGEST], dg);
      write_checkpoint_file(ckpt_file, ck);
      char line[256];
      std::snprintf(line, sizeof line, "checkpoint rollout %zu digest params=%016llx optimizer=%016llx rollout=%016llx "
                    "reward_scale=%016llx", next_rollout, (unsigned long long)dg[0], (unsigned long long)dg[1],
                    (unsigned long long)dg[2], (unsigned long long)dg[3]);
      std::cout << line << " -> " << ckpt_file << std::endl;
    };
    size_t first_rollout = 0;
    if (!resume_file.empty()) { // import everything, then prove it: the device's digest against the file's
      const auto sec = [&](uint32_t id) { return reinterpret_cast<const uint8_t *>(resumed.sections.at(id).data()); };
      auto take = [](const uint8_t *&p, void *dst, size_t n) {
        std::memcpy(dst, p, n);
        p += n;
      };
      std::vector<float> p(n_params), m1(n_params), m2(n_params);
      int64_t adam_step = 0;
      std::memcpy(p.data(), sec(CK_PARAMS), n_params * 4);
      const uint8_t *q = sec(CK_OPTIMIZER);
      take(q, m1.data(), n_params * 4);
      take(q, m2.data(), n_params * 4);
      take(q, &adam_step, 8);
      check(ctx, aleppo_load_params(ctx, p.data(), n_params)); // (resets the Adam state, restored next)
      check(ctx, aleppo_import_optimizer(ctx, m1.data(), m2.data(), adam_step, n_params));
      std::vector<double> rs(3 + E);
      std::memcpy(rs.data(), sec(CK_REWARD_SCALE), rs.size() * 8);
      check(ctx, aleppo_import_reward_scale(ctx, rs.data(), rs.data() + 3, E));
      uint64_t words[ALEPPO_ROLLOUT_STATE_WORDS];
      q = sec(CK_ROLLOUT);
      take(q, words, sizeof(words));
      check(ctx, aleppo_import_rollout_state(ctx, q, words, E));
      q = sec(CK_TRAINER);
      uint64_t u[4];
      take(q, u, sizeof(u));
      if (u[0] > cfg.num_rollouts || u[3] != u[0])
        throw std::runtime_error("resume: checkpoint " + resume_file + " continues at rollout " + std::to_string(u[0]) +
                                 ", this run has " + std::to_string(cfg.num_rollouts));
      first_rollout = (size_t)u[0];
      total_steps = (size_t)u[1];
      episodes = (size_t)u[2];
      take(q, &kl_beta, 4);
      take(q, start_cpu.data(), E);
      take(q, term.data(), E);
      take(q, trunc.data(), E);
      take(q, game_over.data(), E);
      take(q, rewards.data(), E * 4);
      take(q, ep_ret.data(), E * 4);
      take(q, game_ret.data(), E * 4);
      std::vector<uint64_t> l64(E);
      take(q, l64.data(), E * 8);
      std::copy(l64.begin(), l64.end(), ep_len.begin());
      take(q, l64.data(), E * 8);
      std::copy(l64.begin(), l64.end(), game_len.begin());
      for (SyntheticAtari &e : envs) {
        e.load(q);
        q += SyntheticAtari::state_bytes;
      }
      uint64_t want[ALEPPO_DIGEST_COUNT], got[ALEPPO_DIGEST_COUNT];
      std::memcpy(want, sec(CK_DIGEST), sizeof(want));
      check(ctx, aleppo_state_digest(ctx, got));
      for (int k = 0; k < ALEPPO_DIGEST_COUNT; ++k)
        if (want[k] != got[k]) {
          char b[160];
          std::snprintf(b, sizeof b, ": the %s digest after the import is %016llx, the file recorded %016llx",
                        DIGEST_NAMES[k], (unsigned long long)got[k], (unsigned long long)want[k]);
          throw std::runtime_error("resume: checkpoint " + resume_file + b);
        }
      std::cout << "resumed from " << resume_file << " at rollout " << first_rollout << " of " << cfg.num_rollouts
                << ", state digest verified" << std::endl;
    } else {
      rollout(); // the warm rollout before the loop (train.cc:391-396): collected, never trained on
    }
    // test hook: stop (cleanly) right after the checkpoint that continues at this rollout index, as an interruption would
    const long stop_after = std::getenv("ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT")
                                ? std::atol(std::getenv("ALEPPO_TRAINER_STOP_AFTER_CHECKPOINT"))
                                : -1;
    size_t rollouts_done = first_rollout;
    const auto t_begin = std::chrono::steady_clock::now();
    const size_t nmb = (size_t)cfg.num_mini_batches, N = E * T;
    // metrics of every epoch that ran: per minibatch, and the per-sample planes of log_data's histograms ([epochs][N])
    std::vector<aleppo_minibatch_metrics> m((size_t)cfg.num_epochs * nmb);
    std::vector<float> kl((size_t)cfg.num_epochs * nmb), cf((size_t)cfg.num_epochs * nmb);
    std::vector<float> adv_std(cfg.minibatch_advantage_norm ? (size_t)cfg.num_epochs * nmb : 0);
    std::vector<float> mean_kl(kl_pen ? (size_t)cfg.num_epochs * nmb : 0);
    const std::pair<int, const char *> sample_fields[5] = {{ALEPPO_M_TOTAL_LOSSES, "losses"},
                                                           {ALEPPO_M_CLIPPED_LOSSES, "clipped_losses"},
                                                           {ALEPPO_M_VALUE_LOSSES, "value_losses"},
                                                           {ALEPPO_M_ENTROPIES, "entropies"},
                                                           {ALEPPO_M_RATIO, "ratios"}};
    std::vector<std::vector<float>> planes(5, std::vector<float>((size_t)cfg.num_epochs * N));
    for (size_t r = first_rollout; r < cfg.num_rollouts; ++r) {
      std::cout << "Rollout " << r + 1 << " of " << cfg.num_rollouts << std::endl;
      const double lr = cfg.learning_rate * (1.0 - r / static_cast<double>(cfg.num_rollouts)); // train.cc:424-428
      const Log log = rollout();
      double rstats[ALEPPO_REWARD_SCALE_COUNT] = {}, rrms[3] = {0.0, 0.0, 1.0};
      if (cfg.reward_scaling) { // what this rollout's finish_rollout did (the state is global under data parallelism)
        std::vector<double> running(E);
        check(ctx, aleppo_read_batch(ctx, ALEPPO_F_REWARD_SCALE, rstats, sizeof(rstats)));
        check(ctx, aleppo_export_reward_scale(ctx, rrms, running.data(), running.size()));
      }
      double bstats[ALEPPO_BATCH_STATS_COUNT] = {};
      if (cfg.log_batch_stats) { // of the rollout batch as the update below will see it; every rank calls (collective)
        Profile::Span sp(&prof, "read_batch_stats");
        check(ctx, aleppo_read_batch(ctx, ALEPPO_F_BATCH_STATS, bstats, sizeof(bstats)));
      }
      // one call of num_epochs epochs, or - with target_kl - one call per epoch until an epoch's last minibatch is over
      // the target (the Adam schedule and the shuffle keys follow the Adam step, so the calls add up to the same update)
      size_t epochs_run = 0;
      const size_t per_call = cfg.target_kl > 0 ? 1 : (size_t)cfg.num_epochs;
      // this rollout's scheduled hyper-parameters (a function of r alone: the same on every rank)
      std::vector<float> hyper_now(hyper_schedules.size());
      for (size_t k = 0; k < hyper_schedules.size(); ++k) {
        const HyperSchedule &h = hyper_schedules[k];
        hyper_now[k] = (float)(h.v0 + (h.v1 - h.v0) * (r / static_cast<double>(cfg.num_rollouts)));
        set_float_option(h.option, hyper_now[k]);
      }
      if (kl_pen) { // beta of this rollout's update, as its binary32 bit pattern
        int32_t bits;
        std::memcpy(&bits, &kl_beta, 4);
        check(ctx, aleppo_set_option(ctx, ALEPPO_OPT_KL_COEF, bits));
      }
      while (epochs_run < (size_t)cfg.num_epochs) {
        const size_t e0 = epochs_run;
        {
          Profile::Span sp(&prof, "aleppo_train");
          check(ctx, aleppo_train(ctx, lr, (int)per_call, (int)nmb, m.data() + e0 * nmb));
        }
        Profile::Span sp_read(&prof, "read_train_metrics");
        check(ctx, aleppo_read_train_metric(ctx, ALEPPO_M_MEAN_APPROX_KL, kl.data() + e0 * nmb, per_call * nmb));
        check(ctx, aleppo_read_train_metric(ctx, ALEPPO_M_MEAN_CLIP_FRACTION, cf.data() + e0 * nmb, per_call * nmb));
        if (cfg.minibatch_advantage_norm)
          check(ctx, aleppo_read_train_metric(ctx, ALEPPO_M_ADV_STD, adv_std.data() + e0 * nmb, per_call * nmb));
        if (kl_pen)
          check(ctx, aleppo_read_train_metric(ctx, ALEPPO_M_MEAN_KL, mean_kl.data() + e0 * nmb, per_call * nmb));
        for (size_t k = 0; k < 5; ++k)
          check(ctx, aleppo_read_train_metric(ctx, sample_fields[k].first, planes[k].data() + e0 * N, per_call * N));
        epochs_run += per_call;
        if (cfg.target_kl > 0 && kl[epochs_run * nmb - 1] > cfg.target_kl)
          break;
      }
      const size_t nrun = epochs_run * nmb; // minibatches that ran
      Profile::Span sp_log(&prof, "log_data");
      // log_data (train.cc:163-210): x axis = non-reset env steps
      const int64_t step = (int64_t)total_steps;
      if (!log.episode_returns.empty()) {
        logger.add_scalar("mean_episode_return", step, meanf(log.episode_returns));
        logger.add_scalar("mean_episode_length", step, meanf(log.episode_lengths));
        logger.add_histogram("episode_returns", step, log.episode_returns);
        logger.add_histogram("episode_lengths", step,
                             std::vector<float>(log.episode_lengths.begin(), log.episode_lengths.end()));
        if (!log.game_returns.empty()) {
          logger.add_scalar("mean_game_return", step, meanf(log.game_returns));
          logger.add_scalar("mean_game_length", step, meanf(log.game_lengths));
          logger.add_histogram("game_returns", step, log.game_returns);
          logger.add_histogram("game_lengths", step, std::vector<float>(log.game_lengths.begin(), log.game_lengths.end()));
        }
      }
      auto avg = [&](float aleppo_minibatch_metrics::*f) {
        double s = 0;
        for (size_t i = 0; i < nrun; ++i)
          s += m[i].*f;
        return (float)(s / (double)nrun);
      };
      auto avgv = [&](const std::vector<float> &x) { // (computed like mean_ratio)
        double s = 0;
        for (size_t i = 0; i < nrun; ++i)
          s += x[i];
        return (float)(s / (double)nrun);
      };
      logger.add_scalar("mean_clipped_gradient", step, avg(&aleppo_minibatch_metrics::grad_norm));
      logger.add_scalar("mean_loss", step, avg(&aleppo_minibatch_metrics::loss));
      logger.add_scalar("mean_clipped_loss", step, avg(&aleppo_minibatch_metrics::clipped_loss));
      logger.add_scalar("mean_value_loss", step, avg(&aleppo_minibatch_metrics::value_loss));
      logger.add_scalar("mean_entropy", step, avg(&aleppo_minibatch_metrics::entropy));
      logger.add_scalar("mean_ratio", step, avg(&aleppo_minibatch_metrics::ratio));
      logger.add_scalar("mean_approx_kl", step, avgv(kl));
      logger.add_scalar("mean_clip_fraction", step, avgv(cf));
      if (cfg.minibatch_advantage_norm) // (the std each minibatch's advantages were divided by, before the 1e-8)
        logger.add_scalar("mean_advantage_std", step, avgv(adv_std));
      if (cfg.target_kl > 0)
        logger.add_scalar("update_epochs", step, (float)epochs_run);
      if (kl_pen) { // the adaptive KL coefficient (PPO paper section 4) from the last epoch's mean exact KL
        double d = 0;
        for (size_t i = nrun - nmb; i < nrun; ++i)
          d += mean_kl[i];
        d /= (double)nmb;
        logger.add_scalar("kl_coef", step, kl_beta);
        logger.add_scalar("mean_kl", step, (float)d);
        if (cfg.kl_target > 0) {
          if (d < cfg.kl_target / 1.5)
            kl_beta = std::max(0.5f * kl_beta, std::min(kl_beta, KL_BETA_MIN));
          else if (d > 1.5 * cfg.kl_target && std::isfinite(2.0f * kl_beta))
            kl_beta *= 2.0f;
        }
      }
      if (cfg.reward_scaling) { // (rewards_clipped: rank 0's environments)
        logger.add_scalar("reward_scale", step, (float)rstats[ALEPPO_RS_SCALE]);
        logger.add_scalar("return_rms_std", step, (float)std::sqrt(rrms[2]));
        logger.add_scalar("rewards_clipped", step, (float)rstats[ALEPPO_RS_CLIPPED]);
      }
      if (cfg.log_batch_stats) { // (global statistics under data parallelism; a NaN explained variance is logged as NaN)
        logger.add_scalar("explained_variance", step, (float)bstats[ALEPPO_BS_EXPLAINED_VARIANCE]);
        logger.add_scalar("mean_value", step, (float)bstats[ALEPPO_BS_VALUE_MEAN]);
        logger.add_scalar("std_value", step, (float)bstats[ALEPPO_BS_VALUE_STD]);
        logger.add_scalar("mean_return", step, (float)bstats[ALEPPO_BS_RETURN_MEAN]);
        logger.add_scalar("std_return", step, (float)bstats[ALEPPO_BS_RETURN_STD]);
        logger.add_scalar("mean_advantage", step, (float)bstats[ALEPPO_BS_ADVANTAGE_MEAN]);
        logger.add_scalar("std_advantage", step, (float)bstats[ALEPPO_BS_ADVANTAGE_STD]);
      }
      for (size_t k = 0; k < hyper_schedules.size(); ++k) // (the values this rollout's update ran with)
        logger.add_scalar(hyper_schedules[k].name, step, hyper_now[k]);
      logger.add_scalar("learning_rate", step, (float)lr);
      if (cfg.eval_interval > 0 && (r + 1) % cfg.eval_interval == 0) { // between this update and the next rollout
        Profile::Span sp(&prof, "evaluate");
        const EvalLog e = evaluate(r / cfg.eval_interval);
        logger.add_scalar("eval/episode_return_mean", step, e.return_mean);
        logger.add_scalar("eval/episode_return_max", step, e.return_max);
        logger.add_scalar("eval/episode_length_mean", step, e.length_mean);
        logger.add_scalar("eval/episodes", step, (float)e.episodes);
      }
      {
        std::vector<float> gn;
        for (size_t i = 0; i < nrun; ++i)
          gn.push_back(m[i].grad_norm);
        if (gn.size() > 1)
          logger.add_histogram("clipped_gradients", step, gn);
      }
      { // the per-sample histograms of log_data (train.cc:190-207): mask-selected values of the [epochs, M, B] planes
        std::vector<uint8_t> masks(N);
        std::vector<float> adv(N), ret(N), sel;
        check(ctx, aleppo_read_batch(ctx, ALEPPO_F_MASKS, masks.data(), N));
        auto gather = [&](const std::vector<float> &x, size_t reps) { // gather(t, masks): unmasked entries, every epoch
          sel.clear();
          for (size_t r = 0; r < reps; ++r)
            for (size_t i = 0; i < N; ++i)
              if (masks[i])
                sel.push_back(x[r * N + i]);
          return sel;
        };
        for (size_t k = 0; k < 5; ++k) // (every epoch that ran)
          logger.add_histogram(sample_fields[k].second, step, gather(planes[k], epochs_run));
        check(ctx, aleppo_read_batch(ctx, ALEPPO_F_ADVANTAGES, adv.data(), N * 4));
        check(ctx, aleppo_read_batch(ctx, ALEPPO_F_RETURNS, ret.data(), N * 4));
        logger.add_histogram("advantages", step, gather(adv, 1));
        logger.add_histogram("returns", step, gather(ret, 1));
      }
      logger.flush();
      rollouts_done = r + 1;
      if (!ckpt_file.empty() && (r + 1 == cfg.num_rollouts ||
                                 (cfg.checkpoint_interval > 0 && (r + 1) % (size_t)cfg.checkpoint_interval == 0))) {
        save_checkpoint(r + 1);
        if (stop_after == (long)(r + 1)) {
          std::cout << "stopped after the checkpoint of rollout " << r + 1 << std::endl;
          break;
        }
      }
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    size_t pending_starts = 0; // environments whose next slot is an episode-start slot
    for (size_t i = 0; i < E; ++i)
      pending_starts += start_cpu[i];
    // total_steps counts only non-start slots (rollout.cc:225,266): slots = steps + start slots, and the start slots are
    // the E initial ones plus one per finished episode, minus those still pending
    std::cout << "steps " << total_steps << " episodes " << episodes << " pending_starts " << pending_starts << " slots "
              << (rollouts_done + 1) * E * T << " env-steps/s " << (double)((rollouts_done - first_rollout) * E * T) / secs
              << std::endl;
    if (prof.on()) {
      prof.device_summary(ctx);
      prof.save();
    }
    if (const char *dump = std::getenv("ALEPPO_TRAINER_DUMP_FINAL")) { // test hook: the trained parameters
      size_t n = 0;
      check(ctx, aleppo_param_count(ctx, &n));
      std::vector<float> p(n);
      check(ctx, aleppo_export_params(ctx, p.data(), n));
      std::ofstream f(dump, std::ios::binary);
      f.write(reinterpret_cast<const char *>(p.data()), (std::streamsize)(n * sizeof(float)));
    }
    check(ctx, aleppo_host_free(ctx, frames));
    check(ctx, aleppo_host_free(ctx, start_mapped));
    if (eval_frames)
      check(ctx, aleppo_host_free(ctx, eval_frames));
    aleppo_destroy(ctx);
    std::cout << "Success" << std::endl;
    return 0;
  } catch (const std::exception &e) {
    std::cerr << "error: " << e.what() << std::endl;
    return 1;
  }
}
