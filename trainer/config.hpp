// The trainer's configuration: the reference's YAML keys and defaults plus the extension keys (train.cc has the list)
#pragma once
#include "../include/aleppo.h"
#include <cmath>
#include <cstdint>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

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
  // extension: the evaluation's environments live on the device too (aleppo_eval_env_open / aleppo_eval_env_run)
  bool device_evaluation = false;
  // extension: record_video / record_observation honoured on the device (aleppo_rec_*): environment 0 of rank 0 with
  // device_environments, lane 0 of every evaluation with record_evaluation (needs device_evaluation); every
  // record_interval-th episode is written
  bool record_evaluation = false;
  size_t record_interval = 1;
  size_t device_evaluation_steps = 32; // the S of the open and the chunk of every run
  // extension: return-based reward scaling in place of the reward clamp (ALEPPO_OPT_REWARD_SCALE / _CLIP)
  bool reward_scaling = false;
  double reward_scale_clip = 10.0;
  // extension: checkpoint and resume (aleppo_export_rollout_state / aleppo_state_digest and the learner's export pairs)
  std::string checkpoint_path, resume;
  long checkpoint_interval = 0; // 0: only after the last rollout
  bool log_batch_stats = false; // extension: explained variance and value / return / advantage statistics (ALEPPO_F_BATCH_STATS)
  // extension: aleppo_refresh_advantages before every epoch of an update but the first (one aleppo_train call per epoch)
  bool recompute_advantages = false;
  bool log_tensor_stats = false; // extension: per-tensor gradient / parameter norms and update ratios (aleppo_tensor_stats)
  // extension: dormant / dead units and firing rates of the four hidden layers on the batch (aleppo_activation_stats)
  bool log_activation_stats = false;
  size_t activation_stats_interval = 1; // after the update of every n-th rollout
  double dormant_tau = 0.025;           // the dormancy threshold (Sokar et al. 2023)
  // extension: the rank measures of the fc features on the batch (aleppo_feature_rank), after the update of every n-th rollout
  bool log_feature_rank = false;
  size_t feature_rank_interval = 1;
  aleppo_feature_rank_config feature_rank{0.01f, 0.01f, 0, 0}; // delta, eps, centered
  // extension: policy churn (Schaul et al. 2022) - a snapshot before the update of every n-th rollout, aleppo_policy_diff
  // (snapshot, live) after it on the batch it trained on; policy_churn_averaged: also (averaged, live), needs ema_decay
  bool log_policy_churn = false;
  size_t policy_churn_interval = 1;
  bool policy_churn_averaged = false;
  // extension: gradient probes - before the update of every n-th rollout, the gradient noise scale (McCandlish et al. 2018)
  // from aleppo_grad_probe at gradient_stats_small_batch samples and at one minibatch, the per-tensor cosine of the policy
  // term's and the value term's gradient, and the cosine of Adam's first moment with the fresh gradient (aleppo_grad_gram)
  bool log_gradient_stats = false;
  size_t gradient_stats_interval = 1;
  size_t gradient_stats_small_batch = 0; // 0: a quarter of the minibatch
  // extension: ReDo (Sokar et al. 2023) - recycle the dormant units of the held batch (aleppo_recycle_dormant)
  bool recycle_dormant = false;
  // after the update of every n-th rollout.  64: ReDo recycles every 1000 gradient steps; the benched configuration takes
  // 16 minibatch steps per rollout (1 epoch x 16 minibatches), and 1000 / 16 = 62.5 rounds to 64
  size_t recycle_interval = 64;
  double recycle_tau = 0.025;                // the dormancy threshold of the recycle
  int recycle_layers = ALEPPO_RECYCLE_ALL;   // ALEPPO_RECYCLE_* bits (the key: a list of conv1 / conv2 / conv3 / fc)
  // extension: exponentially averaged parameters (aleppo_ema_open / aleppo_ema_update after every trained rollout's update)
  bool ema_decay_set = false;  // the key was given (absent: off)
  double ema_decay = 0;        // in [0, 1)
  bool ema_warmup = false;     // update n (n updates so far) runs with min(ema_decay, (1 + n) / (10 + n)): TensorFlow / timm
  bool eval_averaged = false;  // evaluation acts on the averaged parameters (ALEPPO_OPT_EVAL_PARAMS = 1)
  // extension: regularisation inside the optimizer step (ALEPPO_OPT_WEIGHT_DECAY / ALEPPO_OPT_ANCHOR_COEF) and shrink and
  // perturb after the update of every n-th rollout (aleppo_shrink_perturb)
  double weight_decay = 0;     // torch.optim.AdamW's weight_decay (absent or 0: off)
  double l2_init_coef = 0;     // the pull toward the INITIAL parameters (L2 Init); > 0: the anchor is taken before the first update
  size_t shrink_perturb_interval = 0; // 0: off
  double shrink_perturb_shrink = 1.0; // in [0, 1]
  double shrink_perturb_sigma = 0.0;  // >= 0
  // extension: perturbation saliency videos of environment 0 of rank 0 (aleppo_saliency; trainer/saliency.hpp), after the
  // update of every saliency_interval-th rollout, with the grid stride and the two sigmas of aleppo_saliency_config
  bool record_saliency = false;
  size_t saliency_interval = 1;
  aleppo_saliency_config saliency{5, 15, 5.0, 3.0};
  // extensions
  std::string precision = "fp32", rollout_precision = "fp32";
  bool device_preprocess = false; // emulators hand over raw frame pairs; gray LUT + resize + max run on the device (N2)
  bool device_environments = false; // the training environments live on the device: aleppo_env_open / aleppo_env_rollout
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
// the key's value into v when the key is given; v keeps its default, Config's own initialiser, when it is not
template <class T> static void read_key(const std::map<std::string, std::string> &kv, const char *k, T &v) {
  v = as<T>(kv, k, v);
}
static void read_key(const std::map<std::string, std::string> &kv, const char *k, bool &v) { v = as_bool(kv, k, v); }
// kl_target's rule never halves beta below this (nor raises a smaller initial kl_coef to it): repeated halving would
// otherwise reach 0 through the subnormals, and 0 doubled stays 0
constexpr float KL_BETA_MIN = 1e-6f;
static Config load_config(const std::string &path) { // keys / defaults of src/bin/train.cc:108-136
  const auto kv = parse_yaml(path);
  Config c;
  read_key(kv, "total_environments", c.total_environments);
  read_key(kv, "hidden_size", c.hidden_size);
  read_key(kv, "action_size", c.action_size);
  read_key(kv, "horizon", c.horizon);
  read_key(kv, "max_steps", c.max_steps);
  read_key(kv, "frame_stack", c.frame_stack);
  read_key(kv, "learning_rate", c.learning_rate);
  read_key(kv, "clip_param", c.clip_param);
  read_key(kv, "value_loss_coef", c.value_loss_coef);
  read_key(kv, "entropy_coef", c.entropy_coef);
  read_key(kv, "num_epochs", c.num_epochs);
  read_key(kv, "mini_batch_size", c.mini_batch_size);
  read_key(kv, "num_mini_batches", c.num_mini_batches);
  read_key(kv, "gae_discount", c.gae_discount);
  read_key(kv, "gae_lambda", c.gae_lambda);
  read_key(kv, "max_gradient_norm", c.max_gradient_norm);
  read_key(kv, "num_rollouts", c.num_rollouts);
  read_key(kv, "num_workers", c.num_workers);
  read_key(kv, "worker_batch_size", c.worker_batch_size);
  read_key(kv, "frame_skip", c.frame_skip);
  read_key(kv, "max_return", c.max_return);
  read_key(kv, "record_observation", c.record_observation);
  read_key(kv, "record_video", c.record_video);
  read_key(kv, "cuda_graph", c.cuda_graph);
  read_key(kv, "shuffle_minibatches", c.shuffle_minibatches);
  read_key(kv, "clip_value_loss", c.clip_value_loss);
  read_key(kv, "minibatch_advantage_norm", c.minibatch_advantage_norm);
  read_key(kv, "target_kl", c.target_kl);
  read_key(kv, "kl_coef", c.kl_coef);
  read_key(kv, "kl_target", c.kl_target);
  read_key(kv, "log_batch_stats", c.log_batch_stats);
  read_key(kv, "recompute_advantages", c.recompute_advantages);
  read_key(kv, "log_tensor_stats", c.log_tensor_stats);
  read_key(kv, "log_activation_stats", c.log_activation_stats);
  { // what aleppo_activation_stats would refuse is refused here ("nan" / "inf" do not parse as a number: bad value)
    const long interval = as<long>(kv, "activation_stats_interval", 1);
    if (interval < 1)
      throw std::runtime_error("activation_stats_interval must be positive");
    c.activation_stats_interval = (size_t)interval;
    read_key(kv, "dormant_tau", c.dormant_tau);
    if (!(c.dormant_tau >= 0 && std::isfinite(c.dormant_tau)))
      throw std::runtime_error("dormant_tau must be finite and non-negative");
    for (const char *k : {"activation_stats_interval", "dormant_tau"})
      if (kv.count(k) && !c.log_activation_stats) // (nothing else reads them)
        throw std::runtime_error(std::string(k) + " needs log_activation_stats: true");
  }
  read_key(kv, "log_feature_rank", c.log_feature_rank);
  { // what aleppo_feature_rank would refuse is refused here ("nan" / "inf" do not parse as a number: bad value)
    const long interval = as<long>(kv, "feature_rank_interval", 1);
    if (interval < 1)
      throw std::runtime_error("feature_rank_interval must be positive");
    c.feature_rank_interval = (size_t)interval;
    read_key(kv, "feature_rank_delta", c.feature_rank.delta);
    if (!(c.feature_rank.delta > 0 && c.feature_rank.delta < 1))
      throw std::runtime_error("feature_rank_delta must be in (0, 1)");
    read_key(kv, "feature_rank_eps", c.feature_rank.eps);
    if (!(c.feature_rank.eps >= 0 && std::isfinite(c.feature_rank.eps)))
      throw std::runtime_error("feature_rank_eps must be finite and non-negative");
    c.feature_rank.centered = as_bool(kv, "feature_rank_centered", false) ? 1 : 0;
    for (const char *k : {"feature_rank_interval", "feature_rank_delta", "feature_rank_eps", "feature_rank_centered"})
      if (kv.count(k) && !c.log_feature_rank) // (nothing else reads them)
        throw std::runtime_error(std::string(k) + " needs log_feature_rank: true");
  }
  read_key(kv, "recycle_dormant", c.recycle_dormant);
  { // what aleppo_recycle_dormant would refuse is refused here
    const long interval = as<long>(kv, "recycle_interval", (long)c.recycle_interval);
    if (interval < 1)
      throw std::runtime_error("recycle_interval must be positive");
    c.recycle_interval = (size_t)interval;
    read_key(kv, "recycle_tau", c.recycle_tau);
    if (!(c.recycle_tau >= 0 && std::isfinite(c.recycle_tau)))
      throw std::runtime_error("recycle_tau must be finite and non-negative");
    if (kv.count("recycle_layers")) { // "[conv1, fc]" or "conv1, fc"
      static const std::pair<const char *, int> names[4] = {{"conv1", ALEPPO_RECYCLE_CONV1}, {"conv2", ALEPPO_RECYCLE_CONV2},
                                                            {"conv3", ALEPPO_RECYCLE_CONV3}, {"fc", ALEPPO_RECYCLE_FC}};
      std::string list = kv.at("recycle_layers");
      if (list.size() >= 2 && list.front() == '[' && list.back() == ']')
        list = list.substr(1, list.size() - 2);
      c.recycle_layers = 0;
      std::istringstream ss(list);
      for (std::string item; std::getline(ss, item, ',');) {
        int bit = 0;
        for (const auto &nb : names)
          if (trim(item) == nb.first)
            bit = nb.second;
        if (!bit)
          throw std::runtime_error("recycle_layers: unknown layer '" + trim(item) + "' (conv1, conv2, conv3, fc)");
        c.recycle_layers |= bit;
      }
      if (!c.recycle_layers)
        throw std::runtime_error("recycle_layers must name at least one of conv1, conv2, conv3, fc");
    }
    for (const char *k : {"recycle_interval", "recycle_tau", "recycle_layers"})
      if (kv.count(k) && !c.recycle_dormant) // (nothing else reads them)
        throw std::runtime_error(std::string(k) + " needs recycle_dormant: true");
  }
  read_key(kv, "record_saliency", c.record_saliency);
  { // what aleppo_saliency would refuse is refused here ("nan" / "inf" do not parse as a number: bad value)
    const long interval = as<long>(kv, "saliency_interval", (long)c.saliency_interval);
    if (interval < 1)
      throw std::runtime_error("saliency_interval must be positive");
    c.saliency_interval = (size_t)interval;
    const long stride = as<long>(kv, "saliency_stride", (long)c.saliency.stride);
    if (stride < 2 || stride > 84)
      throw std::runtime_error("saliency_stride must be in [2, 84]");
    c.saliency.stride = (int32_t)stride;
    read_key(kv, "saliency_sigma_mask", c.saliency.sigma_mask);
    if (!(c.saliency.sigma_mask >= 0.5 && c.saliency.sigma_mask <= 16.0))
      throw std::runtime_error("saliency_sigma_mask must be in [0.5, 16]");
    read_key(kv, "saliency_sigma_blur", c.saliency.sigma_blur);
    if (!(c.saliency.sigma_blur >= 0.5 && c.saliency.sigma_blur <= 10.0))
      throw std::runtime_error("saliency_sigma_blur must be in [0.5, 10]");
    for (const char *k : {"saliency_interval", "saliency_stride", "saliency_sigma_mask", "saliency_sigma_blur"})
      if (kv.count(k) && !c.record_saliency) // (nothing else reads them)
        throw std::runtime_error(std::string(k) + " needs record_saliency: true");
  }
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
    read_key(kv, "value_clip_range", c.value_clip_range);
    if (!(c.value_clip_range > 0 && c.value_clip_range < 3.0e38))
      throw std::runtime_error("value_clip_range must be finite and positive");
    if (!c.clip_value_loss) // (nothing else reads it)
      throw std::runtime_error("value_clip_range needs clip_value_loss: true");
  }
  read_key(kv, "reward_scaling", c.reward_scaling);
  if (kv.count("reward_scale_clip")) { // what the option would refuse is refused here (a float: < 3e38 is finite)
    read_key(kv, "reward_scale_clip", c.reward_scale_clip);
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
    read_key(kv, "eval_rule", c.eval_rule);
    if (c.eval_rule != "greedy" && c.eval_rule != "sample" && c.eval_rule != "epsilon")
      throw std::runtime_error("eval_rule must be greedy, sample or epsilon");
    read_key(kv, "eval_temperature", c.eval_temperature);
    if (!(c.eval_temperature > 0 && c.eval_temperature < 3.0e38) || !std::isfinite(1.0f / (float)c.eval_temperature))
      throw std::runtime_error("eval_temperature must be finite and positive");
    read_key(kv, "eval_epsilon", c.eval_epsilon);
    if (!(c.eval_epsilon >= 0 && c.eval_epsilon <= 1))
      throw std::runtime_error("eval_epsilon must be in [0, 1]");
    read_key(kv, "device_evaluation", c.device_evaluation);
    if (c.device_evaluation && interval == 0)
      throw std::runtime_error("device_evaluation needs eval_interval > 0");
    if (kv.count("device_evaluation_steps")) {
      const long steps = as<long>(kv, "device_evaluation_steps", 32);
      if (!c.device_evaluation) // (nothing else reads it)
        throw std::runtime_error("device_evaluation_steps needs device_evaluation: true");
      if (steps < 1 || steps > 1024)
        throw std::runtime_error("device_evaluation_steps must be in [1, 1024]");
      c.device_evaluation_steps = (size_t)steps;
    }
  }
  c.ema_decay_set = kv.count("ema_decay") != 0;
  if (c.ema_decay_set) { // what aleppo_ema_update would refuse is refused here ("nan" / "inf" do not parse: bad value)
    read_key(kv, "ema_decay", c.ema_decay);
    if (!(std::isfinite(c.ema_decay) && c.ema_decay >= 0 && c.ema_decay < 1))
      throw std::runtime_error("ema_decay must be in [0, 1)");
  }
  read_key(kv, "ema_warmup", c.ema_warmup);
  read_key(kv, "eval_averaged", c.eval_averaged);
  for (const char *k : {"ema_warmup", "eval_averaged"})
    if (kv.count(k) && !c.ema_decay_set) // (nothing else reads them; given as false too)
      throw std::runtime_error(std::string(k) + " needs ema_decay");
  if (kv.count("eval_averaged") && c.eval_interval == 0)
    throw std::runtime_error("eval_averaged needs eval_interval > 0");
  // what aleppo_set_option / aleppo_shrink_perturb would refuse is refused here ("nan" / "inf" do not parse: bad value)
  for (const auto &k : {std::make_pair("weight_decay", &c.weight_decay), std::make_pair("l2_init_coef", &c.l2_init_coef)}) {
    read_key(kv, k.first, *k.second);
    const float f = (float)*k.second;
    if (!(std::isfinite(*k.second) && *k.second >= 0 && std::isfinite(f)))
      throw std::runtime_error(std::string(k.first) + " must be finite and non-negative");
  }
  if (kv.count("shrink_perturb_interval")) {
    const long interval = as<long>(kv, "shrink_perturb_interval", 0);
    if (interval < 1)
      throw std::runtime_error("shrink_perturb_interval must be positive");
    c.shrink_perturb_interval = (size_t)interval;
  }
  read_key(kv, "shrink_perturb_shrink", c.shrink_perturb_shrink);
  read_key(kv, "shrink_perturb_sigma", c.shrink_perturb_sigma);
  if (!(std::isfinite(c.shrink_perturb_shrink) && c.shrink_perturb_shrink >= 0 && c.shrink_perturb_shrink <= 1))
    throw std::runtime_error("shrink_perturb_shrink must be in [0, 1]");
  if (!(std::isfinite(c.shrink_perturb_sigma) && c.shrink_perturb_sigma >= 0 && std::isfinite((float)c.shrink_perturb_sigma)))
    throw std::runtime_error("shrink_perturb_sigma must be finite and non-negative");
  for (const char *k : {"shrink_perturb_shrink", "shrink_perturb_sigma"})
    if (kv.count(k) && !c.shrink_perturb_interval) // (nothing else reads them)
      throw std::runtime_error(std::string(k) + " needs shrink_perturb_interval");
  read_key(kv, "log_policy_churn", c.log_policy_churn);
  {
    const long interval = as<long>(kv, "policy_churn_interval", 1);
    if (interval < 1)
      throw std::runtime_error("policy_churn_interval must be positive");
    c.policy_churn_interval = (size_t)interval;
    read_key(kv, "policy_churn_averaged", c.policy_churn_averaged);
    for (const char *k : {"policy_churn_interval", "policy_churn_averaged"})
      if (kv.count(k) && !c.log_policy_churn) // (nothing else reads them; given as false too)
        throw std::runtime_error(std::string(k) + " needs log_policy_churn: true");
    if (c.policy_churn_averaged && !c.ema_decay_set)
      throw std::runtime_error("policy_churn_averaged needs ema_decay");
  }
  read_key(kv, "log_gradient_stats", c.log_gradient_stats);
  {
    const long interval = as<long>(kv, "gradient_stats_interval", 1);
    if (interval < 1)
      throw std::runtime_error("gradient_stats_interval must be positive");
    c.gradient_stats_interval = (size_t)interval;
    const long small = as<long>(kv, "gradient_stats_small_batch", 0);
    if (kv.count("gradient_stats_small_batch") && small < 1)
      throw std::runtime_error("gradient_stats_small_batch must be positive");
    c.gradient_stats_small_batch = (size_t)small;
    for (const char *k : {"gradient_stats_interval", "gradient_stats_small_batch"})
      if (kv.count(k) && !c.log_gradient_stats) // (nothing else reads them; given as false too)
        throw std::runtime_error(std::string(k) + " needs log_gradient_stats: true");
  }
  read_key(kv, "record_evaluation", c.record_evaluation);
  if (c.record_evaluation && !c.device_evaluation)
    throw std::runtime_error("record_evaluation needs device_evaluation: true");
  if (kv.count("record_interval")) {
    const long n = as<long>(kv, "record_interval", 1);
    if (n < 1)
      throw std::runtime_error("record_interval must be positive");
    if (!c.record_video && !c.record_evaluation) // (nothing else reads it)
      throw std::runtime_error("record_interval needs record_video: true or record_evaluation: true");
    c.record_interval = (size_t)n;
  }
  read_key(kv, "checkpoint_path", c.checkpoint_path);
  read_key(kv, "resume", c.resume);
  if (kv.count("checkpoint_interval")) {
    read_key(kv, "checkpoint_interval", c.checkpoint_interval);
    if (c.checkpoint_interval <= 0)
      throw std::runtime_error("checkpoint_interval must be positive");
    if (c.checkpoint_path.empty()) // (there would be nowhere to write to)
      throw std::runtime_error("checkpoint_interval needs checkpoint_path");
  }
  read_key(kv, "deterministic", c.deterministic);
  read_key(kv, "precision", c.precision);
  read_key(kv, "rollout_precision", c.rollout_precision);
  read_key(kv, "device_preprocess", c.device_preprocess);
  read_key(kv, "slot_ahead", c.slot_ahead);
  read_key(kv, "device_environments", c.device_environments);
  read_key(kv, "advantage_norm", c.advantage_norm);
  read_key(kv, "seed", c.seed);
  return c;
}

// ------------------------------------------------------------------ what follows from the config, each decided once
static int precision_of(const Config &c) { return c.precision == "bf16" ? ALEPPO_BF16 : ALEPPO_FP32; }
static int frame_kind(const Config &c) { return c.device_preprocess ? ALEPPO_FRAMES_RAW_PAIR : ALEPPO_FRAMES_84; }
static int eval_rule(const Config &c) {
  return c.eval_rule == "greedy" ? ALEPPO_EVAL_GREEDY
                                 : c.eval_rule == "sample" ? ALEPPO_EVAL_SAMPLE : ALEPPO_EVAL_EPSILON_GREEDY;
}
static float eval_param(const Config &c) { // the rule's parameter: the temperature, epsilon, or nothing
  const int rule = eval_rule(c);
  return rule == ALEPPO_EVAL_SAMPLE ? (float)c.eval_temperature
                                    : rule == ALEPPO_EVAL_EPSILON_GREEDY ? (float)c.eval_epsilon : 0.f;
}
// extension: linear schedules of the clip range, the loss coefficients and the norm limit, one value per rollout
struct HyperSchedule {
  const char *name; // the scalar's tag: the config key it schedules
  int option;
  double v0, v1;
  float at(size_t r, size_t of) const { return (float)(v0 + (v1 - v0) * (r / static_cast<double>(of))); } // rollout r of `of`
};
static std::vector<HyperSchedule> hyper_schedules_of(const Config &c) {
  std::vector<HyperSchedule> s;
  if (c.clip_param_final_set)
    s.push_back({"clip_param", ALEPPO_OPT_CLIP_PARAM, c.clip_param, c.clip_param_final});
  if (c.value_loss_coef_final_set)
    s.push_back({"value_loss_coef", ALEPPO_OPT_VALUE_LOSS_COEF, c.value_loss_coef, c.value_loss_coef_final});
  if (c.entropy_coef_final_set)
    s.push_back({"entropy_coef", ALEPPO_OPT_ENTROPY_COEF, c.entropy_coef, c.entropy_coef_final});
  if (c.max_gradient_norm_final_set)
    s.push_back({"max_gradient_norm", ALEPPO_OPT_MAX_GRAD_NORM, c.max_gradient_norm, c.max_gradient_norm_final});
  return s;
}
// the hparams session record's entries: get_parameters (train.cc:76-105) with the same keys, then every extension key
// that is set (only when set: the records of existing configs stay byte-identical)
struct HParams {
  std::vector<std::pair<std::string, double>> numbers;
  std::vector<std::pair<std::string, bool>> flags;
};
static HParams hparams_of(const Config &c) {
  HParams h;
  h.numbers = {{"total_environments", (double)c.total_environments}, {"hidden_size", (double)c.hidden_size},
               {"action_size", (double)c.action_size}, {"horizon", (double)c.horizon}, {"max_steps", (double)c.max_steps},
               {"frame_stack", (double)c.frame_stack}, {"learning_rate", c.learning_rate}, {"clip_param", c.clip_param},
               {"value_loss_coef", c.value_loss_coef}, {"entropy_coef", c.entropy_coef}, {"num_epochs", (double)c.num_epochs},
               {"mini_batch_size", (double)c.mini_batch_size}, {"num_mini_batches", (double)c.num_mini_batches},
               {"gae_discount", c.gae_discount}, {"gae_lambda", c.gae_lambda}, {"max_gradient_norm", c.max_gradient_norm},
               {"num_rollouts", (double)c.num_rollouts}, {"num_workers", (double)c.num_workers},
               {"worker_batch_size", (double)c.worker_batch_size}, {"frame_skip", (double)c.frame_skip},
               {"max_return", c.max_return}};
  if (c.kl_coef_set)
    h.numbers.emplace_back("kl_coef", c.kl_coef);
  if (c.kl_target_set)
    h.numbers.emplace_back("kl_target", c.kl_target);
  for (const HyperSchedule &s : hyper_schedules_of(c))
    h.numbers.emplace_back(std::string(s.name) + "_final", s.v1);
  if (c.value_clip_range_set)
    h.numbers.emplace_back("value_clip_range", c.value_clip_range);
  if (c.eval_interval > 0)
    h.numbers.insert(h.numbers.end(), {{"eval_interval", (double)c.eval_interval},
                                       {"eval_environments", (double)c.eval_environments},
                                       {"eval_episodes", (double)c.eval_episodes},
                                       {"eval_rule", (double)eval_rule(c)},
                                       {"eval_temperature", c.eval_temperature},
                                       {"eval_epsilon", c.eval_epsilon}});
  if (c.device_evaluation)
    h.numbers.emplace_back("device_evaluation_steps", (double)c.device_evaluation_steps);
  if (c.record_interval != 1)
    h.numbers.emplace_back("record_interval", (double)c.record_interval);
  if (c.ema_decay_set)
    h.numbers.emplace_back("ema_decay", c.ema_decay);
  if (c.log_policy_churn)
    h.numbers.emplace_back("policy_churn_interval", (double)c.policy_churn_interval);
  if (c.log_gradient_stats) {
    h.numbers.emplace_back("gradient_stats_interval", (double)c.gradient_stats_interval);
    if (c.gradient_stats_small_batch)
      h.numbers.emplace_back("gradient_stats_small_batch", (double)c.gradient_stats_small_batch);
  }
  if (c.weight_decay > 0)
    h.numbers.emplace_back("weight_decay", c.weight_decay);
  if (c.l2_init_coef > 0)
    h.numbers.emplace_back("l2_init_coef", c.l2_init_coef);
  if (c.shrink_perturb_interval)
    h.numbers.insert(h.numbers.end(), {{"shrink_perturb_interval", (double)c.shrink_perturb_interval},
                                       {"shrink_perturb_shrink", c.shrink_perturb_shrink},
                                       {"shrink_perturb_sigma", c.shrink_perturb_sigma}});
  h.flags = {{"record_observation", c.record_observation}, {"record_video", c.record_video},
             {"cuda_graph", c.cuda_graph}, {"deterministic", c.deterministic}};
  const std::pair<const char *, bool> when_set[] = {{"shuffle_minibatches", c.shuffle_minibatches},
                                                    {"clip_value_loss", c.clip_value_loss},
                                                    {"minibatch_advantage_norm", c.minibatch_advantage_norm},
                                                    {"log_batch_stats", c.log_batch_stats},
                                                    {"recompute_advantages", c.recompute_advantages},
                                                    {"log_tensor_stats", c.log_tensor_stats},
                                                    {"log_activation_stats", c.log_activation_stats},
                                                    {"log_feature_rank", c.log_feature_rank},
                                                    {"log_policy_churn", c.log_policy_churn},
                                                    {"policy_churn_averaged", c.policy_churn_averaged},
                                                    {"log_gradient_stats", c.log_gradient_stats},
                                                    {"recycle_dormant", c.recycle_dormant},
                                                    {"record_saliency", c.record_saliency},
                                                    {"reward_scaling", c.reward_scaling},
                                                    {"device_environments", c.device_environments},
                                                    {"device_evaluation", c.device_evaluation},
                                                    {"record_evaluation", c.record_evaluation},
                                                    {"ema_warmup", c.ema_warmup},
                                                    {"eval_averaged", c.eval_averaged}};
  for (const auto &f : when_set)
    if (f.second)
      h.flags.emplace_back(f.first, true);
  return h;
}
