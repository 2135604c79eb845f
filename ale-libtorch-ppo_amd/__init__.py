"""ale-libtorch-ppo_amd: host-side mirror (Python, ctypes) of the PPO-over-ALE hot path whose
compute lives in libaleppo.so (hand-written HIP for gfx950, C ABI in include/aleppo.h).

The directory name has a hyphen, so import it through ``__graft_entry__.load_package()``
(module name ``ale_libtorch_ppo_amd``).

Nothing in this package computes on the CPU: every operator calls into the HIP library and
raises if the library or a gfx950 device is missing.  The CPU oracle under ``oracle/`` is test
infrastructure and is never imported from here.

Sub-namespaces mirror the reference's C++ namespaces for this path:
  gae.gae                      <- ai::gae::gae                       (src/ai/gae.h:4-7)
  vision.*                     <- ai::vision::*                      (src/ai/vision.h:6-17)
  losses.compute               <- ai::ppo::losses::compute           (src/ai/ppo/losses.h:22-27)
  Engine                       <- Network + Adam + Rollout/Buffer + ppo::train::train as driven by
                                  main() (src/bin/train.cc:358-458)
"""
import ctypes as C
import os
import struct
from types import SimpleNamespace

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (ALEPPO_LIB_PATH: developer A/B runs of two builds inside one gpurun call; never set by tests or bench)
LIB_PATH = os.environ.get("ALEPPO_LIB_PATH") or os.path.join(_HERE, "libaleppo.so")

OK = 0
ERR_INVALID_ARGUMENT, ERR_RUNTIME, ERR_HIP, ERR_NO_DEVICE = -1, -2, -3, -4
FP32, BF16 = 0, 1
HOST, DEVICE, HOST_MAPPED = 0, 1, 2
FRAMES_84, FRAMES_RAW_PAIR = 0, 1
ROLLOUT_FP32, ROLLOUT_FP16 = 0, 1
ABI_VERSION = 2
UNIQUE_ID_BYTES = 128

FIELDS = dict(observations=0, actions=1, rewards=2, masks=3, logits=4, values=5, advantages=6, returns=7,
              log_probs=8, terminals=9, truncations=10, current_obs=11, next_values=12, batch_stats=13,
              reward_scale=14)
# ALEPPO_F_REWARD_SCALE: the indices of its ALEPPO_REWARD_SCALE_COUNT doubles (aleppo_reward_scale_stat; Engine.reward_scale)
REWARD_SCALE_COUNT = 6
REWARD_SCALE = dict(count=0, mean=1, var=2, scale=3, batch_count=4, clipped=5)
# ALEPPO_F_BATCH_STATS: the indices of its ALEPPO_BATCH_STATS_COUNT doubles (aleppo_batch_stat; Engine.batch_stats)
BATCH_STATS_COUNT = 10
BATCH_STATS = dict(count=0, explained_variance=1, value_mean=2, value_std=3, return_mean=4, return_std=5,
                   advantage_mean=6, advantage_std=7, residual_mean=8, residual_std=9)
METRIC_FIELDS = dict(total_losses=0, clipped_losses=1, value_losses=2, entropies=3, ratio=4, approx_kl=5,
                     clip_fraction=6, kl=11)  # (kl: OPT_KL_PENALTY's exact KL per sample)
# the [epochs, M] masked means of approx_kl / clip_fraction (aleppo_read_train_metric; Engine.train_diagnostics) and of
# OPT_KL_PENALTY's exact KL (Engine.kl_divergence)
METRIC_MEAN_FIELDS = dict(approx_kl=7, clip_fraction=8, kl=12)
# the [epochs, M] statistics of OPT_ADV_NORM_MINIBATCH (aleppo_read_train_metric; Engine.advantage_stats)
METRIC_ADV_FIELDS = dict(mean=9, std=10)
# aleppo_state_digest: the indices of its ALEPPO_DIGEST_COUNT words (aleppo_digest_section; Engine.state_digest)
DIGEST_COUNT = 4
DIGEST_SECTIONS = dict(params=0, optimizer=1, rollout=2, reward_scale=3)
ROLLOUT_STATE_WORDS = 4
# aleppo_tensor_stats: double [TENSOR_STATS_ROWS][TENSOR_STATS_COLS], the rows in libtorch parameters() order plus the whole
# model, the columns of aleppo_tensor_stat, the section bits of aleppo_tensor_stats_section (Engine.tensor_stats)
TENSOR_STATS_ROWS, TENSOR_STATS_COLS = 13, 10
TENSOR_NAMES = ("conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc.w", "fc.b", "action.w", "action.b",
                "value.w", "value.b", "total")
TENSOR_STATS = dict(size=0, param_norm=1, param_maxabs=2, param_nonfinite=3, grad_norm=4, grad_maxabs=5, update_norm=6,
                    update_maxabs=7, update_ratio=8, step_nonfinite=9)
TS_SEC_PARAMS, TS_SEC_STEP = 1, 2
TENSOR_STATS_SECTIONS = dict(params=TS_SEC_PARAMS, step=TS_SEC_STEP, all=TS_SEC_PARAMS | TS_SEC_STEP)
# aleppo_forward_activations / aleppo_activation_stats: the hidden layers (channels, positions per channel; fc: H, 1), the
# rows of the layer table, the columns of aleppo_act_unit_stat and aleppo_act_layer_stat (Engine.forward_activations /
# Engine.activation_stats)
ACT_LAYERS = ("conv1", "conv2", "conv3", "fc")
ACT_LAYER_SHAPES = dict(conv1=(32, 20, 20), conv2=(64, 9, 9), conv3=(64, 7, 7))
ACT_LAYER_ROWS = ACT_LAYERS + ("total",)
# aleppo_export_backward: the outputs in argument order with their aleppo_bwd_tensor bits, and the layer whose shape each
# has (Engine.export_backward)
BWD_TENSORS = dict(conv1=1, conv2=2, conv3=4, fc=8, dfc=16, dconv3=32, dconv2=64, dconv1=128)
BWD_SHAPE_OF = dict(conv1="conv1", conv2="conv2", conv3="conv3", fc="fc", dfc="fc", dconv3="conv3", dconv2="conv2",
                    dconv1="conv1")
ACT_UNIT_COLS, ACT_LAYER_COLS = 5, 8
# aleppo_export_acting: the outputs in argument order with their aleppo_acting_tensor bits (Engine.export_acting)
ACTING_TENSORS = dict(conv1=1, conv2=2, conv3=4, fc_parts=8)
FC_SPLITS = 7
ACT_UNIT_STATS = dict(mean_abs=0, positive_fraction=1, max_abs=2, score=3, nonfinite=4)
ACT_LAYER_STATS = dict(units=0, elements=1, mean_abs=2, positive_fraction=3, max_abs=4, dead=5, dormant=6, nonfinite=7)
# aleppo_recycle_units / aleppo_recycle_dormant: the layer bits, the flags and the rows of counts (Engine.recycle_units /
# Engine.recycle_dormant)
RECYCLE_COUNTS = 5
RECYCLE_CONV1, RECYCLE_CONV2, RECYCLE_CONV3, RECYCLE_FC, RECYCLE_ALL = 1, 2, 4, 8, 15
RECYCLE_LAYERS = dict(conv1=RECYCLE_CONV1, conv2=RECYCLE_CONV2, conv3=RECYCLE_CONV3, fc=RECYCLE_FC, all=RECYCLE_ALL)
RECYCLE_KEEP_MOMENTS = 1
# aleppo_shrink_perturb: its flag (Engine.shrink_perturb)
SP_RESET_MOMENTS = 1
# aleppo_ema_read: the statistics of the exponentially averaged parameters (Engine.ema_stats)
EMA_STATS_COUNT = 6
EMA_STATS = dict(updates=0, decay=1, norm=2, param_norm=3, distance=4, relative_distance=5)
# aleppo_saliency_config's defaults (Engine.saliency / Engine.saliency_perturbed / saliency_tables)
SALIENCY_STRIDE, SALIENCY_SIGMA_MASK, SALIENCY_SIGMA_BLUR, SALIENCY_PLANES = 5, 5.0, 3.0, 15
# aleppo_feature_rank: the indices of its ALEPPO_FR_COUNT doubles (aleppo_feature_rank_stat; Engine.feature_rank)
FR_COUNT = 11
FR_STATS = dict(rows=0, nonfinite_rows=1, sigma_max=2, sigma_min=3, mean_sq_norm=4, effective_rank=5, srank=6, pca_rank=7,
                threshold_rank=8, stable_rank=9, numerical_rank=10)
# aleppo_snapshot_take / aleppo_policy_diff: the parameter sets, the indices of the ALEPPO_PD_COUNT doubles
# (aleppo_policy_diff_stat) and the columns of a per-sample row (Engine.snapshot_take / Engine.policy_diff)
SET_LIVE, SET_AVERAGED, SET_SNAPSHOT = 0, 1, 2
SETS = dict(live=SET_LIVE, averaged=SET_AVERAGED, snapshot=SET_SNAPSHOT)
PD_COUNT = 16
PD_ROW = 8
PD_STATS = dict(rows=0, nonfinite_rows=1, churn=2, mean_kl_ab=3, max_kl_ab=4, mean_kl_ba=5, mean_tv=6, max_tv=7,
                mean_abs_dv=8, max_abs_dv=9, rms_dv=10, mean_entropy_a=11, mean_entropy_b=12, mean_feature_cos=13,
                min_feature_cos=14, feature_rel_change=15)
PD_COLUMNS = dict(kl_ab=0, kl_ba=1, tv=2, dv=3, cos=4, dh2=5, g_a=6, g_b=7)
# gradient probes: the slots, aleppo_grad_take's sources and the rows of a Gram - the 12 tensors, then the whole model
# (Engine.grad_probe / grad_take / grad_vector / load_grad / grad_gram)
GRAD_SLOTS = 4
GRAD_SRC_EXP_AVG, GRAD_SRC_PARAM_DELTA = 0, 1
GRAD_SOURCES = dict(exp_avg=GRAD_SRC_EXP_AVG, delta=GRAD_SRC_PARAM_DELTA)
GRAM_NAMES = TENSOR_NAMES[:12] + ("all",)
# aleppo_refresh_advantages: the indices of its ALEPPO_REFRESH_STATS_COUNT doubles - the ten of BATCH_STATS on the fresh
# values, then aleppo_refresh_stat (Engine.refresh_advantages / Engine.refresh_values)
REFRESH_STATS_COUNT = 13
REFRESH_STATS = dict(BATCH_STATS, value_change_mean=10, value_change_std=11, value_change_maxabs=12)
# aleppo_eval_rule / aleppo_eval_field: the evaluation lanes (Engine.eval_open / eval_push_frames / eval_act / eval_read)
EVAL_GREEDY, EVAL_SAMPLE, EVAL_EPSILON_GREEDY = 0, 1, 2
EVAL_RULES = dict(greedy=EVAL_GREEDY, sample=EVAL_SAMPLE, epsilon=EVAL_EPSILON_GREEDY)
EVAL_FIELDS = dict(observations=0, logits=1, values=2, actions=3)
# aleppo_eval_env_field: the device-resident evaluation environments (Engine.eval_env_open / eval_env_run / eval_env_state /
# eval_env_read / eval_env_episodes)
EEF_FRAMES, EEF_EPISODE_RETURNS, EEF_EPISODE_LENGTHS, EEF_GAME_RETURNS, EEF_GAME_LENGTHS = 0, 1, 2, 3, 4
EVAL_ENV_FIELDS = dict(frames=EEF_FRAMES, episode_returns=EEF_EPISODE_RETURNS, episode_lengths=EEF_EPISODE_LENGTHS,
                       game_returns=EEF_GAME_RETURNS, game_lengths=EEF_GAME_LENGTHS)
# device-resident environments (Engine.env_open / env_rollout / env_state / env_read / env_episodes)
ENV_SYNTHETIC = 0
ENV_FIELDS = dict(frames=0, episode_returns=1, episode_lengths=2, game_returns=3, game_lengths=4, step_ms=5)
# aleppo_env_state, 88 bytes without padding (include/aleppo.h)
ENV_STATE_DTYPE = np.dtype([("rng", "<u8"), ("steps", "<u8"), ("ep_len", "<u8"), ("game_len", "<u8"), ("lives", "<i4"),
                            ("paddle", "<i4"), ("ball_x", "<i4"), ("ball_y", "<i4"), ("prev_x", "<i4"), ("prev_y", "<i4"),
                            ("dx", "<i4"), ("dy", "<i4"), ("bricks", "<i4"), ("episode_return", "<f4"), ("reward", "<f4"),
                            ("ep_ret", "<f4"), ("game_ret", "<f4"), ("start", "u1"), ("game_over", "u1"),
                            ("reserved", "u1", (2,))])
# episode recorders (Engine.rec_open / rec_count / rec_read / rec_clear): aleppo_rec_source, the content bits,
# aleppo_rec_field, and aleppo_rec_step, 32 bytes without padding (include/aleppo.h)
REC_ROLLOUT, REC_EVAL = 0, 1
REC_SOURCES = dict(rollout=REC_ROLLOUT, eval=REC_EVAL)
REC_FRAMES, REC_OBSERVATION = 1, 2
REC_FIELDS = dict(steps=0, logits=1, frames=2, observations=3)
REC_MAX_CAPACITY = 65536
REC_STEP_DTYPE = np.dtype([("ordinal", "<u8"), ("action", "<i4"), ("reward", "<f4"), ("value", "<f4"), ("start", "u1"),
                           ("terminated", "u1"), ("truncated", "u1"), ("game_over", "u1"), ("lives", "<i4"),
                           ("reserved", "<i4")])
KERNEL_CLASSES = dict(ingest=0, gae=1, head=2, adam=3, conv1_fwd=4, conv2_fwd=5, conv3_fwd=6, fc_fwd=7, fc_dgrad=8,
                      fc_wgrad=9, conv3_dgrad=10, conv3_wgrad=11, conv2_dgrad=12, conv2_wgrad=13, conv1_wgrad=14,
                      reduce=15, infer_head=16, act_fused=17, conv_fwd=18, conv_bwd=19, rec_capture=20,
                      act_stats=21, recycle=22, sal_blur=23, sal_perturb=24, sal_score=25, ema=26)

# every symbol include/aleppo.h declares (checked by tests/test_abi.py against the header text)
# aleppo_set_option keys (include/aleppo.h)
OPT_GENERIC_CONV, OPT_DEBUG_NO_PUBLISH, OPT_FORCE_COMM, OPT_SERIAL_UPDATE = 0, 1, 2, 3
OPT_FC_PIPE, OPT_FUSED_ACT, OPT_UPDATE_GRAPH = 4, 6, 7
OPT_GATE_TIMEOUT_MS = 9
OPT_FUSED_FWD = 10
OPT_FUSED_BWD = 11
OPT_MINIBATCH_SHUFFLE = 12
OPT_VALUE_CLIP = 13
OPT_ADV_NORM_MINIBATCH = 14
OPT_KL_PENALTY = 15
OPT_KL_COEF = 16  # (the value is beta's binary32 bit pattern: Engine.set_kl_coef / Engine.kl_coef)
# the per-update hyper-parameters, each as its binary32 bit pattern (Engine.set_hyper / Engine.hyper)
OPT_CLIP_PARAM, OPT_VALUE_CLIP_RANGE, OPT_VALUE_LOSS_COEF, OPT_ENTROPY_COEF, OPT_MAX_GRAD_NORM = 17, 18, 19, 20, 21
# return-based reward scaling in place of the clamp (Engine.set_reward_scaling); the clip as its binary32 bit pattern
OPT_REWARD_SCALE, OPT_REWARD_SCALE_CLIP = 23, 24  # (22 is unassigned)
# which parameters the evaluation lanes act on: 0 live, 1 the averaged set of Engine.ema_open (Engine.eval_use_averaged)
OPT_EVAL_PARAMS = 25
# decoupled weight decay and the pull toward the anchor inside the optimizer step, each as its binary32 bit pattern
# (Engine.set_regularization / Engine.regularization)
OPT_WEIGHT_DECAY, OPT_ANCHOR_COEF = 26, 27
# test hook: the fused bf16 acting launch also stores conv1 / conv2 for Engine.export_acting
OPT_ACT_STORE = 28
REG_OPTIONS = dict(weight_decay=OPT_WEIGHT_DECAY, anchor_coef=OPT_ANCHOR_COEF)
HYPER_OPTIONS = dict(clip_param=OPT_CLIP_PARAM, value_clip_range=OPT_VALUE_CLIP_RANGE,
                     value_loss_coef=OPT_VALUE_LOSS_COEF, entropy_coef=OPT_ENTROPY_COEF,
                     max_grad_norm=OPT_MAX_GRAD_NORM)


def float_bits(x):
    """the IEEE-754 binary32 bit pattern of x (rounded to float32) as the signed int aleppo_set_option takes"""
    return struct.unpack("<i", struct.pack("<f", x))[0]


def bits_float(v):
    """the float32 whose binary32 bit pattern is the low 32 bits of v (what aleppo_get_option returned)"""
    return struct.unpack("<f", struct.pack("<I", v & 0xFFFFFFFF))[0]

EXPORTS = [
    "aleppo_abi_version", "aleppo_create", "aleppo_destroy", "aleppo_last_error", "aleppo_param_count",
    "aleppo_load_params", "aleppo_export_params", "aleppo_export_grads", "aleppo_act", "aleppo_push_frames",
    "aleppo_set_gray_lut", "aleppo_record_step", "aleppo_step", "aleppo_finish_rollout", "aleppo_train",
    "aleppo_read_train_metric", "aleppo_set_batch", "aleppo_read_batch", "aleppo_forward", "aleppo_comm_unique_id",
    "aleppo_comm_init", "aleppo_gae", "aleppo_vision_resize_area", "aleppo_vision_rgb_to_gray", "aleppo_preprocess",
    "aleppo_update_observations", "aleppo_ppo_loss", "aleppo_sample", "aleppo_profile_enable", "aleppo_profile_read",
    "aleppo_profile_reset", "aleppo_synchronize", "aleppo_set_option", "aleppo_export_optimizer",
    "aleppo_import_optimizer", "aleppo_replay_rollout", "aleppo_get_option",
    "aleppo_host_alloc", "aleppo_host_free", "aleppo_arm_step", "aleppo_release_step", "aleppo_device_check",
    "aleppo_read_sample_order", "aleppo_set_batch_values",
    "aleppo_eval_open", "aleppo_eval_push_frames", "aleppo_eval_act", "aleppo_eval_read",
    "aleppo_eval_set_counter",
    "aleppo_export_reward_scale", "aleppo_import_reward_scale", "aleppo_reward_scale",
    "aleppo_export_rollout_state", "aleppo_import_rollout_state", "aleppo_state_digest",
    "aleppo_tensor_stats",
    "aleppo_forward_activations", "aleppo_activation_stats", "aleppo_export_backward", "aleppo_export_acting",
    "aleppo_recycle_units", "aleppo_recycle_dormant",
    "aleppo_ema_open", "aleppo_ema_update", "aleppo_ema_read", "aleppo_ema_export", "aleppo_ema_import",
    "aleppo_saliency_tables", "aleppo_saliency", "aleppo_saliency_perturbed",
    "aleppo_feature_rank",
    "aleppo_snapshot_take", "aleppo_snapshot_export", "aleppo_snapshot_import", "aleppo_policy_diff",
    "aleppo_refresh_advantages", "aleppo_refresh_read",
    "aleppo_grad_probe", "aleppo_grad_take", "aleppo_grad_export", "aleppo_grad_import", "aleppo_grad_gram",
    "aleppo_anchor_take", "aleppo_anchor_import", "aleppo_anchor_export", "aleppo_shrink_perturb",
    "aleppo_env_open", "aleppo_env_rollout", "aleppo_env_export_state", "aleppo_env_import_state", "aleppo_env_read",
    "aleppo_eval_env_open", "aleppo_eval_env_run", "aleppo_eval_env_export_state", "aleppo_eval_env_import_state",
    "aleppo_eval_env_read",
    "aleppo_rec_open", "aleppo_rec_count", "aleppo_rec_read", "aleppo_rec_clear",
]


class AleppoError(RuntimeError):
    """ALEPPO_ERR_RUNTIME / HIP / NO_DEVICE (std::runtime_error in the reference)."""


class AleppoInvalidArgument(ValueError):
    """ALEPPO_ERR_INVALID_ARGUMENT (std::invalid_argument in the reference)."""


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device_ordinal", C.c_int32), ("world_size", C.c_int32),
                ("rank", C.c_int32), ("num_envs", C.c_int32), ("horizon", C.c_int32), ("num_actions", C.c_int32),
                ("hidden_size", C.c_int32), ("frame_stack", C.c_int32), ("precision", C.c_int32),
                ("advantage_norm", C.c_int32), ("max_minibatch", C.c_int32), ("rollout_precision", C.c_int32),
                ("gamma", C.c_float),
                ("lambda_", C.c_float), ("clip_param", C.c_float), ("value_loss_coef", C.c_float),
                ("entropy_coef", C.c_float), ("max_gradient_norm", C.c_float), ("adam_beta1", C.c_float),
                ("adam_beta2", C.c_float), ("adam_eps", C.c_float), ("seed", C.c_uint64)]


class SaliencyConfig(C.Structure):
    _fields_ = [("stride", C.c_int32), ("planes", C.c_int32), ("sigma_mask", C.c_double), ("sigma_blur", C.c_double)]


class FeatureRankConfig(C.Structure):
    _fields_ = [("delta", C.c_float), ("eps", C.c_float), ("centered", C.c_int32), ("reserved", C.c_int32)]


class GradProbeConfig(C.Structure):
    _fields_ = [("policy_term", C.c_int32), ("value_loss_coef", C.c_float), ("entropy_coef", C.c_float),
                ("reserved", C.c_int32)]


class EnvConfig(C.Structure):
    _fields_ = [("kind", C.c_int32), ("frame_kind", C.c_int32), ("seed_base", C.c_uint64), ("max_steps", C.c_uint64),
                ("max_return", C.c_float), ("reserved", C.c_int32)]


class RecConfig(C.Structure):
    _fields_ = [("source", C.c_int32), ("index", C.c_int32), ("content", C.c_int32), ("capacity", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class RecStep(C.Structure):
    _fields_ = [("ordinal", C.c_uint64), ("action", C.c_int32), ("reward", C.c_float), ("value", C.c_float),
                ("start", C.c_uint8), ("terminated", C.c_uint8), ("truncated", C.c_uint8), ("game_over", C.c_uint8),
                ("lives", C.c_int32), ("reserved", C.c_int32)]


class RecCounts(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("dropped", C.c_uint64), ("next_ordinal", C.c_uint64), ("capacity", C.c_int32),
                ("frame_bytes", C.c_int32), ("observation_bytes", C.c_int32), ("actions", C.c_int32)]


class MinibatchMetrics(C.Structure):
    _fields_ = [("loss", C.c_float), ("grad_norm", C.c_float), ("clipped_loss", C.c_float),
                ("value_loss", C.c_float), ("entropy", C.c_float), ("ratio", C.c_float), ("mask_count", C.c_float)]


_lib = None


def lib():
    """Load libaleppo.so; fail loudly when the HIP extension has not been built (no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AleppoError(f"HIP extension missing: {LIB_PATH} (run __graft_entry__.build()); "
                              "this package has no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _lib.aleppo_last_error.restype = C.c_char_p
        _lib.aleppo_last_error.argtypes = [C.c_void_p]
        for name in EXPORTS:
            getattr(_lib, name)  # AttributeError here = ABI drift
    return _lib


def _check(rc, ctx=None):
    if rc == OK:
        return
    msg = lib().aleppo_last_error(ctx)
    msg = msg.decode() if msg else f"aleppo error {rc}"
    if rc == ERR_INVALID_ARGUMENT:
        raise AleppoInvalidArgument(msg)
    raise AleppoError(msg)


def saliency_grid(stride=SALIENCY_STRIDE):
    """G = ceil(84 / stride): the points per axis of the saliency grid (point (gy, gx) has its centre at pixel
    (gy * stride, gx * stride))"""
    return (84 + stride - 1) // stride


def saliency_tables(stride=SALIENCY_STRIDE, sigma_mask=SALIENCY_SIGMA_MASK, sigma_blur=SALIENCY_SIGMA_BLUR,
                    planes=SALIENCY_PLANES):
    """aleppo_saliency_tables: (mask profile uint16 [84], blur taps uint16 [84] - w[0 .. R], zero beyond -, R), the integer
    tables Engine.saliency perturbs with.  Built on the host: no context, no device."""
    cfg = SaliencyConfig(stride, planes, sigma_mask, sigma_blur)
    g, w, r = np.zeros(84, np.uint16), np.zeros(84, np.uint16), C.c_int32()
    _check(lib().aleppo_saliency_tables(C.byref(cfg), _ptr(g), _ptr(w), C.byref(r)))
    return g, w, r.value


def device_check(device=0):
    """aleppo_device_check: raises AleppoError ("no CPU fallback") unless HIP device `device` is a gfx950"""
    _check(lib().aleppo_device_check(C.c_int(device)))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------- stateless operators
def _gae(advantages, rewards, values, next_values, terminals, truncations, episode_starts, gamma, lam, device=0):
    """ai::gae::gae (src/ai/gae.h:4-7): writes `advantages` in place; same argument checks/errors."""
    rewards, values, next_values = _f32(rewards), _f32(values), _f32(next_values)
    if rewards.ndim != 2 or values.ndim != 2 or next_values.ndim != 1 or np.ndim(terminals) != 2 or \
            np.ndim(truncations) != 2 or np.ndim(episode_starts) != 2:
        raise AleppoInvalidArgument("All input tensors must be 2D except next_values which must be 1D.")
    E, T = rewards.shape
    te, tr, st = _u8(terminals), _u8(truncations), _u8(episode_starts)
    if values.shape[0] != E or te.shape[0] != E or tr.shape[0] != E or st.shape[0] != E or next_values.shape[0] != E:
        raise AleppoInvalidArgument("Input tensors must have compatible dimensions.")
    out = np.zeros((E, T), np.float32)
    _check(lib().aleppo_gae(C.c_int(device), _ptr(out), _ptr(rewards), _ptr(values), _ptr(next_values), _ptr(te),
                            _ptr(tr), _ptr(st), C.c_int64(E), C.c_int64(T), C.c_float(gamma), C.c_float(lam)))
    advantages[...] = out
    return advantages


def _resize_frame_stacked_grayscale_images(images, device=0):
    """ai::vision::resize_frame_stacked_grayscale_images (vision.cc:22-32): f32 [B,S,210,160] -> [B,S,84,84]"""
    images = _f32(images)
    assert images.shape[-2:] == (210, 160)
    lead = images.shape[:-2]
    n = int(np.prod(lead)) if lead else 1
    out = np.zeros((n, 84, 84), np.float32)
    _check(lib().aleppo_vision_resize_area(C.c_int(device), _ptr(images), _ptr(out), C.c_int64(n)))
    return out.reshape(lead + (84, 84))


def _rgb_to_grayscale_frame_stacked_images(images, device=0):
    """ai::vision::rgb_to_grayscale_frame_stacked_images (vision.cc:71-84): f32 [B,S,3,84,84] -> [B,S,84,84]"""
    images = _f32(images)
    assert images.shape[-3:] == (3, 84, 84)
    lead = images.shape[:-3]
    n = int(np.prod(lead)) if lead else 1
    out = np.zeros((n, 84, 84), np.float32)
    _check(lib().aleppo_vision_rgb_to_gray(C.c_int(device), _ptr(images), _ptr(out), C.c_int64(n)))
    return out.reshape(lead + (84, 84))


def _preprocess(raw_pairs, lut=None, device=0):
    """fused device preprocessing: u8 [n,2,210,160] (+256-entry LUT) -> u8 [n,84,84]"""
    raw = _u8(raw_pairs)
    assert raw.shape[1:] == (2, 210, 160)
    out = np.zeros((raw.shape[0], 84, 84), np.uint8)
    l = None if lut is None else _u8(lut)
    _check(lib().aleppo_preprocess(C.c_int(device), _ptr(raw), _ptr(l), _ptr(out), C.c_int64(raw.shape[0])))
    return out


def _update_observations(observations, frames, episode_start, device=0):
    """Rollout::update_observations (rollout.cc:184-196) on u8 [E,4,84,84]; returns the new stack."""
    obs = _u8(observations).copy()
    _check(lib().aleppo_update_observations(C.c_int(device), _ptr(obs), _ptr(_u8(frames)), _ptr(_u8(episode_start)),
                                            C.c_int64(obs.shape[0])))
    return obs


def _losses_compute(logits, old_log_probabilities, actions, advantages, values, returns, masks, clip_param,
                    value_loss_coef, entropy_coef, device=0):
    """ai::ppo::losses::compute on normalize_logits(logits) (losses.cc:4-47) + its gradients.
    Returns the reference's Metrics fields plus dlogits / dvalues."""
    logits, olp = _f32(logits), _f32(old_log_probabilities)
    B, A = logits.shape
    o = SimpleNamespace(loss=np.zeros(1, np.float32), clipped_losses=np.zeros(B, np.float32),
                        value_losses=np.zeros(B, np.float32), entropies=np.zeros(B, np.float32),
                        total_losses=np.zeros(B, np.float32), ratio=np.zeros(B, np.float32),
                        dlogits=np.zeros((B, A), np.float32), dvalues=np.zeros(B, np.float32))
    _check(lib().aleppo_ppo_loss(C.c_int(device), _ptr(logits), _ptr(olp), _ptr(_i64(actions)),
                                 _ptr(_f32(advantages)), _ptr(_f32(values)), _ptr(_f32(returns)), _ptr(_u8(masks)),
                                 C.c_int64(B), C.c_int64(A), C.c_float(clip_param), C.c_float(value_loss_coef),
                                 C.c_float(entropy_coef), _ptr(o.loss), _ptr(o.clipped_losses), _ptr(o.value_losses),
                                 _ptr(o.entropies), _ptr(o.total_losses), _ptr(o.ratio), _ptr(o.dlogits),
                                 _ptr(o.dvalues)))
    o.masks = _u8(masks)
    return o


def _sample(probs, q, device=0):
    """torch::multinomial(probs, 1, true) given its Exp(1) noise q (train.cc:374-375): argmax(p/q)."""
    probs, q = _f32(probs), _f32(q)
    a = np.zeros(probs.shape[0], np.int64)
    _check(lib().aleppo_sample(C.c_int(device), _ptr(probs), _ptr(q), _ptr(a), C.c_int64(probs.shape[0]),
                               C.c_int64(probs.shape[1])))
    return a


def _reward_scale(rewards, terminals, truncations, episode_starts, gamma, clip, stats, returns, device=0):
    """aleppo_reward_scale: OPT_REWARD_SCALE's five steps on one rollout, env-major [E,T], through the kernels
    finish_rollout launches.  stats = (count, mean, var), returns = the running returns float64 [E], both BEFORE the
    rollout.  Returns (scaled rewards float32 [E,T], stats after float64 [3], returns after float64 [E], scale float32,
    clipped int); the arguments are not modified."""
    r = _f32(rewards).copy()
    if r.ndim != 2 or np.ndim(terminals) != 2 or np.ndim(truncations) != 2 or np.ndim(episode_starts) != 2:
        raise AleppoInvalidArgument("All input tensors must be 2D except returns which must be 1D.")
    E, T = r.shape
    te, tr, st = _u8(terminals), _u8(truncations), _u8(episode_starts)
    g = np.array(returns, dtype=np.float64).ravel()
    if te.shape != (E, T) or tr.shape != (E, T) or st.shape != (E, T) or g.shape != (E,):
        raise AleppoInvalidArgument("Input tensors must have compatible dimensions.")
    s3 = np.array(stats, dtype=np.float64).ravel()
    if s3.shape != (3,):
        raise AleppoInvalidArgument("stats must be (count, mean, var)")
    scale, clipped = C.c_float(), C.c_int64()
    _check(lib().aleppo_reward_scale(C.c_int(device), _ptr(r), _ptr(te), _ptr(tr), _ptr(st), C.c_int64(E), C.c_int64(T),
                                     C.c_float(gamma), C.c_float(clip), _ptr(s3), _ptr(g), C.byref(scale),
                                     C.byref(clipped)))
    return r, s3, g, np.float32(scale.value), int(clipped.value)


gae = SimpleNamespace(gae=_gae)
rewards = SimpleNamespace(scale=_reward_scale)
vision = SimpleNamespace(resize_frame_stacked_grayscale_images=_resize_frame_stacked_grayscale_images,
                         rgb_to_grayscale_frame_stacked_images=_rgb_to_grayscale_frame_stacked_images,
                         preprocess=_preprocess)
losses = SimpleNamespace(compute=_losses_compute)
sampling = SimpleNamespace(multinomial_with_noise=_sample)
rollout = SimpleNamespace(update_observations=_update_observations)


# ---------------------------------------------------------------------------- engine
def env_shard(total_environments, world_size, rank):
    """env index e -> (rank = e // E_g, e_local = e % E_g): contiguous env blocks per rank."""
    if total_environments % world_size:
        raise AleppoInvalidArgument("total_environments must be divisible by world_size")
    eg = total_environments // world_size
    return range(rank * eg, (rank + 1) * eg)


class Engine:
    """One rank's hot path: network + Adam + rollout buffer + PPO update, all on one MI355X.

    Mirrors what main() wires together (src/bin/train.cc:358-458).  Per slot:
    ``act`` -> caller steps its emulators -> ``step`` (or push_frames + record_step);
    then ``finish_rollout`` and ``train``."""

    def __init__(self, num_envs, horizon, num_actions=4, hidden_size=512, precision=FP32, gamma=0.99, lam=0.95,
                 clip_param=0.1, value_loss_coef=0.5, entropy_coef=0.01, max_gradient_norm=0.5, device=0,
                 world_size=1, rank=0, seed=42, advantage_norm=False, max_minibatch=0, rollout_precision=ROLLOUT_FP32):
        self.cfg = Config(ABI_VERSION, device, world_size, rank, num_envs, horizon, num_actions, hidden_size, 4,
                          precision, int(advantage_norm), max_minibatch, rollout_precision, gamma, lam, clip_param,
                          value_loss_coef, entropy_coef, max_gradient_norm, 0.0, 0.0, 0.0, seed)
        self._ctx = C.c_void_p()
        _check(lib().aleppo_create(C.byref(self.cfg), C.byref(self._ctx)))
        self.E, self.T, self.A, self.H = num_envs, horizon, num_actions, hidden_size
        self._batch_n = num_envs * horizon  # samples in the training arrays (aleppo_set_batch may hold fewer)
        n = C.c_size_t()
        _check(lib().aleppo_param_count(self._ctx, C.byref(n)), self._ctx)
        self.param_count = n.value
        self._f_act = lib().aleppo_act
        self._f_step = lib().aleppo_step
        self._f_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]
        self._act_ptr = C.POINTER(C.c_int64)()
        self._act_out = C.byref(self._act_ptr)
        self.actions = None  # view of the pinned action buffer, valid after the first act
        self._last_B = 1  # samples per minibatch of the last train() (export_backward's default capacity)
        self._ema_open = False  # ema_open has succeeded (run_state carries the average only then)
        self._anchor_on = False  # an anchor_take / load_anchor has succeeded (run_state carries the anchor only then)

    def close(self):
        if getattr(self, "_ctx", None):
            lib().aleppo_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def _c(self, rc):
        _check(rc, self._ctx)

    # -- parameters (libtorch parameters() order) --
    def load_params(self, flat):
        flat = _f32(flat).ravel()
        self._c(lib().aleppo_load_params(self._ctx, _ptr(flat), C.c_size_t(flat.size)))

    def export_params(self):
        out = np.zeros(self.param_count, np.float32)
        self._c(lib().aleppo_export_params(self._ctx, _ptr(out), C.c_size_t(out.size)))
        return out

    def export_grads(self):
        out = np.zeros(self.param_count, np.float32)
        self._c(lib().aleppo_export_grads(self._ctx, _ptr(out), C.c_size_t(out.size)))
        return out

    # -- checkpoint / resume --
    def state_dict(self):
        m = np.zeros(self.param_count, np.float32)
        v = np.zeros(self.param_count, np.float32)
        step = C.c_int64()
        self._c(lib().aleppo_export_optimizer(self._ctx, _ptr(m), _ptr(v), C.byref(step), C.c_size_t(m.size)))
        sd = dict(params=self.export_params(), exp_avg=m, exp_avg_sq=v, step=np.int64(step.value))
        if self.get_option(OPT_REWARD_SCALE):  # (only while the option is on: the keys other callers see stay the same)
            sd["reward_scale"] = self.reward_scale_state()
        return sd

    def load_state_dict(self, sd):
        self.load_params(sd["params"])  # resets Adam, then restore it
        m, v = _f32(sd["exp_avg"]).ravel(), _f32(sd["exp_avg_sq"]).ravel()
        self._c(lib().aleppo_import_optimizer(self._ctx, _ptr(m), _ptr(v), C.c_int64(int(sd["step"])),
                                              C.c_size_t(m.size)))
        if "reward_scale" in sd:
            self.load_reward_scale_state(sd["reward_scale"])

    def rollout_state(self):
        """aleppo_export_rollout_state, between rollouts only: {"observations": uint8 [E,4,84,84] the next act acts on,
        "counter": the acting generator's counter}"""
        obs = np.zeros((self.E, 4, 84, 84), np.uint8)
        words = np.zeros(ROLLOUT_STATE_WORDS, np.uint64)
        self._c(lib().aleppo_export_rollout_state(self._ctx, _ptr(obs), _ptr(words), C.c_size_t(self.E)))
        return dict(observations=obs, counter=int(words[0]))

    def load_rollout_state(self, state):
        """aleppo_import_rollout_state: what rollout_state returned"""
        obs = _u8(state["observations"])
        if obs.shape != (self.E, 4, 84, 84):
            raise AleppoInvalidArgument("rollout state observations must be uint8 [E,4,84,84]")
        words = np.zeros(ROLLOUT_STATE_WORDS, np.uint64)
        words[0] = int(state["counter"])
        self._c(lib().aleppo_import_rollout_state(self._ctx, _ptr(obs), _ptr(words), C.c_size_t(self.E)))

    def run_state(self):
        """the whole run state between rollouts: state_dict() plus "rollout" (rollout_state) and, whether the option is on
        or not, "reward_scale"; a fresh Engine that loads it continues the run bit for bit"""
        sd = self.state_dict()
        sd["reward_scale"] = self.reward_scale_state()
        sd["rollout"] = self.rollout_state()
        if self._ema_open:  # (only while the average is open: the keys other callers see stay the same)
            flat, updates = self.ema_params()
            sd["ema"] = dict(params=flat, updates=np.int64(updates))
        if self._anchor_on:  # (only once there is an anchor)
            sd["anchor"] = self.anchor_params()
        return sd

    def load_run_state(self, sd):
        """what run_state returned"""
        self.load_state_dict(sd)
        self.load_rollout_state(sd["rollout"])
        if "ema" in sd:
            if not self._ema_open:
                self.ema_open()
            self.load_ema(sd["ema"]["params"], int(sd["ema"]["updates"]))
        if "anchor" in sd:
            self.load_anchor(sd["anchor"])

    # -- exponentially averaged parameters --
    def ema_open(self):
        """aleppo_ema_open: allocate the averaged parameters on first use and (re)start them at the live parameters with
        updates = 0"""
        self._c(lib().aleppo_ema_open(self._ctx))
        self._ema_open = True

    def ema_update(self, decay):
        """aleppo_ema_update: average = decay * average + (1 - decay) * parameters, three fp32 operations per element, on
        the device; enqueued, not waited for"""
        self._c(lib().aleppo_ema_update(self._ctx, C.c_double(decay)))

    def ema_stats(self):
        """aleppo_ema_read: {"updates", "decay", "norm", "param_norm", "distance", "relative_distance"} -> float, as the
        last open / update / import left them"""
        out = np.zeros(EMA_STATS_COUNT, np.float64)
        self._c(lib().aleppo_ema_read(self._ctx, _ptr(out)))
        return {name: float(out[i]) for name, i in EMA_STATS.items()}

    def ema_params(self):
        """aleppo_ema_export: (the averaged parameters as flat float32 in libtorch parameters() order, updates)"""
        out = np.zeros(self.param_count, np.float32)
        updates = C.c_int64()
        self._c(lib().aleppo_ema_export(self._ctx, _ptr(out), C.c_size_t(out.size), C.byref(updates)))
        return out, int(updates.value)

    def load_ema(self, flat, updates=0):
        """aleppo_ema_import: what ema_params returned"""
        flat = _f32(flat).ravel()
        self._c(lib().aleppo_ema_import(self._ctx, _ptr(flat), C.c_size_t(flat.size), C.c_int64(int(updates))))

    def eval_use_averaged(self, on):
        """ALEPPO_OPT_EVAL_PARAMS: the evaluation lanes (eval_act, eval_env_run) act on the averaged parameters (True) or
        on the live ones (False, the default); needs ema_open first"""
        self.set_option(OPT_EVAL_PARAMS, 1 if on else 0)

    def state_digest(self):
        """aleppo_state_digest: {"params", "optimizer", "rollout", "reward_scale"} -> int, the 64-bit words of aleppo.h,
        computed on the device; between rollouts only"""
        out = np.zeros(DIGEST_COUNT, np.uint64)
        self._c(lib().aleppo_state_digest(self._ctx, _ptr(out)))
        return {name: int(out[i]) for name, i in DIGEST_SECTIONS.items()}

    def tensor_stats(self, sections="all", raw=False):
        """aleppo_tensor_stats: per-tensor norms, maxima and non-finite counts of the parameters ("params"), of the last
        minibatch's clipped gradient and of the last optimizer step ("step": needs a train() with no load_params /
        load_state_dict since), or both ("all"), reduced on the device.  {tensor: {stat: float}} over TENSOR_NAMES and
        TENSOR_STATS; raw=True: the float64 [13, 10] array.  `sections` may also be the bits themselves.  The columns of a
        section that was not asked for are 0."""
        bits = TENSOR_STATS_SECTIONS[sections] if isinstance(sections, str) else int(sections)
        out = np.zeros((TENSOR_STATS_ROWS, TENSOR_STATS_COLS), np.float64)
        self._c(lib().aleppo_tensor_stats(self._ctx, C.c_int(bits), _ptr(out), C.c_size_t(out.size)))
        if raw:
            return out
        return {t: {name: float(out[r, i]) for name, i in TENSOR_STATS.items()} for r, t in enumerate(TENSOR_NAMES)}

    # -- return-based reward scaling (OPT_REWARD_SCALE) --
    def set_reward_scaling(self, on, clip=10.0):
        """OPT_REWARD_SCALE / OPT_REWARD_SCALE_CLIP: from the next finish_rollout on, divide the rewards by the running
        standard deviation of the discounted return and clip them at +-clip (finite, > 0; rounded to float32) instead of
        clamping them to [-1, 1].  Under data parallelism every rank sets the same values."""
        self.set_option(OPT_REWARD_SCALE_CLIP, float_bits(clip))
        self.set_option(OPT_REWARD_SCALE, int(bool(on)))

    def reward_scale(self):
        """ALEPPO_F_REWARD_SCALE: {count, mean, var, scale, batch_count, clipped} (aleppo.h)"""
        a = self.read_batch("reward_scale")
        return {name: float(a[i]) for name, i in REWARD_SCALE.items()}

    def reward_scale_state(self):
        """aleppo_export_reward_scale: {"stats": float64 [3] (count, mean, var), "returns": float64 [E]}"""
        stats, g = np.zeros(3, np.float64), np.zeros(self.E, np.float64)
        self._c(lib().aleppo_export_reward_scale(self._ctx, _ptr(stats), _ptr(g), C.c_size_t(g.size)))
        return dict(stats=stats, returns=g)

    def load_reward_scale_state(self, state):
        """aleppo_import_reward_scale: what reward_scale_state returned"""
        stats = np.ascontiguousarray(state["stats"], dtype=np.float64).ravel()
        g = np.ascontiguousarray(state["returns"], dtype=np.float64).ravel()
        if stats.size != 3:
            raise AleppoInvalidArgument("reward scale stats must be (count, mean, var)")
        self._c(lib().aleppo_import_reward_scale(self._ctx, _ptr(stats), _ptr(g), C.c_size_t(g.size)))

    # -- rollout --
    def act(self, noise=None):
        p = C.POINTER(C.c_int64)()
        n = None if noise is None else _f32(noise)
        self._c(lib().aleppo_act(self._ctx, _ptr(n), C.byref(p)))
        self.actions = np.ctypeslib.as_array(p, shape=(self.E,))  # view of the pinned buffer
        return self.actions

    def push_frames(self, frames, episode_start, kind=FRAMES_84, device_ptr=None):
        st = _u8(episode_start)
        if device_ptr is not None:
            self._c(lib().aleppo_push_frames(self._ctx, C.c_void_p(device_ptr), kind, DEVICE, _ptr(st)))
        else:
            self._c(lib().aleppo_push_frames(self._ctx, _ptr(_u8(frames)), kind, HOST, _ptr(st)))

    def record_step(self, rewards, terminated, truncated, episode_start):
        self._c(lib().aleppo_record_step(self._ctx, _ptr(_f32(rewards)), _ptr(_u8(terminated)), _ptr(_u8(truncated)),
                                         _ptr(_u8(episode_start))))

    def step(self, frames, rewards, terminated, truncated, episode_start, kind=FRAMES_84, device_ptr=None):
        fr = C.c_void_p(device_ptr) if device_ptr is not None else _ptr(_u8(frames))
        loc = DEVICE if device_ptr is not None else HOST
        self._c(lib().aleppo_step(self._ctx, fr, kind, loc, _ptr(_f32(rewards)), _ptr(_u8(terminated)),
                                  _ptr(_u8(truncated)), _ptr(_u8(episode_start))))

    def arm_step(self, frames_addr, start_addr, kind=FRAMES_84, noise_next=None):
        """aleppo_arm_step: enqueue the next step (frames / episode-start bytes at mapped host addresses the emulators are
        about to fill) and the next slot's acting kernels behind the release word"""
        n = None if noise_next is None else _f32(noise_next)
        self._c(lib().aleppo_arm_step(self._ctx, C.c_void_p(frames_addr), kind, C.c_void_p(start_addr), _ptr(n)))

    def release_step(self, rewards, terminated, truncated):
        """aleppo_release_step: the emulators are done - release the stream, record the slot's scalars"""
        self._c(lib().aleppo_release_step(self._ctx, _ptr(_f32(rewards)), _ptr(_u8(terminated)), _ptr(_u8(truncated))))

    # -- low-overhead variants for tight host loops: raw addresses, no numpy conversions --
    def act_fast(self):
        """aleppo_act with the built-in RNG; returns nothing (read self.actions, a view of the pinned buffer)"""
        rc = self._f_act(self._ctx, None, self._act_out)
        if rc:
            self._c(rc)

    def step_ptr(self, frames_addr, location, kind, rewards_addr, term_addr, trunc_addr, start_addr):
        """aleppo_step on raw addresses (host arrays must stay alive and be C-contiguous of the right dtype)"""
        rc = self._f_step(self._ctx, frames_addr, kind, location, rewards_addr, term_addr, trunc_addr, start_addr)
        if rc:
            self._c(rc)

    def replay_rollout(self, frames_addr, kind, slot_stride_bytes, rewards, terminated, truncated, episode_start,
                       noise=None, location=DEVICE):
        """aleppo_replay_rollout: the T-slot act/step loop over a recorded trace (frames in device or mapped
        page-locked host memory, host [T][E] scalars, optional [T][E][A] sampling noise)"""
        r, te, tr, st = _f32(rewards), _u8(terminated), _u8(truncated), _u8(episode_start)
        for a in (r, te, tr, st):
            if a.shape != (self.T, self.E):
                raise AleppoInvalidArgument("replay_rollout: scalars must be [T][E]")
        nz = None
        if noise is not None:
            nz = _f32(noise)
            if nz.shape != (self.T, self.E, self.A):
                raise AleppoInvalidArgument("replay_rollout: noise must be [T][E][A]")
        self._c(lib().aleppo_replay_rollout(self._ctx, C.c_void_p(frames_addr), int(kind), int(location),
                                            C.c_size_t(slot_stride_bytes), _ptr(r), _ptr(te), _ptr(tr), _ptr(st),
                                            _ptr(nz)))

    def host_alloc(self, nbytes):
        """mapped page-locked host memory for frame buffers (pass its address with location=HOST_MAPPED)"""
        p = C.c_void_p()
        self._c(lib().aleppo_host_alloc(self._ctx, C.c_size_t(nbytes), C.byref(p)))
        return p.value

    def host_free(self, addr):
        self._c(lib().aleppo_host_free(self._ctx, C.c_void_p(addr)))

    def set_gray_lut(self, lut):
        self._c(lib().aleppo_set_gray_lut(self._ctx, _ptr(_u8(lut))))

    def finish_rollout(self, noise=None):
        n = None if noise is None else _f32(noise)
        self._c(lib().aleppo_finish_rollout(self._ctx, _ptr(n)))
        self._batch_n = self.E * self.T

    # -- update --
    def train(self, lr, epochs, num_mini_batches):
        out = (MinibatchMetrics * (epochs * num_mini_batches))()
        self._c(lib().aleppo_train(self._ctx, C.c_double(lr), epochs, num_mini_batches, out))
        self._last_B = self._batch_n // num_mini_batches
        keys = [f[0] for f in MinibatchMetrics._fields_]
        return {k: np.array([getattr(m, k) for m in out], np.float32).reshape(epochs, num_mini_batches) for k in keys}

    def read_train_metric(self, name, epochs, M, B):
        out = np.zeros((epochs, M, B), np.float32)
        self._c(lib().aleppo_read_train_metric(self._ctx, METRIC_FIELDS[name], _ptr(out), C.c_size_t(out.size)))
        return out

    def train_diagnostics(self, epochs, M):
        """{"approx_kl", "clip_fraction"}: float32 [epochs, M] masked means of the last train (aleppo.h: the k3
        approx-KL estimator and the strict clip fraction, over the global unmasked count)"""
        out = {}
        for name in ("approx_kl", "clip_fraction"):
            field = METRIC_MEAN_FIELDS[name]
            a = np.zeros((epochs, M), np.float32)
            self._c(lib().aleppo_read_train_metric(self._ctx, field, _ptr(a), C.c_size_t(a.size)))
            out[name] = a
        return out

    def advantage_stats(self, epochs, M):
        """(mean, std): float32 [epochs, M] statistics OPT_ADV_NORM_MINIBATCH normalised each minibatch's advantages with
        in the last train (aleppo.h: mean_f and (float)std of the unmasked advantages)"""
        out = []
        for field in (METRIC_ADV_FIELDS["mean"], METRIC_ADV_FIELDS["std"]):
            a = np.zeros((epochs, M), np.float32)
            self._c(lib().aleppo_read_train_metric(self._ctx, field, _ptr(a), C.c_size_t(a.size)))
            out.append(a)
        return tuple(out)

    def kl_divergence(self, epochs, M):
        """float32 [epochs, M] masked means of the exact KL(pi_old || pi) OPT_KL_PENALTY computed in the last train
        (global means under data parallelism); the per-sample plane is read_train_metric("kl", ...)"""
        a = np.zeros((epochs, M), np.float32)
        self._c(lib().aleppo_read_train_metric(self._ctx, METRIC_MEAN_FIELDS["kl"], _ptr(a), C.c_size_t(a.size)))
        return a

    def set_kl_coef(self, beta):
        """OPT_KL_COEF: beta of OPT_KL_PENALTY (a finite non-negative float, rounded to float32), passed as its bits"""
        self.set_option(OPT_KL_COEF, struct.unpack("<i", struct.pack("<f", beta))[0])

    def kl_coef(self):
        """the float32 beta of OPT_KL_COEF"""
        return struct.unpack("<f", struct.pack("<I", self.get_option(OPT_KL_COEF) & 0xFFFFFFFF))[0]

    def set_hyper(self, clip_param=None, value_clip_range=None, value_loss_coef=None, entropy_coef=None,
                  max_grad_norm=None):
        """OPT_CLIP_PARAM / OPT_VALUE_CLIP_RANGE / OPT_VALUE_LOSS_COEF / OPT_ENTROPY_COEF / OPT_MAX_GRAD_NORM: the
        hyper-parameters of the next train() calls (None: leave as it is).  Each is rounded to float32 and passed as its
        bits; clip_param, value_clip_range and max_grad_norm must be finite and > 0, the coefficients finite and >= 0.
        Under data parallelism every rank sets the same values."""
        given = dict(clip_param=clip_param, value_clip_range=value_clip_range, value_loss_coef=value_loss_coef,
                     entropy_coef=entropy_coef, max_grad_norm=max_grad_norm)
        for name, x in given.items():
            if x is not None:
                self.set_option(HYPER_OPTIONS[name], float_bits(x))

    def hyper(self):
        """the five current float32 values: {clip_param, value_clip_range, value_loss_coef, entropy_coef,
        max_grad_norm} (the config's until set; value_clip_range follows clip_param until set itself)"""
        return {name: bits_float(self.get_option(opt)) for name, opt in HYPER_OPTIONS.items()}

    def set_regularization(self, weight_decay=None, anchor_coef=None):
        """OPT_WEIGHT_DECAY / OPT_ANCHOR_COEF: decoupled weight decay (torch.optim.AdamW's weight_decay) and the strength of
        the pull toward the anchor (L2 Init) of the next train() calls (None: leave as it is).  Each is rounded to float32
        and passed as its bits; both must be finite and >= 0.  anchor_coef > 0 needs an anchor (anchor_take / load_anchor)
        before train().  Under data parallelism every rank sets the same values and the same anchor."""
        given = dict(weight_decay=weight_decay, anchor_coef=anchor_coef)
        for name, x in given.items():
            if x is not None:
                self.set_option(REG_OPTIONS[name], float_bits(x))

    def regularization(self):
        """the two current float32 values: {weight_decay, anchor_coef} (0.0 until set)"""
        return {name: bits_float(self.get_option(opt)) for name, opt in REG_OPTIONS.items()}

    def anchor_take(self, source="live"):
        """aleppo_anchor_take: anchor = the "live", "averaged" or "snapshot" parameters, by a device copy (enqueued only)"""
        self._c(lib().aleppo_anchor_take(self._ctx, C.c_int(self._set(source))))
        self._anchor_on = True

    def load_anchor(self, flat):
        """aleppo_anchor_import: flat float32 parameters in libtorch parameters() order -> the anchor"""
        flat = _f32(flat).ravel()
        self._c(lib().aleppo_anchor_import(self._ctx, _ptr(flat), C.c_size_t(flat.size)))
        self._anchor_on = True

    def anchor_params(self):
        """aleppo_anchor_export: the anchor as flat float32 in libtorch parameters() order"""
        out = np.zeros(self.param_count, np.float32)
        self._c(lib().aleppo_anchor_export(self._ctx, _ptr(out), C.c_size_t(out.size)))
        return out

    def shrink_perturb(self, shrink, sigma, key=0, reset_moments=False):
        """aleppo_shrink_perturb: every parameter p becomes shrink * p + sigma * xi, xi a fresh He-uniform draw from `key`
        (recycle_units' draw; 0 for a bias), in place on the device; reset_moments zeroes both Adam moments."""
        self._c(lib().aleppo_shrink_perturb(self._ctx, C.c_double(shrink), C.c_double(sigma), C.c_uint64(key),
                                            C.c_int(SP_RESET_MOMENTS if reset_moments else 0)))

    def sample_order(self, epochs):
        """aleppo_read_sample_order: int32 [epochs, N], row e = the logical samples of epoch e in minibatch order
        (identity rows after a contiguous update)."""
        out = np.zeros((epochs, self._batch_n), np.int32)
        self._c(lib().aleppo_read_sample_order(self._ctx, _ptr(out), C.c_size_t(out.size)))
        return out

    def set_batch(self, observations, actions, log_probabilities, advantages, returns, masks, values=None):
        """values: the values the batch was collected with (aleppo_set_batch_values), for OPT_VALUE_CLIP"""
        obs = _u8(observations)
        self._c(lib().aleppo_set_batch(self._ctx, _ptr(obs), _ptr(_i64(actions)), _ptr(_f32(log_probabilities)),
                                       _ptr(_f32(advantages)), _ptr(_f32(returns)), _ptr(_u8(masks)),
                                       C.c_int64(obs.shape[0])))
        self._batch_n = obs.shape[0]
        if values is not None:
            self.set_batch_values(values)

    def set_batch_values(self, values, n=None):
        """aleppo_set_batch_values: float [n] old values of the batch of the last set_batch (n defaults to its size)"""
        v = _f32(values).ravel()
        self._c(lib().aleppo_set_batch_values(self._ctx, _ptr(v), C.c_int64(v.size if n is None else n)))

    def forward(self, observations):
        obs = _u8(observations)
        n = obs.shape[0]
        logits = np.zeros((n, self.A), np.float32)
        values = np.zeros(n, np.float32)
        self._c(lib().aleppo_forward(self._ctx, _ptr(obs), C.c_int64(n), _ptr(logits), _ptr(values)))
        return logits, values

    def forward_activations(self, observations, layers=ACT_LAYERS):
        """aleppo_forward_activations: {layer: float32 array} of the hidden activations of a forward pass on uint8
        [n,4,84,84] observations, in the reference's tensor order - conv1 [n,32,20,20], conv2 [n,64,9,9], conv3 [n,64,7,7]
        (after the ReLU), fc [n,H] (no ReLU: signed).  Only the layers asked for are converted and copied."""
        obs = _u8(observations)
        n = obs.shape[0]
        layers = tuple(layers)
        if not layers or any(l not in ACT_LAYERS for l in layers):
            raise AleppoInvalidArgument(f"layers must be a non-empty subset of {ACT_LAYERS}")
        out = {l: np.zeros((n,) + (ACT_LAYER_SHAPES[l] if l != "fc" else (self.H,)), np.float32) for l in layers}
        self._c(lib().aleppo_forward_activations(self._ctx, _ptr(obs), C.c_int64(n),
                                                 *[_ptr(out.get(l)) for l in ACT_LAYERS]))
        return out

    def export_backward(self, tensors=tuple(BWD_TENSORS), capacity=None):
        """aleppo_export_backward: ({name: float32 array}, B, stored) of what the last minibatch of the last train() left -
        the activations conv1 / conv2 / conv3 / fc and the stored gradients dfc [B,H], dconv3, dconv2, dconv1 (the shapes of
        their activations), B samples each; stored: the BWD_TENSORS bits of what the route kept in memory.  A tensor that was
        asked for and not stored (dconv1 on the fused backward tail) is left out of the dict.  capacity: the samples to make
        room for (default: the minibatch of the last train())."""
        tensors = tuple(tensors)
        if any(t not in BWD_TENSORS for t in tensors):
            raise AleppoInvalidArgument(f"tensors must be a subset of {tuple(BWD_TENSORS)}")
        cap = int(capacity) if capacity is not None else self._last_B
        shape = lambda t: ACT_LAYER_SHAPES[BWD_SHAPE_OF[t]] if BWD_SHAPE_OF[t] != "fc" else (self.H,)
        out = {t: np.zeros((max(cap, 0),) + shape(t), np.float32) for t in tensors}
        n, stored = C.c_int64(0), C.c_uint32(0)
        self._c(lib().aleppo_export_backward(self._ctx, C.c_int64(cap), *[_ptr(out.get(t)) for t in BWD_TENSORS],
                                             C.byref(n), C.byref(stored)))
        return ({t: a[:n.value] for t, a in out.items() if stored.value & BWD_TENSORS[t]}, int(n.value),
                int(stored.value))

    def export_acting(self, tensors=tuple(ACTING_TENSORS), capacity=None):
        """aleppo_export_acting: ({name: float32 array}, n, stored) of what the rollout's last acting forward left - conv1
        [n,32,20,20] and conv2 [n,64,9,9] where the route stored them (OPT_ACT_STORE on the fused bf16 launch), conv3
        [n,64,7,7] and fc_parts [FC_SPLITS,n,H], the fc layer's split-K slices; stored: the ACTING_TENSORS bits.  A tensor
        that was asked for and not stored is left out of the dict.  capacity: the samples to make room for (default E)."""
        tensors = tuple(tensors)
        if any(t not in ACTING_TENSORS for t in tensors):
            raise AleppoInvalidArgument(f"tensors must be a subset of {tuple(ACTING_TENSORS)}")
        cap = int(capacity) if capacity is not None else self.E
        room = max(cap, 0)
        out = {t: np.zeros((FC_SPLITS, room, self.H) if t == "fc_parts" else (room,) + ACT_LAYER_SHAPES[t], np.float32)
               for t in tensors}
        n, stored = C.c_int64(0), C.c_uint32(0)
        self._c(lib().aleppo_export_acting(self._ctx, C.c_int64(cap), *[_ptr(out.get(t)) for t in ACTING_TENSORS],
                                           C.byref(n), C.byref(stored)))
        m = int(n.value)
        if "fc_parts" in out:  # (packed with n, at the front of its room)
            out["fc_parts"] = out["fc_parts"].ravel()[:FC_SPLITS * m * self.H].reshape(FC_SPLITS, m, self.H)
        return ({t: (a if t == "fc_parts" else a[:m]) for t, a in out.items() if stored.value & ACTING_TENSORS[t]}, m,
                int(stored.value))

    def activation_stats(self, observations=None, tau=0.025, raw=False):
        """aleppo_activation_stats: per-unit and per-layer activation statistics reduced on the device - of the batch the
        context holds (observations=None: what train() would train on now) or of uint8 [n,4,84,84] observations.
        {"units": {layer: {stat: float64 [units]}}, "layers": {layer: {stat: float}}} over ACT_LAYERS (+ "total") and
        ACT_UNIT_STATS / ACT_LAYER_STATS; raw=True: the float64 [160 + H, 5] and [5, 8] arrays.  tau: the dormancy
        threshold of the "dormant" count."""
        obs = None if observations is None else _u8(observations)
        n = 0 if obs is None else obs.shape[0]
        units = np.zeros((160 + self.H, ACT_UNIT_COLS), np.float64)
        layers = np.zeros((len(ACT_LAYER_ROWS), ACT_LAYER_COLS), np.float64)
        self._c(lib().aleppo_activation_stats(self._ctx, _ptr(obs), C.c_int64(n), C.c_double(tau), _ptr(units),
                                              C.c_size_t(units.size), _ptr(layers), C.c_size_t(layers.size)))
        if raw:
            return units, layers
        first = (0, 32, 96, 160, 160 + self.H)
        return dict(units={l: {s: units[first[k]:first[k + 1], i].copy() for s, i in ACT_UNIT_STATS.items()}
                           for k, l in enumerate(ACT_LAYERS)},
                    layers={l: {s: float(layers[k, i]) for s, i in ACT_LAYER_STATS.items()}
                            for k, l in enumerate(ACT_LAYER_ROWS)})

    @staticmethod
    def _recycle_layer_bits(layers):
        if isinstance(layers, (int, np.integer)):
            return int(layers)
        names = (layers,) if isinstance(layers, str) else tuple(layers)
        if not names or any(l not in RECYCLE_LAYERS for l in names):
            raise AleppoInvalidArgument(f"layers must be 'all' or a non-empty subset of {ACT_LAYERS}")
        bits = 0
        for l in names:
            bits |= RECYCLE_LAYERS[l]
        return bits

    def recycle_units(self, mask, key=0, keep_moments=False):
        """aleppo_recycle_units: recycle (ReDo) the units of a uint8 / bool [160 + H] mask in the unit order of
        activation_stats - their incoming weights re-initialised from `key`, their outgoing weights zeroed, the Adam
        moments of both reset unless keep_moments.  {layer: masked units} over ACT_LAYERS and "total"."""
        m = _u8(mask).reshape(-1)
        counts = np.zeros(RECYCLE_COUNTS, np.int64)
        self._c(lib().aleppo_recycle_units(self._ctx, _ptr(m), C.c_size_t(m.size), C.c_uint64(key),
                                           C.c_int(RECYCLE_KEEP_MOMENTS if keep_moments else 0), _ptr(counts)))
        return {l: int(counts[k]) for k, l in enumerate(ACT_LAYER_ROWS)}

    def recycle_dormant(self, observations=None, tau=0.025, layers="all", key=0, keep_moments=False):
        """aleppo_recycle_dormant: score the units as activation_stats does (observations=None: the batch the context
        holds), recycle those of `layers` ("all", a layer name, a list of names, or RECYCLE_* bits) whose score is <= tau,
        without the scores leaving the device.  (mask uint8 [160 + H], {layer: recycled units})."""
        obs = None if observations is None else _u8(observations)
        n = 0 if obs is None else obs.shape[0]
        mask = np.zeros(160 + self.H, np.uint8)
        counts = np.zeros(RECYCLE_COUNTS, np.int64)
        self._c(lib().aleppo_recycle_dormant(self._ctx, _ptr(obs), C.c_int64(n), C.c_double(tau),
                                             C.c_int(self._recycle_layer_bits(layers)), C.c_uint64(key),
                                             C.c_int(RECYCLE_KEEP_MOMENTS if keep_moments else 0), _ptr(mask),
                                             C.c_size_t(mask.size), _ptr(counts)))
        return mask, {l: int(counts[k]) for k, l in enumerate(ACT_LAYER_ROWS)}

    def feature_rank(self, observations=None, delta=0.01, eps=0.01, centered=False, spectrum=False, gram=False):
        """aleppo_feature_rank: the rank measures of the fc features from a Gram matrix formed on the device - of the batch
        the context holds (observations=None) or of uint8 [n,4,84,84] observations.  {"stats": {name: float} over FR_STATS,
        "sigma": float64 [H] (descending) with spectrum=True, "gram": float64 [H,H] and "colsum": float64 [H] with
        gram=True; None otherwise}.  centered: the spectrum of the centred features (PCA); "gram" is never centred."""
        obs = None if observations is None else _u8(observations)
        n = 0 if obs is None else obs.shape[0]
        cfg = FeatureRankConfig(delta, eps, int(centered), 0)
        stats = np.zeros(FR_COUNT, np.float64)
        sg = np.zeros(self.H, np.float64) if spectrum else None
        g = np.zeros((self.H, self.H), np.float64) if gram else None
        cs = np.zeros(self.H, np.float64) if gram else None
        self._c(lib().aleppo_feature_rank(self._ctx, _ptr(obs), C.c_int64(n), C.byref(cfg), _ptr(stats),
                                          C.c_size_t(stats.size), _ptr(sg), C.c_size_t(0 if sg is None else sg.size),
                                          _ptr(g), C.c_size_t(0 if g is None else g.size), _ptr(cs),
                                          C.c_size_t(0 if cs is None else cs.size)))
        return dict(stats={k: float(stats[i]) for k, i in FR_STATS.items()}, sigma=sg, gram=g, colsum=cs)

    @staticmethod
    def _set(name):
        if isinstance(name, (int, np.integer)):
            return int(name)
        if name not in SETS:
            raise AleppoInvalidArgument(f"a parameter set is one of {tuple(SETS)}")
        return SETS[name]

    def snapshot_take(self, source="live"):
        """aleppo_snapshot_take: snapshot = the "live" or the "averaged" parameters, by device copies (enqueued only)"""
        self._c(lib().aleppo_snapshot_take(self._ctx, C.c_int(self._set(source))))

    def snapshot_params(self):
        """aleppo_snapshot_export: the snapshot as flat float32 in libtorch parameters() order"""
        out = np.zeros(self.param_count, np.float32)
        self._c(lib().aleppo_snapshot_export(self._ctx, _ptr(out), C.c_size_t(out.size)))
        return out

    def load_snapshot(self, flat):
        """aleppo_snapshot_import: flat float32 parameters (a checkpoint, export_params of another run) -> the snapshot"""
        flat = _f32(flat).ravel()
        self._c(lib().aleppo_snapshot_import(self._ctx, _ptr(flat), C.c_size_t(flat.size)))

    def policy_diff(self, a="snapshot", b="live", observations=None, per_sample=False, transitions=False,
                    outputs=False):
        """aleppo_policy_diff: how far parameter set b's policy, value and fc features are from set a's ("live",
        "averaged", "snapshot") - on the batch the context holds (observations=None) or on uint8 [n,4,84,84]
        observations; both forward passes and the comparison run on the device.  {"stats": {name: float} over PD_STATS,
        "per_sample": float64 [rows, PD_ROW] (columns PD_COLUMNS; a left-out row is NaN) with per_sample=True,
        "transitions": int64 [A, A] ([i, j]: rows whose greedy action went from i to j) with transitions=True,
        "outputs": float32 [2, rows, A + 1] (logits then value, set a first) with outputs=True; None otherwise}."""
        obs = None if observations is None else _u8(observations)
        n = 0 if obs is None else obs.shape[0]
        rows = self._batch_n if obs is None else n
        stats = np.zeros(PD_COUNT, np.float64)
        ps = np.zeros((rows, PD_ROW), np.float64) if per_sample else None
        tr = np.zeros((self.A, self.A), np.int64) if transitions else None
        out = np.zeros((2, rows, self.A + 1), np.float32) if outputs else None
        self._c(lib().aleppo_policy_diff(self._ctx, _ptr(obs), C.c_int64(n), C.c_int(self._set(a)), C.c_int(self._set(b)),
                                         _ptr(stats), C.c_size_t(stats.size), _ptr(ps),
                                         C.c_size_t(0 if ps is None else ps.size), _ptr(tr),
                                         C.c_size_t(0 if tr is None else tr.size), _ptr(out),
                                         C.c_size_t(0 if out is None else out.size)))
        return dict(stats={k: float(stats[i]) for k, i in PD_STATS.items()}, per_sample=ps, transitions=tr, outputs=out)

    # -- gradient probes --
    def grad_probe(self, slot, first=0, n=None, policy=True, value_loss_coef=None, entropy_coef=None):
        """aleppo_grad_probe: gradient slot `slot` = the gradient train() would hand the optimizer for the minibatch of
        samples [first, first + n) of the batch (n=None: to its end), at the live parameters, without a step.  With
        policy=True and both coefficients None the loss is the one train() uses as the options stand (cfg = NULL); else
        policy switches the policy term, and a coefficient left None is the current option's.  Returns the slice's
        unmasked count.  Never a collective: this rank's slice."""
        n = self._batch_n - first if n is None else n
        cfg = None
        if not policy or value_loss_coef is not None or entropy_coef is not None:
            hyper = self.hyper()
            cfg = GradProbeConfig(1 if policy else 0,
                                  hyper["value_loss_coef"] if value_loss_coef is None else value_loss_coef,
                                  hyper["entropy_coef"] if entropy_coef is None else entropy_coef, 0)
        count = C.c_int64()
        self._c(lib().aleppo_grad_probe(self._ctx, C.c_int(slot), C.c_int64(first), C.c_int64(n),
                                        None if cfg is None else C.byref(cfg), C.byref(count)))
        return int(count.value)

    def grad_take(self, slot, source="exp_avg", set="snapshot"):
        """aleppo_grad_take: slot = Adam's first moment as it stands ("exp_avg"), or float32(live - set) per element
        ("delta", set "snapshot" or "averaged"); enqueued only"""
        if source not in GRAD_SOURCES:
            raise AleppoInvalidArgument(f"a gradient source is one of {tuple(GRAD_SOURCES)}")
        which = self._set(set) if source == "delta" else 0
        self._c(lib().aleppo_grad_take(self._ctx, C.c_int(slot), C.c_int(GRAD_SOURCES[source]), C.c_int(which)))

    def grad_vector(self, slot):
        """aleppo_grad_export: the slot as flat float32 in libtorch parameters() order"""
        out = np.zeros(self.param_count, np.float32)
        self._c(lib().aleppo_grad_export(self._ctx, C.c_int(slot), _ptr(out), C.c_size_t(out.size)))
        return out

    def load_grad(self, slot, flat):
        """aleppo_grad_import: a flat float32 vector in libtorch parameters() order -> the slot"""
        flat = _f32(flat).ravel()
        self._c(lib().aleppo_grad_import(self._ctx, C.c_int(slot), _ptr(flat), C.c_size_t(flat.size)))

    def grad_gram(self, slots, raw=False):
        """aleppo_grad_gram: the inner products of the k = len(slots) named slots per tensor, reduced on the device in
        double.  {tensor: float64 [k, k]} over GRAM_NAMES (the 12 tensors, then "all"), plus "nonfinite": {tensor: int},
        the element indices left out because one of the slots is NaN / Inf there; raw=True: (float64 [13, k, k],
        int64 [13])."""
        idx = np.ascontiguousarray(slots, dtype=np.int32).ravel()
        k = int(idx.size)
        gram = np.zeros((TENSOR_STATS_ROWS, k, k), np.float64)
        nf = np.zeros(TENSOR_STATS_ROWS, np.int64)
        self._c(lib().aleppo_grad_gram(self._ctx, _ptr(idx), C.c_int(k), _ptr(gram), C.c_size_t(gram.size), _ptr(nf),
                                       C.c_size_t(nf.size)))
        if raw:
            return gram, nf
        out = {t: gram[r] for r, t in enumerate(GRAM_NAMES)}
        out["nonfinite"] = {t: int(nf[r]) for r, t in enumerate(GRAM_NAMES)}
        return out

    @staticmethod
    def _gram_rows(gram):
        """(names, float64 [rows, k, k]) of what grad_gram returned in either form"""
        if isinstance(gram, dict):
            names = [t for t in gram if t != "nonfinite"]
            return names, np.stack([np.asarray(gram[t], np.float64) for t in names])
        g = np.asarray(gram[0] if isinstance(gram, tuple) else gram, np.float64)
        return list(GRAM_NAMES[:g.shape[0]]), g

    @staticmethod
    def grad_cosines(gram):
        """per tensor G_ij / sqrt(G_ii G_jj) of a Gram (grad_gram's dict, or a float64 [rows, k, k] array); NaN where a
        norm is 0.  Host arithmetic only.  The same form as the argument."""
        names, g = Engine._gram_rows(gram)
        d = np.einsum("rii->ri", g)
        den = np.sqrt(d[:, :, None] * d[:, None, :])
        with np.errstate(divide="ignore", invalid="ignore"):
            cos = np.where(den > 0, g / den, np.nan)
        return {t: cos[r] for r, t in enumerate(names)} if isinstance(gram, dict) else cos

    @staticmethod
    def noise_scale_from_gram(gram, b_small, b_big):
        """McCandlish et al. 2018, Appendix A, per tensor from the Gram of (g_small, g_big), the gradients of nested slices
        with b_small < b_big unmasked samples: |G|^2 = (b_big |g_big|^2 - b_small |g_small|^2) / (b_big - b_small),
        S = (|g_small|^2 - |g_big|^2) / (1 / b_small - 1 / b_big), B_simple = S / |G|^2.  {"g2", "s", "b_simple"}, each
        in the form of the argument.  Host arithmetic only."""
        if not 0 < b_small < b_big:
            raise AleppoInvalidArgument("the noise scale needs 0 < b_small < b_big unmasked samples")
        names, g = Engine._gram_rows(gram)
        small, big = g[:, 0, 0], g[:, 1, 1]
        g2 = (b_big * big - b_small * small) / (b_big - b_small)
        s = (small - big) / (1.0 / b_small - 1.0 / b_big)
        with np.errstate(divide="ignore", invalid="ignore"):
            res = dict(g2=g2, s=s, b_simple=s / g2)
        if isinstance(gram, dict):
            return {k: {t: float(v[r]) for r, t in enumerate(names)} for k, v in res.items()}
        return res

    @staticmethod
    def interference_from_gram(gram):
        """from the Gram of the three pure probes (policy, value, entropy): their per-tensor norms and the three pairwise
        cosines.  {"norms": {term: ...}, "cosines": {"policy_value", "policy_entropy", "value_entropy"}}, each entry in
        the form of the argument.  Host arithmetic only."""
        names, g = Engine._gram_rows(gram)
        cos = Engine.grad_cosines(g)
        form = (lambda v: {t: float(v[r]) for r, t in enumerate(names)}) if isinstance(gram, dict) else (lambda v: v)
        return dict(norms={t: form(np.sqrt(g[:, i, i])) for i, t in enumerate(("policy", "value", "entropy"))},
                    cosines=dict(policy_value=form(cos[:, 0, 1]), policy_entropy=form(cos[:, 0, 2]),
                                 value_entropy=form(cos[:, 1, 2])))

    def gradient_noise_scale(self, n_small, n_big, first=0, slots=(0, 1)):
        """two probes (the loss as the options stand) on the nested slices [first, first + n_small) and [first, first +
        n_big) into `slots`, then noise_scale_from_gram with their unmasked counts as the batch sizes: {"g2", "s",
        "b_simple"} per tensor and for "all", plus "counts"."""
        b_small = self.grad_probe(slots[0], first, n_small)
        b_big = self.grad_probe(slots[1], first, n_big)
        res = self.noise_scale_from_gram(self.grad_gram(slots), b_small, b_big)
        res["counts"] = (b_small, b_big)
        return res

    def gradient_interference(self, first=0, n=None, slots=(0, 1, 2)):
        """three probes on samples [first, first + n) into `slots` - the policy term alone {1, 0, 0}, the value term alone
        {0, 1, 0}, the entropy term alone {0, 0, 1} - then interference_from_gram: the per-tensor norms and the three
        pairwise cosines (policy_value < 0 in the trunk: the critic pulls against the actor there)."""
        self.grad_probe(slots[0], first, n, policy=True, value_loss_coef=0.0, entropy_coef=0.0)
        self.grad_probe(slots[1], first, n, policy=False, value_loss_coef=1.0, entropy_coef=0.0)
        self.grad_probe(slots[2], first, n, policy=False, value_loss_coef=0.0, entropy_coef=1.0)
        return self.interference_from_gram(self.grad_gram(slots))

    def refresh_advantages(self, source="live", stats=True):
        """aleppo_refresh_advantages: between two train() calls on one rollout batch, forward the batch and the post-rollout
        observation under parameter set `source` ("live", "averaged", "snapshot") on the device, keep the values in a
        second plane (refresh_values) and overwrite advantages / returns with a new GAE scan on them (with the
        normalisation of finish_rollout under advantage_norm: then a collective with a communicator).  {name: float} over
        REFRESH_STATS with stats=True - the BATCH_STATS layout with the fresh values against the returns and advantages as
        they stood at entry, then mean / std / max-abs of v_fresh - v_collected (this rank's samples) - else None."""
        st = np.zeros(REFRESH_STATS_COUNT, np.float64) if stats else None
        self._c(lib().aleppo_refresh_advantages(self._ctx, C.c_int(self._set(source)), _ptr(st),
                                                C.c_size_t(0 if st is None else st.size)))
        return None if st is None else {name: float(st[i]) for name, i in REFRESH_STATS.items()}

    def refresh_values(self):
        """aleppo_refresh_read: (values float32 [E,T], next_values float32 [E]) of the last refresh_advantages, as stored
        (rounded to half with ROLLOUT_FP16)"""
        v = np.zeros((self.E, self.T), np.float32)
        nv = np.zeros(self.E, np.float32)
        self._c(lib().aleppo_refresh_read(self._ctx, _ptr(v), C.c_size_t(v.size), _ptr(nv), C.c_size_t(nv.size)))
        return v, nv

    def _saliency_source(self, observations, first, n):
        obs = None if observations is None else _u8(observations)
        if obs is not None:
            n = obs.shape[0] if n is None else n
        elif n is None:
            n = self._batch_n - first
        return obs, int(first), int(n)

    def saliency(self, observations=None, first=0, n=None, stride=SALIENCY_STRIDE, sigma_mask=SALIENCY_SIGMA_MASK,
                 sigma_blur=SALIENCY_SIGMA_BLUR, planes=SALIENCY_PLANES, outputs=False):
        """aleppo_saliency: perturbation saliency (Greydanus et al. 2018) of uint8 [n,4,84,84] observations, or
        (observations=None) of samples [first, first + n) of the batch the context holds, in read_batch's env-major order.
        {"policy": float32 [n,G,G], "value": float32 [n,G,G]} with G = saliency_grid(stride): 0.5 |z - z'|^2 of the logits
        and 0.5 (v - v')^2 of the value under a local blur around grid point (gy, gx) = pixel (gy * stride, gx * stride).
        outputs=True adds "outputs", float32 [n, G*G + 1, A + 1]: row 0 the unperturbed logits and value, row 1 + p those
        of position p = gy * G + gx."""
        obs, first, n = self._saliency_source(observations, first, n)
        G = saliency_grid(stride) if 1 <= stride <= 84 else 1  # (a bad stride is the library's to refuse)
        res = dict(policy=np.zeros((max(n, 0), G, G), np.float32), value=np.zeros((max(n, 0), G, G), np.float32))
        if outputs:
            res["outputs"] = np.zeros((max(n, 0), G * G + 1, self.A + 1), np.float32)
        cfg = SaliencyConfig(stride, planes, sigma_mask, sigma_blur)
        self._c(lib().aleppo_saliency(self._ctx, _ptr(obs), C.c_int64(first), C.c_int64(n), C.byref(cfg),
                                      _ptr(res["policy"]), _ptr(res["value"]), _ptr(res.get("outputs"))))
        return res

    def saliency_perturbed(self, observations=None, first=0, n=None, stride=SALIENCY_STRIDE,
                           sigma_mask=SALIENCY_SIGMA_MASK, sigma_blur=SALIENCY_SIGMA_BLUR, planes=SALIENCY_PLANES,
                           position_first=0, position_count=None):
        """aleppo_saliency_perturbed: uint8 [n, position_count, 4, 84, 84], the perturbed stacks saliency() forwards for the
        positions [position_first, position_first + position_count) of each sample (default: to the end of the grid)."""
        obs, first, n = self._saliency_source(observations, first, n)
        G = saliency_grid(stride) if 1 <= stride <= 84 else 1
        count = G * G - position_first if position_count is None else position_count
        out = np.zeros((max(n, 0), max(count, 0), 4, 84, 84), np.uint8)
        cfg = SaliencyConfig(stride, planes, sigma_mask, sigma_blur)
        self._c(lib().aleppo_saliency_perturbed(self._ctx, _ptr(obs), C.c_int64(first), C.c_int64(n), C.byref(cfg),
                                                C.c_int64(position_first), C.c_int64(count), _ptr(out)))
        return out

    def read_batch(self, name):
        E, T, A = self.E, self.T, self.A
        shapes = dict(observations=((E, T, 4, 84, 84), np.uint8), actions=((E, T), np.int64),
                      rewards=((E, T), np.float32), masks=((E, T), np.uint8), logits=((E, T, A), np.float32),
                      values=((E, T), np.float32), advantages=((E, T), np.float32), returns=((E, T), np.float32),
                      log_probs=((E, T, A), np.float32), terminals=((E, T), np.uint8),
                      truncations=((E, T), np.uint8), current_obs=((E, 4, 84, 84), np.uint8),
                      next_values=((E,), np.float32), batch_stats=((BATCH_STATS_COUNT,), np.float64),
                      reward_scale=((REWARD_SCALE_COUNT,), np.float64))
        shp, dt = shapes[name]
        out = np.zeros(shp, dt)
        self._c(lib().aleppo_read_batch(self._ctx, FIELDS[name], _ptr(out), C.c_size_t(out.nbytes)))
        return out

    def batch_stats(self):
        """ALEPPO_F_BATCH_STATS: dict of ten floats (count, explained_variance, value / return / advantage / residual mean
        and std) over the unmasked samples of the batch the context holds, reduced on the device when called; a
        collective with a communicator (aleppo.h)"""
        a = self.read_batch("batch_stats")
        return {name: float(a[i]) for name, i in BATCH_STATS.items()}

    # -- evaluation lanes --
    def eval_open(self, lanes):
        """aleppo_eval_open: `lanes` frame stacks of their own (1..4096) with their own scratch and action buffer; again
        with the same count: zero stacks, the built-in noise stream from its start"""
        self._c(lib().aleppo_eval_open(self._ctx, C.c_int32(int(lanes))))
        self.eval_lanes = int(lanes)

    def eval_push_frames(self, frames, episode_start, kind=FRAMES_84, device_ptr=None):
        """aleppo_eval_push_frames: push_frames for the evaluation lanes"""
        st = _u8(episode_start)
        if device_ptr is not None:
            self._c(lib().aleppo_eval_push_frames(self._ctx, C.c_void_p(device_ptr), kind, DEVICE, _ptr(st)))
        else:
            self._c(lib().aleppo_eval_push_frames(self._ctx, _ptr(_u8(frames)), kind, HOST, _ptr(st)))

    def eval_act(self, rule="greedy", temperature=1.0, epsilon=0.0, noise=None):
        """aleppo_eval_act: int64 [L] actions (a view of the lanes' pinned buffer, valid until the next eval_act) under
        rule "greedy", "sample" (temperature; noise: Exp(1) draws [L, A]) or "epsilon" (epsilon; noise: uniforms (u, w)
        [L, 2]); noise None: the built-in generator"""
        r = EVAL_RULES[rule] if isinstance(rule, str) else int(rule)
        param = temperature if r == EVAL_SAMPLE else epsilon if r == EVAL_EPSILON_GREEDY else 0.0
        n = None if noise is None else _f32(noise)
        p = C.POINTER(C.c_int64)()
        self._c(lib().aleppo_eval_act(self._ctx, C.c_int(r), C.c_float(param), _ptr(n), C.byref(p)))
        return np.ctypeslib.as_array(p, shape=(self.eval_lanes,))

    def eval_set_counter(self, counter):
        """aleppo_eval_set_counter: the evaluation counter n of the built-in generator (the next eval_act draws block n)"""
        self._c(lib().aleppo_eval_set_counter(self._ctx, C.c_uint64(int(counter))))

    def eval_read(self, name):
        """aleppo_eval_read: "observations" uint8 [L,4,84,84] (the stacks now), or "logits" float32 [L,A] / "values"
        float32 [L] / "actions" int64 [L] of the last eval_act"""
        L = getattr(self, "eval_lanes", 1)
        shp, dt = dict(observations=((L, 4, 84, 84), np.uint8), logits=((L, self.A), np.float32),
                       values=((L,), np.float32), actions=((L,), np.int64))[name]
        out = np.zeros(shp, dt)
        self._c(lib().aleppo_eval_read(self._ctx, EVAL_FIELDS[name], _ptr(out), C.c_size_t(out.nbytes)))
        return out

    # -- device-resident environments --
    def env_open(self, frame_kind=FRAMES_84, seed_base=0, max_steps=108000, max_return=-1.0, kind=ENV_SYNTHETIC,
                 reserved=0):
        """aleppo_env_open: E synthetic environments in device memory, environment e seeded seed_base + e, rendering
        84x84 frames or raw 2 x 210x160 pairs; again with the same arguments: the environments start over"""
        cfg = EnvConfig(int(kind), int(frame_kind), int(seed_base), int(max_steps), float(max_return), int(reserved))
        self._c(lib().aleppo_env_open(self._ctx, C.byref(cfg)))
        self.env_frame_kind = int(frame_kind)

    def env_rollout(self):
        """aleppo_env_rollout: all T slots - act, environment step and render, ingest - enqueued without a host wait;
        finish_rollout comes next"""
        self._c(lib().aleppo_env_rollout(self._ctx))

    def env_state(self):
        """aleppo_env_export_state: a structured array [E] of ENV_STATE_DTYPE; between rollouts only"""
        st = np.zeros(self.E, ENV_STATE_DTYPE)
        self._c(lib().aleppo_env_export_state(self._ctx, _ptr(st), C.c_size_t(self.E)))
        return st

    def load_env_state(self, state):
        """aleppo_env_import_state: what env_state returned (values a run cannot reach are refused)"""
        st = np.ascontiguousarray(state, dtype=ENV_STATE_DTYPE)
        self._c(lib().aleppo_env_import_state(self._ctx, _ptr(st), C.c_size_t(st.size)))

    def env_read(self, name):
        """aleppo_env_read: "frames" uint8 [E,84,84] / [E,2,210,160] (the frame buffer now); the last env_rollout's
        time-major [T,E] log planes "episode_returns" / "game_returns" float32 and "episode_lengths" / "game_lengths"
        uint32 (0: nothing ended in that slot); "step_ms" float64 [2] (mean ms of the environment kernel, launches
        timed while profile() was on)"""
        E, T = self.E, self.T
        fshape = (E, 2, 210, 160) if getattr(self, "env_frame_kind", FRAMES_84) == FRAMES_RAW_PAIR else (E, 84, 84)
        shp, dt = dict(frames=(fshape, np.uint8), episode_returns=((T, E), np.float32),
                       episode_lengths=((T, E), np.uint32), game_returns=((T, E), np.float32),
                       game_lengths=((T, E), np.uint32), step_ms=((2,), np.float64))[name]
        out = np.zeros(shp, dt)
        self._c(lib().aleppo_env_read(self._ctx, ENV_FIELDS[name], _ptr(out), C.c_size_t(out.nbytes)))
        return out

    def env_episodes(self):
        """the last env_rollout's episode log, compacted in slot-then-environment order: (returns float32, lengths
        uint32, game_returns, game_lengths) of the episodes / games that ended in it"""
        el, gl = self.env_read("episode_lengths").ravel(), self.env_read("game_lengths").ravel()
        return (self.env_read("episode_returns").ravel()[el > 0], el[el > 0],
                self.env_read("game_returns").ravel()[gl > 0], gl[gl > 0])

    # -- device-resident evaluation environments --
    def eval_env_open(self, frame_kind=FRAMES_84, seed_base=0, max_steps=108000, max_return=-1.0, run_steps=64,
                      kind=ENV_SYNTHETIC, reserved=0):
        """aleppo_eval_env_open: one synthetic environment per evaluation lane in device memory, lane l seeded
        seed_base + l; run_steps: the most steps one eval_env_run may take (the rows of the log planes); again with
        another seed_base: the environments start over under the new seeds, the stacks and the counter stay"""
        cfg = EnvConfig(int(kind), int(frame_kind), int(seed_base), int(max_steps), float(max_return), int(reserved))
        self._c(lib().aleppo_eval_env_open(self._ctx, C.byref(cfg), C.c_int32(int(run_steps))))
        self.eval_env_frame_kind, self.eval_env_run_steps = int(frame_kind), int(run_steps)

    def eval_env_run(self, rule="greedy", temperature=1.0, epsilon=0.0, steps=1):
        """aleppo_eval_env_run: `steps` evaluation steps - act, environment step and render, ingest - enqueued without a
        host wait, under eval_act's rules with the built-in generator"""
        r = EVAL_RULES[rule] if isinstance(rule, str) else int(rule)
        param = temperature if r == EVAL_SAMPLE else epsilon if r == EVAL_EPSILON_GREEDY else 0.0
        self._c(lib().aleppo_eval_env_run(self._ctx, C.c_int(r), C.c_float(param), C.c_int32(int(steps))))

    def eval_env_state(self):
        """aleppo_eval_env_export_state: a structured array [L] of ENV_STATE_DTYPE"""
        st = np.zeros(self.eval_lanes, ENV_STATE_DTYPE)
        self._c(lib().aleppo_eval_env_export_state(self._ctx, _ptr(st), C.c_size_t(st.size)))
        return st

    def load_eval_env_state(self, state):
        """aleppo_eval_env_import_state: what eval_env_state returned (values a run cannot reach are refused)"""
        st = np.ascontiguousarray(state, dtype=ENV_STATE_DTYPE)
        self._c(lib().aleppo_eval_env_import_state(self._ctx, _ptr(st), C.c_size_t(st.size)))

    def eval_env_read(self, name):
        """aleppo_eval_env_read: "frames" uint8 [L,84,84] / [L,2,210,160] (the frame buffer now); the last eval_env_run's
        step-major [S,L] log planes "episode_returns" / "game_returns" float32 and "episode_lengths" / "game_lengths"
        uint32 (0: nothing ended in that step; rows past the run's steps are zero)"""
        L, S = getattr(self, "eval_lanes", 1), getattr(self, "eval_env_run_steps", 1)
        raw = getattr(self, "eval_env_frame_kind", FRAMES_84) == FRAMES_RAW_PAIR
        shp, dt = dict(frames=((L, 2, 210, 160) if raw else (L, 84, 84), np.uint8), episode_returns=((S, L), np.float32),
                       episode_lengths=((S, L), np.uint32), game_returns=((S, L), np.float32),
                       game_lengths=((S, L), np.uint32))[name]
        out = np.zeros(shp, dt)
        self._c(lib().aleppo_eval_env_read(self._ctx, EVAL_ENV_FIELDS[name], _ptr(out), C.c_size_t(out.nbytes)))
        return out

    def eval_env_episodes(self):
        """the last eval_env_run's episode log, compacted in step-then-lane order: (returns float32, lengths uint32,
        game_returns, game_lengths) of the episodes / games that ended in it"""
        el, gl = self.eval_env_read("episode_lengths").ravel(), self.eval_env_read("game_lengths").ravel()
        return (self.eval_env_read("episode_returns").ravel()[el > 0], el[el > 0],
                self.eval_env_read("game_returns").ravel()[gl > 0], gl[gl > 0])

    # -- episode recorders --
    def rec_open(self, source="rollout", index=0, frames=True, observation=True, capacity=None):
        """aleppo_rec_open: record environment `index` of env_rollout ("rollout") or lane `index` of eval_env_run ("eval")
        into an append log of `capacity` rows (default: T, or the evaluation environments' run_steps); again with the
        same arguments: an empty log, ordinal 0"""
        src = REC_SOURCES[source] if isinstance(source, str) else int(source)
        if capacity is None:
            capacity = self.T if src == REC_ROLLOUT else getattr(self, "eval_env_run_steps", 1)
        cfg = RecConfig(src, int(index), (REC_FRAMES if frames else 0) | (REC_OBSERVATION if observation else 0),
                        int(capacity))
        self._c(lib().aleppo_rec_open(self._ctx, C.byref(cfg)))

    def rec_count(self, source="rollout"):
        """aleppo_rec_count: dict(rows, dropped, next_ordinal, capacity, frame_bytes, observation_bytes, actions); host
        state, no synchronise"""
        src = REC_SOURCES[source] if isinstance(source, str) else int(source)
        n = RecCounts()
        self._c(lib().aleppo_rec_count(self._ctx, C.c_int(src), C.byref(n)))
        return {k: int(getattr(n, k)) for k, _ in RecCounts._fields_}

    def rec_read(self, source, name, first=0, rows=None):
        """aleppo_rec_read: rows [first, first + rows) (default: to the end of the log) of "steps" (REC_STEP_DTYPE
        [rows]), "logits" (float32 [rows, A]), "frames" (uint8 [rows, 84, 84] or [rows, 2, 210, 160]) or "observations"
        (uint8 [rows, 84, 84])"""
        src = REC_SOURCES[source] if isinstance(source, str) else int(source)
        n = self.rec_count(src)
        if rows is None:
            rows = max(n["rows"] - int(first), 0)
        rows = int(rows)
        if name == "steps":
            out = np.zeros(rows, REC_STEP_DTYPE)
        elif name == "logits":
            out = np.zeros((rows, self.A), np.float32)
        elif name == "frames":
            out = np.zeros((rows, 2, 210, 160) if n["frame_bytes"] == 2 * 210 * 160 else (rows, 84, 84), np.uint8)
        else:
            out = np.zeros((rows, 84, 84), np.uint8)
        buf = out if out.size else np.zeros(1, np.uint8)  # (dst is never null, even for no rows)
        self._c(lib().aleppo_rec_read(self._ctx, C.c_int(src), C.c_int(REC_FIELDS[name]), C.c_uint64(int(first)),
                                      C.c_uint64(rows), _ptr(buf), C.c_size_t(out.nbytes)))
        return out

    def rec_clear(self, source="rollout"):
        """aleppo_rec_clear: rows = dropped = 0; the ordinal stays"""
        src = REC_SOURCES[source] if isinstance(source, str) else int(source)
        self._c(lib().aleppo_rec_clear(self._ctx, C.c_int(src)))

    # -- multi GPU --
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
        _check(lib().aleppo_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id):
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._c(lib().aleppo_comm_init(self._ctx, buf))

    # -- measurement --
    def profile(self, on=True):
        self._c(lib().aleppo_profile_enable(self._ctx, int(on)))

    def profile_reset(self):
        self._c(lib().aleppo_profile_reset(self._ctx))

    def profile_read(self, name):
        ms = C.c_double()
        n = C.c_int64()
        self._c(lib().aleppo_profile_read(self._ctx, KERNEL_CLASSES[name], C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_option(self, option, value):
        """aleppo_set_option: per-context A/B switches (OPT_*)"""
        self._c(lib().aleppo_set_option(self._ctx, int(option), int(value)))

    def get_option(self, option):
        v = C.c_int64()
        self._c(lib().aleppo_get_option(self._ctx, int(option), C.byref(v)))
        return v.value

    def set_generic_conv(self, on):
        """A/B switch: run bf16 convolutions on the generic gather-GEMM kernels (this context only)."""
        self.set_option(OPT_GENERIC_CONV, on)

    def synchronize(self):
        self._c(lib().aleppo_synchronize(self._ctx))


def learning_rate(lr0, rollout_index, num_rollouts):
    """linear anneal of main() (src/bin/train.cc:424-428)"""
    return lr0 * (1.0 - rollout_index / float(num_rollouts))
