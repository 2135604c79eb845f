// common.hpp - internal context, HBM layout and launcher declarations of libaleppo.so.
// Public boundary: include/aleppo.h.  Layout rationale: DESIGN.md.
#pragma once
#include "../../include/aleppo.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

namespace aleppo {

constexpr int FRAME_PIX = 84 * 84;          // 7056 packed pixels per stack (one u32 = 4 frames of one pixel)
constexpr int RAW_H = 210, RAW_W = 160;
constexpr int A1_PIX = 400, A1_C = 32;      // conv1 out 20x20x32 (NHWC)
constexpr int A2_PIX = 81, A2_C = 64;       // conv2 out 9x9x64
constexpr int A3_PIX = 49, A3_C = 64;       // conv3 out 7x7x64
constexpr int FC_IN = 3136;
constexpr int MAX_ACTIONS = 18;
constexpr int FC_SPLITS = 7; // split-K slices of the acting-size fc forward (3136 = 7 * 448)
// split-K slice caps of the wgrad slabs (gemm_launch.hip) and of the head kernel's partial slabs
constexpr int MAXS_C1 = 256, MAXS_C2 = 256, MAXS_C3 = 256, MAXS_FC = 8, MAXS_HEAD = 256;
// floats per reduced per-minibatch metric record (metrics_reduce_kernel): the sums of fields 0-4, the unmasked count,
// the sums of approx-KL and clip fraction, and the sum of the exact KL of ALEPPO_OPT_KL_PENALTY (0 with the option off)
constexpr int METRIC_REC = 9;

// ---- internal flat parameter layout (fp32 master, Adam moments, gradient share it) ----
// order chosen so that what backward finishes FIRST is at the FRONT: bucket 0 = heads + fc can be
// all-reduced while the conv backward still runs.  Every tensor starts 64-float aligned;
// pads are zero and stay zero under Adam.
enum ParamId { P_WH = 0, P_BH, P_WFC, P_BFC, P_W3, P_B3, P_W2, P_B2, P_W1, P_B1, P_COUNT };
struct ParamLayout {
  size_t off[P_COUNT + 1]; // off[P_COUNT] = total (padded)
  size_t size[P_COUNT];
  size_t bucket0_end;      // = off[P_W3]
  int H, A;
  void init(int H_, int A_);
  size_t total() const { return off[P_COUNT]; }
  size_t reference_count() const; // libtorch parameters() element count
};
// reference (libtorch parameters() order, NCHW) <-> internal (NHWC-k order) permutation, on the host
void params_to_internal(const ParamLayout &L, const float *ref, float *internal);
void params_to_reference(const ParamLayout &L, const float *internal, float *ref);
// A stored parameter set next to the live one (P / Pc), in the same layout: the averaged set, the snapshot, the anchor.
// Allocated on first use and written only through the param_set_* helpers of api_internal.hpp.
struct ParamSet {
  float *P = nullptr; // fp32, internal layout, L.total() floats (pads zero)
  void *Pc = nullptr; // compute copy of P in T (same layout); == P for fp32; nullptr for a set that is never forwarded
  bool on = false;    // a take or an import has succeeded
};

// sample n of a batch lives in obs slot  (n / TP) * s1 + (n % TP) * s0 + base   (units: u32 pixels)
// idx != nullptr (ALEPPO_OPT_MINIBATCH_SHUFFLE): logical sample n is first replaced by idx[n].  The kernels that read
// observations come in two instantiations, contiguous (IDX = false: idx is never read) and indexed, chosen by the launcher.
struct SampleMap {
  int TP;
  long s1, s0, base;
  int n0; // first sample of this launch (minibatch offset)
  const int32_t *idx = nullptr; // [n0 + ns] order of the launch's samples, or nullptr: contiguous
};
// u32-pixel offset of the stack of batch sample nn (n0 already added); IDX: nn goes through the order table first
template <bool IDX> __device__ __forceinline__ long sample_off(const SampleMap &m, long nn) {
  if constexpr (IDX)
    nn = m.idx[nn];
  return (nn / m.TP) * m.s1 + (nn % m.TP) * m.s0 + m.base;
}

struct ProfClass {
  std::vector<hipEvent_t> start, stop;
  size_t used = 0;
};

struct Hyper {
  float clip, c_v, c_e, max_norm;
};
// The kernels read them, and the value-clip range, from a DEVICE block (ALEPPO_OPT_CLIP_PARAM, ALEPPO_OPT_VALUE_CLIP_RANGE,
// ALEPPO_OPT_VALUE_LOSS_COEF, ALEPPO_OPT_ENTROPY_COEF, ALEPPO_OPT_MAX_GRAD_NORM): float [HYPER_BLOCK], 16-byte aligned,
// uploaded in front of every update, so that a captured update follows values changed between calls.  The head kernels
// read slots 0-3 as one 16-byte load, the Adam kernel slot 4.  Slots 5-6: f_wd = (float)(lr * weight decay) and f_an =
// (float)(lr * anchor coefficient) of the call (ALEPPO_OPT_WEIGHT_DECAY, ALEPPO_OPT_ANCHOR_COEF), which reg_step_kernel
// alone reads.
enum { HYPER_CLIP = 0, HYPER_VCLIP = 1, HYPER_CV = 2, HYPER_CE = 3, HYPER_MAX_NORM = 4, HYPER_WD = 5, HYPER_ANCHOR = 6,
       HYPER_BLOCK = 8 };

// Kernel-selection switches of ONE context (aleppo_set_option; initial values from the environment, read once in
// aleppo_create).  The launch helpers read them through tuning(): a thread-local pointer that every stateful entry
// point aims at its context first - the switches are per context, not per process.
struct Tuning {
  bool patch_conv = true;     // sample-stationary bf16 conv kernels (false: generic gather-GEMMs)
  bool fc_pipe = true;        // pipelined LDS-DMA fc GEMMs at minibatch sizes > 256
  bool fused_fwd = true;      // the update's conv1 -> conv2 -> conv3 forward as one launch (conv_fwd_fused.hpp)
  int fused_bwd = 1;          // conv2 dgrad + conv2 wgrad + conv1 wgrad as one launch (conv_bwd_fused.hpp): 0 never, 1 at
                              // minibatches >= 2048 samples (below, its fixed costs outweigh the bytes: v1.yaml's 1280), 2 always
  int fused_act = 1;          // frame ingest fused in front of the acting convolutions: 0 never, 1 where faster, 2 always
};
const Tuning &tuning();
void set_tuning(const Tuning *t); // nullptr -> process defaults
Tuning tuning_from_env();

struct Ctx {
  aleppo_config cfg{};
  int E = 0, T = 0, A = 0, H = 0, prec = 0, world = 1, rank = 0;
  long N = 0;          // E*T samples per rollout on this rank
  long maxB = 0;       // activation capacity in samples
  long batch_n = 0;    // samples currently in the training arrays
  ParamLayout L;
  std::string err;
  hipStream_t stream = nullptr, comm_stream = nullptr, wg_stream = nullptr;
  hipEvent_t ev_bucket0 = nullptr, ev_comm0 = nullptr, ev_tmp = nullptr;
  hipEvent_t ev_head = nullptr, ev_dz3 = nullptr, ev_dz2 = nullptr, ev_wg = nullptr; // dgrad chain -> wgrad side stream
  void *nccl_comm = nullptr;

  // ---- rollout storage (time-major scalars, env-major packed observation slots) ----
  uint32_t *obs = nullptr;     // [E][T+1][7056] packed stacks; slot T = bootstrap observation
  uint8_t *step_rec = nullptr; // [T] records of { float r[E]; u8 term[E]; u8 trunc[E]; u8 start[E] }
  size_t step_rec_bytes = 0;
  // float planes of the rollout buffer are stored as RT = float or IEEE half (cfg.rollout_precision): rt16 / rsz
  bool rt16 = false;
  size_t rsz = 4;              // bytes per stored plane element
  void *values_tm = nullptr;   // RT [T+1][E]
  void *logits_tm = nullptr;   // RT [T+1][E][A]
  int *actions_tm = nullptr;   // [T][E]
  uint8_t *lut = nullptr;      // [256]
  uint8_t *d_start = nullptr;  // [E] episode-start flags of the slot being ingested
  uint8_t *d_frames = nullptr; // staging for host frames (max(E*2*210*160))
  float *d_noise = nullptr;    // [2][E][A] (two staging halves: a slot may be enqueued while the previous one is pending)
  int *d_err = nullptr;        // device error word (flag overlap)
  unsigned int *d_done = nullptr; // arrival counter of the head kernel's ticket publish
  long long ticket = 0;        // last ticket published to h_actions[E]
  // pinned, GPU-visible hand-off words of the slot-ahead gate (gate_kernel): [0] release sequence (host writes),
  // [1] time-out report (the gate writes the sequence number it gave up on; 0 = none)
  unsigned long long *h_go = nullptr;
  unsigned long long go_seq = 0; // last sequence number a gate was enqueued for (64 bits: never wraps)
  unsigned long long gate_timeout_ticks = 0; // the gate's exit condition, in 100 MHz wall-clock ticks
  // a failure that leaves the rollout / learner state undefined (a gate that timed out, an update that failed half way):
  // every later stateful call but aleppo_destroy returns this error again
  bool failed = false;
  std::string fail_msg;
  unsigned noise_flip = 0;
  // aleppo_arm_step / aleppo_release_step: a step (and the next slot's acting kernels) enqueued behind the release word
  bool armed = false;
  const uint8_t *armed_start = nullptr; // the caller's mapped episode-start bytes of the armed step
  int act_queued_slot = -1;             // slot whose acting kernels + head are already enqueued (aleppo_act only waits)
  long long act_queued_ticket = 0;
  // pinned host staging
  int64_t *h_actions = nullptr; // [E]
  uint8_t *h_step = nullptr;    // one step record (aleppo_record_step path)
  uint8_t *h_rec = nullptr;     // [T] step records filled by aleppo_step, uploaded once at finish_rollout
  int rec_uploaded = 0;         // slots of h_rec already in device memory
  int rec_direct = 0;           // slots written straight to the device by aleppo_record_step
  uint8_t *h_frames = nullptr;
  float *h_noise = nullptr;
  int *h_err = nullptr;
  int pre_acted = -1;     // slot whose conv stack + split-K fc already ran (fused into aleppo_step); -1: none
  int t = 0;              // next slot to fill
  bool need_carry = false; // copy slot T -> slot 0 before the next rollout's first act
  uint64_t rng_counter = 0;
  // ---- training arrays, env-major n = e*T + t ----
  void *adv_n = nullptr, *ret_n = nullptr, *oldlp_n = nullptr; // RT [N], [N], [N][A]
  int *act_n = nullptr;
  uint8_t *mask_n = nullptr;
  float *mask_counts = nullptr; // [M_max] global unmasked count per minibatch
  // ---- network state ----
  float *P = nullptr, *G = nullptr, *M1 = nullptr, *M2 = nullptr; // fp32, internal layout
  void *Pc = nullptr;   // compute copy of P in T (same layout); == P for fp32
  void *W2d = nullptr, *W3d = nullptr, *WfcT = nullptr; // dgrad-transposed copies in T
  int64_t adam_step = 0;
  // ---- activations (T unless noted) ----
  void *a1 = nullptr, *a2 = nullptr, *a3 = nullptr; // [maxB][400][32], [maxB][81][64], [maxB][49][64]
  float *h = nullptr;                               // [maxB][H] fp32
  float *hpart = nullptr;                           // [FC_SPLITS][E][H] acting-size fc partial sums
  void *dh = nullptr;                               // [maxB][H] T
  void *dz3 = nullptr, *dz2 = nullptr, *dz1 = nullptr;
  float *logits_b = nullptr, *values_b = nullptr;   // [maxB][A], [maxB] (forward-only API / debug)
  // ---- gradient slabs ----
  float *slab = nullptr;
  size_t slab_floats = 0;
  size_t slab_off[11] = {0}; // W1 b1 W2 b2 W3 b3 Wfc bfc Wh bh
  float *adv_stats = nullptr;
  float *sumsq_part = nullptr; // [1024]
  // ---- per-sample train metrics [mi][B] x 7 (aleppo_metric_field 0-6), and reduced [mi][METRIC_REC] (metrics_reduce_kernel)
  float *metric_ps = nullptr;
  size_t metric_cap = 0; // floats per field
  size_t metric_red_cap = 0;
  float *metric_red = nullptr, *h_metric_red = nullptr;
  float *grad_norms = nullptr; // [mi]
  float *adam_sched = nullptr, *h_adam_sched = nullptr; // [mi][2] step scalars of one aleppo_train call (device / pinned)
  // ---- ALEPPO_OPT_MINIBATCH_SHUFFLE: per-epoch sample order and the per-sample planes gathered into it ([epochs][N])
  bool shuffle = false;
  size_t shuf_cap = 0;        // samples (epochs * N) the buffers below hold
  int shuf_epochs_cap = 0;    // epochs the key buffers hold
  int32_t *order = nullptr;   // [epochs][N]
  int *act_p = nullptr;
  void *oldlp_p = nullptr, *adv_p = nullptr, *ret_p = nullptr; // RT [epochs][N][A], [epochs][N], [epochs][N]
  void *val_p = nullptr;      // RT [epochs][N]: the old values in that order (ALEPPO_OPT_VALUE_CLIP)
  uint8_t *mask_p = nullptr;
  float *mask_counts_ep = nullptr; // [epochs * M] global unmasked count per (epoch, minibatch)
  uint32_t *shuf_keys = nullptr, *h_shuf_keys = nullptr; // [epochs][4] Feistel round keys of one call (device / pinned)
  bool last_shuffled = false;
  // ---- ALEPPO_OPT_VALUE_CLIP: the values the batch was collected with, env-major RT [N] (allocated on first use)
  bool value_clip = false;
  void *val_n = nullptr;
  enum ValSrc { VAL_NONE = 0, VAL_ROLLOUT = 1, VAL_CALLER = 2 };
  int val_src = VAL_NONE; // VAL_ROLLOUT: val_n is filled from values_tm inside the update; VAL_CALLER: aleppo_set_batch_values
  bool caller_batch = false; // the batch came from aleppo_set_batch
  // ---- ALEPPO_OPT_ADV_NORM_MINIBATCH: per-minibatch advantage statistics (grown with the metric storage, [metric_red_cap])
  bool adv_norm_mb = false;
  double *advn_part = nullptr;                    // [mi][4] (n, S, Q, 0) partial sums (data parallel: all-reduced)
  float *advn_stats = nullptr, *h_advn_stats = nullptr; // [mi][4] (mean_f, inv_f, std, 0) (device / pinned)
  bool last_advn = false;                         // the last aleppo_train ran with the option (h_advn_stats holds it)
  // ---- ALEPPO_OPT_KL_PENALTY / ALEPPO_OPT_KL_COEF: the exact-KL plane and beta (allocated on first use)
  bool kl_pen = false;
  uint32_t kl_coef_bits = 0;                     // beta as an IEEE-754 binary32 bit pattern (finite, non-negative)
  float *kl_ps = nullptr;                        // [mi][B] per-sample exact KL, kl_cap floats (grown with metric_ps)
  size_t kl_cap = 0;
  float *kl_beta = nullptr, *h_kl_beta = nullptr; // [1] beta, uploaded at each aleppo_train (device / pinned)
  bool last_kl = false;                          // the last aleppo_train ran with the option (kl_ps / slot 8 hold it)
  // ---- ALEPPO_OPT_CLIP_PARAM / _VALUE_CLIP_RANGE / _VALUE_LOSS_COEF / _ENTROPY_COEF / _MAX_GRAD_NORM: the current values
  // (from the config until set), and the device block the update's kernels read them from (aleppo_create; never moved)
  Hyper hyper{};                                 // current clip range, coefficients and norm limit
  float value_clip_range = 0.f;                  // ALEPPO_OPT_VALUE_CLIP_RANGE; follows hyper.clip until set itself
  bool vclip_range_set = false;
  float last_max_norm = 0.f;                     // hyper.max_norm of the last aleppo_train (aleppo_export_grads)
  float *hyper_blk = nullptr, *h_hyper_blk = nullptr; // [HYPER_BLOCK], uploaded at each aleppo_train (device / pinned)
  // ---- ALEPPO_OPT_WEIGHT_DECAY / ALEPPO_OPT_ANCHOR_COEF: the two coefficients as binary32 bit patterns (finite, >= 0), and
  // the anchor of aleppo_anchor_take / aleppo_anchor_import: a fourth parameter set, fp32 only, never forwarded, allocated
  // on first use and written by those two calls alone.  Either coefficient non-zero: the update launches reg_step_kernel
  // in adam_kernel's place
  uint32_t wd_bits = 0, anchor_coef_bits = 0;
  ParamSet anchor;                 // (no compute copy: Pc stays nullptr)
  // ---- ALEPPO_OPT_REWARD_SCALE / _CLIP: device storage allocated on first use (ensure_rs_storage), never moved
  bool reward_scale = false;
  float reward_scale_clip = 10.0f;
  double *rs_blk = nullptr;   // [RS_BLOCK] the state block
  double *rs_g[2] = {nullptr, nullptr}; // [E] running returns: rs_g[rs_cur] is the state, the other the scan's output
  int rs_cur = 0;             // (flipped once a rollout is accepted: a refused one leaves the state as it was)
  double *rs_part = nullptr;  // [rs_blocks(E)][4] partials, then [4] the sums for the all-reduce
  // ---- captured update (ALEPPO_OPT_UPDATE_GRAPH): the epochs x minibatches loop as one hipGraph, re-captured when
  // the shape (or a baked pointer) changes; the first call of a shape runs eagerly (one-time kernel attribute set-up)
  bool update_graph = false;
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  struct GraphKey {
    int epochs = 0, M = 0, two = 0;
    long N = 0;
    const void *metric_ps = nullptr, *metric_red = nullptr;
    const void *order = nullptr; // shuffled updates: the order / gathered-plane storage (nullptr: contiguous)
    int vclip = 0;               // ALEPPO_OPT_VALUE_CLIP: 0 off, else 1 + the ValSrc the old values come from
    const void *advn = nullptr;  // ALEPPO_OPT_ADV_NORM_MINIBATCH: the statistics storage (nullptr: off)
    int klpen = 0;               // ALEPPO_OPT_KL_PENALTY (beta is a device value and not part of the key)
    const void *kl_ps = nullptr; // ... its per-sample plane (nullptr: off)
    int reg = 0;                 // reg_step_kernel in adam_kernel's place (the coefficients are device values, not part of the key)
    const void *anchor = nullptr; // ... the anchor it reads (nullptr: none yet, or adam_kernel)
    bool operator==(const GraphKey &o) const {
      return epochs == o.epochs && M == o.M && two == o.two && N == o.N && metric_ps == o.metric_ps &&
             metric_red == o.metric_red && order == o.order && vclip == o.vclip && advn == o.advn &&
             klpen == o.klpen && kl_ps == o.kl_ps && reg == o.reg && anchor == o.anchor;
    }
  } graph_key, warm_key;
  long graph_replays = 0;
  int last_epochs = 0, last_M = 0;
  long last_B = 0;
  // ---- profiling ----
  Tuning tune;
  hipError_t async_err = hipSuccess; // first failure of a call whose status could not be returned on the spot
  // ---- every device / pinned-host allocation of the context (api_internal.hpp, memory): aleppo_destroy frees these two
  // registries, and nothing is freed anywhere else
  std::vector<void *> owned_dev, owned_host;
  // ---- boundary staging (aleppo_set_batch / aleppo_forward / aleppo_read_batch), grown on demand
  void *rb_tmp[2] = {nullptr, nullptr}; // aleppo_read_batch scratch
  size_t rb_cap[2] = {0, 0};
  uint8_t *stage_u8 = nullptr;   // NCHW uint8 observations as uploaded
  size_t stage_u8_cap = 0;
  uint32_t *stage_obs = nullptr; // packed stacks of aleppo_forward's samples (never the rollout slots)
  size_t stage_obs_cap = 0;
  unsigned long long *dg_out = nullptr; // aleppo_state_digest's four words (allocated on first use)
  // ---- aleppo_tensor_stats: the per-chunk partial records and the 130 doubles (allocated on first use; its size is a
  // function of (H, A) only), and what the STEP section is recomputed from
  void *ts_scratch = nullptr;
  bool ts_step_valid = false;           // an aleppo_train has succeeded and no load_params / import_optimizer since
  float ts_sched[2] = {0.f, 0.f};       // the two schedule scalars of the last optimizer step that ran
  // ---- aleppo_forward_activations / aleppo_activation_stats: the NCHW float export staging (grown on demand) and the
  // statistics' partial records + the two tables (allocated on first use; its size is a function of the context's shape)
  float *ax_buf = nullptr;
  size_t ax_cap = 0;                    // bytes
  void *as_scratch = nullptr;
  // ---- aleppo_export_backward: host marks only.  What the last minibatch of an update leaves in a1 .. a3 / h / dh /
  // dz3 .. dz1: its sample count (0: nothing to export), the split-K slabs of h, whether the route stored dz1.  bwd_enq is
  // what enqueue_minibatch noted last (a capture keeps its copy in bwd_graph for the replays); aleppo_train makes it bwd
  // once the update has run, and whatever else writes the activation scratch (net_forward, the acting forward) clears bwd
  struct BwdMark {
    long B = 0;
    int hparts = 1;
    bool dz1 = false;
  } bwd, bwd_enq, bwd_graph;
  // ---- aleppo_export_acting: host marks only, like bwd.  What the last acting forward of the rollout (aleppo_act's,
  // aleppo_step's pre-computed one, aleppo_finish_rollout's bootstrap) left in a1 .. a3 / hpart: its sample count (0: nothing
  // to export) and whether the route stored a1 / a2.  act_forward on the rollout's scratch and aleppo_step's fused launch
  // set it; whatever else runs the network in that scratch or replaces the parameters clears it (acted_clear)
  struct ActMark {
    int n = 0;
    bool a12 = false;
  } acted;
  bool act_store = false; // ALEPPO_OPT_ACT_STORE: the fused acting launch also writes a1 / a2 (act_conv_kernel<MODE, true>)
  // ---- aleppo_feature_rank: the Gram blocks, column sums, split partials and row flags (allocated on first use; its size
  // is a function of (H, maxB))
  void *fr_scratch = nullptr;
  // ---- aleppo_recycle_units / aleppo_recycle_dormant: the unit mask, uint8 [160 + H] (allocated on first use)
  uint8_t *rc_mask = nullptr;
  // ---- aleppo_ema_open: the exponentially averaged parameters; nothing below is allocated, and nothing is enqueued for it,
  // on a context that never opens them
  ParamSet averaged;               // (on: aleppo_ema_open has succeeded)
  double *ema_blk = nullptr;       // [EMA_MAX_BLOCKS][3] workgroup partials, then the ALEPPO_EMA_STATS_COUNT doubles
  int64_t ema_updates = 0;
  bool eval_averaged = false;      // ALEPPO_OPT_EVAL_PARAMS: the evaluation lanes act on the averaged set
  // ---- aleppo_snapshot_take / aleppo_snapshot_import: the caller's third parameter set, and aleppo_policy_diff's scratch
  // (policy_diff_plan); each is allocated on first use and never again, nothing is enqueued for them on a context that
  // never makes the calls
  ParamSet snapshot;
  void *pd_scratch = nullptr;
  // ---- gradient probes (aleppo_grad_probe / _take / _import / _gram): the ALEPPO_GRAD_SLOTS gradient slots, ONE allocation
  // of that many padded vectors made by the first call that writes one; the probe's private blocks - GP_BLOCK floats the
  // head reads (device / pinned) and the per-sample planes it writes, [8][maxB]: the seven metric fields and the exact KL -
  // and the Gram's partial records and results.  Each is allocated on first use and never again; nothing is enqueued for
  // them on a context that never makes the calls, aleppo_train never reads them and aleppo_state_digest does not cover them
  float *grad_slots = nullptr;
  bool grad_written[ALEPPO_GRAD_SLOTS] = {false, false, false, false};
  float *gp_blk = nullptr, *h_gp_blk = nullptr;
  float *gp_ps = nullptr;
  void *gg_scratch = nullptr;
  // ---- aleppo_refresh_advantages: the second values plane, RT [T+1][E] time-major like values_tm (which it never
  // replaces), and the statistics' scratch; each is allocated on first use and never again, nothing is enqueued for them on
  // a context that never makes the call
  void *fresh_tm = nullptr;
  bool fresh_valid = false;        // fresh_tm belongs to the batch the context holds (aleppo_refresh_read)
  bool batch_refused = false;      // the last aleppo_finish_rollout refused its flags (its planes are not refreshed)
  double *rf_scratch = nullptr;    // [16] results | [RSTAT_SUMS] sums | [bstat_blocks(N)][RSTAT_SUMS] partials
  // ---- aleppo_saliency / aleppo_saliency_perturbed: nothing below is allocated, and nothing is enqueued for it, on a context
  // that never calls them; each buffer is allocated on first use and grown on demand like stage_obs
  uint32_t *sal_blur = nullptr;  // packed blurred stacks of the samples one forward chunk touches
  uint32_t *sal_stage = nullptr; // packed perturbed stacks of one forward chunk (at most maxB)
  float *sal_base = nullptr;     // [n][A] logits, then [n] values of the unperturbed samples
  float *sal_out = nullptr;      // [n][P] policy scores, [n][P] value scores, then [n][P + 1][A + 1] outputs when asked for
  uint8_t *sal_u8 = nullptr;     // NCHW uint8 of one chunk of aleppo_saliency_perturbed
  size_t sal_blur_cap = 0, sal_stage_cap = 0, sal_base_cap = 0, sal_out_cap = 0, sal_u8_cap = 0; // bytes
  // ---- evaluation lanes (aleppo_eval_open): L frame stacks of their own, their own acting scratch, upload staging and
  // action hand-off; nothing below is allocated, and nothing is enqueued for it, on a context that never opens them
  int ev_L = 0;                    // 0: not opened
  uint32_t *ev_obs = nullptr;      // [L][7056] packed stacks, updated in place by ingest_kernel
  void *ev_a1 = nullptr, *ev_a2 = nullptr, *ev_a3 = nullptr; // conv activations at L samples (a1 / a2: unfused convs only)
  float *ev_hpart = nullptr;       // [FC_SPLITS][L][H]
  float *ev_logits = nullptr, *ev_values = nullptr; // [L][A], [L] of the last aleppo_eval_act (always fp32)
  int *ev_actions = nullptr;       // [L]
  uint8_t *ev_d_frames = nullptr, *ev_h_frames = nullptr; // frame staging (device / pinned), L raw pairs
  uint8_t *ev_d_start = nullptr, *ev_h_start = nullptr;   // [L] episode-start flags
  float *ev_d_noise = nullptr, *ev_h_noise = nullptr;     // [L][max(A, 2)]
  int64_t *ev_h_actions = nullptr; // [L] + the ticket word, mapped pinned (aleppo_eval_act's *actions_pinned)
  unsigned int *ev_d_done = nullptr; // arrival counter of eval_head_kernel's ticket publish
  long long ev_ticket = 0;
  uint64_t ev_counter = 0;         // evaluation counter n of the built-in generator
  bool ev_acted = false;           // ev_logits / ev_values / ev_actions hold an aleppo_eval_act
  hipEvent_t ev_staged = nullptr;  // the last upload out of the pinned staging buffers has run
  // ---- device-resident environments (aleppo_env_open): ONE allocation - the frame buffer, two state arrays that
  // alternate slot by slot (env_step_kernel reads one and writes the other) and the four [T][E] episode-log planes; nothing
  // below is allocated, and nothing is enqueued for it, on a context that never opens them
  bool env_open = false;
  aleppo_env_config env_cfg{};
  uint8_t *env_blk = nullptr;      // the allocation; the frames are at its start (16-byte aligned)
  aleppo_env_state *env_state[2] = {nullptr, nullptr};
  int env_cur = 0;                 // env_state[env_cur] is the state between two slots
  float *env_log = nullptr;        // [4][T][E]: episode returns, episode lengths (u32), game returns, game lengths (u32)
  bool rec_on_device = false;      // the rollout being collected wrote its step records on the device (aleppo_env_rollout)
  ProfClass env_prof;              // ALEPPO_ENV_F_STEP_MS: events around the environment kernel while profiling is on
  // ---- device-resident evaluation environments (aleppo_eval_env_open), one per evaluation lane: ONE allocation - the
  // frame buffer, two alternating state arrays, the four [S][L] log planes and the L start-at-entry bytes the ingest reads;
  // members of their own (nothing of env_* above); nothing is allocated or enqueued on a context that never opens them
  bool ee_open = false;
  aleppo_env_config ee_cfg{};
  int ee_S = 0;                    // max_run_steps: the rows of a log plane
  uint8_t *ee_blk = nullptr;       // the allocation; the frames are at its start (16-byte aligned)
  aleppo_env_state *ee_state[2] = {nullptr, nullptr};
  int ee_cur = 0;                  // ee_state[ee_cur] is the state between two steps
  float *ee_log = nullptr;         // [4][S][L]: episode returns, episode lengths (u32), game returns, game lengths (u32)
  uint8_t *ee_start = nullptr;     // [L] start-at-entry bytes of the last step
  // ---- episode recorders (aleppo_rec_open), one per aleppo_rec_source: ONE allocation each - steps [cap] | frames [cap] |
  // observations [cap] | logits [cap][A], the two middle planes only where they are part of the content; rows / dropped /
  // ordinal are host state (every step of a source takes exactly one row, so the host addresses the row at enqueue);
  // nothing is allocated or enqueued on a context that never opens one
  struct Recorder {
    bool open = false;
    aleppo_rec_config cfg{};
    uint8_t *blk = nullptr;
    aleppo_rec_step *steps = nullptr;
    uint8_t *frames = nullptr, *obs = nullptr; // nullptr: not part of cfg.content
    float *logits = nullptr;
    size_t frame_bytes = 0;        // of one row of the frames plane (fixed by the source's frame kind)
    uint64_t rows = 0, dropped = 0, ordinal = 0;
  } rec[2];
  bool prof_on = false;
  bool serial_update = false; // ALEPPO_OPT_SERIAL_UPDATE: every update kernel on the main stream
  bool dbg_no_publish = false;
  bool force_comm = false;
  ProfClass prof[ALEPPO_K_COUNT];
};

int set_err(Ctx *c, int code, const std::string &msg);
#define HIPCHK(c, x)                                                                                                   \
  do {                                                                                                                 \
    hipError_t e_ = (x);                                                                                               \
    if (e_ != hipSuccess)                                                                                              \
      return set_err((c), ALEPPO_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));                           \
  } while (0)

// ------------------------------------------------------------------ kernel launchers (kernels.hip)
constexpr int MAX_ENVS_PER_RANK = 8192;
struct StartBits { // episode-start flags of one slot as a kernel argument (bit e of word e/32)
  uint32_t w[MAX_ENVS_PER_RANK / 32];
};
void launch_ingest(hipStream_t s, bool raw, const uint8_t *frames, const uint8_t *lut, const uint8_t *start,
                   const StartBits *sbits, uint32_t *obs, int E, int slots, int t_src, int t_dst);
void launch_copy_slot(hipStream_t s, uint32_t *obs, int E, int slots, int src, int dst);
void launch_gate(hipStream_t s, unsigned long long *go_dev, unsigned long long seq, unsigned long long timeout_ticks);
void launch_infer_head(hipStream_t s, const float *hpart, const float *bfc, const float *Wh, const float *bh,
                       const float *noise, uint64_t seed, uint64_t counter, void *logits_t, void *values_t,
                       int *actions_t, int64_t *pinned, unsigned int *done_ctr, long long ticket, int E, int H, int A,
                       const float *probs_in = nullptr, bool rt16 = false);
// head of the evaluation lanes: rule = aleppo_eval_rule, param = 1 / tau (SAMPLE) or epsilon (EPSILON_GREEDY); key = the
// Philox key of the evaluation stream, counter = the evaluation counter; fp32 outputs; pinned / done_ctr never null
void launch_eval_head(hipStream_t s, const float *hpart, const float *bfc, const float *Wh, const float *bh,
                      const float *noise, uint64_t key, uint64_t counter, int rule, float param, float *logits,
                      float *values, int *actions, int64_t *pinned, unsigned int *done_ctr, long long ticket, int L, int H,
                      int A);
void launch_gae(hipStream_t s, uint8_t *step_rec, size_t rec_bytes, const void *values_tm, const void *logits_tm,
                const int *actions_tm, void *adv_n, void *ret_n, void *oldlp_n, int *act_n, uint8_t *mask_n, int *err,
                int E, int T, int A, float gamma, float lambda, bool clamp = true, bool rt16 = false);

// ALEPPO_OPT_REWARD_SCALE.  The state block is double [RS_BLOCK] in device memory: the running (count, mean, var), the
// scale s (a float, widened), the sample count of the last scaled rollout, and the clip counter as a 64-bit integer.
enum { RS_COUNT = 0, RS_MEAN = 1, RS_VAR = 2, RS_SCALE = 3, RS_BATCH_COUNT = 4, RS_CLIPPED = 5, RS_BLOCK = 8 };
// stage 1: the forward scan over the step records; g_in / g_out: the running returns [E] before / after, part:
// [rs_blocks(E)][4] = (n, S, Q, 0) per workgroup, err: set when flags overlap (like gae_kernel).  Stage 2 adds the partials
// in index order and merges them into the block rs (sums_out == nullptr), or writes the three sums for an all-reduce
// that launch_rs_finalise merges afterwards.
int rs_blocks(int E);
void launch_rs_scan(hipStream_t s, const uint8_t *step_rec, size_t rec_bytes, const double *g_in, double *g_out,
                    double *part, int *err, int E, int T, float gamma);
void launch_rs_reduce(hipStream_t s, const double *part, int nblk, double *sums_out, double *rs, const int *err);
void launch_rs_finalise(hipStream_t s, const double *sums, double *rs, const int *err);
// launch_gae with step 5 of ALEPPO_OPT_REWARD_SCALE in place of the clamp: s from rs[RS_SCALE], the clip as an argument
void launch_gae_scaled(hipStream_t s, uint8_t *step_rec, size_t rec_bytes, const void *values_tm, const void *logits_tm,
                       const int *actions_tm, void *adv_n, void *ret_n, void *oldlp_n, int *act_n, uint8_t *mask_n,
                       int *err, int E, int T, int A, float gamma, float lambda, double *rs, float clip, bool rt16);

void launch_adv_norm(hipStream_t s, void *adv_n, const uint8_t *mask_n, float *stats, long n, int phase, bool rt16);
void launch_plane_to_float(hipStream_t s, const void *src, float *dst, long n, bool rt16);
void launch_plane_from_float(hipStream_t s, const float *src, void *dst, long n, bool rt16);
void launch_mask_count(hipStream_t s, const uint8_t *mask_n, float *counts, long B, int M);
// ALEPPO_OPT_ADV_NORM_MINIBATCH: block per minibatch i < nmb over adv / mask + i*B.  part == nullptr: stats[i][4] =
// (mean_f, inv_f, std, 0) of aleppo.h; else part[i][4] = (n, S, Q, 0) in double, for an all-reduce and launch_advn_finalise
void launch_advn_stats(hipStream_t s, const void *adv, const uint8_t *mask, long B, int nmb, double *part, float *stats,
                       bool rt16);
void launch_advn_finalise(hipStream_t s, const double *part, float *stats, int nmb);
// ALEPPO_F_BATCH_STATS: stage 1, block b < bstat_blocks(n) over samples [b * BSTAT_CHUNK, ...) writes part[b][BSTAT_SUMS] =
// (n, S_v, Q_v, S_R, Q_R, S_a, Q_a, S_d, Q_d) in double; val is time-major [T+1][E] when E > 0, sample-major when E == 0.
// Stage 2 adds the partials in index order into sums[BSTAT_SUMS] (when not null) and / or finalises them into
// result[ALEPPO_BATCH_STATS_COUNT]; launch_bstat_finalise does the latter from all-reduced sums.
constexpr int BSTAT_CHUNK = 4096, BSTAT_SUMS = 9;
int bstat_blocks(long n);
void launch_bstat_partial(hipStream_t s, const void *val, const void *ret, const void *adv, const uint8_t *mask, long n,
                          int E, int T, double *part, bool rt16);
void launch_bstat_reduce(hipStream_t s, const double *part, int nblk, double *sums, double *result);
void launch_bstat_finalise(hipStream_t s, const double *sums, double *result);
// aleppo_refresh_advantages' statistics, siblings of the two stages above with the same order: val is the fresh plane and
// val0 the collected one (both time-major [T+1][E]); a partial is the nine sums, then S and Q of d' = val - val0 and the
// maximum of |d'|.  Stage 2 adds (takes the maximum of) the partials in index order and writes
// result[ALEPPO_REFRESH_STATS_COUNT]: the ten of ALEPPO_F_BATCH_STATS, then the mean, population std and maximum of d'.
constexpr int RSTAT_SUMS = 12;
void launch_rstat_partial(hipStream_t s, const void *val, const void *val0, const void *ret, const void *adv,
                          const uint8_t *mask, long n, int E, int T, double *part, bool rt16);
void launch_rstat_reduce(hipStream_t s, const double *part, int nblk, double *result);
// aleppo_refresh_advantages (refresh.hip): the value head alone on the ns fc rows of one forward chunk, rounded to RT and
// stored time-major - sample n = n0 + r = e*T + t at fresh_tm[t*E + e], or (boot: the post-rollout observations, r = e) at
// row T.  wv / bv: the value row of the head weights and its bias
void launch_value_refresh(hipStream_t s, const float *h, const float *wv, const float *bv, void *fresh_tm, long n0,
                          long ns, int H, int E, int T, bool boot, bool rt16);
// ALEPPO_OPT_MINIBATCH_SHUFFLE: order[e][i] = the keyed bijection of aleppo.h (round keys rk[e][4], domain 2^(2h)) and the
// per-sample planes gathered into that order: act / oldlp / adv / ret / mask_p[e][i] = plane[order[e][i]]
// (val_n != nullptr, ALEPPO_OPT_VALUE_CLIP: also val_p[e][i] = val_n[order[e][i]])
void launch_shuffle_gather(hipStream_t s, const uint32_t *rk, int h, long N, int epochs, int A, int32_t *order,
                           const int *act_n, const void *oldlp_n, const void *adv_n, const void *ret_n,
                           const void *val_n, const uint8_t *mask_n, int *act_p, void *oldlp_p, void *adv_p,
                           void *ret_p, void *val_p, uint8_t *mask_p, bool rt16);
// vold: the values the samples were collected with (ALEPPO_OPT_VALUE_CLIP), or nullptr for the reference's value loss;
// ps_kl / ps_cf: the per-sample approx-KL and clip-fraction planes (always written);
// advs: this minibatch's (mean_f, inv_f) of ALEPPO_OPT_ADV_NORM_MINIBATCH, or nullptr for the advantages as stored;
// klb: ALEPPO_OPT_KL_PENALTY's beta (device float [1]) and ps_kle its per-sample exact-KL plane, or nullptr (off)
struct HeadTrainArgs {
  const float *h, *Wh, *bh;
  const int *act;
  const void *oldlp, *adv, *ret, *vold; // planes of RT (float, or f16 with rt16)
  const uint8_t *mask;
  const float *mask_count;
  void *dh;
  int prec;
  float *ps_total, *ps_clipped, *ps_value, *ps_entropy, *ps_ratio, *ps_kl, *ps_cf;
  float *slab_w, *slab_b;
  int nblk;
  long B;
  int H, A;
  float *logits_out = nullptr, *values_out = nullptr;
  int hparts = 1;
  bool rt16 = false; // oldlp / adv / ret / vold are f16 planes
  const float *advs = nullptr, *klb = nullptr;
  float *ps_kle = nullptr;
};
// hp: the device block of the hyper-parameter options (slots HYPER_CLIP .. HYPER_CE; head_train.hip)
void launch_head_train(hipStream_t s, const HeadTrainArgs &a, const float *hp);
struct ReduceSeg {
  const float *slab;
  int S;
  long n;
  long dst;
};
void launch_reduce_slabs(hipStream_t s, const ReduceSeg *segs, int nseg, float *G);
// squares G[0, n_main) in nblk_main blocks + the two tail tensors (slab sums fused when tail[i].slab != nullptr);
// returns the number of partials written (<= 1024)
int launch_sumsq(hipStream_t s, float *G, long n_main, float *partials, int nblk_main, const ReduceSeg tail[2]);
// clip + Adam over the whole flat vector; also refreshes the compute copy Pc (bf16) and the dgrad-side transposed weight
// layouts WfcT / W3d / W2d (both precisions) from the updated parameters in the same pass
void launch_adam(hipStream_t s, float *P, const float *G_in, float *M1, float *M2, void *Pc,
                 void *WfcT, void *W3d, void *W2d, const ParamLayout &L, int prec, const float *partials, int nblk,
                 const float *hpd,   // the device block of the hyper-parameter options: slot HYPER_MAX_NORM is the limit
                 const float *sched, // device: { lr / (1 - beta1^t), sqrt(1 - beta2^t) } of this step
                 float beta1, float beta2, float eps, float *grad_norm_out,
                 // reg: reg_step_kernel instead of adam_kernel - the same step, then p -= f_wd * p0 + f_an * (p0 - a) with the
                 // factors of slots HYPER_WD / HYPER_ANCHOR and a = anchor[i] (nullptr: +0.0f)
                 bool reg = false, const float *anchor = nullptr);
void launch_pack_dgrad(hipStream_t s, const float *P, const ParamLayout &L, void *W2d, void *W3d, void *WfcT,
                       int prec);
void launch_cast_params(hipStream_t s, const float *P, void *Pc, long n);
// out: [epochs * M][METRIC_REC] records; kle: the exact-KL plane of ALEPPO_OPT_KL_PENALTY (slot 8), or nullptr
void launch_metrics_reduce(hipStream_t s, const float *ps, size_t field_stride, const uint8_t *mask_n, long B, int M,
                           int epochs, float *out, const float *kle = nullptr);
void launch_obs_unpack(hipStream_t s, const uint32_t *obs, uint8_t *out, long nsamp, SampleMap map);
void launch_obs_pack(hipStream_t s, const uint8_t *in, uint32_t *obs, long nsamp, SampleMap map);
void launch_transpose_tm_pitched(hipStream_t s, const void *src_tm, size_t pitch, void *dst_em, int E, int T, int inner,
                                 int elem);
// aleppo_state_digest: zeroes out[ALEPPO_DIGEST_COUNT] and adds the four sections of aleppo.h into it - the learner from the
// internal layout (step: the Adam step), the rollout from the packed stacks of `slot` of obs [E][slots][7056] (counter: the
// acting generator's), the reward-scale state from its block and running returns.  Reads only.
void launch_state_digest(hipStream_t s, const float *P, const float *M1, const float *M2, const ParamLayout &L,
                         int64_t step, const uint32_t *obs, int slots, int slot, int E, uint64_t counter,
                         const double *rs_blk, const double *rs_g, unsigned long long *out);
// aleppo_tensor_stats (tensor_stats.hip): one read-only pass over the padded flat vectors in chunks of TS_CHUNK floats per
// internal tensor (one workgroup and one pair of partial records per chunk), then one small launch that adds the partials
// per exported tensor in index order and writes double [ALEPPO_TENSOR_STATS_ROWS][ALEPPO_TENSOR_STATS_COLS] behind the
// records.  sections: aleppo_tensor_stats_section bits; without ALEPPO_TS_SEC_STEP only P is read.  coef: the clip factor
// of aleppo_export_grads; step_size / bc2_sqrt / eps: adam_element's scalars of the last optimizer step.
constexpr int TS_CHUNK = 4096;
// the chunk grid the two passes of this structure share (aleppo_tensor_stats, aleppo_grad_gram)
struct TsLayout {
  uint32_t off[P_COUNT], size[P_COUNT]; // in floats, of the internal tensors
  uint32_t split[P_COUNT];              // first element of the tensor's second exported row (== size: there is none)
  uint32_t first[P_COUNT + 1];          // first chunk of each tensor; first[P_COUNT] = the grid
};
// exported row r = (internal tensor, which side of its split)
struct TsRow {
  int tensor, half;
};
__host__ __device__ inline TsRow ts_row(int r) {
  constexpr int T[12] = {P_W1, P_B1, P_W2, P_B2, P_W3, P_B3, P_WFC, P_BFC, P_WH, P_BH, P_WH, P_BH};
  return TsRow{T[r], r >= 10 ? 1 : 0};
}
TsLayout ts_layout(const ParamLayout &L);
__device__ __forceinline__ bool ts_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
// sum over the 64 lanes by a fixed tree, valid in lane 0
__device__ __forceinline__ double ts_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_down(v, o, 64);
  return v;
}
size_t tensor_stats_scratch_bytes(const ParamLayout &L);
void launch_tensor_stats(hipStream_t s, const float *P, const float *G, const float *M1, const float *M2,
                         const ParamLayout &L, int sections, float coef, float step_size, float bc2_sqrt, float eps,
                         void *scratch, const double **out_dev);
// aleppo_grad_gram (grad_gram.hip): the Gram of K <= ALEPPO_GRAD_SLOTS padded vectors per exported tensor, over the chunk grid
// above (one workgroup and one pair of partial records per chunk), then one small launch that adds the partials per
// exported tensor in index order and writes double [ALEPPO_TENSOR_STATS_ROWS][K][K], then int64 [ALEPPO_TENSOR_STATS_ROWS]
// (the left-out element indices), behind the records.  It only reads the vectors.
size_t grad_gram_scratch_bytes(const ParamLayout &L);
void launch_grad_gram(hipStream_t s, const float *const *vec, int K, const ParamLayout &L, void *scratch,
                      const double **out_dev);
// aleppo_grad_take's ALEPPO_GRAD_SRC_PARAM_DELTA: out = a - b, one fp32 subtraction per element of the padded vectors
void launch_grad_delta(hipStream_t s, const float *a, const float *b, float *out, long n);
// The probe's private device block: the hyper block the head reads (HYPER_BLOCK floats, 16-byte aligned), the advantage
// record (mean_f, inv_f, std, 0), beta, and the slice's unmasked count
enum { GP_HYPER = 0, GP_ADVS = 8, GP_BETA = 12, GP_COUNT = 16, GP_BLOCK = 20 };
// aleppo_forward_activations / aleppo_activation_stats (activation_stats.hip).  Export: layer 0-2 = a1 / a2 / a3 of ns
// samples, NHWC of T -> float NCHW.  Statistics: the batch is forwarded in chunks of at most maxB samples; after each
// forward one read-only launch over a1 / a2 / a3 / h writes one partial record per (workgroup, unit) behind the records of
// the chunks before it (done[layer]: records written so far, advanced by the launcher); the final launch adds each unit's
// records in that order and writes double [units][ALEPPO_ACT_UNIT_COLS] and [ALEPPO_ACT_LAYER_ROWS][ALEPPO_ACT_LAYER_COLS]
// behind the records.  The plan (record areas per layer, scratch bytes) is a function of (precision, H, samples, maxB).
struct ActStatsPlan {
  size_t rec_base[4]; // first record of conv1, conv2, conv3, fc
  size_t records, units, bytes;
};
ActStatsPlan act_stats_plan(int prec, int H, long total, long maxB);
void launch_act_stats_partial(hipStream_t s, int prec, const void *a1, const void *a2, const void *a3, const float *h,
                              int H, long ns, const ActStatsPlan &pl, size_t done[4], void *scratch);
void launch_act_stats_final(hipStream_t s, int H, long total, double tau, const ActStatsPlan &pl, const size_t done[4],
                            void *scratch, const double **units_dev, const double **layers_dev);
void launch_act_export(hipStream_t s, int prec, int layer, const void *a, float *out, long ns);
// aleppo_export_backward: a row-major plane of T (dh), n elements (a multiple of 8) -> float, widened exactly
// (activation_stats.hip); h as the head training kernel sees it, the hparts split-K slabs [hparts][B][H] added in its
// order -> float [B][H] (head_train.hip: the same device function)
void launch_plane_export(hipStream_t s, int prec, const void *src, float *out, long n);
void launch_h_export(hipStream_t s, const float *h, int hparts, long B, int H, float *out);
// aleppo_feature_rank (feature_rank.hip).  The plan is a function of (H, maxB): nb 64-column blocks, tiles = nb (nb + 1) / 2
// upper blocks of 4096 doubles.  Scratch: the result - double [tiles][64][64] blocks of G, [H] column sums, [2] (the rows
// left out, a pad) - then the partial results of up to FR_MAX_SPLITS row splits in the same form, then the row flags
// (uint32 [maxB], 1 = every feature of the row is finite).  launch_feature_rank_chunk: the three launches of one forward
// chunk h [ns][H] - flags, Gram + column sums per split, the reduce that adds the splits in order and sets (first) or adds
// to the result.  fr_tile: the block of G that holds element (i, j), i <= j.
constexpr int FR_MAX_SPLITS = 16, FR_SPLIT_ROWS = 256;
struct FeatureRankPlan {
  int H, nb, tiles;
  size_t result_doubles; // tiles * 4096 + H + 2
  size_t bytes;
};
FeatureRankPlan feature_rank_plan(int H, long maxB);
inline size_t fr_tile(int nb, int bi, int bj) { return (size_t)bi * nb - (size_t)bi * (bi - 1) / 2 + (size_t)(bj - bi); }
void launch_feature_rank_chunk(hipStream_t s, const float *h, long ns, bool first, const FeatureRankPlan &pl, void *scratch);
// aleppo_policy_diff (policy_diff.hip).  The plan is a function of (H, A, cap, maxB), cap = the most rows a call can bring.
// Scratch, every area 256-byte aligned: logits [2][cap][A] and values [2][cap] of the two sets (fp32), set a's h
// [maxB][H], the per-sample table double [cap][ALEPPO_PD_ROW], the workgroup partials double [PD_PART][PD_MAX_BLOCKS], the
// running totals double [PD_PART], the ALEPPO_PD_COUNT stats, the transition counts uint64 [MAX_ACTIONS][MAX_ACTIONS].
// A partial / total record: PD_SUMS sums (pd_sum), then the four order-free extrema (pd_ext).
// launch_policy_diff_chunk: the two launches of one forward chunk of ns rows that start at row n0 - the comparison (one
// wave per row, grid = min(ceil(ns / 4), PD_MAX_BLOCKS), a function of ns alone) and the finalising launch that adds the
// partials in index order and sets (first) or adds to the totals.  launch_policy_diff_stats, after the last chunk: the
// stats from the totals.  The transition counts are only added to: the caller clears them before the first chunk.
constexpr int PD_MAX_BLOCKS = 1024, PD_SUMS = 13, PD_PART = 17;
enum pd_sum { PD_S_ROWS, PD_S_NONFINITE, PD_S_CHURN, PD_S_KL_AB, PD_S_KL_BA, PD_S_TV, PD_S_ABS_DV, PD_S_DV2, PD_S_ENT_A,
              PD_S_ENT_B, PD_S_COS, PD_S_DH2, PD_S_HA2 };
enum pd_ext { PD_X_MAX_KL_AB = PD_SUMS, PD_X_MAX_TV, PD_X_MAX_ABS_DV, PD_X_MIN_COS };
struct PolicyDiffPlan {
  int H, A;
  long cap;
  size_t logits[2], values[2], h_a, rows, part, total, stats, trans; // byte offsets
  size_t bytes;
};
PolicyDiffPlan policy_diff_plan(int H, int A, long cap, long maxB);
void launch_policy_diff_chunk(hipStream_t s, const float *h_b, long n0, long ns, bool first, const PolicyDiffPlan &pl,
                              void *scratch);
void launch_policy_diff_stats(hipStream_t s, const PolicyDiffPlan &pl, void *scratch);
// aleppo_recycle_units / aleppo_recycle_dormant (recycle.hip).  mask: uint8 [160 + H] in device memory, 4-byte aligned, in
// the unit order of aleppo_activation_stats.  launch_recycle_mask forms it from that entry point's device-side unit table
// (mask[u] = layer bit of u in layers && SCORE_u <= tau); launch_recycle is the one pass over P / M1 / M2 in the internal
// layout (key: splitmix64 of the call's key); the caller rebuilds the derived copies (params_rewritten).
void launch_recycle_mask(hipStream_t s, const double *units_dev, int H, double tau, int layers, uint8_t *mask);
void launch_recycle(hipStream_t s, const ParamLayout &L, const uint8_t *mask, unsigned long long key, bool keep_moments,
                    float *P, float *M1, float *M2);
// aleppo_shrink_perturb (recycle.hip: it shares the draw and the layout-to-export index map with the pass above): one pass
// over P, p' = lam * p + sg * xi as three fp32 operations; key: splitmix64 of the call's key.  Pads are not written.
void launch_shrink_perturb(hipStream_t s, const ParamLayout &L, unsigned long long key, float lam, float sg, float *P);
// aleppo_saliency / aleppo_saliency_perturbed (saliency.hip).  SalTables: aleppo_saliency_tables' two tables, passed by value.
// blur: samples [s0, s0 + count) of the call (sample s of the call is sample map.n0 + s of obs under map) -> blur[0 .. count),
// lane k only where bit k of planes is set.  perturb: pairs [j0, j0 + ns) of the call, pair j = sample j / per at position
// p0 + j % per, -> stage[0 .. ns); blur_s0: the sample blur[0] holds.  score: pairs [i0, i0 + ns) with per = P, p0 = 0 - rows
// [0, ns) of logits / values against row (sample) of base_*, into policy / value [i] and, when not null, outputs [n][P+1][A+1].
struct SalTables {
  uint16_t g[84], w[84];
  int32_t radius;
};
void launch_sal_blur(hipStream_t s, const uint32_t *obs, SampleMap map, long s0, long count, const SalTables &tb,
                     int planes, uint32_t *blur);
void launch_sal_perturb(hipStream_t s, const uint32_t *obs, SampleMap map, const uint32_t *blur, long blur_s0,
                        const SalTables &tb, int planes, int stride, int G, long j0, long ns, int per, int p0,
                        uint32_t *stage);
void launch_sal_score(hipStream_t s, const float *base_logits, const float *base_values, const float *logits,
                      const float *values, long i0, long ns, int P, int A, float *policy, float *value, float *outputs);
// aleppo_ema_update (ema.hip).  launch_ema: the one streaming pass over the padded vector - Pe = d * Pe + w * P as three fp32
// operations (update), Pec = (T)Pe where Pec != Pe, and one (sum Pe^2, sum P^2, sum (P - Pe)^2) partial in double per
// workgroup into blk; update == false: the sums alone, nothing is stored to Pe / Pec (open, import).  launch_ema_final adds
// the partials in index order and writes the ALEPPO_EMA_STATS_COUNT doubles at ema_stats(blk).
constexpr int EMA_MAX_BLOCKS = 2048;
inline double *ema_stats(double *blk) { return blk + (size_t)EMA_MAX_BLOCKS * 3; }
constexpr size_t EMA_BLK_BYTES = ((size_t)EMA_MAX_BLOCKS * 3 + ALEPPO_EMA_STATS_COUNT) * sizeof(double);
int launch_ema(hipStream_t s, bool update, const float *P, float *Pe, void *Pec, long n, float d, float w, double *blk);
void launch_ema_final(hipStream_t s, int nblk, long long updates, float d, double *blk);
void launch_heads_fwd(hipStream_t s, const float *h, const float *Wh, const float *bh, float *logits, float *values,
                      long n, int H, int A);
void launch_logsoftmax_rows(hipStream_t s, const float *in, float *out, long rows, int A);
// float-in / float-out free functions of ai::vision (library-only in the reference, vision.cc:8-32,:71-84)
void launch_area_resize(hipStream_t s, const float *in, float *out, long n);
void launch_rgb_to_gray(hipStream_t s, const float *in, float *out, long n);

// ------------------------------------------------------------------ GEMM launchers (gemm_launch.hip)
// prec selects T (ALEPPO_FP32 / ALEPPO_BF16); all pointers are device pointers of the matching type.
void conv1_fwd(hipStream_t s, int prec, const uint32_t *obs, SampleMap map, const void *W1, const float *b1, void *a1,
               long ns);
void conv2_fwd(hipStream_t s, int prec, const void *a1, const void *W2, const float *b2, void *a2, long ns);
void conv3_fwd(hipStream_t s, int prec, const void *a2, const void *W3, const float *b3, void *a3, long ns);
// returns the number of split-K partial slabs written to h ([parts][ns][H], slab 0 carries the bias); 1 unless
// max_parts > 1 allows the pipelined bf16 kernel to split K (the consumer then adds the slabs)
int fc_fwd(hipStream_t s, int prec, const void *a3, const void *Wfc, const float *bfc, float *h, long ns, int H,
           int max_parts = 1);
constexpr int FC_FWD_MAX_PARTS = 4;
void fc_fwd_splitk(hipStream_t s, int prec, const void *a3, const void *Wfc, float *hpart, long ns, int H);
void fc_dgrad(hipStream_t s, int prec, const void *dh, const void *WfcT, const void *a3, void *dz3, long ns, int H);
void conv3_dgrad(hipStream_t s, int prec, const void *dz3, const void *W3d, const void *a2, void *dz2, long ns);
void conv2_dgrad(hipStream_t s, int prec, const void *dz2, const void *W2d, const void *a1, void *dz1, long ns);
// wgrads write split-K slabs; return the number of slices S used (slab holds S*[M*N] then bias S*[M])
int fc_wgrad(hipStream_t s, int prec, const void *dh, const void *a3, float *slab_w, float *slab_b, long ns, int H);
int fc_wgrad_slices(int prec, long ns); // number of split-K slices fc_wgrad will use for ns samples
int conv3_wgrad(hipStream_t s, int prec, const void *dz3, const void *a2, float *slab_w, float *slab_b, long ns);
int conv2_wgrad(hipStream_t s, int prec, const void *dz2, const void *a1, float *slab_w, float *slab_b, long ns);
int conv1_wgrad(hipStream_t s, int prec, const void *dz1, const uint32_t *obs, SampleMap map, float *slab_w,
                float *slab_b, long ns);

// ------------------------------------------------------------------ sample-stationary bf16 conv kernels (conv_patch_launch.hip)
inline bool use_patch_kernels() { return tuning().patch_conv; } // false: ALEPPO_OPT_GENERIC_CONV / ALEPPO_GENERIC_CONV=1
void patch_conv1_fwd(hipStream_t s, const uint32_t *obs, SampleMap map, const void *W1, const float *b1, void *a1,
                     long ns);
void patch_conv2_fwd(hipStream_t s, const void *a1, const void *W2, const float *b2, void *a2, long ns);
void patch_conv3_fwd(hipStream_t s, const void *a2, const void *W3, const float *b3, void *a3, long ns);
void patch_conv3_dgrad(hipStream_t s, const void *dz3, const void *W3d, const void *a2, void *dz2, long ns);
void patch_conv2_dgrad(hipStream_t s, const void *dz2, const void *W2d, const void *a1, void *dz1, long ns);
// conv1 -> conv2 -> conv3 of the acting batch in one launch; ingest_mode 1 / 2 first forms every environment's stack from
// a new 84x84 frame / raw frame pair (fused frame ingest: see ActIngestParams in conv_patch.hpp)
void patch_fwd_fused(hipStream_t s, const uint32_t *obs, SampleMap map, const void *W1, const float *b1, const void *W2,
                     const float *b2, const void *W3, const float *b3, void *a1, void *a2, void *a3, long ns);
int patch_conv_bwd_fused(hipStream_t s, const void *dz2, const void *a1, const uint32_t *obs, SampleMap map, const void *W2d,
                         float *sw2, float *sb2, float *sw1, float *sb1, long ns);
void patch_act_convs(hipStream_t s, uint32_t *obs, SampleMap map, const void *W1, const float *b1, const void *W2,
                     const float *b2, const void *W3, const float *b3, void *a3, long ns, int ingest_mode = 0,
                     const uint8_t *frames = nullptr, const uint8_t *lut = nullptr, const StartBits *sbits = nullptr,
                     long src_delta = 0, const uint8_t *start_bytes = nullptr, void *a1_store = nullptr,
                     void *a2_store = nullptr); // a1_store / a2_store (both or neither): the storing instantiation
int patch_conv1_wgrad(hipStream_t s, const void *dz1, const uint32_t *obs, SampleMap map, float *sw, float *sb,
                      long ns);
int patch_conv2_wgrad(hipStream_t s, const void *dz2, const void *a1, float *sw, float *sb, long ns);
int patch_conv3_wgrad(hipStream_t s, const void *dz3, const void *a2, float *sw, float *sb, long ns);

} // namespace aleppo

struct aleppo_ctx : aleppo::Ctx {};
