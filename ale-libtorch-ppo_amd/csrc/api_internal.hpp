// api_internal.hpp - what the C ABI's translation units share (api_core.hip, api_rollout.hip, api_train.hip,
// api_batch.hip, api_eval.hip, api_eval_env.hip, api_env.hip, api_rec.hip, api_state.hip, api_acts.hip, api_recycle.hip, api_ema.hip, api_saliency.hip, api_feature_rank.hip, api_policy_diff.hip, api_refresh.hip, api_reg.hip, api_grad_probe.hip, api_ops.hip): the entry-point guard macros, the memory
// ownership helpers (dalloc / halloc / grow over ctx_alloc / ctx_host_alloc / ctx_grow) and the other host-side helpers.
// Host code only; the helpers are defined in api_core.hip unless noted.
#pragma once
#include "common.hpp"
#include <algorithm>
#include <cmath>
#include <atomic>
#include <chrono>
#include <thread>
#include <mutex>
#include <cstring>
#include <initializer_list>
#include <rccl/rccl.h>

// ------------------------------------------------------------------ helpers
// every stateful entry point: the caller's thread may have another device current, and the kernel-selection switches
// are this context's
#define CHECK_CTX_ANY(c)                                                                                               \
  do {                                                                                                                 \
    if (!(c))                                                                                                          \
      return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "null context");                                            \
    if (hipSetDevice((c)->cfg.device_ordinal) != hipSuccess)                                                           \
      return set_err(const_cast<aleppo_ctx *>(c), ALEPPO_ERR_HIP, "hipSetDevice failed");                              \
    set_tuning(&(c)->tune);                                                                                            \
    if ((c)->failed)                                                                                                   \
      return set_err(const_cast<aleppo_ctx *>(c), ALEPPO_ERR_RUNTIME, (c)->fail_msg);                                  \
  } while (0)
// Between aleppo_arm_step and aleppo_release_step the stream is parked on the release word: anything that enqueues behind
// it and then waits (or rewrites what the parked kernels read) would dead-lock, so every entry point but the release
// refuses.
#define CHECK_CTX(c)                                                                                                   \
  do {                                                                                                                 \
    CHECK_CTX_ANY(c);                                                                                                  \
    if ((c)->armed)                                                                                                    \
      return set_err(const_cast<aleppo_ctx *>(c), ALEPPO_ERR_RUNTIME,                                                  \
                     "a step is armed: call aleppo_release_step first");                                               \
  } while (0)
#define CHECK_ASYNC(c)                                                                                                 \
  do {                                                                                                                 \
    if ((c)->async_err != hipSuccess) {                                                                                \
      const hipError_t e_ = (c)->async_err;                                                                            \
      (c)->async_err = hipSuccess;                                                                                     \
      return set_err((c), ALEPPO_ERR_HIP, std::string("asynchronous HIP failure: ") + hipGetErrorString(e_));          \
    }                                                                                                                  \
  } while (0)
#define NCCLCHK(c, x)                                                                                                  \
  do {                                                                                                                 \
    ncclResult_t r_ = (x);                                                                                             \
    if (r_ != ncclSuccess)                                                                                             \
      return set_err((c), ALEPPO_ERR_HIP, std::string(#x) + ": " + ncclGetErrorString(r_));                            \
  } while (0)

namespace aleppo {

// A failure after which the rollout / learner state is undefined: the context refuses every later call (sticky), any
// gate still on the stream is released so that the stream drains, and nothing is freed or reused before aleppo_destroy
// (kernels that are still queued may read the caller's frame buffers until then).
int fail_ctx(Ctx *c, int code, const std::string &msg);

inline size_t tsz(const Ctx *c) { return c->prec == ALEPPO_BF16 ? 2 : 4; }
// ---- memory.  Everything a context allocates goes through the helpers below, which register the pointer in
// c->owned_dev / c->owned_host; aleppo_destroy frees the two registries and NOTHING else frees.  A context only ever
// touches its OWN streams after aleppo_create: no null-stream operation, no hipFree, no hipDeviceSynchronize.  Those calls
// wait for (hipFree / hipHostFree / hipDeviceSynchronize) or are ordered against (null stream) other streams of the
// device - and another context's stream may be parked behind its release word, which only ITS owner thread lifts
// (the cause of the two-context hang of round 2).  So a buffer that is outgrown, or that a failed open leaves
// behind, simply stays in the registry until destroy.  On failure every helper leaves *p == nullptr.
enum AllocForm {
  ALLOC_RAW,   // plain hipMalloc
  ALLOC_ZEROED // at least 16 bytes, zero-filled on c->stream, and the fill waited for: a kernel on another stream of the
               // context could otherwise use the buffer first and have its results wiped afterwards (round 2: a late fill of
               // the ticket counter / the metric planes)
};
hipError_t ctx_alloc(Ctx *c, void **p, size_t bytes, AllocForm form);
hipError_t ctx_host_alloc(Ctx *c, void **p, size_t bytes, unsigned flags);
// a (pointer, capacity) pair grown on demand: nothing if need <= *cap, else a new buffer of `bytes` bytes and *cap = need
// (the units of the capacity are the site's); a failure leaves (nullptr, 0)
hipError_t ctx_grow(Ctx *c, void **p, size_t *cap, size_t need, size_t bytes, AllocForm form);
template <class T> hipError_t dalloc(Ctx *c, T **p, size_t bytes) {
  return ctx_alloc(c, reinterpret_cast<void **>(p), bytes, ALLOC_ZEROED);
}
template <class T> hipError_t halloc(Ctx *c, T **p, size_t bytes, unsigned flags) {
  return ctx_host_alloc(c, reinterpret_cast<void **>(p), bytes, flags);
}
template <class T> hipError_t grow(Ctx *c, T **p, size_t *cap, size_t need, size_t bytes, AllocForm form) {
  return ctx_grow(c, reinterpret_cast<void **>(p), cap, need, bytes, form);
}
template <class T> hipError_t grow(Ctx *c, T **p, size_t *cap, size_t bytes, AllocForm form) { // a capacity in bytes
  return ctx_grow(c, reinterpret_cast<void **>(p), cap, bytes, bytes, form);
}
// host <-> device copy on the context's main stream, complete when the call returns
hipError_t copy_sync(Ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind);

// a failure inside a helper that cannot return a status is kept in the context and reported by CHECK_ASYNC at the end of
// the entry point (never dropped)
inline void note(Ctx *c, hipError_t e) {
  if (e != hipSuccess && c->async_err == hipSuccess)
    c->async_err = e;
}
void prof_begin(Ctx *c, int cls, hipStream_t st = nullptr);
void prof_end(Ctx *c, int cls, hipStream_t st = nullptr); // same stream as the matching prof_begin

inline SampleMap train_map(const Ctx *c, long n0) {
  // sample n = e*T + t lives in slot (e, t) of obs [E][T+1][7056]
  return SampleMap{c->T, (long)(c->T + 1) * FRAME_PIX, (long)FRAME_PIX, 0, (int)n0};
}
inline SampleMap slot_map(const Ctx *c, int t) {
  return SampleMap{1, (long)(c->T + 1) * FRAME_PIX, 0, (long)t * FRAME_PIX, 0};
}

inline const float *Pf(const Ctx *c, ParamId id) { return c->P + c->L.off[id]; }
// element i of a rollout plane stored as RT (float or half)
inline void *rp(const Ctx *c, void *plane, size_t i) { return static_cast<char *>(plane) + i * c->rsz; }
inline const void *Pcw(const Ctx *c, ParamId id) {
  return static_cast<const char *>(c->Pc) + c->L.off[id] * tsz(c);
}
// The parameter set an acting forward reads: the fp32 vector (biases, heads) and its compute-type copy (convolution and fc
// weights), both in the internal layout.  The rollout's acting and the update use the live view; the evaluation lanes
// (eval_act_enqueue) use eval_view - the averaged set of aleppo_ema_open under ALEPPO_OPT_EVAL_PARAMS = 1.
struct ParamView {
  const float *P;
  const void *Pc;
};
inline ParamView live_view(const Ctx *c) { return ParamView{c->P, c->Pc}; }
inline ParamView eval_view(const Ctx *c) {
  return c->eval_averaged ? ParamView{c->averaged.P, c->averaged.Pc} : live_view(c);
}
inline const float *Pf(const Ctx *c, const ParamView &v, ParamId id) { return v.P + c->L.off[id]; }
inline const void *Pcw(const Ctx *c, const ParamView &v, ParamId id) {
  return static_cast<const char *>(v.Pc) + c->L.off[id] * tsz(c);
}

// conv stack forward for ns samples addressed by map -> c->h
// returns the number of split-K partial slabs of h (1 unless max_parts allows the pipelined fc kernel to split)
int net_forward(Ctx *c, const uint32_t *obs, SampleMap map, long ns, int max_parts = 1); // on the live parameters
int net_forward(Ctx *c, const ParamView &pv, const uint32_t *obs, SampleMap map, long ns, int max_parts = 1);
// the view of ALEPPO_SET_LIVE / _AVERAGED / _SNAPSHOT (aleppo_snapshot_take, aleppo_policy_diff): ALEPPO_ERR_RUNTIME for a
// set that does not exist yet, ALEPPO_ERR_INVALID_ARGUMENT for an unknown one; *view is written on success only
int set_view(aleppo_ctx *c, int set, ParamView *view);
// what a call refuses on a set that no take, import or open has filled yet (set_view, the exports, ALEPPO_OPT_EVAL_PARAMS)
constexpr const char *NO_AVERAGED = "no averaged parameters: call aleppo_ema_open first";
constexpr const char *NO_SNAPSHOT = "no snapshot: call aleppo_snapshot_take or aleppo_snapshot_import first";
constexpr const char *NO_ANCHOR = "no anchor: call aleppo_anchor_take or aleppo_anchor_import first";

// P was rewritten in place (aleppo_load_params, the recycle pass, aleppo_shrink_perturb): the compute copy and the packed
// dgrad weights are rebuilt on the main stream, and what aleppo_step pre-computed (pre_acted) and aleppo_tensor_stats'
// last step (ts_step_valid) are forgotten
void params_rewritten(Ctx *c);
// the acting scratch (a1 .. a3 / hpart) no longer holds the rollout's last acting forward on the parameters as they stand:
// aleppo_export_acting has nothing to read (net_forward, source_open, the update, params_rewritten, an imported rollout state)
inline void acted_clear(Ctx *c) { c->acted = Ctx::ActMark(); }
// a vector in the internal layout (device) -> the caller's flat array in the reference's order, with aleppo_export_params'
// count check; waits for the stream
int export_flat(aleppo_ctx *c, const float *dev, float *flat, size_t count);
// the reverse: `refusal` (ALEPPO_ERR_INVALID_ARGUMENT) unless flat holds the reference's element count, then the
// permutation, the stream's synchronise, a zero fill of each of zero_first (device vectors of L.total() floats) and the
// copy; complete when it returns.  A call that has more to refuse, or storage to allocate, checks the count itself first.
int upload_flat(aleppo_ctx *c, float *dev, const float *flat, size_t count, const char *refusal,
                std::initializer_list<float *> zero_first = {});
// ---- the stored parameter sets (ParamSet, common.hpp).  None of the helpers sets s->on: the entry point does, last.
// Storage on first use, zero-filled: the fp32 vector and - compute_copy - its copy in T, a second allocation in bf16
// contexts and an alias in fp32 ones (like Pc / P); *extra, where given, is allocated with them (aleppo_ema_open's
// block).  All or nothing: a failure ("<who>: allocation failed: ...") assigns nothing, and what was allocated stays in
// the registry until aleppo_destroy.  A set that has storage: nothing, and *extra is left alone.
int param_set_storage(aleppo_ctx *c, ParamSet *s, bool compute_copy, const char *who, void **extra = nullptr,
                      size_t extra_bytes = 0);
// s = src, device to device on the main stream (the compute copy only where s has one of its own)
int param_set_copy(aleppo_ctx *c, ParamSet *s, const ParamView &src);
// s = flat (upload_flat), then the cast into a compute copy of its own (enqueued)
int param_set_upload(aleppo_ctx *c, ParamSet *s, const float *flat, size_t count, const char *refusal);
// ALEPPO_ERR_RUNTIME with `none` while !s.on, else export_flat
int param_set_export(aleppo_ctx *c, const ParamSet &s, const char *none, float *flat, size_t count);
// api_ema.hip, also for aleppo_load_params: the average restarts at the live parameters (the set's copy, updates 0, the
// statistics of that state), enqueued on the main stream.  Call only where c->averaged has storage.
int ema_restart(aleppo_ctx *c);

// the permutation of aleppo.h (aleppo_read_sample_order), also what the keyed passes mix the caller's key with
inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

inline uint32_t float_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// clip_grad_norm_'s factor of the LAST optimizer step, as adam_kernel formed it: one fp32 quotient of the stored pre-clip
// norm and the limit that update ran with, clamped to 1 (aleppo_export_grads, aleppo_tensor_stats); 1 before any update
inline float last_clip_coef(const Ctx *c) {
  const size_t nm = (size_t)c->last_epochs * c->last_M;
  if (nm == 0)
    return 1.0f;
  const float norm = c->h_metric_red[nm * METRIC_REC + nm - 1];
  const float coef = c->last_max_norm / (norm + 1e-6f);
  return std::fmin(coef, 1.0f);
}

// the device the stateless operators and aleppo_create run on (process-default kernel switches)
int select_device(int ordinal);

// storage that more than one subsystem grows or reads.  api_train.hip: the per-sample metric planes (also the float
// staging of aleppo_set_batch's half planes) and ALEPPO_OPT_VALUE_CLIP's old-values plane; api_rollout.hip:
// ALEPPO_OPT_REWARD_SCALE's state
int ensure_metric_storage(aleppo_ctx *c, int epochs, int M, long B);
// api_batch.hip: NCHW uint8 observations of the caller -> c->stage_u8 (device)
int stage_observations(aleppo_ctx *c, const uint8_t *observations, int64_t n);
int ensure_val_storage(aleppo_ctx *c);
// ---- a source of samples for net_forward, checked and opened: the caller's observations staged into c->stage_obs (never
// the rollout's slots), or - null observations - samples of the batch the context holds, in place.  Every call that
// forwards samples outside the rollout and the update goes check -> open -> walk; nothing else sets a walk up by hand.
struct SampleSource {
  const uint32_t *obs = nullptr; // the packed stacks
  SampleMap map{};               // ... and where sample i of the source lies in them: map.n0 is the source's first sample
  long total = 0;                // samples
};
// The check refuses and enqueues nothing.  source_check: null observations need n == 0 and mean the whole batch, the
// caller's come n at a time, at most maxB (the messages are aleppo_activation_stats', the first of the callers).
// source_check_window (saliency): samples [first, first + n) of the batch, or n observations with first == 0.
int source_check(aleppo_ctx *c, const uint8_t *observations, int64_t n);
int source_check_window(aleppo_ctx *c, const uint8_t *observations, int64_t first, int64_t n);
// The open, arguments already checked: the stream's synchronise, pre_acted = -1 (a1 / a2 / a3 / h are shared scratch, and
// net_forward drops aleppo_export_backward's mark itself), then the upload and the pack of the caller's n observations,
// or the batch's slots from sample `first` (n == 0: all that follow).
int source_open(aleppo_ctx *c, const uint8_t *observations, int64_t first, int64_t n, SampleSource *src);
// The walk: chunks of at most maxB samples in order; body(map, n0, ns) -> int gets the map of samples [n0, n0 + ns) of
// the source, forwards them on whatever parameter sets it needs (net_forward(c, view, src.obs, map, ns)) and enqueues its
// pass over the activations; a non-zero return ends the walk and is returned.
template <class Body> int source_walk(aleppo_ctx *c, const SampleSource &src, Body body) {
  for (long n0 = 0; n0 < src.total; n0 += c->maxB) {
    const long ns = std::min(c->maxB, src.total - n0);
    SampleMap map = src.map;
    map.n0 += (int)n0;
    if (int rc = body(map, n0, ns))
      return rc;
  }
  return ALEPPO_OK;
}
// api_acts.hip, also for aleppo_recycle_dormant (api_recycle.hip): what aleppo_activation_stats refuses in tau, and the
// measurement itself with the arguments already checked - everything up to and including the finalising launch is
// enqueued, *units_dev / *layers_dev are the two tables in device memory
int act_stats_check_tau(aleppo_ctx *c, double tau);
int act_stats_measure(aleppo_ctx *c, const uint8_t *observations, int64_t n, double tau, const double **units_dev,
                      const double **layers_dev);
// api_rollout.hip, for aleppo_env_rollout (api_env.hip): slot `slot`'s acting kernels and head, and the GPU side of a step
// whose episode-start flags are bytes already in device memory (start_device)
int act_enqueue(aleppo_ctx *c, const float *noise, int slot);
// api_rollout.hip, also for the evaluation lanes (api_eval.hip): the acting forward up to the head (patch kernels, or
// conv1 -> conv2 -> conv3; then the split-K fc) at n samples into the given scratch, and where a kernel reads the
// caller's frames (*dev_frames; null for ALEPPO_HOST, which the caller stages itself)
void act_forward(aleppo_ctx *c, const ParamView &pv, uint32_t *obs, SampleMap map, void *a1, void *a2, void *a3,
                 float *hpart, int n, bool profiled);
int resolve_frames(aleppo_ctx *c, const uint8_t *frames, int location, const uint8_t **dev_frames);
int step_enqueue(aleppo_ctx *c, const uint8_t *df, int kind, int location, const StartBits *sb, const uint8_t *start_mapped,
                 int t, const uint8_t *start_device = nullptr);
// api_eval.hip, also for the device-resident evaluation (api_eval_env.hip): THE check of aleppo_eval_act's rule / param /
// noise (*kparam: what the head kernel takes), and one evaluation step's acting half - act_forward on the lanes' stacks,
// the evaluation head with device noise dn (or the built-in generator), then ev_ticket++ / ev_counter++
int eval_check_rule(aleppo_ctx *c, int rule, float param, bool has_noise, float *kparam);
int eval_act_enqueue(aleppo_ctx *c, int rule, float kparam, const float *dn);
// api_env.hip, also for api_eval_env.hip: the constructor's state of environment seed_base + e with start = 1 and reward 0,
// and what aleppo_env_import_state refuses in one environment's state (null: nothing)
void env_initial(const aleppo_env_config &cfg, std::vector<aleppo_env_state> &st);
const char *env_state_invalid(const aleppo_env_state &s);
// api_rec.hip, for aleppo_env_rollout / aleppo_eval_env_run: one step of `source` has just been enqueued up to and including
// its ingest - take the next row (the capture launch) or count the step as dropped, and advance the ordinal.  in: the state
// array the step's environment kernel READ; t: the rollout slot (ALEPPO_REC_ROLLOUT).  Call only where rec[source].open.
void rec_capture(aleppo_ctx *c, int source, const aleppo_env_state *in, int t);
// a step of `source` that the host drove: the ordinal advances, no row is taken
inline void rec_tick(Ctx *c, int source) {
  if (c->rec[source].open)
    c->rec[source].ordinal++;
}
// api_train.hip, for aleppo_grad_probe (api_grad_probe.hip): what aleppo_train's prologue and the gradient half of its
// minibatch (enqueue_gradient) enqueue for ONE contiguous minibatch of n samples from batch sample `first`, on the routes a
// minibatch of n samples takes, with the gradient landing in dst and conv1's slabs reduced into it.  Arguments already
// checked.  blk: the probe's device block (common.hpp GP_*), uploaded - its count and, with policy and
// ALEPPO_OPT_ADV_NORM_MINIBATCH, its advantage record are written here; !policy: the head goes through the
// advantage-record entry point and reads the record as uploaded.  ps: [8][maxB] per-sample planes.  Never a collective.
int grad_probe_enqueue(aleppo_ctx *c, long first, long n, bool policy, float *blk, float *ps, float *dst);
extern const double RS_INITIAL[RS_BLOCK];
int ensure_rs_storage(aleppo_ctx *c);
bool rs_state_valid(const double stats[3]);

} // namespace aleppo
