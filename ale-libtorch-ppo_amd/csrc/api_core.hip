// api_core.hip - C ABI (include/aleppo.h), the context itself: errors, kernel-selection switches, the parameter layout,
// the shared host helpers (api_internal.hpp), lifetime, parameter and optimizer I/O, communicator, options, profiling.
// Host-side orchestration only; every number is produced by a HIP kernel on the device - there is no CPU fallback (a
// missing device is ALEPPO_ERR_NO_DEVICE).
#include "api_internal.hpp"

using namespace aleppo;

namespace aleppo {

static thread_local std::string g_err;
int set_err(Ctx *c, int code, const std::string &msg) {
  if (c)
    c->err = msg;
  g_err = msg;
  return code;
}

// ------------------------------------------------------------------ per-context kernel-selection switches
static thread_local const Tuning *g_tuning = nullptr;
Tuning tuning_from_env() { // read once per context, in aleppo_create
  auto flag = [](const char *name, bool dflt) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) != 0 : dflt;
  };
  Tuning t;
  t.patch_conv = !flag("ALEPPO_GENERIC_CONV", false);
  t.fc_pipe = flag("ALEPPO_FC_PIPE", true);
  t.fused_fwd = flag("ALEPPO_FWD_FUSED", true);
  if (const char *e = std::getenv("ALEPPO_BWD_FUSED"))
    t.fused_bwd = std::atoi(e);
  if (const char *e = std::getenv("ALEPPO_FUSED_ACT"))
    t.fused_act = std::atoi(e);
  return t;
}
const Tuning &tuning() {
  static const Tuning dflt = tuning_from_env();
  return g_tuning ? *g_tuning : dflt;
}
void set_tuning(const Tuning *t) { g_tuning = t; }

// ------------------------------------------------------------------ parameter layout
static inline size_t align64(size_t x) { return (x + 63) / 64 * 64; }
void ParamLayout::init(int H_, int A_) {
  H = H_;
  A = A_;
  size[P_WH] = (size_t)(A + 1) * H;
  size[P_BH] = (size_t)A + 1;
  size[P_WFC] = (size_t)H * FC_IN;
  size[P_BFC] = (size_t)H;
  size[P_W3] = 64 * 576;
  size[P_B3] = 64;
  size[P_W2] = 64 * 512;
  size[P_B2] = 64;
  size[P_W1] = 32 * 256;
  size[P_B1] = 32;
  off[0] = 0;
  for (int i = 0; i < P_COUNT; ++i)
    off[i + 1] = off[i] + align64(size[i]);
  bucket0_end = off[P_W3];
}
size_t ParamLayout::reference_count() const {
  size_t n = 0;
  for (int i = 0; i < P_COUNT; ++i)
    n += size[i];
  return n;
}

// libtorch parameters() order: c1w[32,4,8,8] c1b c2w[64,32,4,4] c2b c3w[64,64,3,3] c3b fcw[H,3136] fcb aw[A,H] ab
// vw[1,H] vb.  Internal: conv weights [oc][(kh,kw,c)]; fc weight columns in (y,x,c) order (NHWC flatten) instead
// of libtorch's (c,y,x); heads stacked [A+1][H] (value head last).
template <bool TO_INTERNAL> static void permute_params(const ParamLayout &L, const float *src, float *dst) {
  const int H = L.H, A = L.A;
  size_t r = 0; // running reference offset
  auto conv = [&](int OC, int C, int KH, int KW, ParamId wid, ParamId bid) {
    const size_t wn = (size_t)OC * C * KH * KW;
    for (int oc = 0; oc < OC; ++oc)
      for (int c = 0; c < C; ++c)
        for (int kh = 0; kh < KH; ++kh)
          for (int kw = 0; kw < KW; ++kw) {
            const size_t ri = r + (((size_t)oc * C + c) * KH + kh) * KW + kw;
            const size_t ii = L.off[wid] + (size_t)oc * (KH * KW * C) + (size_t)(kh * KW + kw) * C + c;
            if (TO_INTERNAL)
              dst[ii] = src[ri];
            else
              dst[ri] = src[ii];
          }
    r += wn;
    for (int oc = 0; oc < OC; ++oc) {
      if (TO_INTERNAL)
        dst[L.off[bid] + oc] = src[r + oc];
      else
        dst[r + oc] = src[L.off[bid] + oc];
    }
    r += OC;
  };
  conv(32, 4, 8, 8, P_W1, P_B1);
  conv(64, 32, 4, 4, P_W2, P_B2);
  conv(64, 64, 3, 3, P_W3, P_B3);
  for (int o = 0; o < H; ++o)
    for (int c = 0; c < 64; ++c)
      for (int p = 0; p < 49; ++p) {
        const size_t ri = r + (size_t)o * FC_IN + c * 49 + p, ii = L.off[P_WFC] + (size_t)o * FC_IN + p * 64 + c;
        if (TO_INTERNAL)
          dst[ii] = src[ri];
        else
          dst[ri] = src[ii];
      }
  r += (size_t)H * FC_IN;
  auto lin = [&](size_t n, size_t ioff) {
    for (size_t i = 0; i < n; ++i) {
      if (TO_INTERNAL)
        dst[ioff + i] = src[r + i];
      else
        dst[r + i] = src[ioff + i];
    }
    r += n;
  };
  lin(H, L.off[P_BFC]);
  lin((size_t)A * H, L.off[P_WH]);          // action_head.weight
  lin(A, L.off[P_BH]);                      // action_head.bias
  lin(H, L.off[P_WH] + (size_t)A * H);      // value_head.weight
  lin(1, L.off[P_BH] + A);                  // value_head.bias
}
void params_to_internal(const ParamLayout &L, const float *ref, float *internal) {
  std::fill(internal, internal + L.total(), 0.0f);
  permute_params<true>(L, ref, internal);
}
void params_to_reference(const ParamLayout &L, const float *internal, float *ref) {
  permute_params<false>(L, internal, ref);
}

// ------------------------------------------------------------------ helpers (declared in api_internal.hpp)
// A failure after which the rollout / learner state is undefined: the context refuses every later call (sticky), any
// gate still on the stream is released so that the stream drains, and nothing is freed or reused before aleppo_destroy
// (kernels that are still queued may read the caller's frame buffers until then).
int fail_ctx(Ctx *c, int code, const std::string &msg) {
  c->failed = true;
  c->fail_msg = msg + " - the context is unusable: destroy it";
  c->armed = false;
  c->act_queued_slot = -1;
  if (c->h_go)
    __atomic_store_n(c->h_go, ~0ull, __ATOMIC_RELEASE);
  return set_err(c, code, c->fail_msg);
}

// host <-> device copy on the context's main stream, complete when the call returns
hipError_t copy_sync(Ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
  return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}
// memory: allocate and register; aleppo_destroy alone frees (why: api_internal.hpp)
hipError_t ctx_alloc(Ctx *c, void **p, size_t bytes, AllocForm form) {
  *p = nullptr;
  if (form == ALLOC_ZEROED && !bytes)
    bytes = 16;
  void *q = nullptr;
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess)
    return e;
  if (q)
    c->owned_dev.push_back(q);
  if (form == ALLOC_ZEROED) {
    e = hipMemsetAsync(q, 0, bytes, c->stream);
    if (e == hipSuccess)
      e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess)
      return e;
  }
  *p = q;
  return hipSuccess;
}
hipError_t ctx_host_alloc(Ctx *c, void **p, size_t bytes, unsigned flags) {
  *p = nullptr;
  void *q = nullptr;
  const hipError_t e = hipHostMalloc(&q, bytes, flags);
  if (e != hipSuccess)
    return e;
  if (q)
    c->owned_host.push_back(q);
  *p = q;
  return hipSuccess;
}
hipError_t ctx_grow(Ctx *c, void **p, size_t *cap, size_t need, size_t bytes, AllocForm form) {
  if (need <= *cap)
    return hipSuccess;
  *cap = 0;
  const hipError_t e = ctx_alloc(c, p, bytes, form);
  if (e == hipSuccess)
    *cap = need;
  return e;
}

void prof_begin(Ctx *c, int cls, hipStream_t st) {
  if (!c->prof_on)
    return;
  if (!st)
    st = c->stream;
  ProfClass &p = c->prof[cls];
  if (p.used == p.start.size()) {
    hipEvent_t a = nullptr, b = nullptr;
    note(c, hipEventCreate(&a));
    note(c, hipEventCreate(&b));
    p.start.push_back(a);
    p.stop.push_back(b);
  }
  note(c, hipEventRecord(p.start[p.used], st));
}
void prof_end(Ctx *c, int cls, hipStream_t st) { // same stream as the matching prof_begin
  if (!c->prof_on)
    return;
  if (!st)
    st = c->stream;
  ProfClass &p = c->prof[cls];
  note(c, hipEventRecord(p.stop[p.used], st));
  p.used++;
}

// conv stack forward for ns samples addressed by map -> c->h, on the parameter set pv
// returns the number of split-K partial slabs of h (1 unless max_parts allows the pipelined fc kernel to split)
int net_forward(Ctx *c, const ParamView &pv, const uint32_t *obs, SampleMap map, long ns, int max_parts) {
  c->bwd.B = 0; // a1 / a2 / a3 / h no longer hold an update's last minibatch (aleppo_train sets the mark after its last)
  acted_clear(c);
  if (c->prec == ALEPPO_BF16 && use_patch_kernels() && tuning().fused_fwd) { // one launch: a1 / a2 are only written
    prof_begin(c, ALEPPO_K_CONV_FWD);
    patch_fwd_fused(c->stream, obs, map, Pcw(c, pv, P_W1), Pf(c, pv, P_B1), Pcw(c, pv, P_W2), Pf(c, pv, P_B2),
                    Pcw(c, pv, P_W3), Pf(c, pv, P_B3), c->a1, c->a2, c->a3, ns);
    prof_end(c, ALEPPO_K_CONV_FWD);
    prof_begin(c, ALEPPO_K_FC_FWD);
    const int parts = fc_fwd(c->stream, c->prec, c->a3, Pcw(c, pv, P_WFC), Pf(c, pv, P_BFC), c->h, ns, c->H, max_parts);
    prof_end(c, ALEPPO_K_FC_FWD);
    return parts;
  }
  prof_begin(c, ALEPPO_K_CONV1_FWD);
  conv1_fwd(c->stream, c->prec, obs, map, Pcw(c, pv, P_W1), Pf(c, pv, P_B1), c->a1, ns);
  prof_end(c, ALEPPO_K_CONV1_FWD);
  prof_begin(c, ALEPPO_K_CONV2_FWD);
  conv2_fwd(c->stream, c->prec, c->a1, Pcw(c, pv, P_W2), Pf(c, pv, P_B2), c->a2, ns);
  prof_end(c, ALEPPO_K_CONV2_FWD);
  prof_begin(c, ALEPPO_K_CONV3_FWD);
  conv3_fwd(c->stream, c->prec, c->a2, Pcw(c, pv, P_W3), Pf(c, pv, P_B3), c->a3, ns);
  prof_end(c, ALEPPO_K_CONV3_FWD);
  prof_begin(c, ALEPPO_K_FC_FWD);
  const int parts = fc_fwd(c->stream, c->prec, c->a3, Pcw(c, pv, P_WFC), Pf(c, pv, P_BFC), c->h, ns, c->H, max_parts);
  prof_end(c, ALEPPO_K_FC_FWD);
  return parts;
}

int net_forward(Ctx *c, const uint32_t *obs, SampleMap map, long ns, int max_parts) {
  return net_forward(c, live_view(c), obs, map, ns, max_parts);
}

int set_view(aleppo_ctx *c, int set, ParamView *view) {
  switch (set) {
  case ALEPPO_SET_LIVE:
    *view = live_view(c);
    return ALEPPO_OK;
  case ALEPPO_SET_AVERAGED:
  case ALEPPO_SET_SNAPSHOT: { // (the anchor is never a view: fp32 only, never forwarded)
    const bool avg = set == ALEPPO_SET_AVERAGED;
    const ParamSet &s = avg ? c->averaged : c->snapshot;
    if (!s.on)
      return set_err(c, ALEPPO_ERR_RUNTIME, avg ? NO_AVERAGED : NO_SNAPSHOT);
    *view = ParamView{s.P, s.Pc};
    return ALEPPO_OK;
  }
  }
  return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "unknown parameter set (ALEPPO_SET_LIVE / _AVERAGED / _SNAPSHOT)");
}

void params_rewritten(Ctx *c) {
  if (c->prec == ALEPPO_BF16)
    launch_cast_params(c->stream, c->P, c->Pc, (long)c->L.total());
  launch_pack_dgrad(c->stream, c->P, c->L, c->W2d, c->W3d, c->WfcT, c->prec);
  c->pre_acted = -1;
  c->ts_step_valid = false;
  acted_clear(c);
}

int export_flat(aleppo_ctx *c, const float *dev, float *flat, size_t count) {
  if (!flat || count != c->L.reference_count())
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "export: wrong element count");
  std::vector<float> tmp(c->L.total());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, copy_sync(c, tmp.data(), dev, tmp.size() * 4, hipMemcpyDeviceToHost));
  params_to_reference(c->L, tmp.data(), flat);
  return ALEPPO_OK;
}
int upload_flat(aleppo_ctx *c, float *dev, const float *flat, size_t count, const char *refusal,
                std::initializer_list<float *> zero_first) {
  if (!flat || count != c->L.reference_count())
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, refusal);
  std::vector<float> tmp(c->L.total());
  params_to_internal(c->L, flat, tmp.data());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (float *z : zero_first)
    HIPCHK(c, hipMemsetAsync(z, 0, tmp.size() * 4, c->stream));
  HIPCHK(c, copy_sync(c, dev, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice)); // (own stream only: api_internal.hpp, memory)
  return ALEPPO_OK;
}

int param_set_storage(aleppo_ctx *c, ParamSet *s, bool compute_copy, const char *who, void **extra, size_t extra_bytes) {
  if (s->P)
    return ALEPPO_OK;
  const size_t n = c->L.total();
  const bool own_copy = compute_copy && c->prec == ALEPPO_BF16;
  float *p = nullptr;
  void *pc = nullptr, *x = nullptr;
  hipError_t e = dalloc(c, &p, n * 4);
  if (e == hipSuccess && own_copy)
    e = dalloc(c, &pc, n * 2);
  if (e == hipSuccess && extra)
    e = dalloc(c, &x, extra_bytes);
  if (e != hipSuccess)
    return set_err(c, ALEPPO_ERR_HIP, std::string(who) + ": allocation failed: " + hipGetErrorString(e));
  s->P = p;
  s->Pc = own_copy ? pc : compute_copy ? static_cast<void *>(p) : nullptr;
  if (extra)
    *extra = x;
  return ALEPPO_OK;
}
static bool own_compute_copy(const ParamSet &s) { return s.Pc && s.Pc != static_cast<const void *>(s.P); }
int param_set_copy(aleppo_ctx *c, ParamSet *s, const ParamView &src) {
  const size_t n = c->L.total();
  HIPCHK(c, hipMemcpyAsync(s->P, src.P, n * 4, hipMemcpyDeviceToDevice, c->stream));
  if (own_compute_copy(*s))
    HIPCHK(c, hipMemcpyAsync(s->Pc, src.Pc, n * 2, hipMemcpyDeviceToDevice, c->stream));
  return ALEPPO_OK;
}
int param_set_upload(aleppo_ctx *c, ParamSet *s, const float *flat, size_t count, const char *refusal) {
  if (int rc = upload_flat(c, s->P, flat, count, refusal))
    return rc;
  if (own_compute_copy(*s))
    launch_cast_params(c->stream, s->P, s->Pc, (long)c->L.total());
  return ALEPPO_OK;
}
int param_set_export(aleppo_ctx *c, const ParamSet &s, const char *none, float *flat, size_t count) {
  if (!s.on)
    return set_err(c, ALEPPO_ERR_RUNTIME, none);
  return export_flat(c, s.P, flat, count);
}

// ------------------------------------------------------------------ sample sources (api_internal.hpp)
int source_check(aleppo_ctx *c, const uint8_t *observations, int64_t n) {
  const bool batch = observations == nullptr;
  if (batch && n != 0)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "activation_stats: null observations need n == 0 (the context's batch)");
  if (!batch && (n <= 0 || n > c->maxB))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "activation_stats: n exceeds capacity");
  if (batch && c->batch_n <= 0)
    return set_err(c, ALEPPO_ERR_RUNTIME, "no batch: call aleppo_finish_rollout or aleppo_set_batch first");
  return ALEPPO_OK;
}
int source_check_window(aleppo_ctx *c, const uint8_t *observations, int64_t first, int64_t n) {
  if (!observations) {
    if (c->batch_n <= 0)
      return set_err(c, ALEPPO_ERR_RUNTIME, "no batch: call aleppo_finish_rollout or aleppo_set_batch first");
    if (first < 0 || n <= 0 || first > c->batch_n || n > c->batch_n - first)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "saliency: [first, first + n) must lie inside the batch");
  } else if (first != 0 || n <= 0 || n > c->maxB) {
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, first != 0 ? "saliency: first must be 0 with observations"
                                                              : "saliency: n exceeds capacity");
  }
  return ALEPPO_OK;
}
int source_open(aleppo_ctx *c, const uint8_t *observations, int64_t first, int64_t n, SampleSource *src) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->pre_acted = -1;
  acted_clear(c);
  if (!observations) { // sample n = e*T + t of the batch lives in slot (e, t) of obs
    *src = SampleSource{c->obs, train_map(c, (long)first), n ? (long)n : c->batch_n - (long)first};
    return ALEPPO_OK;
  }
  if (int rc = stage_observations(c, observations, n))
    return rc;
  HIPCHK(c, grow(c, &c->stage_obs, &c->stage_obs_cap, (size_t)n * FRAME_PIX * 4, ALLOC_RAW));
  *src = SampleSource{c->stage_obs, SampleMap{1, (long)FRAME_PIX, 0, 0, 0}, (long)n}; // sample i at stage_obs + i * 7056
  launch_obs_pack(c->stream, c->stage_u8, c->stage_obs, n, src->map);
  return ALEPPO_OK;
}

} // namespace aleppo

// ------------------------------------------------------------------ lifetime
extern "C" int aleppo_abi_version(void) { return ALEPPO_ABI_VERSION; }
extern "C" const char *aleppo_last_error(const aleppo_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

namespace aleppo {
int select_device(int ordinal) {
  set_tuning(nullptr); // (the stateless operators and aleppo_create run on the process defaults)
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return set_err(nullptr, ALEPPO_ERR_NO_DEVICE,
                   "no HIP device visible: libaleppo has no CPU fallback (needs an MI355X / gfx950)");
  if (ordinal < 0 || ordinal >= n)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "device_ordinal out of range");
  if (hipSetDevice(ordinal) != hipSuccess)
    return set_err(nullptr, ALEPPO_ERR_HIP, "hipSetDevice failed");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, ordinal) != hipSuccess)
    return set_err(nullptr, ALEPPO_ERR_HIP, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_err(nullptr, ALEPPO_ERR_NO_DEVICE,
                   std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  return ALEPPO_OK;
}
} // namespace aleppo

extern "C" int aleppo_device_check(int device_ordinal) { return select_device(device_ordinal); }

extern "C" int aleppo_create(const aleppo_config *cfg, aleppo_ctx **out) {
  if (!cfg || !out)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (cfg->abi_version != ALEPPO_ABI_VERSION)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "abi_version mismatch");
  // same checks as Rollout::Rollout (rollout.cc:48-59) where they apply
  if (cfg->num_envs <= 0)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "Total environments must be greater than 0.");
  if (cfg->num_envs > MAX_ENVS_PER_RANK)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "num_envs per rank must be <= 8192");
  if (cfg->horizon <= 0)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "Horizon must be greater than 0.");
  if (cfg->frame_stack != 4)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "frame_stack must be 4 (conv1 has 4 input channels)");
  if (cfg->num_actions < 1 || cfg->num_actions > MAX_ACTIONS)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "num_actions must be in [1,18]");
  if (cfg->hidden_size < 32 || cfg->hidden_size > 512 || cfg->hidden_size % 32)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "hidden_size must be a multiple of 32 in [32,512]");
  if (cfg->precision != ALEPPO_FP32 && cfg->precision != ALEPPO_BF16)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "precision must be ALEPPO_FP32 or ALEPPO_BF16");
  if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "bad world_size / rank");
  if (cfg->rollout_precision != ALEPPO_ROLLOUT_FP32 && cfg->rollout_precision != ALEPPO_ROLLOUT_FP16)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "rollout_precision must be ALEPPO_ROLLOUT_FP32 or _FP16");
  int rc = select_device(cfg->device_ordinal);
  if (rc)
    return rc;

  aleppo_ctx *c = new aleppo_ctx();
  c->cfg = *cfg;
  c->hyper = Hyper{cfg->clip_param, cfg->value_loss_coef, cfg->entropy_coef, cfg->max_gradient_norm};
  c->value_clip_range = cfg->clip_param;
  c->tune = tuning_from_env();
  set_tuning(&c->tune);
  if (c->cfg.adam_beta1 == 0.f)
    c->cfg.adam_beta1 = 0.9f;
  if (c->cfg.adam_beta2 == 0.f)
    c->cfg.adam_beta2 = 0.999f;
  if (c->cfg.adam_eps == 0.f)
    c->cfg.adam_eps = 1e-5f;
  c->E = cfg->num_envs;
  c->T = cfg->horizon;
  c->A = cfg->num_actions;
  c->H = cfg->hidden_size;
  c->prec = cfg->precision;
  c->world = cfg->world_size;
  c->rank = cfg->rank;
  c->N = (long)c->E * c->T;
  c->rt16 = cfg->rollout_precision == ALEPPO_ROLLOUT_FP16;
  c->rsz = c->rt16 ? 2 : 4;
  c->maxB = cfg->max_minibatch > 0 ? std::max<long>(cfg->max_minibatch, c->E) : std::max<long>(c->N, c->E);
  c->L.init(c->H, c->A);
  const int E = c->E, T = c->T, A = c->A, H = c->H;
  const size_t ts = tsz(c), PT = c->L.total();
#define CK(x)                                                                                                          \
  do {                                                                                                                 \
    hipError_t e_ = (x);                                                                                               \
    if (e_ != hipSuccess) {                                                                                            \
      set_err(nullptr, ALEPPO_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));                               \
      aleppo_destroy(c);                                                                                               \
      return ALEPPO_ERR_HIP;                                                                                           \
    }                                                                                                                  \
  } while (0)
  CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  // (the update's two side streams are created by the first aleppo_train: a context that only acts holds ONE stream.
  // The runtime multiplexes streams onto GPU_MAX_HW_QUEUES - default 4 - hardware queues, and a kernel that lands in the
  // queue of another context's parked stream waits behind its gate: tests/tools/parkprobe.hip)
  CK(hipEventCreateWithFlags(&c->ev_bucket0, hipEventDisableTiming));
  CK(hipEventCreateWithFlags(&c->ev_comm0, hipEventDisableTiming));
  CK(hipEventCreateWithFlags(&c->ev_tmp, hipEventDisableTiming));
  for (hipEvent_t *e : {&c->ev_head, &c->ev_dz3, &c->ev_dz2, &c->ev_wg})
    CK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  CK(dalloc(c, &c->obs, (size_t)E * (T + 1) * FRAME_PIX * 4));
  c->step_rec_bytes = ((size_t)7 * E + 15) / 16 * 16;
  CK(dalloc(c, &c->step_rec, c->step_rec_bytes * T));
  CK(dalloc(c, &c->values_tm, (size_t)(T + 1) * E * c->rsz));
  CK(dalloc(c, &c->logits_tm, (size_t)(T + 1) * E * A * c->rsz));
  CK(dalloc(c, &c->actions_tm, (size_t)(T + 1) * E * 4));
  CK(dalloc(c, &c->lut, 256));
  CK(dalloc(c, &c->d_start, (size_t)E));
  CK(dalloc(c, &c->d_frames, (size_t)E * 2 * RAW_H * RAW_W));
  CK(dalloc(c, &c->d_noise, (size_t)2 * E * A * 4));
  CK(dalloc(c, &c->d_err, 16));
  CK(dalloc(c, &c->d_done, 16));
  {
    uint8_t ident[256];
    for (int i = 0; i < 256; ++i)
      ident[i] = (uint8_t)i;
    CK(copy_sync(c, c->lut, ident, 256, hipMemcpyHostToDevice));
  }
  CK(halloc(c, &c->h_actions, (size_t)(E + 8) * 8, hipHostMallocMapped));
  CK(halloc(c, &c->h_step, c->step_rec_bytes + E, hipHostMallocDefault));
  CK(halloc(c, &c->h_rec, c->step_rec_bytes * T, hipHostMallocDefault));
  std::memset(c->h_rec, 0, c->step_rec_bytes * T);
  CK(halloc(c, &c->h_frames, (size_t)E * 2 * RAW_H * RAW_W, hipHostMallocDefault));
  CK(halloc(c, &c->h_noise, (size_t)2 * E * A * 4, hipHostMallocDefault));
  CK(halloc(c, &c->h_go, 64, hipHostMallocMapped));
  std::memset(c->h_go, 0, 64);
  {
    // exit condition of the slot-ahead gate (gate_kernel): an emulator step takes milliseconds, so two minutes mean the
    // host is gone.  ALEPPO_GATE_TIMEOUT_MS / ALEPPO_OPT_GATE_TIMEOUT_MS change it (the tests use 100 ms).
    const char *e = std::getenv("ALEPPO_GATE_TIMEOUT_MS");
    const double ms = e ? std::max(1.0, std::atof(e)) : 120000.0;
    c->gate_timeout_ticks = (unsigned long long)(ms * 1e5); // 100 MHz wall clock
  }
  CK(halloc(c, &c->h_err, 16, hipHostMallocDefault));
  std::memset(c->h_actions, 0, (size_t)(E + 8) * 8);
  CK(dalloc(c, &c->adv_n, (size_t)c->N * c->rsz));
  CK(dalloc(c, &c->ret_n, (size_t)c->N * c->rsz));
  CK(dalloc(c, &c->oldlp_n, (size_t)c->N * A * c->rsz));
  CK(dalloc(c, &c->act_n, (size_t)c->N * 4));
  CK(dalloc(c, &c->mask_n, (size_t)c->N));
  CK(dalloc(c, &c->mask_counts, 4096 * 4));
  CK(dalloc(c, &c->P, PT * 4));
  CK(dalloc(c, &c->G, PT * 4));
  CK(dalloc(c, &c->M1, PT * 4));
  CK(dalloc(c, &c->M2, PT * 4));
  if (c->prec == ALEPPO_BF16)
    CK(dalloc(c, &c->Pc, PT * 2));
  else
    c->Pc = c->P; // (an alias: never registered)
  CK(dalloc(c, &c->W2d, (size_t)4 * 32 * 256 * ts));
  CK(dalloc(c, &c->W3d, (size_t)64 * 576 * ts));
  CK(dalloc(c, &c->WfcT, (size_t)FC_IN * H * ts));
  const size_t mb = (size_t)c->maxB;
  CK(dalloc(c, &c->a1, mb * A1_PIX * A1_C * ts));
  CK(dalloc(c, &c->a2, mb * A2_PIX * A2_C * ts));
  CK(dalloc(c, &c->a3, mb * FC_IN * ts));
  CK(dalloc(c, &c->dz1, mb * A1_PIX * A1_C * ts));
  CK(dalloc(c, &c->dz2, mb * A2_PIX * A2_C * ts));
  CK(dalloc(c, &c->dz3, mb * FC_IN * ts));
  CK(dalloc(c, &c->h, (size_t)FC_FWD_MAX_PARTS * mb * H * 4)); // up to FC_FWD_MAX_PARTS split-K slabs
  CK(dalloc(c, &c->hpart, (size_t)FC_SPLITS * E * H * 4));
  CK(dalloc(c, &c->dh, mb * H * ts));
  CK(dalloc(c, &c->logits_b, mb * A * 4));
  CK(dalloc(c, &c->values_b, mb * 4));
  // slabs: [W1|b1|W2|b2|W3|b3|Wfc|bfc|Wh|bh]
  c->slab_off[0] = 0;
  const size_t sl[10] = {(size_t)MAXS_C1 * 32 * 256,       (size_t)MAXS_C1 * 32, (size_t)MAXS_C2 * 64 * 512,
                         (size_t)MAXS_C2 * 64,              (size_t)MAXS_C3 * 64 * 576, (size_t)MAXS_C3 * 64,
                         (size_t)MAXS_FC * H * FC_IN,       (size_t)MAXS_HEAD * H, (size_t)MAXS_HEAD * (A + 1) * H,
                         (size_t)MAXS_HEAD * (A + 1)};
  for (int i = 0; i < 10; ++i)
    c->slab_off[i + 1] = c->slab_off[i] + align64(sl[i]);
  c->slab_floats = c->slab_off[10];
  CK(dalloc(c, &c->slab, c->slab_floats * 4));
  CK(dalloc(c, &c->sumsq_part, 1024 * 4));
  CK(dalloc(c, &c->adv_stats, 64));
  // the hyper-parameter block of ALEPPO_OPT_CLIP_PARAM and its kin, filled and uploaded at each aleppo_train
  CK(dalloc(c, &c->hyper_blk, HYPER_BLOCK * 4));
  CK(halloc(c, &c->h_hyper_blk, HYPER_BLOCK * 4, hipHostMallocDefault));
  CK(hipStreamSynchronize(c->stream)); // (own streams only: api_internal.hpp, memory)
#undef CK
  *out = c;
  return ALEPPO_OK;
}

extern "C" void aleppo_destroy(aleppo_ctx *c) {
  if (!c)
    return;
  set_tuning(nullptr);
  (void)hipSetDevice(c->cfg.device_ordinal);
  if (c->h_go) // an armed step parks the stream on the release word: let it go before waiting for it
    __atomic_store_n(c->h_go, ~0ull, __ATOMIC_RELEASE);
  for (hipStream_t st : {c->wg_stream, c->comm_stream, c->stream})
    if (st)
      hipStreamSynchronize(st);
  // From here on hipFree / hipHostFree: each waits for every stream of the device.  If another context of this process
  // has a step armed on another thread, that wait lasts until its owner releases it (never call aleppo_destroy from the
  // thread that owns an armed context: INTEGRATION.md, threading).
  if (c->graph_exec)
    hipGraphExecDestroy(c->graph_exec);
  if (c->graph)
    hipGraphDestroy(c->graph);
  if (c->nccl_comm)
    ncclCommDestroy(static_cast<ncclComm_t>(c->nccl_comm));
  for (void *p : c->owned_dev)
    hipFree(p);
  for (void *p : c->owned_host)
    hipHostFree(p);
  for (auto &pc : c->prof)
    for (size_t i = 0; i < pc.start.size(); ++i) {
      hipEventDestroy(pc.start[i]);
      hipEventDestroy(pc.stop[i]);
    }
  for (size_t i = 0; i < c->env_prof.start.size(); ++i) {
    hipEventDestroy(c->env_prof.start[i]);
    hipEventDestroy(c->env_prof.stop[i]);
  }
  for (hipEvent_t e : {c->ev_bucket0, c->ev_comm0, c->ev_tmp, c->ev_head, c->ev_dz3, c->ev_dz2, c->ev_wg,
                       c->ev_staged})
    if (e)
      hipEventDestroy(e);
  if (c->stream)
    hipStreamDestroy(c->stream);
  if (c->comm_stream)
    hipStreamDestroy(c->comm_stream);
  if (c->wg_stream)
    hipStreamDestroy(c->wg_stream);
  delete c;
}

extern "C" int aleppo_synchronize(aleppo_ctx *c) {
  CHECK_CTX(c);
  for (hipStream_t st : {c->wg_stream, c->comm_stream, c->stream})
    if (st)
      HIPCHK(c, hipStreamSynchronize(st));
  return ALEPPO_OK;
}

// ------------------------------------------------------------------ parameters
extern "C" int aleppo_param_count(const aleppo_ctx *c, size_t *count) {
  CHECK_CTX(c);
  if (!count)
    return ALEPPO_ERR_INVALID_ARGUMENT;
  *count = c->L.reference_count();
  return ALEPPO_OK;
}
extern "C" int aleppo_load_params(aleppo_ctx *c, const float *flat, size_t count) {
  CHECK_CTX(c);
  if (int rc = upload_flat(c, c->P, flat, count, "load_params: wrong element count", {c->M1, c->M2, c->G}))
    return rc;
  c->adam_step = 0;
  params_rewritten(c);
  if (c->averaged.on) // the average restarts at the loaded parameters, as Adam does
    if (int rc = ema_restart(c))
      return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ALEPPO_OK;
}
extern "C" int aleppo_export_params(aleppo_ctx *c, float *flat, size_t count) {
  CHECK_CTX(c);
  return export_flat(c, c->P, flat, count);
}
extern "C" int aleppo_export_grads(aleppo_ctx *c, float *flat, size_t count) {
  CHECK_CTX(c);
  // clip_grad_norm_ scales in place (train.cc:42-44); the Adam kernel applies the same factor on the fly and leaves G as the
  // backward pass produced it (a separate scaled copy cost 4 bytes per parameter and optimizer step).  The factor is one
  // fp32 product of the stored pre-clip norm: applied here it gives the bits the kernel multiplied into its update.
  const int rc = export_flat(c, c->G, flat, count);
  if (rc || c->last_epochs * c->last_M == 0)
    return rc;
  const float coef = last_clip_coef(c); // (with the limit that update ran with)
  for (size_t i = 0; i < count; ++i)
    flat[i] *= coef;
  return ALEPPO_OK;
}

extern "C" int aleppo_export_optimizer(aleppo_ctx *c, float *exp_avg, float *exp_avg_sq, int64_t *step,
                                       size_t count) {
  CHECK_CTX(c);
  if (!step)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null step");
  int rc = export_flat(c, c->M1, exp_avg, count);
  if (rc)
    return rc;
  rc = export_flat(c, c->M2, exp_avg_sq, count);
  if (rc)
    return rc;
  *step = c->adam_step;
  return ALEPPO_OK;
}
extern "C" int aleppo_import_optimizer(aleppo_ctx *c, const float *exp_avg, const float *exp_avg_sq, int64_t step,
                                       size_t count) {
  CHECK_CTX(c);
  static const char *const refusal = "import_optimizer: bad argument";
  if (!exp_avg || !exp_avg_sq || count != c->L.reference_count() || step < 0) // (before the first moment is written)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, refusal);
  if (int rc = upload_flat(c, c->M1, exp_avg, count, refusal))
    return rc;
  if (int rc = upload_flat(c, c->M2, exp_avg_sq, count, refusal))
    return rc;
  c->adam_step = step;
  c->ts_step_valid = false; // (aleppo_tensor_stats: these moments are not the last step's)
  return ALEPPO_OK;
}

extern "C" int aleppo_host_alloc(aleppo_ctx *c, size_t bytes, void **ptr) {
  CHECK_CTX(c);
  if (!ptr || bytes == 0)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "host_alloc: bad argument");
  *ptr = nullptr;
  HIPCHK(c, hipHostMalloc(ptr, bytes, hipHostMallocMapped));
  std::memset(*ptr, 0, bytes);
  return ALEPPO_OK;
}
extern "C" int aleppo_host_free(aleppo_ctx *c, void *ptr) {
  CHECK_CTX(c);
  if (!ptr)
    return ALEPPO_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream)); // a kernel may still be reading it
  HIPCHK(c, hipHostFree(ptr));
  return ALEPPO_OK;
}

// ------------------------------------------------------------------ multi-GPU
extern "C" int aleppo_comm_unique_id(uint8_t id[ALEPPO_UNIQUE_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) == ALEPPO_UNIQUE_ID_BYTES, "unique id size");
  ncclUniqueId u;
  ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess)
    return set_err(nullptr, ALEPPO_ERR_HIP, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  std::memcpy(id, &u, sizeof(u));
  return ALEPPO_OK;
}
extern "C" int aleppo_comm_init(aleppo_ctx *c, const uint8_t id[ALEPPO_UNIQUE_ID_BYTES]) {
  CHECK_CTX(c);
  if (c->nccl_comm)
    return set_err(c, ALEPPO_ERR_RUNTIME, "communicator already initialised");
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  HIPCHK(c, hipSetDevice(c->cfg.device_ordinal));
  ncclComm_t comm;
  NCCLCHK(c, ncclCommInitRank(&comm, c->world, u, c->rank));
  c->nccl_comm = comm;
  return ALEPPO_OK;
}

// ------------------------------------------------------------------ options, profiling
extern "C" int aleppo_set_option(aleppo_ctx *c, int option, int value) {
  CHECK_CTX(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // a captured update holds the kernels the switches selected when it was recorded: any change re-arms the capture -
  // except beta (ALEPPO_OPT_KL_COEF) and the five hyper-parameter options, device values uploaded at each aleppo_train,
  // which a replay reads as they are
  const bool hyper_opt = option == ALEPPO_OPT_CLIP_PARAM || option == ALEPPO_OPT_VALUE_CLIP_RANGE ||
                         option == ALEPPO_OPT_VALUE_LOSS_COEF || option == ALEPPO_OPT_ENTROPY_COEF ||
                         option == ALEPPO_OPT_MAX_GRAD_NORM;
  // (the two reward-scaling options are read by aleppo_finish_rollout alone: the update does not see them)
  const bool rollout_opt = option == ALEPPO_OPT_REWARD_SCALE || option == ALEPPO_OPT_REWARD_SCALE_CLIP;
  // (nor does ALEPPO_OPT_EVAL_PARAMS, which the evaluation lanes read alone)
  // ALEPPO_OPT_WEIGHT_DECAY / ALEPPO_OPT_ANCHOR_COEF are device values too; what they select - adam_kernel where both are zero,
  // reg_step_kernel otherwise - is part of the graph key (api_train.hip), so only a change of that choice re-arms the capture
  const bool reg_opt = option == ALEPPO_OPT_WEIGHT_DECAY || option == ALEPPO_OPT_ANCHOR_COEF;
  if (option != ALEPPO_OPT_KL_COEF && !hyper_opt && !rollout_opt && !reg_opt && option != ALEPPO_OPT_EVAL_PARAMS) {
    c->graph_key = Ctx::GraphKey();
    c->warm_key = Ctx::GraphKey();
  }
  if (option == ALEPPO_OPT_GENERIC_CONV)
    c->tune.patch_conv = value == 0;
  else if (option == ALEPPO_OPT_FC_PIPE)
    c->tune.fc_pipe = value != 0;
  else if (option == ALEPPO_OPT_FUSED_ACT)
    c->tune.fused_act = value; // 0: never, 1: where it is faster (default), 2: always
  else if (option == ALEPPO_OPT_FUSED_FWD)
    c->tune.fused_fwd = value != 0;
  else if (option == ALEPPO_OPT_ACT_STORE) {
    if (value != 0 && value != 1)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "ALEPPO_OPT_ACT_STORE: 0 (off) or 1 (the fused acting launch also stores conv1 / conv2)");
    c->act_store = value != 0;
  }
  else if (option == ALEPPO_OPT_FUSED_BWD)
    c->tune.fused_bwd = value; // 0: never, 1: at minibatches >= 2048 samples (default), 2: always
  else if (option == ALEPPO_OPT_DEBUG_NO_PUBLISH)
    c->dbg_no_publish = value != 0;
  else if (option == ALEPPO_OPT_SERIAL_UPDATE)
    c->serial_update = value != 0;
  else if (option == ALEPPO_OPT_FORCE_COMM)
    c->force_comm = value != 0;
  else if (option == ALEPPO_OPT_MINIBATCH_SHUFFLE)
    c->shuffle = value != 0;
  else if (option == ALEPPO_OPT_VALUE_CLIP) {
    if (value != 0 && value != 1)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "ALEPPO_OPT_VALUE_CLIP: 0 (off) or 1 (clip at config.clip_param)");
    c->value_clip = value != 0;
  } else if (option == ALEPPO_OPT_ADV_NORM_MINIBATCH) {
    if (value != 0 && value != 1)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "ALEPPO_OPT_ADV_NORM_MINIBATCH: 0 (off) or 1 (normalise each minibatch's advantages)");
    c->adv_norm_mb = value != 0;
  } else if (option == ALEPPO_OPT_KL_PENALTY) {
    if (value != 0 && value != 1)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "ALEPPO_OPT_KL_PENALTY: 0 (off) or 1 (exact KL, beta KL added to the loss)");
    c->kl_pen = value != 0;
  } else if (option == ALEPPO_OPT_REWARD_SCALE) {
    if (value != 0 && value != 1)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "ALEPPO_OPT_REWARD_SCALE: 0 (clamp to [-1, 1]) or 1 (divide by the running return's std, clip)");
    c->reward_scale = value != 0;
  } else if (option == ALEPPO_OPT_REWARD_SCALE_CLIP) {
    if (value < 1 || value >= 0x7F800000) // the bits of a finite float > 0: see ALEPPO_OPT_KL_COEF below
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "ALEPPO_OPT_REWARD_SCALE_CLIP: the binary32 bits of a finite float > 0 (not zero, Inf or NaN)");
    const uint32_t bits = (uint32_t)value;
    std::memcpy(&c->reward_scale_clip, &bits, 4);
  } else if (option == ALEPPO_OPT_KL_COEF) {
    // the bit pattern of a finite non-negative float: [0, 0x7F800000) (-0.0 and every negative float or NaN have the
    // sign bit set and are negative as an int; +Inf is 0x7F800000 and the positive NaNs lie above it)
    if (value < 0 || value >= 0x7F800000)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "ALEPPO_OPT_KL_COEF: the binary32 bits of a finite non-negative float (not -0.0, Inf or NaN)");
    c->kl_coef_bits = (uint32_t)value;
  } else if (reg_opt) {
    if (value < 0 || value >= 0x7F800000) // as for ALEPPO_OPT_KL_COEF
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "ALEPPO_OPT_WEIGHT_DECAY / ALEPPO_OPT_ANCHOR_COEF: the binary32 bits of a finite non-negative float "
                     "(not -0.0, Inf or NaN)");
    (option == ALEPPO_OPT_WEIGHT_DECAY ? c->wd_bits : c->anchor_coef_bits) = (uint32_t)value;
  } else if (hyper_opt) {
    // the bits of a finite float, > 0 or (the two coefficients) >= 0: as an int, [1 or 0, 0x7F800000) - see above
    const bool zero_ok = option == ALEPPO_OPT_VALUE_LOSS_COEF || option == ALEPPO_OPT_ENTROPY_COEF;
    if (value < (zero_ok ? 0 : 1) || value >= 0x7F800000)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     zero_ok ? "ALEPPO_OPT_VALUE_LOSS_COEF / ALEPPO_OPT_ENTROPY_COEF: the binary32 bits of a finite "
                               "non-negative float (not -0.0, Inf or NaN)"
                             : "ALEPPO_OPT_CLIP_PARAM / ALEPPO_OPT_VALUE_CLIP_RANGE / ALEPPO_OPT_MAX_GRAD_NORM: the "
                               "binary32 bits of a finite float > 0 (not zero, Inf or NaN)");
    float f;
    const uint32_t bits = (uint32_t)value;
    std::memcpy(&f, &bits, 4);
    if (option == ALEPPO_OPT_CLIP_PARAM)
      c->hyper.clip = f;
    else if (option == ALEPPO_OPT_VALUE_CLIP_RANGE) {
      c->value_clip_range = f;
      c->vclip_range_set = true;
    } else if (option == ALEPPO_OPT_VALUE_LOSS_COEF)
      c->hyper.c_v = f;
    else if (option == ALEPPO_OPT_ENTROPY_COEF)
      c->hyper.c_e = f;
    else
      c->hyper.max_norm = f;
  } else if (option == ALEPPO_OPT_EVAL_PARAMS) {
    if (value != 0 && value != 1)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "ALEPPO_OPT_EVAL_PARAMS: 0 (the live parameters) or 1 (the averaged set of aleppo_ema_open)");
    if (value == 1 && !c->averaged.on)
      return set_err(c, ALEPPO_ERR_RUNTIME, std::string("ALEPPO_OPT_EVAL_PARAMS: ") + NO_AVERAGED);
    c->eval_averaged = value != 0;
  } else if (option == ALEPPO_OPT_UPDATE_GRAPH)
    c->update_graph = value != 0;
  else if (option == ALEPPO_OPT_GATE_TIMEOUT_MS)
    c->gate_timeout_ticks = (unsigned long long)std::max(1, value) * 100000ull; // 100 MHz wall clock
  else
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "unknown option");
  return ALEPPO_OK;
}
extern "C" int aleppo_get_option(aleppo_ctx *c, int option, int64_t *value) {
  CHECK_CTX(c);
  if (!value)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null value");
  switch (option) {
  case ALEPPO_OPT_GENERIC_CONV: *value = c->tune.patch_conv ? 0 : 1; break;
  case ALEPPO_OPT_DEBUG_NO_PUBLISH: *value = c->dbg_no_publish; break;
  case ALEPPO_OPT_FORCE_COMM: *value = c->force_comm; break;
  case ALEPPO_OPT_SERIAL_UPDATE: *value = c->serial_update; break;
  case ALEPPO_OPT_FC_PIPE: *value = c->tune.fc_pipe; break;
  case ALEPPO_OPT_FUSED_ACT: *value = c->tune.fused_act; break;
  case ALEPPO_OPT_FUSED_FWD: *value = c->tune.fused_fwd; break;
  case ALEPPO_OPT_ACT_STORE: *value = c->act_store; break;
  case ALEPPO_OPT_FUSED_BWD: *value = c->tune.fused_bwd; break;
  case ALEPPO_OPT_UPDATE_GRAPH: *value = c->graph_replays; break;
  case ALEPPO_OPT_MINIBATCH_SHUFFLE: *value = c->shuffle; break;
  case ALEPPO_OPT_VALUE_CLIP: *value = c->value_clip; break;
  case ALEPPO_OPT_ADV_NORM_MINIBATCH: *value = c->adv_norm_mb; break;
  case ALEPPO_OPT_KL_PENALTY: *value = c->kl_pen; break;
  case ALEPPO_OPT_KL_COEF: *value = (int64_t)c->kl_coef_bits; break;
  case ALEPPO_OPT_CLIP_PARAM: *value = (int64_t)float_bits(c->hyper.clip); break;
  case ALEPPO_OPT_VALUE_CLIP_RANGE:
    *value = (int64_t)float_bits(c->vclip_range_set ? c->value_clip_range : c->hyper.clip);
    break;
  case ALEPPO_OPT_VALUE_LOSS_COEF: *value = (int64_t)float_bits(c->hyper.c_v); break;
  case ALEPPO_OPT_ENTROPY_COEF: *value = (int64_t)float_bits(c->hyper.c_e); break;
  case ALEPPO_OPT_MAX_GRAD_NORM: *value = (int64_t)float_bits(c->hyper.max_norm); break;
  case ALEPPO_OPT_GATE_TIMEOUT_MS: *value = (int64_t)(c->gate_timeout_ticks / 100000ull); break;
  case ALEPPO_OPT_REWARD_SCALE: *value = c->reward_scale; break;
  case ALEPPO_OPT_REWARD_SCALE_CLIP: *value = (int64_t)float_bits(c->reward_scale_clip); break;
  case ALEPPO_OPT_EVAL_PARAMS: *value = c->eval_averaged; break;
  case ALEPPO_OPT_WEIGHT_DECAY: *value = (int64_t)c->wd_bits; break;
  case ALEPPO_OPT_ANCHOR_COEF: *value = (int64_t)c->anchor_coef_bits; break;
  default: return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "unknown option");
  }
  return ALEPPO_OK;
}
extern "C" int aleppo_profile_enable(aleppo_ctx *c, int on) {
  CHECK_CTX(c);
  c->prof_on = on != 0;
  return ALEPPO_OK;
}
extern "C" int aleppo_profile_reset(aleppo_ctx *c) {
  CHECK_CTX(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (auto &p : c->prof)
    p.used = 0;
  c->env_prof.used = 0;
  return ALEPPO_OK;
}
extern "C" int aleppo_profile_read(aleppo_ctx *c, int cls, double *avg_ms, int64_t *launches) {
  CHECK_CTX(c);
  if (cls < 0 || cls >= ALEPPO_K_COUNT || !avg_ms || !launches)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "profile_read: bad argument");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ProfClass &p = c->prof[cls];
  double tot = 0;
  for (size_t i = 0; i < p.used; ++i) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, p.start[i], p.stop[i]));
    tot += ms;
  }
  *launches = (int64_t)p.used;
  *avg_ms = p.used ? tot / (double)p.used : 0.0;
  return ALEPPO_OK;
}
