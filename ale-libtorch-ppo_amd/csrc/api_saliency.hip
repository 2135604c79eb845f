// api_saliency.hip - C ABI (include/aleppo.h), perturbation saliency: aleppo_saliency_tables, aleppo_saliency,
// aleppo_saliency_perturbed.  The two stateful calls open a SampleSource (api_internal.hpp) over a window of the
// batch or the caller's observations, walk it for the unperturbed outputs, and only read the learner; what they write is their own
// staging, the shared activation scratch and logits_b / values_b.
#include "api_internal.hpp"

using namespace aleppo;

static const aleppo_saliency_config SAL_DEFAULT = {5, 15, 5.0, 3.0};

// nullptr: valid; else what is wrong
static const char *sal_config_invalid(const aleppo_saliency_config &k) {
  if (k.stride < 2 || k.stride > 84)
    return "saliency: stride must be in [2, 84]";
  if (!(k.sigma_mask >= 0.5 && k.sigma_mask <= 16.0))
    return "saliency: sigma_mask must be in [0.5, 16]";
  if (!(k.sigma_blur >= 0.5 && k.sigma_blur <= 10.0))
    return "saliency: sigma_blur must be in [0.5, 10]";
  if (k.planes < 1 || k.planes > 15)
    return "saliency: planes must be in [1, 15]";
  return nullptr;
}

// the two tables of a valid config, in double (aleppo.h)
static void sal_tables(const aleppo_saliency_config &k, uint16_t g[84], uint16_t w[84], int32_t *radius) {
  for (int i = 0; i < 84; ++i)
    g[i] = (uint16_t)std::rint(4096.0 * std::exp(-(double)(i * i) / (2.0 * k.sigma_mask * k.sigma_mask)));
  const int R = (int)(4.0 * k.sigma_blur + 0.5);
  double e[84] = {0.0}, sum = 0.0;
  for (int j = 0; j <= R; ++j)
    e[j] = std::exp(-(double)(j * j) / (2.0 * k.sigma_blur * k.sigma_blur));
  for (int j = -R; j <= R; ++j) // in the order j = -R .. R
    sum += e[j < 0 ? -j : j];
  long total = 0;
  for (int j = 0; j < 84; ++j) {
    w[j] = j <= R ? (uint16_t)std::rint(4096.0 * e[j] / sum) : (uint16_t)0;
    total += (j == 0 ? 1 : 2) * (long)w[j];
  }
  w[0] = (uint16_t)((long)w[0] + 4096 - total); // the centre tap takes the rounding residue: the taps add up to 4096
  *radius = R;
}

extern "C" int aleppo_saliency_tables(const aleppo_saliency_config *cfg, uint16_t mask_g[84], uint16_t blur_w[84],
                                      int32_t *radius) {
  const aleppo_saliency_config k = cfg ? *cfg : SAL_DEFAULT;
  if (const char *bad = sal_config_invalid(k))
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, bad);
  if (!mask_g || !blur_w || !radius)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "saliency_tables: null argument");
  uint16_t g[84], w[84];
  int32_t R = 0;
  sal_tables(k, g, w, &R);
  std::memcpy(mask_g, g, sizeof(g));
  std::memcpy(blur_w, w, sizeof(w));
  *radius = R;
  return ALEPPO_OK;
}

namespace {
struct SalCall { // a checked call: the parameters, the grid and - once opened - where the samples are
  aleppo_saliency_config k;
  SalTables tb;
  int G = 0, P = 0;
  SampleSource src;
};

// what both calls refuse in cfg and in their source of samples (nothing is enqueued or written)
int sal_check(aleppo_ctx *c, const uint8_t *observations, int64_t first, int64_t n, const aleppo_saliency_config *cfg,
              SalCall *call) {
  call->k = cfg ? *cfg : SAL_DEFAULT;
  if (const char *bad = sal_config_invalid(call->k))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, bad);
  if (int rc = source_check_window(c, observations, first, n))
    return rc;
  sal_tables(call->k, call->tb.g, call->tb.w, &call->tb.radius);
  call->G = (84 + call->k.stride - 1) / call->k.stride;
  call->P = call->G * call->G;
  return ALEPPO_OK;
}

// pairs [j0, j0 + ns) of a call of n samples with `per` positions from p0 per sample -> c->sal_stage[0 .. ns): the blur of
// the samples the range touches, then the blend.  The blur runs ahead: when a chunk touches a sample sal_blur does not hold,
// the window moves to the chunk's first sample and takes as many of the samples behind it as sal_blur has room for (up to
// SAL_BLUR_WINDOW), so that a launch has workgroups for the whole chip and most chunks need none.
constexpr long SAL_BLUR_WINDOW = 128; // samples (3.6 MB of blurred stacks, 512 workgroups)
struct SalBlurred {
  long lo = 0, hi = -1; // samples sal_blur holds
};
// samples sal_blur must have room for: what one chunk can touch, or the window
long sal_blur_room(const aleppo_ctx *c, long pairs, int per, long n) {
  const long chunk = std::min(c->maxB, pairs);
  return std::min(n, std::max((chunk - 1) / per + 2, SAL_BLUR_WINDOW));
}
void sal_perturb_chunk(aleppo_ctx *c, const SalCall &call, SalBlurred *held, long j0, long ns, int per, int p0, long n,
                       long room) {
  const long lo = j0 / per, hi = (j0 + ns - 1) / per;
  if (lo < held->lo || hi > held->hi) {
    const long count = std::min(room, n - lo); // (>= hi - lo + 1: room covers what a chunk can touch)
    prof_begin(c, ALEPPO_K_SAL_BLUR);
    launch_sal_blur(c->stream, call.src.obs, call.src.map, lo, count, call.tb, call.k.planes, c->sal_blur);
    prof_end(c, ALEPPO_K_SAL_BLUR);
    held->lo = lo, held->hi = lo + count - 1;
  }
  prof_begin(c, ALEPPO_K_SAL_PERTURB);
  launch_sal_perturb(c->stream, call.src.obs, call.src.map, c->sal_blur, held->lo, call.tb, call.k.planes, call.k.stride,
                     call.G, j0, ns, per, p0, c->sal_stage);
  prof_end(c, ALEPPO_K_SAL_PERTURB);
}
// the staging both calls need: `pairs` pairs in chunks of at most maxB, `per` of them per sample, n samples
int sal_ensure_staging(aleppo_ctx *c, long pairs, int per, long n) {
  HIPCHK(c, grow(c, &c->sal_blur, &c->sal_blur_cap, (size_t)sal_blur_room(c, pairs, per, n) * FRAME_PIX * 4, ALLOC_RAW));
  HIPCHK(c, grow(c, &c->sal_stage, &c->sal_stage_cap, (size_t)std::min(c->maxB, pairs) * FRAME_PIX * 4, ALLOC_RAW));
  return ALEPPO_OK;
}
const SampleMap SAL_STAGE_MAP{1, (long)FRAME_PIX, 0, 0, 0}; // pair q of a chunk at sal_stage + q * 7056
} // namespace

extern "C" int aleppo_saliency(aleppo_ctx *c, const uint8_t *observations, int64_t first, int64_t n,
                               const aleppo_saliency_config *cfg, float *policy, float *value, float *outputs) {
  CHECK_CTX(c);
  if (!policy || !value)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "saliency: null argument");
  SalCall call;
  if (int rc = sal_check(c, observations, first, n, cfg, &call))
    return rc;
  const int P = call.P, A = c->A;
  const long pairs = (long)n * P;
  const size_t out_floats = (size_t)n * (P + 1) * (A + 1);
  if (int rc = source_open(c, observations, first, n, &call.src))
    return rc;
  if (int rc = sal_ensure_staging(c, pairs, P, (long)n))
    return rc;
  HIPCHK(c, grow(c, &c->sal_base, &c->sal_base_cap, (size_t)n * (A + 1) * 4, ALLOC_RAW));
  HIPCHK(c, grow(c, &c->sal_out, &c->sal_out_cap, (2 * (size_t)pairs + (outputs ? out_floats : 0)) * 4, ALLOC_RAW));
  float *base_logits = c->sal_base, *base_values = c->sal_base + (size_t)n * A;
  float *d_policy = c->sal_out, *d_value = d_policy + pairs, *d_outputs = outputs ? d_value + pairs : nullptr;
  // the unperturbed samples first: their outputs are kept in a buffer of their own
  source_walk(c, call.src, [&](const SampleMap &map, long n0, long ns) {
    net_forward(c, call.src.obs, map, ns);
    launch_heads_fwd(c->stream, c->h, Pf(c, P_WH), Pf(c, P_BH), base_logits + (size_t)n0 * A, base_values + n0, ns, c->H,
                     A);
    return ALEPPO_OK;
  });
  SalBlurred held;
  const long room = sal_blur_room(c, pairs, P, (long)n);
  for (long i0 = 0; i0 < pairs; i0 += c->maxB) { // a chunk boundary may fall inside one sample's positions
    const long ns = std::min(c->maxB, pairs - i0);
    sal_perturb_chunk(c, call, &held, i0, ns, P, 0, (long)n, room);
    net_forward(c, c->sal_stage, SAL_STAGE_MAP, ns);
    launch_heads_fwd(c->stream, c->h, Pf(c, P_WH), Pf(c, P_BH), c->logits_b, c->values_b, ns, c->H, A);
    prof_begin(c, ALEPPO_K_SAL_SCORE);
    launch_sal_score(c->stream, base_logits, base_values, c->logits_b, c->values_b, i0, ns, P, A, d_policy, d_value,
                     d_outputs);
    prof_end(c, ALEPPO_K_SAL_SCORE);
  }
  HIPCHK(c, hipGetLastError());
  std::vector<float> host(2 * (size_t)pairs + (outputs ? out_floats : 0)); // a failed call writes nothing
  HIPCHK(c, hipMemcpyAsync(host.data(), c->sal_out, host.size() * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  std::memcpy(policy, host.data(), (size_t)pairs * 4);
  std::memcpy(value, host.data() + pairs, (size_t)pairs * 4);
  if (outputs)
    std::memcpy(outputs, host.data() + 2 * (size_t)pairs, out_floats * 4);
  return ALEPPO_OK;
}

extern "C" int aleppo_saliency_perturbed(aleppo_ctx *c, const uint8_t *observations, int64_t first, int64_t n,
                                         const aleppo_saliency_config *cfg, int64_t position_first,
                                         int64_t position_count, uint8_t *out) {
  CHECK_CTX(c);
  if (!out)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "saliency_perturbed: null argument");
  SalCall call;
  if (int rc = sal_check(c, observations, first, n, cfg, &call))
    return rc;
  if (position_first < 0 || position_count <= 0 || position_first >= call.P || position_count > call.P - position_first)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "saliency_perturbed: [position_first, position_first + position_count) must lie inside the grid");
  const int per = (int)position_count, p0 = (int)position_first;
  const long pairs = (long)n * per;
  constexpr size_t STACK = (size_t)4 * FRAME_PIX; // bytes of one stack, packed or NCHW
  if (int rc = source_open(c, observations, first, n, &call.src))
    return rc;
  if (int rc = sal_ensure_staging(c, pairs, per, (long)n))
    return rc;
  HIPCHK(c, grow(c, &c->sal_u8, &c->sal_u8_cap, (size_t)std::min(c->maxB, pairs) * STACK, ALLOC_RAW));
  std::vector<uint8_t> host((size_t)pairs * STACK); // a failed call writes nothing
  SalBlurred held;
  const long room = sal_blur_room(c, pairs, per, (long)n);
  for (long j0 = 0; j0 < pairs; j0 += c->maxB) {
    const long ns = std::min(c->maxB, pairs - j0);
    sal_perturb_chunk(c, call, &held, j0, ns, per, p0, (long)n, room);
    launch_obs_unpack(c->stream, c->sal_stage, c->sal_u8, ns, SAL_STAGE_MAP);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, copy_sync(c, host.data() + (size_t)j0 * STACK, c->sal_u8, (size_t)ns * STACK, hipMemcpyDeviceToHost));
  }
  CHECK_ASYNC(c);
  std::memcpy(out, host.data(), host.size());
  return ALEPPO_OK;
}
