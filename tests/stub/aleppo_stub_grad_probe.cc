// TEST INFRASTRUCTURE - aleppo_stub.cc plus host-only aleppo_grad_probe / aleppo_grad_take / aleppo_grad_gram, so that the
// trainer's log_gradient_stats keys - which probes it makes, where they go relative to the update, how often - run without
// a GPU.  The stand-in's aleppo_train is renamed while it is included and defined again here: every update and every one of
// the three calls is RECORDED, one line on stderr ("stub: aleppo_train", "stub: aleppo_grad_probe slot=<s> first=<f> n=<n>
// cfg=<null | policy,c_v,c_e>", "stub: aleppo_grad_take slot=<s> source=<o> set=<t>", "stub: aleppo_grad_gram slots=<a,b,..>"),
// the calls are COUNTED and the counts printed when the process ends ("stub: aleppo_grad_probe calls: N", ...), so that a run
// with the key off shows that it never called any.  The stand-in has no network, so a slot holds a made-up vector of three
// components PER ROW r of the Gram, chosen so that every logged figure names what was probed:
//   cfg == NULL, n samples:  (1, 8 / sqrt(n), 0)   |g|^2 = 1 + 64 / n: the noise scale of two such probes is |G|^2 = 1, S = 64
//   {1, 0, 0}:               (2, 0, 0)
//   {0, 1, 0}:               3 (c_r, 0, sqrt(1 - c_r^2)),  c_r = (r + 1) / 16: the policy / value cosine of row r is c_r
//   any other cfg:           (0, 0, 1)
//   ALEPPO_GRAD_SRC_EXP_AVG: zero at the first take (Adam before its first step), (0.6, 0.8, 0) afterwards
// and gram[r][i][j] is the dot product.  The unmasked count is n.  Validation follows the header: an armed step, the slot,
// the slice against num_envs * horizon, cfg, the source, the counts, slots that nothing has written.  One context per
// process (the trainer's).  Never linked into anything but trainer/train_gradprobe_stub.
#define aleppo_train stub_plain_train
#include "aleppo_stub.cc"
#undef aleppo_train
#include <cmath>

namespace {
struct StubSlot {
  enum Kind { EMPTY, FULL, POLICY, VALUE, OTHER, MOMENT_ZERO, MOMENT } kind = EMPTY;
  double n = 0;
  void at(int r, double v[3]) const {
    const double c = (r + 1) / 16.0;
    v[0] = v[1] = v[2] = 0;
    switch (kind) {
    case FULL: v[0] = 1, v[1] = 8 / std::sqrt(n); break;
    case POLICY: v[0] = 2; break;
    case VALUE: v[0] = 3 * c, v[2] = 3 * std::sqrt(1 - c * c); break;
    case OTHER: v[2] = 1; break;
    case MOMENT: v[0] = 0.6, v[1] = 0.8; break;
    default: break;
    }
  }
};
struct StubGradProbe {
  long probes = 0, takes = 0, grams = 0;
  StubSlot slot[ALEPPO_GRAD_SLOTS];
  ~StubGradProbe() {
    std::fprintf(stderr, "stub: aleppo_grad_probe calls: %ld\nstub: aleppo_grad_take calls: %ld\nstub: aleppo_grad_gram calls: %ld\n",
                 probes, takes, grams);
  }
} g_gp;
bool stub_bad_slot(int s) { return s < 0 || s >= ALEPPO_GRAD_SLOTS; }
} // namespace

extern "C" {
int aleppo_train(aleppo_ctx *c, double lr, int epochs, int M, aleppo_minibatch_metrics *out) {
  std::fprintf(stderr, "stub: aleppo_train\n");
  return stub_plain_train(c, lr, epochs, M, out);
}
int aleppo_grad_probe(aleppo_ctx *c, int slot, int64_t first, int64_t n, const aleppo_grad_probe_config *cfg,
                      int64_t *unmasked_out) {
  g_gp.probes++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  const int64_t N = (int64_t)c->cfg.num_envs * c->cfg.horizon;
  if (stub_bad_slot(slot) || n < 1 || first < 0 || first > N - n)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: grad_probe: bad slot or slice");
  if (cfg && ((cfg->policy_term != 0 && cfg->policy_term != 1) || !(cfg->value_loss_coef >= 0) || !(cfg->entropy_coef >= 0) ||
              !std::isfinite(cfg->value_loss_coef) || !std::isfinite(cfg->entropy_coef) || cfg->reserved != 0))
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: grad_probe: bad cfg");
  StubSlot &s = g_gp.slot[slot];
  s.n = (double)n;
  if (!cfg) {
    s.kind = StubSlot::FULL;
    std::fprintf(stderr, "stub: aleppo_grad_probe slot=%d first=%lld n=%lld cfg=null\n", slot, (long long)first, (long long)n);
  } else {
    const bool pure = cfg->entropy_coef == 0;
    s.kind = pure && cfg->policy_term == 1 && cfg->value_loss_coef == 0   ? StubSlot::POLICY
             : pure && cfg->policy_term == 0 && cfg->value_loss_coef == 1 ? StubSlot::VALUE
                                                                           : StubSlot::OTHER;
    std::fprintf(stderr, "stub: aleppo_grad_probe slot=%d first=%lld n=%lld cfg=%d,%g,%g\n", slot, (long long)first,
                 (long long)n, cfg->policy_term, (double)cfg->value_loss_coef, (double)cfg->entropy_coef);
  }
  if (unmasked_out)
    *unmasked_out = n;
  return ALEPPO_OK;
}
int aleppo_grad_take(aleppo_ctx *c, int slot, int source, int set) {
  g_gp.takes++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (stub_bad_slot(slot) || source != ALEPPO_GRAD_SRC_EXP_AVG || set != 0)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: grad_take: bad argument (the stand-in has the first moment only)");
  g_gp.slot[slot].kind = g_gp.takes == 1 ? StubSlot::MOMENT_ZERO : StubSlot::MOMENT;
  std::fprintf(stderr, "stub: aleppo_grad_take slot=%d source=%d set=%d\n", slot, source, set);
  return ALEPPO_OK;
}
int aleppo_grad_gram(aleppo_ctx *c, const int32_t *slots, int k, double *gram, size_t gram_count, int64_t *nonfinite,
                     size_t nonfinite_count) {
  g_gp.grams++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  const size_t rows = ALEPPO_TENSOR_STATS_ROWS;
  if (!slots || k < 1 || k > ALEPPO_GRAD_SLOTS || !gram || gram_count != rows * k * k ||
      (nonfinite ? nonfinite_count != rows : nonfinite_count != 0))
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: grad_gram: bad argument");
  std::string list;
  for (int i = 0; i < k; ++i) {
    if (stub_bad_slot(slots[i]))
      return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: grad_gram: bad slot");
    if (g_gp.slot[slots[i]].kind == StubSlot::EMPTY)
      return fail(c, ALEPPO_ERR_RUNTIME, "stub: grad_gram: nothing has written one of the named slots");
    list += (i ? "," : "") + std::to_string(slots[i]);
  }
  std::fprintf(stderr, "stub: aleppo_grad_gram slots=%s\n", list.c_str());
  for (size_t r = 0; r < rows; ++r)
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) {
        double a[3], b[3];
        g_gp.slot[slots[i]].at((int)r, a);
        g_gp.slot[slots[j]].at((int)r, b);
        gram[(r * k + i) * k + j] = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
      }
  for (size_t r = 0; nonfinite && r < rows; ++r)
    nonfinite[r] = 0;
  return ALEPPO_OK;
}
}
