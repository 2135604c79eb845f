// TEST INFRASTRUCTURE - aleppo_stub_env.cc plus host-only regularisation, so that the trainer's weight_decay / l2_init_coef /
// shrink_perturb_* keys - the options, the anchor taken once before the first update, the checkpoint section, the resume -
// run without a GPU.  The stand-in's aleppo_set_option is renamed while it is included and defined again here:
// ALEPPO_OPT_WEIGHT_DECAY and ALEPPO_OPT_ANCHOR_COEF are validated as the header says (the bits of a finite non-negative
// float) and RECORDED ("stub: aleppo_set_option ALEPPO_OPT_WEIGHT_DECAY bits=<hex>" / "... ALEPPO_OPT_ANCHOR_COEF
// bits=<hex>"), everything else is passed on.  The anchor is a copy of the stand-in's own parameter array:
// aleppo_anchor_take records "stub: aleppo_anchor_take source=<set> trains=<n>" - n the aleppo_train calls so far, so that a
// test sees that it came before update 1 - aleppo_anchor_import / aleppo_anchor_export record their names.  The stand-in's
// aleppo_train is renamed too: the one here refuses an anchor coefficient > 0 without an anchor, as the header says, counts
// the call, runs the stand-in's step and then pulls every parameter toward the anchor by the decoupled rule
// p -= (float)(lr * la) * (p - a), so that a resumed run only ends where the uninterrupted one does if the anchor came
// back.  aleppo_shrink_perturb validates its arguments as the header says, RECORDS them ("stub: aleppo_shrink_perturb
// shrink=<%.17g> sigma=<%.17g> key=<hex> flags=<int> trains=<n>") and scales the parameters by (float)shrink; there is no draw.  The
// calls are COUNTED and the counts are printed when the process ends ("stub: aleppo_anchor_take calls: N", "stub:
// aleppo_shrink_perturb calls: N"), so that a run with the keys off shows that it never called them.  One context per
// process (the trainer's).  Never linked into anything but trainer/train_reg_stub.
#define aleppo_set_option stub_plain_set_option
#define aleppo_train stub_plain_train
#include "aleppo_stub_env.cc"
#undef aleppo_set_option
#undef aleppo_train
#include <cmath>

namespace {
struct StubReg {
  uint32_t wd_bits = 0, la_bits = 0;
  bool anchor_on = false;
  std::vector<float> anchor;
  long trains = 0, take_calls = 0, sp_calls = 0;
  ~StubReg() {
    std::fprintf(stderr, "stub: aleppo_anchor_take calls: %ld\n", take_calls);
    std::fprintf(stderr, "stub: aleppo_shrink_perturb calls: %ld\n", sp_calls);
  }
} g_reg;
} // namespace

extern "C" {
int aleppo_set_option(aleppo_ctx *c, int option, int value) {
  if (option != ALEPPO_OPT_WEIGHT_DECAY && option != ALEPPO_OPT_ANCHOR_COEF)
    return stub_plain_set_option(c, option, value);
  if (value < 0 || value >= 0x7F800000)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: the binary32 bits of a finite non-negative float");
  const bool wd = option == ALEPPO_OPT_WEIGHT_DECAY;
  (wd ? g_reg.wd_bits : g_reg.la_bits) = (uint32_t)value;
  std::fprintf(stderr, "stub: aleppo_set_option %s bits=%08x\n", wd ? "ALEPPO_OPT_WEIGHT_DECAY" : "ALEPPO_OPT_ANCHOR_COEF",
               (unsigned)value);
  return ALEPPO_OK;
}
int aleppo_train(aleppo_ctx *c, double lr, int epochs, int M, aleppo_minibatch_metrics *out) {
  if (g_reg.la_bits != 0 && !g_reg.anchor_on)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: ALEPPO_OPT_ANCHOR_COEF > 0 needs an anchor");
  g_reg.trains++;
  if (int rc = stub_plain_train(c, lr, epochs, M, out))
    return rc;
  float la;
  std::memcpy(&la, &g_reg.la_bits, 4);
  const float f_an = (float)(lr * (double)la);
  if (g_reg.la_bits != 0)
    for (size_t i = 0; i < c->params.size(); ++i)
      c->params[i] -= f_an * (c->params[i] - g_reg.anchor[i]);
  return ALEPPO_OK;
}
int aleppo_anchor_take(aleppo_ctx *c, int source_set) {
  g_reg.take_calls++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (source_set != ALEPPO_SET_LIVE) // (the stand-in has the live set only: the trainer never uses another)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: anchor_take: the stand-in has the live set only");
  g_reg.anchor = c->params;
  g_reg.anchor_on = true;
  std::fprintf(stderr, "stub: aleppo_anchor_take source=%d trains=%ld\n", source_set, g_reg.trains);
  return ALEPPO_OK;
}
int aleppo_anchor_import(aleppo_ctx *c, const float *flat, size_t count) {
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (!flat || count != c->params.size())
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: anchor_import: wrong element count");
  g_reg.anchor.assign(flat, flat + count);
  g_reg.anchor_on = true;
  std::fprintf(stderr, "stub: aleppo_anchor_import trains=%ld\n", g_reg.trains);
  return ALEPPO_OK;
}
int aleppo_anchor_export(aleppo_ctx *c, float *flat, size_t count) {
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (!g_reg.anchor_on)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: no anchor");
  if (!flat || count != g_reg.anchor.size())
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: anchor_export: wrong element count");
  std::memcpy(flat, g_reg.anchor.data(), count * 4);
  std::fprintf(stderr, "stub: aleppo_anchor_export\n");
  return ALEPPO_OK;
}
int aleppo_shrink_perturb(aleppo_ctx *c, double shrink, double sigma, uint64_t key, int flags) {
  g_reg.sp_calls++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  if (!std::isfinite(shrink) || !(shrink >= 0.0 && shrink <= 1.0) || !std::isfinite(sigma) || !(sigma >= 0.0) ||
      (flags & ~ALEPPO_SP_RESET_MOMENTS))
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: shrink_perturb: bad argument");
  std::fprintf(stderr, "stub: aleppo_shrink_perturb shrink=%.17g sigma=%.17g key=%016llx flags=%d trains=%ld\n", shrink, sigma,
               (unsigned long long)key, flags, g_reg.trains);
  for (float &p : c->params)
    p *= (float)shrink;
  return ALEPPO_OK;
}
}
