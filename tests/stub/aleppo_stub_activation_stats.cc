// TEST INFRASTRUCTURE - aleppo_stub_env.cc plus a host-only aleppo_activation_stats, so that the trainer's
// log_activation_stats key runs without a GPU.  The stand-in has no network, so every number is made up - but as a
// function of the arguments, so that a test can tell that tau and the batch source arrive: unit i of a layer of C units has
// SCORE 2 (i + 1) / (C + 1) (mean 1), MEAN_ABS = SCORE / (layer + 1), POSITIVE_FRACTION 1 / 2, MAX_ABS = 2 MEAN_ABS; a
// layer's DORMANT is the count of its SCOREs <= tau, DEAD its row index, ELEMENTS = C * samples * PIX with samples =
// num_envs * horizon (the batch source; the caller source is refused: the trainer never uses it).  Validation follows the
// header: tau, null pointers, counts, an armed step.  It COUNTS its calls and says so on stderr when the process ends
// ("stub: aleppo_activation_stats calls: N"), so that a run with the key off shows that it never called it.  Never linked
// into anything but trainer/train_astats_stub.
#include "aleppo_stub_env.cc"
#include <cmath>

namespace {
struct CallCount {
  long n = 0;
  ~CallCount() { std::fprintf(stderr, "stub: aleppo_activation_stats calls: %ld\n", n); }
} g_act_calls;
} // namespace

extern "C" int aleppo_activation_stats(aleppo_ctx *c, const uint8_t *observations, int64_t n, double tau, double *units,
                                       size_t unit_count, double *layers, size_t layer_count) {
  g_act_calls.n++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  const int H = c->cfg.hidden_size;
  if (!(tau >= 0) || !std::isfinite(tau) || !units || !layers || unit_count != (size_t)(160 + H) * ALEPPO_ACT_UNIT_COLS ||
      layer_count != (size_t)ALEPPO_ACT_LAYER_ROWS * ALEPPO_ACT_LAYER_COLS || observations || n != 0)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: activation_stats: bad argument (the stand-in has the batch source only)");
  const double samples = (double)c->cfg.num_envs * c->cfg.horizon;
  const int C[4] = {32, 64, 64, H}, PIX[4] = {400, 81, 49, 1};
  double tot[ALEPPO_ACT_LAYER_COLS] = {}, tot_s = 0, tot_p = 0;
  double *u = units;
  for (int l = 0; l < 4; ++l) {
    double dormant = 0, sum_mean = 0, mx = 0;
    for (int i = 0; i < C[l]; ++i, u += ALEPPO_ACT_UNIT_COLS) {
      const double score = 2.0 * (i + 1) / (C[l] + 1), mean = score / (l + 1);
      u[ALEPPO_ACT_MEAN_ABS] = mean, u[ALEPPO_ACT_POSITIVE_FRACTION] = 0.5, u[ALEPPO_ACT_MAX_ABS] = 2 * mean;
      u[ALEPPO_ACT_SCORE] = score, u[ALEPPO_ACT_NONFINITE] = 0;
      dormant += score <= tau ? 1 : 0;
      sum_mean += mean;
      mx = std::max(mx, 2 * mean);
    }
    const double K = samples * PIX[l], elements = C[l] * K;
    const double row[ALEPPO_ACT_LAYER_COLS] = {(double)C[l], elements, sum_mean / C[l], 0.5, mx, (double)l, dormant, 0};
    std::memcpy(layers + l * ALEPPO_ACT_LAYER_COLS, row, sizeof(row));
    tot[ALEPPO_ACT_L_UNITS] += C[l], tot[ALEPPO_ACT_L_ELEMENTS] += elements, tot[ALEPPO_ACT_L_DEAD] += l;
    tot[ALEPPO_ACT_L_DORMANT] += dormant;
    tot[ALEPPO_ACT_L_MAX_ABS] = std::max(tot[ALEPPO_ACT_L_MAX_ABS], mx);
    tot_s += sum_mean * K, tot_p += 0.5 * elements;
  }
  tot[ALEPPO_ACT_L_MEAN_ABS] = tot_s / tot[ALEPPO_ACT_L_ELEMENTS];
  tot[ALEPPO_ACT_L_POSITIVE_FRACTION] = tot_p / tot[ALEPPO_ACT_L_ELEMENTS];
  std::memcpy(layers + 4 * ALEPPO_ACT_LAYER_COLS, tot, sizeof(tot));
  return ALEPPO_OK;
}
