// TEST INFRASTRUCTURE - aleppo_stub_env.cc plus a host-only aleppo_feature_rank, so that the trainer's log_feature_rank
// keys run without a GPU.  The stand-in has no network, so it fills a closed-form Gram - but runs the library's own host
// half (csrc/feature_rank_host.hpp: centring, eigenvalue solver, metrics) on it, so that a test can tell that delta, eps
// and centered arrive and that the trainer logs the stat it names: with n = num_envs * horizon samples,
//   G = n * diag(1, 1/4, 1/16, ..., 4^-7, 0, ...)    s = (n / 2, 0, ...)
// so sigma_i = sqrt(n) 2^-i for i < 8 (uncentred), and centred G[0][0] becomes 3 n / 4.  The batch source only (the
// trainer never uses the other).  Validation follows the header.  It COUNTS its calls and says so on stderr when the
// process ends ("stub: aleppo_feature_rank calls: N"), so that a run with the key off shows that it never called it.  Never
// linked into anything but trainer/train_frank_stub.
#include "aleppo_stub_env.cc"
#include "../../ale-libtorch-ppo_amd/csrc/feature_rank_host.hpp"
#include <cmath>

namespace {
struct FrCallCount {
  long n = 0;
  ~FrCallCount() { std::fprintf(stderr, "stub: aleppo_feature_rank calls: %ld\n", n); }
} g_fr_calls;
} // namespace

extern "C" int aleppo_feature_rank(aleppo_ctx *c, const uint8_t *observations, int64_t n,
                                   const aleppo_feature_rank_config *cfg, double *stats, size_t stat_count, double *sigma,
                                   size_t sigma_count, double *gram, size_t gram_count, double *colsum,
                                   size_t colsum_count) {
  g_fr_calls.n++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  const size_t H = (size_t)c->cfg.hidden_size;
  const aleppo_feature_rank_config k = cfg ? *cfg : aleppo_feature_rank_config{0.01f, 0.01f, 0, 0};
  if (!stats || stat_count != ALEPPO_FR_COUNT || (sigma && sigma_count != H) || (gram && gram_count != H * H) ||
      (colsum && colsum_count != H) || !(k.delta > 0 && k.delta < 1) || !(k.eps >= 0) || !std::isfinite(k.eps) ||
      (k.centered != 0 && k.centered != 1) || k.reserved != 0 || observations || n != 0)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: feature_rank: bad argument (the stand-in has the batch source only)");
  const double rows = (double)c->cfg.num_envs * c->cfg.horizon;
  std::vector<double> g(H * H, 0.0), s(H, 0.0), sg(H, 0.0);
  for (size_t i = 0; i < std::min<size_t>(H, 8); ++i)
    g[i * H + i] = rows * std::ldexp(1.0, -2 * (int)i);
  s[0] = rows / 2;
  if (!aleppo_fr::solve(g.data(), s.data(), (int)H, rows, 0.0, k.centered != 0, k.delta, k.eps, stats, sg.data()))
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: feature_rank: the solver did not converge");
  if (sigma)
    std::memcpy(sigma, sg.data(), H * sizeof(double));
  if (gram)
    std::memcpy(gram, g.data(), H * H * sizeof(double));
  if (colsum)
    std::memcpy(colsum, s.data(), H * sizeof(double));
  return ALEPPO_OK;
}
