// api_feature_rank.hip - C ABI (include/aleppo.h), the representation: aleppo_feature_rank.  It walks a SampleSource
// (api_internal.hpp: aleppo_activation_stats' sources) on the live parameters, reads h with the kernels of feature_rank.hip, copies the Gram blocks and the column sums once and solves on the host (feature_rank_host.hpp).
#include "api_internal.hpp"
#include "feature_rank_host.hpp"

using namespace aleppo;

static_assert(sizeof(aleppo_feature_rank_config) == 16, "aleppo_feature_rank_config layout");
static_assert((int)aleppo_fr::FR_COUNT == ALEPPO_FR_COUNT && (int)aleppo_fr::FR_NUMERICAL_RANK == ALEPPO_FR_NUMERICAL_RANK,
              "feature_rank_host.hpp mirrors aleppo_feature_rank_stat");

extern "C" int aleppo_feature_rank(aleppo_ctx *c, const uint8_t *observations, int64_t n,
                                   const aleppo_feature_rank_config *cfg, double *stats, size_t stat_count, double *sigma,
                                   size_t sigma_count, double *gram, size_t gram_count, double *colsum,
                                   size_t colsum_count) {
  CHECK_CTX(c);
  const aleppo_feature_rank_config defaults{0.01f, 0.01f, 0, 0};
  const aleppo_feature_rank_config k = cfg ? *cfg : defaults;
  const size_t H = (size_t)c->H;
  if (!stats || stat_count != ALEPPO_FR_COUNT)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "feature_rank: stats must be given and stat_count be ALEPPO_FR_COUNT");
  if ((sigma && sigma_count != H) || (gram && gram_count != H * H) || (colsum && colsum_count != H))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "feature_rank: sigma_count and colsum_count must be H, gram_count H * H");
  if (!(k.delta > 0.f && k.delta < 1.f))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "feature_rank: delta must be in (0, 1)");
  if (!(k.eps >= 0.f) || !std::isfinite(k.eps))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "feature_rank: eps must be finite and non-negative");
  if ((k.centered != 0 && k.centered != 1) || k.reserved != 0)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "feature_rank: centered must be 0 or 1 and reserved 0");
  if (int rc = source_check(c, observations, n))
    return rc;
  const FeatureRankPlan pl = feature_rank_plan(c->H, c->maxB);
  if (!c->fr_scratch)
    HIPCHK(c, dalloc(c, &c->fr_scratch, pl.bytes));
  SampleSource src;
  if (int rc = source_open(c, observations, 0, n, &src))
    return rc;
  source_walk(c, src, [&](const SampleMap &map, long n0, long ns) {
    net_forward(c, src.obs, map, ns);
    prof_begin(c, ALEPPO_K_ACT_STATS); // (the class of the read-only passes over the activations)
    launch_feature_rank_chunk(c->stream, c->h, ns, n0 == 0, pl, c->fr_scratch);
    prof_end(c, ALEPPO_K_ACT_STATS);
    return ALEPPO_OK;
  });
  HIPCHK(c, hipGetLastError());
  std::vector<double> res(pl.result_doubles);
  HIPCHK(c, hipMemcpyAsync(res.data(), c->fr_scratch, res.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  // the full symmetric matrix from the upper blocks: G[i][j], i <= j, as computed; G[j][i] its copy
  std::vector<double> g(H * H), sg(H), st(ALEPPO_FR_COUNT);
  for (size_t i = 0; i < H; ++i)
    for (size_t j = i; j < H; ++j) {
      const double v = res[fr_tile(pl.nb, (int)(i / 64), (int)(j / 64)) * 4096 + (i % 64) * 64 + j % 64];
      g[i * H + j] = v;
      g[j * H + i] = v;
    }
  const double *s = res.data() + (size_t)pl.tiles * 4096;
  const double left_out = s[H], rows = (double)src.total - left_out;
  if (!aleppo_fr::solve(g.data(), s, (int)H, rows, left_out, k.centered != 0, (double)k.delta, (double)k.eps, st.data(),
                        sg.data()))
    return set_err(c, ALEPPO_ERR_RUNTIME, "feature_rank: the eigenvalue iteration did not converge");
  std::memcpy(stats, st.data(), st.size() * sizeof(double));
  if (sigma)
    std::memcpy(sigma, sg.data(), H * sizeof(double));
  if (gram)
    std::memcpy(gram, g.data(), H * H * sizeof(double));
  if (colsum)
    std::memcpy(colsum, s, H * sizeof(double));
  return ALEPPO_OK;
}
