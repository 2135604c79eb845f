// api_policy_diff.hip - C ABI (include/aleppo.h), policy churn: aleppo_snapshot_take, aleppo_snapshot_export,
// aleppo_snapshot_import, aleppo_policy_diff.  The snapshot (c->snapshot, a ParamSet with a compute copy) lives next to
// the live and the averaged parameters in the same layout and only these calls write it.  aleppo_policy_diff walks a
// SampleSource (api_internal.hpp), forwards each chunk once per set through net_forward's ParamView form and compares
// with the kernels of policy_diff.hip.  Nothing here writes P, the moments, the
// gradient, the averaged set or anything aleppo_train reads, and everything goes onto the context's main stream only.
#include "api_internal.hpp"

using namespace aleppo;

extern "C" int aleppo_snapshot_take(aleppo_ctx *c, int source_set) {
  CHECK_CTX(c);
  if (source_set == ALEPPO_SET_SNAPSHOT)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "snapshot_take: the source must be ALEPPO_SET_LIVE or ALEPPO_SET_AVERAGED");
  ParamView src{};
  if (int rc = set_view(c, source_set, &src))
    return rc;
  if (int rc = param_set_storage(c, &c->snapshot, true, "snapshot"))
    return rc;
  if (int rc = param_set_copy(c, &c->snapshot, src))
    return rc;
  c->snapshot.on = true;
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_snapshot_export(aleppo_ctx *c, float *flat, size_t count) {
  CHECK_CTX(c);
  return param_set_export(c, c->snapshot, NO_SNAPSHOT, flat, count);
}

extern "C" int aleppo_snapshot_import(aleppo_ctx *c, const float *flat, size_t count) {
  CHECK_CTX(c);
  static const char *const refusal = "snapshot_import: wrong element count";
  if (!flat || count != c->L.reference_count()) // (here too: a refused call allocates nothing)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, refusal);
  if (int rc = param_set_storage(c, &c->snapshot, true, "snapshot"))
    return rc;
  if (int rc = param_set_upload(c, &c->snapshot, flat, count, refusal))
    return rc;
  HIPCHK(c, hipGetLastError());
  c->snapshot.on = true;
  CHECK_ASYNC(c);
  return ALEPPO_OK;
}

extern "C" int aleppo_policy_diff(aleppo_ctx *c, const uint8_t *observations, int64_t n, int set_a, int set_b,
                                  double *stats, size_t stat_count, double *per_sample, size_t per_sample_count,
                                  int64_t *transitions, size_t transition_count, float *outputs, size_t output_count) {
  CHECK_CTX(c);
  const size_t H = (size_t)c->H, A = (size_t)c->A;
  if (!stats || stat_count != ALEPPO_PD_COUNT)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "policy_diff: stats must be given and stat_count be ALEPPO_PD_COUNT");
  ParamView view[2];
  if (int rc = set_view(c, set_a, &view[0]))
    return rc;
  if (int rc = set_view(c, set_b, &view[1]))
    return rc;
  if (int rc = source_check(c, observations, n))
    return rc;
  const size_t rows = (size_t)(observations ? n : c->batch_n);
  if ((per_sample && per_sample_count != rows * ALEPPO_PD_ROW) || (transitions && transition_count != A * A) ||
      (outputs && output_count != 2 * rows * (A + 1)))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "policy_diff: per_sample_count must be rows * ALEPPO_PD_ROW, transition_count A * A, output_count "
                   "2 * rows * (A + 1)");
  // the scratch holds the largest sample count either source can bring (aleppo_set_batch takes at most N samples)
  const PolicyDiffPlan pl = policy_diff_plan(c->H, c->A, std::max(c->N, c->maxB), c->maxB);
  if (!c->pd_scratch)
    HIPCHK(c, dalloc(c, &c->pd_scratch, pl.bytes));
  char *base = static_cast<char *>(c->pd_scratch);
  auto fl = [&](size_t off) { return reinterpret_cast<float *>(base + off); };
  HIPCHK(c, hipMemsetAsync(base + pl.trans, 0, MAX_ACTIONS * MAX_ACTIONS * sizeof(unsigned long long), c->stream));
  SampleSource src;
  if (int rc = source_open(c, observations, 0, n, &src))
    return rc;
  const int rc = source_walk(c, src, [&](const SampleMap &map, long n0, long ns) -> int {
    for (int k = 0; k < 2; ++k) {
      net_forward(c, view[k], src.obs, map, ns);
      launch_heads_fwd(c->stream, c->h, Pf(c, view[k], P_WH), Pf(c, view[k], P_BH), fl(pl.logits[k]) + (size_t)n0 * A,
                       fl(pl.values[k]) + n0, ns, c->H, c->A);
      if (k == 0) // set b's forward overwrites h
        HIPCHK(c, hipMemcpyAsync(fl(pl.h_a), c->h, (size_t)ns * H * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    prof_begin(c, ALEPPO_K_ACT_STATS); // (the class of the read-only passes over the activations)
    launch_policy_diff_chunk(c->stream, c->h, n0, ns, n0 == 0, pl, c->pd_scratch);
    prof_end(c, ALEPPO_K_ACT_STATS);
    return ALEPPO_OK;
  });
  if (rc)
    return rc;
  launch_policy_diff_stats(c->stream, pl, c->pd_scratch);
  HIPCHK(c, hipGetLastError());
  // the results pass through host temporaries: a failed call writes nothing
  double st[ALEPPO_PD_COUNT];
  std::vector<double> ps(per_sample ? rows * ALEPPO_PD_ROW : 0);
  std::vector<unsigned long long> tr(transitions ? (size_t)MAX_ACTIONS * MAX_ACTIONS : 0);
  std::vector<float> lg[2], vl[2];
  HIPCHK(c, hipMemcpyAsync(st, base + pl.stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  if (per_sample)
    HIPCHK(c, hipMemcpyAsync(ps.data(), base + pl.rows, ps.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (transitions)
    HIPCHK(c, hipMemcpyAsync(tr.data(), base + pl.trans, tr.size() * sizeof(tr[0]), hipMemcpyDeviceToHost, c->stream));
  if (outputs)
    for (int k = 0; k < 2; ++k) {
      lg[k].resize(rows * A);
      vl[k].resize(rows);
      HIPCHK(c, hipMemcpyAsync(lg[k].data(), fl(pl.logits[k]), rows * A * 4, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(vl[k].data(), fl(pl.values[k]), rows * 4, hipMemcpyDeviceToHost, c->stream));
    }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  CHECK_ASYNC(c);
  std::memcpy(stats, st, sizeof(st));
  if (per_sample)
    std::memcpy(per_sample, ps.data(), ps.size() * sizeof(double));
  if (transitions)
    for (size_t i = 0; i < A; ++i)
      for (size_t j = 0; j < A; ++j)
        transitions[i * A + j] = (int64_t)tr[i * MAX_ACTIONS + j];
  if (outputs)
    for (int k = 0; k < 2; ++k)
      for (size_t r = 0; r < rows; ++r) {
        float *o = outputs + ((size_t)k * rows + r) * (A + 1);
        std::memcpy(o, lg[k].data() + r * A, A * 4);
        o[A] = vl[k][r];
      }
  return ALEPPO_OK;
}
