// policy_diff.hip - the kernels of aleppo_policy_diff (the definitions are in aleppo.h): two forward passes of the same rows
// on two parameter sets -> the per-sample comparison, its sums, extrema and the greedy-action transition counts.
//   compare  one wave per row, four rows per workgroup, a grid-stride loop over the chunk's rows (the grid is a function of
//            the row count alone).  The wave reads the two fc rows as quads (16-byte loads; a row is H * 4 bytes, H a
//            multiple of 32, so every row is 128-byte aligned and H / 4 quads cover it whatever H % 64 is), widens, and
//            keeps <h_a,h_b>, |h_a|^2, |h_b|^2 and |h_b - h_a|^2 in double per lane in the order of its loop; the xor
//            butterfly of block_sum.hpp adds the 64 lanes.  Lanes < A test the logits, lane 0 the values, every lane its
//            fc elements: one non-finite number leaves the row out.  Lane 0 then does the softmax arithmetic of both sets
//            in double (A <= 18) and carries the wave's running sums and extrema; the four waves' are combined as
//            (w0 + w1) + (w2 + w3) into one record per workgroup.  The greedy pair (g_a, g_b) is counted in LDS and added
//            to the global integer counts: integer adds, exact in any order.
//   final    PD_PART workgroups: workgroup k stages entry k of every record in LDS and one thread adds them (or takes their
//            extremum) in index order, then sets or adds to the running total k of the call.
//   stats    once per call, after the last chunk: one thread writes the ALEPPO_PD_COUNT stats from the totals.
// No floating-point atomics; every figure is a function of the inputs alone.
#include "block_sum.hpp"
#include "common.hpp"
#include <algorithm>

namespace aleppo {

static_assert(PD_X_MIN_COS + 1 == PD_PART, "a record is the sums, then the four extrema");

__device__ __forceinline__ bool pd_is_max(int k) { return k >= PD_X_MAX_KL_AB && k <= PD_X_MAX_ABS_DV; }
__device__ __forceinline__ double pd_identity(int k) {
  return k < PD_SUMS ? 0.0 : pd_is_max(k) ? -HUGE_VAL : HUGE_VAL;
}
__device__ __forceinline__ double pd_join(int k, double a, double b) {
  return k < PD_SUMS ? a + b : pd_is_max(k) ? fmax(a, b) : fmin(a, b);
}

// log-softmax of A fp32 logits in double: z = l - max l, lse = log(sum exp z) in index order, logp = z - lse; the lowest
// index of the maximum (the ALEPPO_EVAL_GREEDY rule)
__device__ __forceinline__ int pd_log_softmax(const float *__restrict__ l, int A, double *logp) {
  int g = 0;
  double m = (double)l[0];
  for (int i = 1; i < A; ++i)
    if ((double)l[i] > m) {
      m = (double)l[i];
      g = i;
    }
  double s = 0.0;
  for (int i = 0; i < A; ++i) {
    logp[i] = (double)l[i] - m;
    s += exp(logp[i]);
  }
  const double lse = log(s);
  for (int i = 0; i < A; ++i)
    logp[i] -= lse;
  return g;
}

// lane 0's half of one finite row: the softmax arithmetic of both sets, the row of the per-sample table, the wave's
// running record and the transition count.  pa / pb: A doubles of LDS each, the wave's own
__device__ __forceinline__ void pd_row(const float *__restrict__ la, const float *__restrict__ lb, double va, double vb,
                                       double dab, double daa, double dbb, double ddd, int A, double *pa, double *pb,
                                       double *__restrict__ out, double *acc, unsigned int *cnt) {
  const int ga = pd_log_softmax(la, A, pa), gb = pd_log_softmax(lb, A, pb);
  double kl_ab = 0.0, kl_ba = 0.0, tv = 0.0, ea = 0.0, eb = 0.0;
  for (int i = 0; i < A; ++i) {
    const double p = exp(pa[i]), q = exp(pb[i]);
    kl_ab += p * (pa[i] - pb[i]);
    kl_ba += q * (pb[i] - pa[i]);
    tv += fabs(p - q);
    ea -= p * pa[i];
    eb -= q * pb[i];
  }
  tv *= 0.5;
  const double dv = vb - va;
  const double cs = (daa == 0.0 || dbb == 0.0) ? 1.0 : dab / sqrt(daa * dbb);
  out[0] = kl_ab;
  out[1] = kl_ba;
  out[2] = tv;
  out[3] = dv;
  out[4] = cs;
  out[5] = ddd;
  out[6] = (double)ga;
  out[7] = (double)gb;
  acc[PD_S_ROWS] += 1.0;
  acc[PD_S_CHURN] += ga != gb ? 1.0 : 0.0;
  acc[PD_S_KL_AB] += kl_ab;
  acc[PD_S_KL_BA] += kl_ba;
  acc[PD_S_TV] += tv;
  acc[PD_S_ABS_DV] += fabs(dv);
  acc[PD_S_DV2] += dv * dv;
  acc[PD_S_ENT_A] += ea;
  acc[PD_S_ENT_B] += eb;
  acc[PD_S_COS] += cs;
  acc[PD_S_DH2] += ddd;
  acc[PD_S_HA2] += daa;
  acc[PD_X_MAX_KL_AB] = fmax(acc[PD_X_MAX_KL_AB], kl_ab);
  acc[PD_X_MAX_TV] = fmax(acc[PD_X_MAX_TV], tv);
  acc[PD_X_MAX_ABS_DV] = fmax(acc[PD_X_MAX_ABS_DV], fabs(dv));
  acc[PD_X_MIN_COS] = fmin(acc[PD_X_MIN_COS], cs);
  atomicAdd(&cnt[ga * A + gb], 1u);
}

__global__ __launch_bounds__(256) void policy_diff_kernel(
    const float *__restrict__ la, const float *__restrict__ va, const float *__restrict__ ha,
    const float *__restrict__ lb, const float *__restrict__ vb, const float *__restrict__ hb, long ns, int H, int A,
    double *__restrict__ rows, double *__restrict__ part, unsigned long long *__restrict__ trans) {
  __shared__ unsigned int cnt[MAX_ACTIONS * MAX_ACTIONS];
  __shared__ double rec[4][PD_PART];
  __shared__ double logp[4][2][MAX_ACTIONS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < A * A; i += 256)
    cnt[i] = 0u;
  __syncthreads();
  double acc[PD_PART]; // (lane 0's are the wave's)
#pragma unroll
  for (int k = 0; k < PD_PART; ++k)
    acc[k] = pd_identity(k);
  const int quads = H / 4;
  for (long r = (long)blockIdx.x * 4 + wave; r < ns; r += (long)gridDim.x * 4) { // (r is the wave's: no lane leaves early)
    const float4 *a4 = reinterpret_cast<const float4 *>(ha + (size_t)r * H);
    const float4 *b4 = reinterpret_cast<const float4 *>(hb + (size_t)r * H);
    double dab = 0.0, daa = 0.0, dbb = 0.0, ddd = 0.0;
    int bad = 0;
    for (int q = lane; q < quads; q += 64) {
      const float4 x = a4[q], y = b4[q];
      const double xv[4] = {x.x, x.y, x.z, x.w}, yv[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double d = yv[k] - xv[k];
        dab += xv[k] * yv[k];
        daa += xv[k] * xv[k];
        dbb += yv[k] * yv[k];
        ddd += d * d;
        bad |= !isfinite(xv[k]) || !isfinite(yv[k]);
      }
    }
    if (lane < A)
      bad |= !isfinite(la[r * A + lane]) || !isfinite(lb[r * A + lane]);
    if (lane == 0)
      bad |= !isfinite(va[r]) || !isfinite(vb[r]);
    bad = wave_sum(bad);
    dab = wave_sum(dab);
    daa = wave_sum(daa);
    dbb = wave_sum(dbb);
    ddd = wave_sum(ddd);
    if (lane == 0) {
      double *out = rows + (size_t)r * ALEPPO_PD_ROW;
      if (bad) {
        acc[PD_S_NONFINITE] += 1.0;
        for (int k = 0; k < ALEPPO_PD_ROW; ++k)
          out[k] = __builtin_nan("");
      } else {
        pd_row(la + r * A, lb + r * A, (double)va[r], (double)vb[r], dab, daa, dbb, ddd, A, logp[wave][0], logp[wave][1],
               out, acc, cnt);
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < PD_PART; ++k)
      rec[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < PD_PART) {
    const int k = threadIdx.x;
    part[(size_t)k * PD_MAX_BLOCKS + blockIdx.x] = pd_join(k, pd_join(k, rec[0][k], rec[1][k]), pd_join(k, rec[2][k], rec[3][k]));
  }
  for (int i = threadIdx.x; i < A * A; i += 256)
    if (cnt[i])
      atomicAdd(&trans[(i / A) * MAX_ACTIONS + i % A], (unsigned long long)cnt[i]);
}

// workgroup k: entry k of every record (part is [PD_PART][PD_MAX_BLOCKS]: the loads are contiguous) -> LDS, then one thread
// joins them in index order and sets or joins the running total
__global__ __launch_bounds__(64) void policy_diff_final_kernel(const double *__restrict__ part, int nblk, int first,
                                                               double *__restrict__ total) {
  __shared__ double s[PD_MAX_BLOCKS];
  const int k = blockIdx.x;
  for (int b = threadIdx.x; b < nblk; b += 64)
    s[b] = part[(size_t)k * PD_MAX_BLOCKS + b];
  __syncthreads();
  if (threadIdx.x != 0)
    return;
  double a = pd_identity(k);
  if (k < PD_SUMS) { // (the kind is chosen outside the loops, so that the LDS reads of each run ahead of its chain of joins)
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) // index order
      a += s[b];
  } else if (pd_is_max(k)) {
#pragma unroll 8
    for (int b = 0; b < nblk; ++b)
      a = fmax(a, s[b]);
  } else {
#pragma unroll 8
    for (int b = 0; b < nblk; ++b)
      a = fmin(a, s[b]);
  }
  if (!first)
    a = pd_join(k, total[k], a);
  total[k] = a;
}

__global__ __launch_bounds__(64) void policy_diff_stats_kernel(const double *__restrict__ t, double *__restrict__ stats) {
  if (threadIdx.x != 0)
    return;
  const double n = t[PD_S_ROWS];
  stats[ALEPPO_PD_ROWS] = n;
  stats[ALEPPO_PD_NONFINITE_ROWS] = t[PD_S_NONFINITE];
  if (n == 0.0) {
    for (int k = ALEPPO_PD_CHURN; k < ALEPPO_PD_COUNT; ++k)
      stats[k] = 0.0;
    return;
  }
  stats[ALEPPO_PD_CHURN] = t[PD_S_CHURN] / n;
  stats[ALEPPO_PD_MEAN_KL_AB] = t[PD_S_KL_AB] / n;
  stats[ALEPPO_PD_MAX_KL_AB] = t[PD_X_MAX_KL_AB];
  stats[ALEPPO_PD_MEAN_KL_BA] = t[PD_S_KL_BA] / n;
  stats[ALEPPO_PD_MEAN_TV] = t[PD_S_TV] / n;
  stats[ALEPPO_PD_MAX_TV] = t[PD_X_MAX_TV];
  stats[ALEPPO_PD_MEAN_ABS_DV] = t[PD_S_ABS_DV] / n;
  stats[ALEPPO_PD_MAX_ABS_DV] = t[PD_X_MAX_ABS_DV];
  stats[ALEPPO_PD_RMS_DV] = sqrt(t[PD_S_DV2] / n);
  stats[ALEPPO_PD_MEAN_ENTROPY_A] = t[PD_S_ENT_A] / n;
  stats[ALEPPO_PD_MEAN_ENTROPY_B] = t[PD_S_ENT_B] / n;
  stats[ALEPPO_PD_MEAN_FEATURE_COS] = t[PD_S_COS] / n;
  stats[ALEPPO_PD_MIN_FEATURE_COS] = t[PD_X_MIN_COS];
  stats[ALEPPO_PD_FEATURE_REL_CHANGE] = t[PD_S_HA2] > 0.0 ? sqrt(t[PD_S_DH2] / t[PD_S_HA2]) : 0.0;
}

PolicyDiffPlan policy_diff_plan(int H, int A, long cap, long maxB) {
  PolicyDiffPlan pl{};
  pl.H = H;
  pl.A = A;
  pl.cap = cap;
  size_t at = 0;
  auto area = [&](size_t bytes) {
    const size_t o = at;
    at += (bytes + 255) / 256 * 256;
    return o;
  };
  for (int k = 0; k < 2; ++k) {
    pl.logits[k] = area((size_t)cap * A * 4);
    pl.values[k] = area((size_t)cap * 4);
  }
  pl.h_a = area((size_t)maxB * H * 4);
  pl.rows = area((size_t)cap * ALEPPO_PD_ROW * sizeof(double));
  pl.part = area((size_t)PD_MAX_BLOCKS * PD_PART * sizeof(double));
  pl.total = area(PD_PART * sizeof(double));
  pl.stats = area(ALEPPO_PD_COUNT * sizeof(double));
  pl.trans = area((size_t)MAX_ACTIONS * MAX_ACTIONS * sizeof(unsigned long long));
  pl.bytes = at;
  return pl;
}

void launch_policy_diff_chunk(hipStream_t s, const float *h_b, long n0, long ns, bool first, const PolicyDiffPlan &pl,
                              void *scratch) {
  char *base = static_cast<char *>(scratch);
  auto f = [&](size_t off) { return reinterpret_cast<float *>(base + off); };
  auto d = [&](size_t off) { return reinterpret_cast<double *>(base + off); };
  const int nblk = (int)std::min<long>((ns + 3) / 4, PD_MAX_BLOCKS);
  hipLaunchKernelGGL(policy_diff_kernel, dim3(nblk), dim3(256), 0, s, f(pl.logits[0]) + (size_t)n0 * pl.A,
                     f(pl.values[0]) + n0, f(pl.h_a), f(pl.logits[1]) + (size_t)n0 * pl.A, f(pl.values[1]) + n0, h_b, ns,
                     pl.H, pl.A, d(pl.rows) + (size_t)n0 * ALEPPO_PD_ROW, d(pl.part),
                     reinterpret_cast<unsigned long long *>(base + pl.trans));
  hipLaunchKernelGGL(policy_diff_final_kernel, dim3(PD_PART), dim3(64), 0, s, d(pl.part), nblk, first ? 1 : 0, d(pl.total));
}

void launch_policy_diff_stats(hipStream_t s, const PolicyDiffPlan &pl, void *scratch) {
  char *base = static_cast<char *>(scratch);
  hipLaunchKernelGGL(policy_diff_stats_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const double *>(base + pl.total),
                     reinterpret_cast<double *>(base + pl.stats));
}

} // namespace aleppo
