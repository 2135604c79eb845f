// feature_rank_host.hpp - the host half of aleppo_feature_rank (the definitions are in aleppo.h): the centring, the
// symmetric eigenvalue solver and the rank metrics.  Plain C++ in double, single-threaded, no HIP and no library beyond
// <cmath>: libaleppo.so, a plain g++ test object and the trainer's stand-in compile this very file.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace aleppo_fr {

enum { // = aleppo_feature_rank_stat
  FR_ROWS = 0, FR_NONFINITE_ROWS = 1, FR_SIGMA_MAX = 2, FR_SIGMA_MIN = 3, FR_MEAN_SQ_NORM = 4, FR_EFFECTIVE_RANK = 5,
  FR_SRANK = 6, FR_PCA_RANK = 7, FR_THRESHOLD_RANK = 8, FR_STABLE_RANK = 9, FR_NUMERICAL_RANK = 10, FR_COUNT = 11
};

// Gc[i][j] = G[i][j] - (s[i] * s[j]) / n, in place
inline void center_gram(double *g, const double *s, int H, double n) {
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < H; ++j)
      g[(size_t)i * H + j] -= (s[i] * s[j]) / n;
}

// Householder reduction of the symmetric a [m][m] (row-major; only its lower triangle is read, all of it is destroyed) to
// tridiagonal form: d = the diagonal, e[1 .. m-1] = the sub-diagonal (e[0] = 0).  Row i = m-1 .. 2 is annihilated left of
// its sub-diagonal element by the reflector I - v v^T / h; both sweeps over the trailing lower triangle run along rows.
inline void tridiagonalise(double *a, int m, double *d, double *e) {
  std::vector<double> p((size_t)m);
  for (int i = m - 1; i >= 2; --i) {
    double *v = a + (size_t)i * m; // row i, columns 0 .. i-1, becomes the reflector's vector
    const int l = i - 1;
    double big = 0.0;
    for (int k = 0; k <= l; ++k)
      big = std::max(big, std::fabs(v[k]));
    double off = 0.0;
    for (int k = 0; k < l; ++k)
      off = std::max(off, std::fabs(v[k]));
    if (off == 0.0) { // nothing to annihilate
      e[i] = v[l];
      continue;
    }
    double h = 0.0;
    for (int k = 0; k <= l; ++k) {
      v[k] /= big;
      h += v[k] * v[k];
    }
    const double f = v[l], g = f >= 0.0 ? -std::sqrt(h) : std::sqrt(h);
    e[i] = big * g;
    h -= f * g; // = |v|^2 / 2 once v[l] = f - g
    v[l] = f - g;
    // p = A v / h over the leading l+1 rows and columns, A from its lower triangle
    for (int j = 0; j <= l; ++j)
      p[j] = 0.0;
    for (int j = 0; j <= l; ++j) {
      const double *row = a + (size_t)j * m;
      const double vj = v[j];
      double dot = 0.0;
      for (int k = 0; k < j; ++k) {
        dot += row[k] * v[k];
        p[k] += row[k] * vj;
      }
      p[j] += dot + row[j] * vj;
    }
    double vp = 0.0;
    for (int j = 0; j <= l; ++j) {
      p[j] /= h;
      vp += v[j] * p[j];
    }
    const double kk = vp / (h + h);
    for (int j = 0; j <= l; ++j)
      p[j] -= kk * v[j]; // q = p - K v
    for (int j = 0; j <= l; ++j) { // A <- A - v q^T - q v^T
      double *row = a + (size_t)j * m;
      const double vj = v[j], qj = p[j];
      for (int k = 0; k <= j; ++k)
        row[k] -= vj * p[k] + qj * v[k];
    }
  }
  if (m >= 2)
    e[1] = a[(size_t)m]; // a[1][0]
  e[0] = 0.0;
  for (int i = 0; i < m; ++i)
    d[i] = a[(size_t)i * m + i];
}

// the eigenvalues of the symmetric tridiagonal (d, e as tridiagonalise leaves them) by QL with implicit Wilkinson shifts,
// into d (unordered); e is destroyed.  false: a block took more than 60 sweeps (does not happen on finite input)
inline bool tridiagonal_eigenvalues(double *d, double *e, int m) {
  for (int i = 1; i < m; ++i)
    e[i - 1] = e[i];
  if (m > 0)
    e[m - 1] = 0.0;
  for (int l = 0; l < m; ++l) {
    for (int iter = 0;; ++iter) {
      int k = l;
      for (; k < m - 1; ++k) { // the first negligible sub-diagonal element at or after l
        const double dd = std::fabs(d[k]) + std::fabs(d[k + 1]);
        if (std::fabs(e[k]) <= 2.220446049250313e-16 * dd)
          break;
      }
      if (k == l)
        break;
      if (iter == 60)
        return false;
      double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
      double r = std::hypot(g, 1.0);
      g = d[k] - d[l] + e[l] / (g + (g >= 0.0 ? r : -r));
      double s = 1.0, c = 1.0, p = 0.0;
      int i = k - 1;
      for (; i >= l; --i) {
        double f = s * e[i];
        const double b = c * e[i];
        r = std::hypot(f, g);
        e[i + 1] = r;
        if (r == 0.0) { // recover from underflow
          d[i + 1] -= p;
          e[k] = 0.0;
          break;
        }
        s = f / r;
        c = g / r;
        g = d[i + 1] - p;
        r = (d[i] - g) * s + 2.0 * c * b;
        p = s * r;
        d[i + 1] = g + p;
        g = c * r - b;
      }
      if (r == 0.0 && i >= l)
        continue;
      d[l] -= p;
      e[l] = g;
      e[k] = 0.0;
    }
  }
  return true;
}

// the eigenvalues of the symmetric g [H][H] (row-major, read only), descending, into lambda [H].  The matrix is scaled by
// an exact power of two so that its largest element is in [0.5, 1), and the eigenvalues are scaled back.
inline bool symmetric_eigenvalues(const double *g, int H, double *lambda) {
  double big = 0.0;
  for (size_t i = 0; i < (size_t)H * H; ++i)
    big = std::max(big, std::fabs(g[i]));
  if (big == 0.0 || !std::isfinite(big)) {
    for (int i = 0; i < H; ++i)
      lambda[i] = 0.0;
    return big == 0.0;
  }
  int ex = 0;
  std::frexp(big, &ex);
  std::vector<double> a((size_t)H * H), e((size_t)H);
  for (size_t i = 0; i < a.size(); ++i)
    a[i] = std::ldexp(g[i], -ex);
  tridiagonalise(a.data(), H, lambda, e.data());
  const bool ok = tridiagonal_eigenvalues(lambda, e.data(), H);
  std::sort(lambda, lambda + H, [](double x, double y) { return x > y; });
  for (int i = 0; i < H; ++i)
    lambda[i] = std::ldexp(lambda[i], ex);
  return ok;
}

// stats [FR_COUNT] and sigma [H] from the eigenvalues lambda [H] (descending) of G or Gc, the diagonal sum of G, n rows
// that entered and `nonfinite` that were left out
inline void rank_metrics(const double *lambda, int H, double n, double nonfinite, double trace, double delta, double eps,
                         double *stats, double *sigma) {
  for (int k = 0; k < FR_COUNT; ++k)
    stats[k] = 0.0;
  stats[FR_ROWS] = n;
  stats[FR_NONFINITE_ROWS] = nonfinite;
  double S1 = 0.0, S2 = 0.0;
  for (int i = 0; i < H; ++i) {
    sigma[i] = std::sqrt(std::max(lambda[i], 0.0));
    S1 += sigma[i];
    S2 += sigma[i] * sigma[i];
  }
  if (!(n > 0.0) || S1 == 0.0) {
    for (int i = 0; i < H; ++i)
      sigma[i] = 0.0;
    return;
  }
  stats[FR_SIGMA_MAX] = sigma[0];
  stats[FR_SIGMA_MIN] = sigma[H - 1];
  stats[FR_MEAN_SQ_NORM] = trace / n;
  double ent = 0.0;
  for (int i = 0; i < H; ++i) {
    const double p = sigma[i] / S1;
    if (p > 0.0)
      ent -= p * std::log(p);
  }
  stats[FR_EFFECTIVE_RANK] = std::exp(ent);
  const double rootn = std::sqrt(n), tol = std::max(n, (double)H) * 0x1p-23 * sigma[0];
  double c1 = 0.0, c2 = 0.0;
  int srank = 0, pca = 0, thr = 0, num = 0;
  for (int i = 0; i < H; ++i) {
    c1 += sigma[i];
    c2 += sigma[i] * sigma[i];
    if (!srank && c1 >= (1.0 - delta) * S1)
      srank = i + 1;
    if (!pca && c2 >= (1.0 - delta) * S2)
      pca = i + 1;
    thr += sigma[i] / rootn > eps ? 1 : 0;
    num += sigma[i] > tol ? 1 : 0;
  }
  stats[FR_SRANK] = srank ? srank : H;
  stats[FR_PCA_RANK] = pca ? pca : H;
  stats[FR_THRESHOLD_RANK] = thr;
  stats[FR_STABLE_RANK] = S2 / (sigma[0] * sigma[0]);
  stats[FR_NUMERICAL_RANK] = num;
}

// everything after the copy: g [H][H] the full symmetric Gram, s [H] the column sums -> stats, sigma [H].  work: H * H
// doubles when centered (untouched otherwise).  false: the solver did not converge
inline bool solve(const double *g, const double *s, int H, double n, double nonfinite, bool centered, double delta,
                  double eps, double *stats, double *sigma) {
  double trace = 0.0;
  for (int i = 0; i < H; ++i)
    trace += g[(size_t)i * H + i];
  std::vector<double> lambda((size_t)H, 0.0);
  bool ok = true;
  if (n > 0.0) {
    if (centered) {
      std::vector<double> gc(g, g + (size_t)H * H);
      center_gram(gc.data(), s, H, n);
      ok = symmetric_eigenvalues(gc.data(), H, lambda.data());
    } else
      ok = symmetric_eigenvalues(g, H, lambda.data());
  }
  rank_metrics(lambda.data(), H, n, nonfinite, trace, delta, eps, stats, sigma);
  return ok;
}

} // namespace aleppo_fr
