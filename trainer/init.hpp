// Orthogonal init (train.cc:212-228)
#pragma once
#include <cmath>
#include <cstdint>
#include <random>
#include <vector>

// rows x cols matrix of N(0,1), orthonormalised (modified Gram-Schmidt on the smaller dimension), times gain
static void orthogonal(float *w, size_t rows, size_t cols, double gain, std::mt19937_64 &g) {
  std::normal_distribution<double> nd(0.0, 1.0);
  const bool tr = rows < cols;
  const size_t R = tr ? cols : rows, C = tr ? rows : cols; // R >= C: orthonormal columns
  std::vector<double> a(R * C);
  for (auto &v : a)
    v = nd(g);
  for (size_t j = 0; j < C; ++j) {
    for (size_t k = 0; k < j; ++k) {
      double dot = 0;
      for (size_t i = 0; i < R; ++i)
        dot += a[i * C + j] * a[i * C + k];
      for (size_t i = 0; i < R; ++i)
        a[i * C + j] -= dot * a[i * C + k];
    }
    double n = 0;
    for (size_t i = 0; i < R; ++i)
      n += a[i * C + j] * a[i * C + j];
    n = std::sqrt(n);
    for (size_t i = 0; i < R; ++i)
      a[i * C + j] /= n;
  }
  for (size_t r = 0; r < rows; ++r)
    for (size_t c = 0; c < cols; ++c)
      w[r * cols + c] = (float)(gain * (tr ? a[c * C + r] : a[r * C + c]));
}
static std::vector<float> init_params(size_t H, size_t A, uint64_t seed) { // libtorch parameters() order
  std::mt19937_64 g(seed);
  const double s2 = std::sqrt(2.0);
  struct T {
    size_t rows, cols;
    double gain;
  };
  const T t[6] = {{32, 4 * 8 * 8, s2}, {64, 32 * 4 * 4, s2}, {64, 64 * 3 * 3, s2}, {H, 3136, s2}, {A, H, 0.01}, {1, H, 1.0}};
  std::vector<float> p;
  for (const T &x : t) {
    const size_t o = p.size();
    p.resize(o + x.rows * x.cols + x.rows, 0.0f); // weight then zero bias
    orthogonal(p.data() + o, x.rows, x.cols, x.gain, g);
  }
  return p;
}
