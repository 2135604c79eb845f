// Saliency videos from the library's perturbation saliency (aleppo_saliency; Greydanus et al. 2018): one file per
// recorded rollout in the video directory, environment 0's T samples of the batch the context holds.
//   saliency_<rollout>.y4m  uncompressed YUV4MPEG2, "YUV4MPEG2 W84 H84 F15:1 Ip A1:1 C444 XALEPPO_Y=channel0_newest\n", then
//                           per sample "FRAME\n" + the Y, U and V planes of 84 * 84 bytes each; <rollout> counts from 1
//   Y  channel 0 of the sample's stack as aleppo_read_batch(ALEPPO_F_OBSERVATIONS) returns it: the newest of its four frames
//   U  128 + rint(127 * S_policy / max S_policy): the actor's saliency shows blue
//   V  128 + rint(127 * S_value / max S_value): the critic's saliency shows red
// Pixel (y, x) takes the score of grid point (min(G - 1, (y + d / 2) / d), min(G - 1, (x + d / 2) / d)), d the stride.  The
// maxima are taken over the file; a maximum that is zero or not finite gives 128 everywhere.  Written as .part and renamed.
#pragma once
#include "../include/aleppo.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <filesystem>
#include <stdexcept>
#include <string>
#include <vector>

// weak like the other optional entry points (train.cc): a library without it refuses the key at start-up
#pragma weak aleppo_saliency

// check: the caller's error handler; E, T: this rank's environments and the horizon
template <class Check>
static void write_saliency_y4m(aleppo_ctx *ctx, Check &&check, const std::string &dir, size_t rollout, size_t E, size_t T,
                               const aleppo_saliency_config &k) {
  constexpr size_t PIX = 84 * 84;
  const size_t d = (size_t)k.stride, G = (84 + d - 1) / d, P = G * G;
  std::vector<float> policy(T * P), value(T * P);
  check(ctx, aleppo_saliency(ctx, nullptr, 0, (int64_t)T, &k, policy.data(), value.data(), nullptr));
  std::vector<uint8_t> obs(E * T * 4 * PIX); // (the existing batch read: the whole batch; environment 0 is its first T samples)
  check(ctx, aleppo_read_batch(ctx, ALEPPO_F_OBSERVATIONS, obs.data(), obs.size()));
  auto maximum = [](const std::vector<float> &s) {
    double m = 0;
    for (float v : s)
      if (!std::isnan(m) && !(v <= m)) // (a NaN is taken and kept, so that it shows as a non-finite maximum)
        m = (double)v;
    return m;
  };
  const double max_policy = maximum(policy), max_value = maximum(value);
  auto byte_of = [](float s, double m) {
    if (!(std::isfinite(m) && m > 0))
      return (uint8_t)128;
    const double b = 128.0 + std::rint(127.0 * (double)s / m);
    return (uint8_t)(b < 0 ? 0 : b > 255 ? 255 : b);
  };
  std::filesystem::create_directories(dir);
  const std::string name = dir + "/saliency_" + std::to_string(rollout) + ".y4m";
  std::FILE *f = std::fopen((name + ".part").c_str(), "wb");
  if (!f)
    throw std::runtime_error("cannot write " + name);
  std::fprintf(f, "YUV4MPEG2 W84 H84 F15:1 Ip A1:1 C444 XALEPPO_Y=channel0_newest\n");
  size_t cell[84]; // the grid index of a pixel coordinate
  for (size_t i = 0; i < 84; ++i)
    cell[i] = std::min(G - 1, (i + d / 2) / d);
  std::vector<uint8_t> u(PIX), v(PIX);
  for (size_t t = 0; t < T; ++t) {
    const float *sp = policy.data() + t * P, *sv = value.data() + t * P;
    for (size_t y = 0; y < 84; ++y)
      for (size_t x = 0; x < 84; ++x) {
        const size_t p = cell[y] * G + cell[x];
        u[y * 84 + x] = byte_of(sp[p], max_policy);
        v[y * 84 + x] = byte_of(sv[p], max_value);
      }
    std::fwrite("FRAME\n", 1, 6, f);
    std::fwrite(obs.data() + t * 4 * PIX, 1, PIX, f); // sample t of environment 0, channel 0
    std::fwrite(u.data(), 1, PIX, f);
    std::fwrite(v.data(), 1, PIX, f);
  }
  const bool ok = !std::ferror(f);
  if (std::fclose(f) != 0 || !ok)
    throw std::runtime_error("cannot write " + name);
  std::filesystem::rename(name + ".part", name);
}
