// TEST INFRASTRUCTURE - aleppo_stub_env.cc plus a host-only aleppo_saliency, so that the trainer's record_saliency keys run
// without a GPU.  The stand-in has no network and perturbs nothing: it RECORDS its arguments, one line per call on stderr
// ("stub: aleppo_saliency first=<int> n=<int> stride=<int> planes=<int> sigma_mask=<%.17g> sigma_blur=<%.17g> batch=<0|1>
// outputs=<0|1>"), and answers with scores that are a closed formula of (sample, gy, gx), so that a test can work out every
// byte of the file the trainer writes: with p = gy * G + gx and s the sample's index in the batch,
//   S_policy = (s + 1) * p        S_value = (s + 1) * (P - 1 - p)
// At stride 84 the grid is one point and both are zero everywhere: the zero-maximum case.  Validation follows the header:
// the parameters, the outputs, the source (the batch source only: the trainer never uses the other), the range, an armed
// step.  It COUNTS its calls and says so when the process ends ("stub: aleppo_saliency calls: N"), so that a run with the key
// off shows that it never called it.  Never linked into anything but trainer/train_sal_stub.
#include "aleppo_stub_env.cc"

namespace {
struct SaliencyCallCount {
  long n = 0;
  ~SaliencyCallCount() { std::fprintf(stderr, "stub: aleppo_saliency calls: %ld\n", n); }
} g_saliency_calls;
} // namespace

extern "C" int aleppo_saliency(aleppo_ctx *c, const uint8_t *observations, int64_t first, int64_t n,
                               const aleppo_saliency_config *cfg, float *policy, float *value, float *outputs) {
  g_saliency_calls.n++;
  if (c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: a step is armed");
  const aleppo_saliency_config k = cfg ? *cfg : aleppo_saliency_config{5, 15, 5.0, 3.0};
  const int64_t N = (int64_t)c->cfg.num_envs * c->cfg.horizon;
  if (k.stride < 2 || k.stride > 84 || !(k.sigma_mask >= 0.5 && k.sigma_mask <= 16.0) ||
      !(k.sigma_blur >= 0.5 && k.sigma_blur <= 10.0) || k.planes < 1 || k.planes > 15 || !policy || !value || observations ||
      first < 0 || n <= 0 || first + n > N)
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: saliency: bad argument (the stand-in has the batch source only)");
  std::fprintf(stderr, "stub: aleppo_saliency first=%lld n=%lld stride=%d planes=%d sigma_mask=%.17g sigma_blur=%.17g batch=%d "
                       "outputs=%d\n",
               (long long)first, (long long)n, (int)k.stride, (int)k.planes, k.sigma_mask, k.sigma_blur, observations ? 0 : 1,
               outputs ? 1 : 0);
  const int64_t G = (84 + k.stride - 1) / k.stride, P = G * G;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t p = 0; p < P; ++p) {
      policy[i * P + p] = (float)((first + i + 1) * p);
      value[i * P + p] = (float)((first + i + 1) * (P - 1 - p));
    }
  return ALEPPO_OK;
}
