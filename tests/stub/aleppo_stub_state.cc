// TEST INFRASTRUCTURE - aleppo_stub.cc plus host-only stand-ins for the entry points a checkpoint needs, so that the
// trainer's checkpoint FILE handling (framing, atomic rename, refusals, the digest comparison on resume) runs without a
// GPU.  The "state" is what the stub has: its parameters, its action counter (the acting generator's counter) and a
// moment / running-return / stack pattern derived from them.  Never linked into anything but trainer/train_ckpt_stub.
#include "aleppo_stub.cc"

static uint64_t stub_mix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static std::vector<float> g_m1, g_m2;
static int64_t g_step = 0;
static std::vector<double> g_rs;
static std::vector<uint8_t> g_obs;
static void stub_state_init(aleppo_ctx *c) {
  const size_t E = (size_t)c->cfg.num_envs;
  if (g_m1.size() != c->params.size()) {
    g_m1.assign(c->params.size(), 0.f);
    g_m2.assign(c->params.size(), 0.f);
  }
  if (g_rs.size() != 3 + E) {
    g_rs.assign(3 + E, 0.0);
    g_rs[0] = 1e-4, g_rs[2] = 1.0;
  }
  if (g_obs.size() != E * 4 * 84 * 84)
    g_obs.assign(E * 4 * 84 * 84, 0);
}
extern "C" {
int aleppo_export_optimizer(aleppo_ctx *c, float *m1, float *m2, int64_t *step, size_t n) {
  stub_state_init(c);
  if (n != c->params.size())
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: wrong count");
  std::memcpy(m1, g_m1.data(), n * 4);
  std::memcpy(m2, g_m2.data(), n * 4);
  *step = (int64_t)c->tick; // (moves with the run; the rollout state brings it back)
  return ALEPPO_OK;
}
int aleppo_import_optimizer(aleppo_ctx *c, const float *m1, const float *m2, int64_t step, size_t n) {
  stub_state_init(c);
  if (n != c->params.size())
    return fail(c, ALEPPO_ERR_INVALID_ARGUMENT, "stub: wrong count");
  std::memcpy(g_m1.data(), m1, n * 4);
  std::memcpy(g_m2.data(), m2, n * 4);
  g_step = step;
  return ALEPPO_OK;
}
int aleppo_export_reward_scale(aleppo_ctx *c, double stats[3], double *returns, size_t E) {
  stub_state_init(c);
  std::memcpy(stats, g_rs.data(), 24);
  std::memcpy(returns, g_rs.data() + 3, E * 8);
  return ALEPPO_OK;
}
int aleppo_import_reward_scale(aleppo_ctx *c, const double stats[3], const double *returns, size_t E) {
  stub_state_init(c);
  std::memcpy(g_rs.data(), stats, 24);
  std::memcpy(g_rs.data() + 3, returns, E * 8);
  return ALEPPO_OK;
}
int aleppo_export_rollout_state(aleppo_ctx *c, uint8_t *obs, uint64_t words[4], size_t E) {
  stub_state_init(c);
  if (c->t != 0 || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: export_rollout_state mid-rollout");
  g_obs[0] = (uint8_t)c->checksum; // (what the ingested frames left behind)
  std::memcpy(obs, g_obs.data(), E * 4 * 84 * 84);
  words[0] = c->tick;
  words[1] = words[2] = words[3] = 0;
  return ALEPPO_OK;
}
int aleppo_import_rollout_state(aleppo_ctx *c, const uint8_t *obs, const uint64_t words[4], size_t E) {
  stub_state_init(c);
  if (c->t != 0 || c->armed)
    return fail(c, ALEPPO_ERR_RUNTIME, "stub: import_rollout_state mid-rollout");
  std::memcpy(g_obs.data(), obs, E * 4 * 84 * 84);
  c->checksum = g_obs[0];
  c->tick = words[0];
  return ALEPPO_OK;
}
// not the digest of aleppo.h (tests/checkpoint_ref.py restates that one): any function of the state serves the file test.
// ALEPPO_STUB_DIGEST_FLIP=<section> corrupts one word, the way a state that did not survive the import would
int aleppo_state_digest(aleppo_ctx *c, uint64_t out[4]) {
  stub_state_init(c);
  uint64_t p = 0;
  for (size_t i = 0; i < c->params.size(); i += 101) {
    uint32_t b;
    std::memcpy(&b, &c->params[i], 4);
    p += stub_mix(((uint64_t)i << 32) | b);
  }
  out[0] = p;
  out[1] = stub_mix(c->tick) + (uint64_t)g_m1.size();
  out[2] = stub_mix(c->tick ^ 0x55) + (uint8_t)c->checksum;
  uint64_t bits;
  std::memcpy(&bits, &g_rs[0], 8);
  out[3] = stub_mix(bits);
  if (const char *f = std::getenv("ALEPPO_STUB_DIGEST_FLIP"))
    out[std::atoi(f) & 3] ^= 1;
  return ALEPPO_OK;
}
}
