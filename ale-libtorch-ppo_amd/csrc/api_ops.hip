// api_ops.hip - C ABI (include/aleppo.h), the stateless operators: the production kernels on caller arrays, with a
// process-wide arena per device (OpArena / OpScope / DevBuf).
#include "api_internal.hpp"

using namespace aleppo;

// ------------------------------------------------------------------ stateless operators
// Device memory and the stream of the stateless operators: a process-wide arena per device, grown in chunks that are
// never freed, and a non-blocking stream of its own.  (hipFree, hipDeviceSynchronize and null-stream work would wait for,
// or order themselves against, every other stream of the device - a context's stream parked behind its release word
// included)  One operator call at a time per device (mutex); a call's buffers live until it returns.
namespace {
struct OpArena {
  std::mutex mu;
  hipStream_t st = nullptr;
  struct Chunk {
    char *p;
    size_t cap, used;
  };
  std::vector<Chunk> chunks;
};
OpArena &op_arena(int dev) {
  static OpArena a[64];
  return a[dev & 63];
}
struct OpScope;
thread_local OpScope *g_op = nullptr;
struct OpScope {
  OpArena &ar;
  std::unique_lock<std::mutex> lk;
  hipStream_t st = nullptr;
  hipError_t err = hipSuccess;
  explicit OpScope(int dev) : ar(op_arena(dev)), lk(ar.mu) {
    if (!ar.st)
      err = hipStreamCreateWithFlags(&ar.st, hipStreamNonBlocking);
    st = ar.st;
    for (auto &ch : ar.chunks)
      ch.used = 0;
    g_op = this;
  }
  ~OpScope() { g_op = nullptr; }
  hipError_t alloc(void **out, size_t bytes) {
    bytes = (std::max<size_t>(bytes, 16) + 255) / 256 * 256;
    for (auto &ch : ar.chunks)
      if (ch.cap - ch.used >= bytes) {
        *out = ch.p + ch.used;
        ch.used += bytes;
        return hipSuccess;
      }
    OpArena::Chunk ch{nullptr, std::max<size_t>(bytes, (size_t)32 << 20), bytes};
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&ch.p), ch.cap);
    if (e != hipSuccess)
      return e;
    ar.chunks.push_back(ch);
    *out = ch.p;
    return hipSuccess;
  }
  hipError_t sync() { return hipStreamSynchronize(st); }
  hipError_t down(void *dst, const void *src, size_t bytes) { // device -> host, complete on return
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? sync() : e;
  }
};
struct DevBuf { // a buffer of the current operator call (arena memory: nothing to free)
  void *p = nullptr;
  hipError_t up(const void *src, size_t bytes) {
    hipError_t e = g_op->alloc(&p, bytes);
    if (e == hipSuccess && src)
      e = hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, g_op->st);
    else if (e == hipSuccess)
      e = hipMemsetAsync(p, 0, bytes ? bytes : 16, g_op->st);
    // (pageable host sources are staged before the call returns; waiting here keeps the caller's buffer rule simple)
    return e == hipSuccess ? g_op->sync() : e;
  }
  template <class T> T *as() { return static_cast<T *>(p); }
};
} // namespace
#define OPCHK(x)                                                                                                       \
  do {                                                                                                                 \
    hipError_t e_ = (x);                                                                                               \
    if (e_ != hipSuccess)                                                                                              \
      return set_err(nullptr, ALEPPO_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));                         \
  } while (0)

// ai::gae::gae through the production scan kernel: the host arrays are laid out as the rollout's time-major step
// records + value plane (the layout aleppo_finish_rollout hands the kernel), gae_kernel runs with clamp = 0 (ai::gae::gae
// does not clamp; Buffer::get does, buffer.cc:67) and the env-major advantage array comes back as is.
extern "C" int aleppo_gae(int dev, float *advantages, const float *rewards, const float *values,
                          const float *next_values, const uint8_t *terminals, const uint8_t *truncations,
                          const uint8_t *episode_starts, int64_t E, int64_t T, float gamma, float lambda) {
  if (!advantages || !rewards || !values || !next_values || !terminals || !truncations || !episode_starts)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT,
                   "All input tensors must be 2D except next_values which must be 1D."); // gae.cc:8-13
  if (E <= 0 || T <= 0)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "Input tensors must have compatible dimensions."); // :14-21
  int rc = select_device(dev);
  if (rc)
    return rc;
  OpScope op(dev);
  OPCHK(op.err);
  const size_t n = (size_t)E * T, rb = ((size_t)7 * E + 15) / 16 * 16;
  std::vector<uint8_t> rec(rb * T, 0);
  std::vector<float> vtm((size_t)(T + 1) * E);
  for (int64_t t = 0; t < T; ++t) {
    uint8_t *r = rec.data() + (size_t)t * rb;
    for (int64_t e = 0; e < E; ++e) {
      reinterpret_cast<float *>(r)[e] = rewards[e * T + t];
      r[4 * E + e] = terminals[e * T + t];
      r[5 * E + e] = truncations[e * T + t];
      r[6 * E + e] = episode_starts[e * T + t];
      vtm[(size_t)t * E + e] = values[e * T + t];
    }
  }
  for (int64_t e = 0; e < E; ++e)
    vtm[(size_t)T * E + e] = next_values[e];
  DevBuf drec, dv, a, r, m, er;
  OPCHK(drec.up(rec.data(), rec.size()));
  OPCHK(dv.up(vtm.data(), vtm.size() * 4));
  OPCHK(a.up(nullptr, n * 4));
  OPCHK(r.up(nullptr, n * 4));
  OPCHK(m.up(nullptr, n));
  OPCHK(er.up(nullptr, 16));
  launch_gae(op.st, drec.as<uint8_t>(), rb, dv.as<float>(), nullptr, nullptr, a.as<float>(), r.as<float>(), nullptr,
             nullptr, m.as<uint8_t>(), er.as<int>(), (int)E, (int)T, 0, gamma, lambda, /*clamp=*/false);
  int err = 0;
  OPCHK(op.down(&err, er.p, 4));
  if (err)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT,
                   "Episode starts, terminals, and truncations must be mutually exclusive."); // gae.cc:49-53
  OPCHK(op.down(advantages, a.p, n * 4));
  return ALEPPO_OK;
}

// ALEPPO_OPT_REWARD_SCALE through the production kernels: the host arrays are laid out as the rollout's step records, then
// rs_scan_kernel, rs_reduce_kernel and gae_scaled_kernel run as aleppo_finish_rollout runs them (the GAE on a zero value
// plane, its advantages discarded: what is wanted of it is step 5, the scaled rewards in place and the clip count).
extern "C" int aleppo_reward_scale(int dev, float *rewards, const uint8_t *terminals, const uint8_t *truncations,
                                   const uint8_t *episode_starts, int64_t E, int64_t T, float gamma, float clip,
                                   double stats[3], double *returns, float *scale_out, int64_t *clipped_out) {
  if (!rewards || !terminals || !truncations || !episode_starts || !stats || !returns)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "All input tensors must be 2D except returns which must be 1D.");
  if (E <= 0 || T <= 0 || E > INT32_MAX || T > INT32_MAX)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "Input tensors must have compatible dimensions.");
  if (!(clip > 0.f) || !std::isfinite(clip) || !std::isfinite(gamma))
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "reward_scale: clip must be finite and > 0, gamma finite");
  if (!rs_state_valid(stats))
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT,
                   "reward_scale: count must be finite and > 0, mean finite, var finite and >= 0");
  for (int64_t e = 0; e < E; ++e)
    if (!std::isfinite(returns[e]))
      return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "reward_scale: a running return is not finite");
  int rc = select_device(dev);
  if (rc)
    return rc;
  OpScope op(dev);
  OPCHK(op.err);
  const size_t n = (size_t)E * T, rb = ((size_t)7 * E + 15) / 16 * 16;
  std::vector<uint8_t> rec(rb * T, 0);
  for (int64_t t = 0; t < T; ++t) {
    uint8_t *r = rec.data() + (size_t)t * rb;
    for (int64_t e = 0; e < E; ++e) {
      reinterpret_cast<float *>(r)[e] = rewards[e * T + t];
      r[4 * E + e] = terminals[e * T + t];
      r[5 * E + e] = truncations[e * T + t];
      r[6 * E + e] = episode_starts[e * T + t];
    }
  }
  double blk[RS_BLOCK];
  std::memcpy(blk, RS_INITIAL, sizeof(blk));
  blk[RS_COUNT] = stats[0];
  blk[RS_MEAN] = stats[1];
  blk[RS_VAR] = stats[2];
  const int nblk = rs_blocks((int)E);
  DevBuf drec, dblk, gin, gout, part, dv, a, r, m, er;
  OPCHK(drec.up(rec.data(), rec.size()));
  OPCHK(dblk.up(blk, sizeof(blk)));
  OPCHK(gin.up(returns, (size_t)E * 8));
  OPCHK(gout.up(nullptr, (size_t)E * 8));
  OPCHK(part.up(nullptr, (size_t)nblk * 4 * 8));
  OPCHK(dv.up(nullptr, (size_t)(T + 1) * E * 4));
  OPCHK(a.up(nullptr, n * 4));
  OPCHK(r.up(nullptr, n * 4));
  OPCHK(m.up(nullptr, n));
  OPCHK(er.up(nullptr, 16));
  launch_rs_scan(op.st, drec.as<uint8_t>(), rb, gin.as<double>(), gout.as<double>(), part.as<double>(), er.as<int>(),
                 (int)E, (int)T, gamma);
  launch_rs_reduce(op.st, part.as<double>(), nblk, nullptr, dblk.as<double>(), er.as<int>());
  launch_gae_scaled(op.st, drec.as<uint8_t>(), rb, dv.as<float>(), nullptr, nullptr, a.as<float>(), r.as<float>(),
                    nullptr, nullptr, m.as<uint8_t>(), er.as<int>(), (int)E, (int)T, 0, gamma, 0.f, dblk.as<double>(),
                    clip, false);
  int err = 0;
  OPCHK(op.down(&err, er.p, 4));
  if (err)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT,
                   "Episode starts, terminals, and truncations must be mutually exclusive."); // gae.cc:49-53
  OPCHK(op.down(rec.data(), drec.p, rec.size()));
  OPCHK(op.down(blk, dblk.p, sizeof(blk)));
  OPCHK(op.down(returns, gout.p, (size_t)E * 8));
  for (int64_t t = 0; t < T; ++t)
    for (int64_t e = 0; e < E; ++e)
      rewards[e * T + t] = reinterpret_cast<const float *>(rec.data() + (size_t)t * rb)[e];
  stats[0] = blk[RS_COUNT];
  stats[1] = blk[RS_MEAN];
  stats[2] = blk[RS_VAR];
  if (scale_out)
    *scale_out = (float)blk[RS_SCALE];
  if (clipped_out) {
    unsigned long long cl;
    std::memcpy(&cl, &blk[RS_CLIPPED], 8);
    *clipped_out = (int64_t)cl;
  }
  return ALEPPO_OK;
}

extern "C" int aleppo_vision_resize_area(int dev, const float *images, float *out, int64_t n) {
  if (!images || !out || n <= 0)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "bad argument");
  int rc = select_device(dev);
  if (rc)
    return rc;
  OpScope op(dev);
  OPCHK(op.err);
  DevBuf i, o;
  OPCHK(i.up(images, (size_t)n * RAW_H * RAW_W * 4));
  OPCHK(o.up(nullptr, (size_t)n * FRAME_PIX * 4));
  launch_area_resize(op.st, i.as<float>(), o.as<float>(), n);
  OPCHK(op.down(out, o.p, (size_t)n * FRAME_PIX * 4));
  return ALEPPO_OK;
}
extern "C" int aleppo_vision_rgb_to_gray(int dev, const float *images, float *out, int64_t n) {
  if (!images || !out || n <= 0)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "bad argument");
  int rc = select_device(dev);
  if (rc)
    return rc;
  OpScope op(dev);
  OPCHK(op.err);
  DevBuf i, o;
  OPCHK(i.up(images, (size_t)n * 3 * FRAME_PIX * 4));
  OPCHK(o.up(nullptr, (size_t)n * FRAME_PIX * 4));
  launch_rgb_to_gray(op.st, i.as<float>(), o.as<float>(), n);
  OPCHK(op.down(out, o.p, (size_t)n * FRAME_PIX * 4));
  return ALEPPO_OK;
}

// The two frame operators run the production ingest kernel on a scratch pair of observation slots
// ([n][2 slots][7056] packed stacks, slot 0 = before, slot 1 = after) and convert at the boundary.
static int ingest_op(bool raw, const uint8_t *frames, size_t frame_bytes, const uint8_t *lut256,
                     const uint8_t *obs_nchw_in, const uint8_t *start, uint8_t *obs_nchw_out, int64_t n) {
  if (n > MAX_ENVS_PER_RANK)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "at most 8192 environments per call");
  OpScope &op = *g_op; // opened by the caller
  DevBuf f, l, st, nchw, slots;
  OPCHK(f.up(frames, frame_bytes));
  uint8_t ident[256];
  for (int i = 0; i < 256; ++i)
    ident[i] = (uint8_t)i;
  OPCHK(l.up(lut256 ? lut256 : ident, 256));
  std::vector<uint8_t> ones;
  if (!start) {
    ones.assign((size_t)n, 1);
    start = ones.data();
  }
  OPCHK(st.up(start, (size_t)n));
  OPCHK(nchw.up(obs_nchw_in, (size_t)n * 4 * FRAME_PIX)); // (zeros when there is no previous stack)
  OPCHK(slots.up(nullptr, (size_t)n * 2 * FRAME_PIX * 4));
  launch_obs_pack(op.st, nchw.as<uint8_t>(), slots.as<uint32_t>(), n, SampleMap{1, 2L * FRAME_PIX, 0, 0, 0});
  launch_ingest(op.st, raw, f.as<uint8_t>(), l.as<uint8_t>(), st.as<uint8_t>(), nullptr, slots.as<uint32_t>(), (int)n,
                2, 0, 1);
  launch_obs_unpack(op.st, slots.as<uint32_t>(), nchw.as<uint8_t>(), n, SampleMap{1, 2L * FRAME_PIX, 0, FRAME_PIX, 0});
  OPCHK(op.sync());
  OPCHK(op.down(obs_nchw_out, nchw.p, (size_t)n * 4 * FRAME_PIX));
  return ALEPPO_OK;
}
extern "C" int aleppo_preprocess(int dev, const uint8_t *raw_pairs, const uint8_t *lut256, uint8_t *out, int64_t n) {
  if (!raw_pairs || !out || n <= 0)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "bad argument");
  int rc = select_device(dev);
  if (rc)
    return rc;
  OpScope op(dev);
  OPCHK(op.err);
  // every environment in an episode-start slot: the new frame is broadcast to all four stack planes; plane 0 is it
  std::vector<uint8_t> stack((size_t)n * 4 * FRAME_PIX);
  rc = ingest_op(true, raw_pairs, (size_t)n * 2 * RAW_H * RAW_W, lut256, nullptr, nullptr, stack.data(), n);
  if (rc)
    return rc;
  for (int64_t e = 0; e < n; ++e)
    std::memcpy(out + (size_t)e * FRAME_PIX, stack.data() + (size_t)e * 4 * FRAME_PIX, FRAME_PIX);
  return ALEPPO_OK;
}
extern "C" int aleppo_update_observations(int dev, uint8_t *observations, const uint8_t *frames,
                                          const uint8_t *episode_start, int64_t E) {
  if (!observations || !frames || !episode_start || E <= 0)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "bad argument");
  int rc = select_device(dev);
  if (rc)
    return rc;
  OpScope op(dev);
  OPCHK(op.err);
  return ingest_op(false, frames, (size_t)E * FRAME_PIX, nullptr, observations, episode_start, observations, E);
}

// ai::ppo::losses::compute through the production head kernel (head_train_kernel<float>): the caller's raw logits and
// values become the first A + 1 components of a 32-wide hidden vector and the head weights an identity block, so the
// kernel's "head linear layer" reproduces them exactly (x * 1 + 0 + ... is exact in fp32) and its dh output IS
// (dlogits, dvalue).  The scalar loss is the masked mean the update reports (metrics_reduce_kernel, as aleppo_train).
extern "C" int aleppo_ppo_loss(int dev, const float *logits, const float *old_lp, const int64_t *actions,
                               const float *advantages, const float *values, const float *returns,
                               const uint8_t *masks, int64_t B, int64_t A, float clip, float c_v, float c_e,
                               float *loss, float *clipped, float *value_losses, float *entropies, float *total_losses,
                               float *ratio, float *dlogits, float *dvalues) {
  if (!logits || !old_lp || !actions || !advantages || !values || !returns || !masks || B <= 0 || A <= 0 ||
      A > MAX_ACTIONS)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "bad argument");
  std::vector<int> a32((size_t)B);
  for (int64_t i = 0; i < B; ++i) {
    if (actions[i] < 0 || actions[i] >= A)
      return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "action index out of range");
    a32[(size_t)i] = (int)actions[i];
  }
  int rc = select_device(dev);
  if (rc)
    return rc;
  OpScope op(dev);
  OPCHK(op.err);
  constexpr int H = 32; // >= MAX_ACTIONS + 1
  std::vector<float> h((size_t)B * H, 0.f), Wh((size_t)(A + 1) * H, 0.f), bh((size_t)A + 1, 0.f);
  for (int64_t i = 0; i < B; ++i) {
    for (int64_t k = 0; k < A; ++k)
      h[(size_t)i * H + k] = logits[i * A + k];
    h[(size_t)i * H + A] = values[i];
  }
  for (int64_t k = 0; k <= A; ++k)
    Wh[(size_t)k * H + k] = 1.0f;
  const int nblk = (int)std::min<int64_t>(MAXS_HEAD, (B + 15) / 16);
  DevBuf dh_in, dW, db, ol, ac, ad, re, ma, cnt, dh_out, ps, sw, sb, red, hyp;
  OPCHK(dh_in.up(h.data(), h.size() * 4));
  OPCHK(dW.up(Wh.data(), Wh.size() * 4));
  OPCHK(db.up(bh.data(), bh.size() * 4));
  OPCHK(ol.up(old_lp, (size_t)B * A * 4));
  OPCHK(ac.up(a32.data(), (size_t)B * 4));
  OPCHK(ad.up(advantages, (size_t)B * 4));
  OPCHK(re.up(returns, (size_t)B * 4));
  OPCHK(ma.up(masks, (size_t)B));
  OPCHK(cnt.up(nullptr, 16));
  OPCHK(dh_out.up(nullptr, (size_t)B * H * 4));
  OPCHK(ps.up(nullptr, (size_t)7 * B * 4)); // aleppo_metric_field 0-6 (5-6 are not returned)
  OPCHK(sw.up(nullptr, (size_t)nblk * (A + 1) * H * 4));
  OPCHK(sb.up(nullptr, (size_t)nblk * (A + 1) * 4));
  OPCHK(red.up(nullptr, 8 * 4));
  float hblk[HYPER_BLOCK] = {}; // the kernel reads its hyper-parameters from a device block (common.hpp HYPER_*)
  hblk[HYPER_CLIP] = clip, hblk[HYPER_VCLIP] = clip, hblk[HYPER_CV] = c_v, hblk[HYPER_CE] = c_e;
  OPCHK(hyp.up(hblk, sizeof(hblk)));
  launch_mask_count(op.st, ma.as<uint8_t>(), cnt.as<float>(), B, 1); // losses.cc:19 masks.sum()
  float *p = ps.as<float>();
  HeadTrainArgs ha{}; // (hparts = 1, float planes: the struct's defaults)
  ha.h = dh_in.as<float>();
  ha.Wh = dW.as<float>();
  ha.bh = db.as<float>();
  ha.act = ac.as<int>();
  ha.oldlp = ol.as<float>();
  ha.adv = ad.as<float>();
  ha.ret = re.as<float>();
  ha.vold = nullptr;
  ha.mask = ma.as<uint8_t>();
  ha.mask_count = cnt.as<float>();
  ha.dh = dh_out.p;
  ha.prec = ALEPPO_FP32;
  ha.ps_total = p;
  ha.ps_clipped = p + B;
  ha.ps_value = p + 2 * B;
  ha.ps_entropy = p + 3 * B;
  ha.ps_ratio = p + 4 * B;
  ha.ps_kl = p + 5 * B;
  ha.ps_cf = p + 6 * B;
  ha.slab_w = sw.as<float>();
  ha.slab_b = sb.as<float>();
  ha.nblk = nblk;
  ha.B = B;
  ha.H = H;
  ha.A = (int)A;
  launch_head_train(op.st, ha, hyp.as<float>());
  launch_metrics_reduce(op.st, p, (size_t)B, ma.as<uint8_t>(), B, 1, 1, red.as<float>());
  OPCHK(op.sync());
  float r8[8];
  OPCHK(op.down(r8, red.p, sizeof(r8)));
  if (loss)
    *loss = r8[0] / r8[5];
  float *per[5] = {total_losses, clipped, value_losses, entropies, ratio}; // order of the kernel's metric planes
  for (int k = 0; k < 5; ++k)
    if (per[k])
      OPCHK(op.down(per[k], p + (size_t)k * B, (size_t)B * 4));
  if (dlogits || dvalues) {
    std::vector<float> d((size_t)B * H);
    OPCHK(op.down(d.data(), dh_out.p, d.size() * 4));
    for (int64_t i = 0; i < B; ++i) {
      if (dlogits)
        for (int64_t k = 0; k < A; ++k)
          dlogits[i * A + k] = d[(size_t)i * H + k];
      if (dvalues)
        dvalues[i] = d[(size_t)i * H + A];
    }
  }
  return ALEPPO_OK;
}
// multinomial(probs, 1, true) given its noise through the production acting head (infer_head_kernel in its probs mode:
// same division, same wave arg-max, same stores)
extern "C" int aleppo_sample(int dev, const float *probs, const float *q, int64_t *actions, int64_t E, int64_t A) {
  if (!probs || !q || !actions || E <= 0 || A <= 0 || A > MAX_ACTIONS)
    return set_err(nullptr, ALEPPO_ERR_INVALID_ARGUMENT, "bad argument");
  int rc = select_device(dev);
  if (rc)
    return rc;
  OpScope op(dev);
  OPCHK(op.err);
  DevBuf p, qq, a;
  OPCHK(p.up(probs, (size_t)E * A * 4));
  OPCHK(qq.up(q, (size_t)E * A * 4));
  OPCHK(a.up(nullptr, (size_t)E * 4));
  launch_infer_head(op.st, nullptr, nullptr, nullptr, nullptr, qq.as<float>(), 0, 0, nullptr, nullptr, a.as<int>(),
                    nullptr, nullptr, 0, (int)E, 32, (int)A, p.as<float>());
  std::vector<int> a32((size_t)E);
  OPCHK(op.down(a32.data(), a.p, (size_t)E * 4));
  for (int64_t e = 0; e < E; ++e)
    actions[e] = a32[(size_t)e];
  return ALEPPO_OK;
}
