// api_rollout.hip - C ABI (include/aleppo.h), the rollout protocol: act, push, record, step, arm / release, replay, the
// gray LUT, aleppo_finish_rollout (GAE), and ALEPPO_OPT_REWARD_SCALE's state with its import and export.
#include "api_internal.hpp"

using namespace aleppo;

// ------------------------------------------------------------------ rollout
// The acting forward at n samples of obs addressed by map, into the caller's scratch: conv stack + split-K fc; the head
// kernel finishes the fc reduction.  pv: the parameter set it reads (the rollout: live_view; the evaluation lanes:
// eval_view).  profiled: the rollout's launches are bracketed for --profile, evaluation's are not.
void aleppo::act_forward(aleppo_ctx *c, const ParamView &pv, uint32_t *obs, SampleMap map, void *a1, void *a2, void *a3,
                         float *hpart, int n, bool profiled) {
  const auto begin = [&](int cls) {
    if (profiled)
      prof_begin(c, cls);
  };
  const auto end = [&](int cls) {
    if (profiled)
      prof_end(c, cls);
  };
  const bool rollout = a3 == c->a3; // (the evaluation lanes bring scratch of their own: no mark, no ALEPPO_OPT_ACT_STORE)
  if (c->prec == ALEPPO_BF16 && use_patch_kernels()) { // one launch: a1/a2 never leave LDS (but ALEPPO_OPT_ACT_STORE)
    const bool store = rollout && c->act_store;
    begin(ALEPPO_K_CONV1_FWD);
    patch_act_convs(c->stream, obs, map, Pcw(c, pv, P_W1), Pf(c, pv, P_B1), Pcw(c, pv, P_W2), Pf(c, pv, P_B2),
                    Pcw(c, pv, P_W3), Pf(c, pv, P_B3), a3, n, 0, nullptr, nullptr, nullptr, 0, nullptr,
                    store ? a1 : nullptr, store ? a2 : nullptr);
    end(ALEPPO_K_CONV1_FWD);
    if (rollout)
      c->acted = Ctx::ActMark{n, store};
  } else {
    if (rollout)
      c->acted = Ctx::ActMark{n, true};
    begin(ALEPPO_K_CONV1_FWD);
    conv1_fwd(c->stream, c->prec, obs, map, Pcw(c, pv, P_W1), Pf(c, pv, P_B1), a1, n);
    end(ALEPPO_K_CONV1_FWD);
    begin(ALEPPO_K_CONV2_FWD);
    conv2_fwd(c->stream, c->prec, a1, Pcw(c, pv, P_W2), Pf(c, pv, P_B2), a2, n);
    end(ALEPPO_K_CONV2_FWD);
    begin(ALEPPO_K_CONV3_FWD);
    conv3_fwd(c->stream, c->prec, a2, Pcw(c, pv, P_W3), Pf(c, pv, P_B3), a3, n);
    end(ALEPPO_K_CONV3_FWD);
  }
  begin(ALEPPO_K_FC_FWD);
  fc_fwd_splitk(c->stream, c->prec, a3, Pcw(c, pv, P_WFC), hpart, n, c->H);
  end(ALEPPO_K_FC_FWD);
}

static int do_act(aleppo_ctx *c, const float *noise, int slot, void *logits_dst, void *values_dst, int *actions_dst,
                  bool publish) {
  c->bwd.B = 0; // (a1 / a2 / a3 are the acting scratch too: aleppo_export_backward has nothing to read any more)
  if (c->pre_acted != slot)
    act_forward(c, live_view(c), c->obs, slot_map(c, slot), c->a1, c->a2, c->a3, c->hpart, c->E, true);
  c->pre_acted = -1; // (consumed; a3 / hpart are scratch again)
  const float *dn = nullptr;
  if (noise) { // (two staging halves: with a gated replay the next slot is enqueued before this copy has run)
    const size_t half = (size_t)(c->noise_flip++ & 1u) * c->E * c->A;
    std::memcpy(c->h_noise + half, noise, (size_t)c->E * c->A * 4);
    HIPCHK(c, hipMemcpyAsync(c->d_noise + half, c->h_noise + half, (size_t)c->E * c->A * 4, hipMemcpyHostToDevice,
                             c->stream));
    dn = c->d_noise + half;
  }
  int64_t *pinned_dev = nullptr;
  HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void **>(&pinned_dev), c->h_actions, 0));
  prof_begin(c, ALEPPO_K_INFER_HEAD);
  if (publish)
    c->ticket++;
  if (c->dbg_no_publish)
    pinned_dev = nullptr;
  launch_infer_head(c->stream, c->hpart, Pf(c, P_BFC), Pf(c, P_WH), Pf(c, P_BH), dn, c->cfg.seed, c->rng_counter++,
                    logits_dst, values_dst, actions_dst, pinned_dev, publish ? c->d_done : nullptr, c->ticket, c->E, c->H,
                    c->A, nullptr, c->rt16);
  prof_end(c, ALEPPO_K_INFER_HEAD);
  HIPCHK(c, hipGetLastError());
  return ALEPPO_OK;
}

// enqueue slot c->t's acting kernels (whatever aleppo_step has not already run) + the head that publishes the actions
int aleppo::act_enqueue(aleppo_ctx *c, const float *noise, int slot) {
  if (slot >= c->T)
    return set_err(c, ALEPPO_ERR_RUNTIME, "rollout buffer is full: call aleppo_finish_rollout");
  if (slot == 0 && c->need_carry) { // slot T of the previous rollout is this rollout's first observation
    launch_copy_slot(c->stream, c->obs, c->E, c->T + 1, c->T, 0);
    c->need_carry = false;
  }
  const size_t o = (size_t)slot * c->E;
  return do_act(c, noise, slot, rp(c, c->logits_tm, o * c->A), rp(c, c->values_tm, o), c->actions_tm + o, true);
}
// The gate's exit condition fired: the stream ran (or will run) a slot whose frames the host never released.
static int check_gate(aleppo_ctx *c) {
  const unsigned long long rep = __atomic_load_n(c->h_go + 1, __ATOMIC_ACQUIRE);
  if (!rep)
    return ALEPPO_OK;
  char b[256];
  std::snprintf(b, sizeof b,
                "the slot-ahead gate %llu was not released within %.0f ms (released so far: %llu): the device went on "
                "without the host's frames",
                rep, (double)c->gate_timeout_ticks / 1e5, __atomic_load_n(c->h_go, __ATOMIC_RELAXED));
  return fail_ctx(c, ALEPPO_ERR_RUNTIME, b);
}
// wait for the ticket the head kernel publishes after the actions (bounded spin, then a real sync)
// stream_parked: the stream already holds the NEXT slot behind the release word (gated replay) - a stream sync would
// wait for a release only this thread can give, so the wait only spins (and yields once the slot is clearly a long one)
static int act_wait(aleppo_ctx *c, long long ticket, bool stream_parked = false) {
  volatile long long *tk = reinterpret_cast<volatile long long *>(c->h_actions + c->E);
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  bool slow = false;
  if (c->dbg_no_publish)
    HIPCHK(c, hipStreamSynchronize(c->stream));
  while (!c->dbg_no_publish && *tk != ticket) {
    if (slow)
      std::this_thread::yield();
    else
      __builtin_ia32_pause();
    if ((++spins & 1023u) == 0) {
      const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (slow) {
        if (int rc = check_gate(c))
          return rc;
        // Backstop only (no hand-off of this design waits on anything but the head kernel in front of it): say what the
        // stream and the hand-off words look like, so that a missing ticket can be told from a stuck stream.
        if (waited > 60.0 + (double)c->gate_timeout_ticks / 1e8) {
          const hipError_t q = hipStreamQuery(c->stream);
          unsigned int done = 0xFFFFFFFFu; // the head's arrival counter, read on the (idle) side stream
          if ((c->comm_stream || hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking) == hipSuccess) &&
              hipMemcpyAsync(c->h_err + 1, c->d_done, 4, hipMemcpyDeviceToHost, c->comm_stream) == hipSuccess) {
            for (int i = 0; i < 1000 && hipStreamQuery(c->comm_stream) == hipErrorNotReady; ++i)
              std::this_thread::sleep_for(std::chrono::milliseconds(1));
            if (hipStreamQuery(c->comm_stream) == hipSuccess)
              done = (unsigned int)c->h_err[1];
          }
          char b[384];
          std::snprintf(b, sizeof b,
                        "the acting head's ticket did not arrive within %.0f s: expected %lld, pinned word %lld, release "
                        "word %llu, last gate %llu, gate report %llu, head arrival counter %u of %d, stream %s",
                        waited, ticket, (long long)*tk, __atomic_load_n(c->h_go, __ATOMIC_RELAXED), c->go_seq,
                        __atomic_load_n(c->h_go + 1, __ATOMIC_RELAXED), done, (c->E + 3) / 4,
                        q == hipSuccess ? "idle" : q == hipErrorNotReady ? "busy" : hipGetErrorString(q));
          return fail_ctx(c, ALEPPO_ERR_RUNTIME, b);
        }
      } else if (waited > 2e-3) {
        if (stream_parked) {
          slow = true;
          continue;
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        break;
      }
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return check_gate(c);
}
extern "C" int aleppo_act(aleppo_ctx *c, const float *noise, const int64_t **actions_pinned) {
  CHECK_CTX(c);
  int rc = ALEPPO_OK;
  if (c->act_queued_slot == c->t && c->t < c->T) { // enqueued by aleppo_arm_step (with ITS noise): only the wait is left
    c->act_queued_slot = -1;
    rc = act_wait(c, c->act_queued_ticket);
  } else {
    rc = act_enqueue(c, noise, c->t);
    if (rc == ALEPPO_OK)
      rc = act_wait(c, c->ticket);
  }
  if (rc)
    return rc;
  if (actions_pinned)
    *actions_pinned = c->h_actions;
  return ALEPPO_OK;
}

// Where a kernel reads the caller's frames.  ALEPPO_DEVICE: where they are; ALEPPO_HOST_MAPPED: the page-locked host buffer
// in place, through its device address; ALEPPO_HOST: *dev_frames stays null - the caller stages them in its own buffers.
// Touches nothing but *dev_frames and, on a refusal, the context's error.
int aleppo::resolve_frames(aleppo_ctx *c, const uint8_t *frames, int location, const uint8_t **dev_frames) {
  *dev_frames = nullptr;
  if (location == ALEPPO_DEVICE) {
    if (reinterpret_cast<uintptr_t>(frames) % 16)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "device frames must be 16-byte aligned");
    *dev_frames = frames;
  } else if (location == ALEPPO_HOST_MAPPED) {
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, const_cast<uint8_t *>(frames), 0) != hipSuccess || !dp)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                     "ALEPPO_HOST_MAPPED frames must lie in mapped page-locked host memory (hipHostMalloc / hipHostRegister)");
    if (reinterpret_cast<uintptr_t>(dp) % 16)
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "mapped frames must be 16-byte aligned");
    *dev_frames = static_cast<const uint8_t *>(dp);
  } else if (location != ALEPPO_HOST) {
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "unknown frame location");
  }
  return ALEPPO_OK;
}

static int upload_frames(aleppo_ctx *c, const uint8_t *frames, int kind, int location, const uint8_t **dev_frames) {
  const int rc = resolve_frames(c, frames, location, dev_frames);
  if (rc || *dev_frames)
    return rc;
  const size_t bytes = (size_t)c->E * (kind == ALEPPO_FRAMES_RAW_PAIR ? 2 * RAW_H * RAW_W : FRAME_PIX);
  std::memcpy(c->h_frames, frames, bytes);
  HIPCHK(c, hipMemcpyAsync(c->d_frames, c->h_frames, bytes, hipMemcpyHostToDevice, c->stream));
  *dev_frames = c->d_frames;
  return ALEPPO_OK;
}

static int do_push(aleppo_ctx *c, const uint8_t *frames, int kind, int location, const uint8_t *episode_start) {
  if (!frames || !episode_start)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  if (kind != ALEPPO_FRAMES_84 && kind != ALEPPO_FRAMES_RAW_PAIR)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "unknown frame kind");
  if (c->t >= c->T)
    return set_err(c, ALEPPO_ERR_RUNTIME, "rollout buffer is full: call aleppo_finish_rollout");
  // staging buffers are reused every step: wait for the previous upload (normally long finished: act() syncs)
  HIPCHK(c, hipEventSynchronize(c->ev_tmp));
  uint8_t *hs = c->h_step + c->step_rec_bytes;
  std::memcpy(hs, episode_start, c->E);
  HIPCHK(c, hipMemcpyAsync(c->d_start, hs, c->E, hipMemcpyHostToDevice, c->stream));
  const uint8_t *df = nullptr;
  int rc = upload_frames(c, frames, kind, location, &df);
  if (rc)
    return rc;
  c->pre_acted = -1;
  prof_begin(c, ALEPPO_K_INGEST);
  launch_ingest(c->stream, kind == ALEPPO_FRAMES_RAW_PAIR, df, c->lut, c->d_start, nullptr, c->obs, c->E, c->T + 1,
                c->t, c->t + 1);
  prof_end(c, ALEPPO_K_INGEST);
  HIPCHK(c, hipGetLastError());
  return ALEPPO_OK;
}
static int do_record(aleppo_ctx *c, const float *rewards, const uint8_t *terminated, const uint8_t *truncated,
                     const uint8_t *episode_start) {
  if (!rewards || !terminated || !truncated || !episode_start)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  if (c->t >= c->T)
    return set_err(c, ALEPPO_ERR_RUNTIME, "rollout buffer is full: call aleppo_finish_rollout");
  const int E = c->E;
  std::memcpy(c->h_step, rewards, (size_t)E * 4);
  std::memcpy(c->h_step + 4 * (size_t)E, terminated, E);
  std::memcpy(c->h_step + 5 * (size_t)E, truncated, E);
  std::memcpy(c->h_step + 6 * (size_t)E, episode_start, E);
  std::memcpy(c->h_rec + (size_t)c->t * c->step_rec_bytes, c->h_step, (size_t)7 * E); // uploaded at finish_rollout
  c->t++;
  rec_tick(c, ALEPPO_REC_ROLLOUT);
  return ALEPPO_OK;
}

// the GPU side of a step: slot t's new frames -> observation slot t + 1 (+ its convolutions and fc where fused).  The
// episode-start flags come as a kernel-argument bitmask (sb) or, for a step enqueued before the emulator has produced
// them (aleppo_arm_step), as bytes in mapped host memory (start_mapped: host pointer, start_dev: its device address), or,
// for a slot the device-resident environments stepped (aleppo_env_rollout), as bytes in device memory (start_device).
int aleppo::step_enqueue(aleppo_ctx *c, const uint8_t *df, int kind, int location, const StartBits *sb,
                         const uint8_t *start_mapped, int t, const uint8_t *start_device) {
  const int E = c->E;
  uint8_t *start_dev = const_cast<uint8_t *>(start_device); // (only ever read)
  if (start_mapped)
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void **>(&start_dev), const_cast<uint8_t *>(start_mapped), 0));
  // Fused ingest pays for given 84x84 frames (15.7 -> 14.4 ms per 128-slot rollout+update with the frames in mapped host
  // memory) and for raw pairs read over the bus (one environment's pair is staged by ONE workgroup with nine 16-byte
  // loads per thread in flight).  Raw pairs resident in HBM stay on the stand-alone ingest kernel: there the palette
  // lookups of 67 K source bytes per environment are spread over all 256 CUs instead of the 128 acting workgroups
  // (measured: 5.01 vs 5.10 ms per rollout).
  const bool fuse = c->prec == ALEPPO_BF16 && use_patch_kernels() && c->tune.fused_act &&
                    !(kind == ALEPPO_FRAMES_RAW_PAIR && location != ALEPPO_HOST_MAPPED && c->tune.fused_act < 2);
  c->bwd.B = 0; // (as in do_act: the fused launch below writes a3)
  if (fuse) {
    // ONE launch forms slot t+1's stack from the new frames AND runs conv1 -> conv2 -> conv3 on it, then the split-K fc:
    // when the next aleppo_act (or aleppo_finish_rollout's bootstrap) arrives only the head + sampling kernel is left.
    // A slot's critical path is 3 dependent launches instead of 4 and the stack skips one HBM round trip.
    const SampleMap map = slot_map(c, t + 1);
    prof_begin(c, ALEPPO_K_ACT_FUSED);
    patch_act_convs(c->stream, c->obs, map, Pcw(c, P_W1), Pf(c, P_B1), Pcw(c, P_W2), Pf(c, P_B2), Pcw(c, P_W3),
                    Pf(c, P_B3), c->a3, E, kind == ALEPPO_FRAMES_RAW_PAIR ? 2 : 1, df, c->lut, sb, -(long)FRAME_PIX,
                    start_dev, c->act_store ? c->a1 : nullptr, c->act_store ? c->a2 : nullptr);
    c->acted = Ctx::ActMark{E, c->act_store};
    prof_end(c, ALEPPO_K_ACT_FUSED);
    prof_begin(c, ALEPPO_K_FC_FWD);
    fc_fwd_splitk(c->stream, c->prec, c->a3, Pcw(c, P_WFC), c->hpart, E, c->H);
    prof_end(c, ALEPPO_K_FC_FWD);
    c->pre_acted = t + 1;
  } else {
    if (start_mapped) // (every thread of the stand-alone kernel reads its flag: from HBM, not across the bus)
      HIPCHK(c, hipMemcpyAsync(c->d_start, start_mapped, E, hipMemcpyHostToDevice, c->stream));
    prof_begin(c, ALEPPO_K_INGEST);
    launch_ingest(c->stream, kind == ALEPPO_FRAMES_RAW_PAIR, df, c->lut,
                  start_device ? start_device : start_mapped ? c->d_start : nullptr, sb, c->obs, E, c->T + 1, t, t + 1);
    prof_end(c, ALEPPO_K_INGEST);
    c->pre_acted = -1;
  }
  return ALEPPO_OK;
}

extern "C" int aleppo_push_frames(aleppo_ctx *c, const uint8_t *frames, int kind, int location,
                                  const uint8_t *episode_start) {
  CHECK_CTX(c);
  int rc = do_push(c, frames, kind, location, episode_start);
  if (rc == ALEPPO_OK)
    HIPCHK(c, hipEventRecord(c->ev_tmp, c->stream));
  return rc;
}
extern "C" int aleppo_record_step(aleppo_ctx *c, const float *rewards, const uint8_t *terminated,
                                  const uint8_t *truncated, const uint8_t *episode_start) {
  CHECK_CTX(c);
  HIPCHK(c, hipEventSynchronize(c->ev_tmp));
  return do_record(c, rewards, terminated, truncated, episode_start);
}
extern "C" int aleppo_step(aleppo_ctx *c, const uint8_t *frames, int kind, int location, const float *rewards,
                           const uint8_t *terminated, const uint8_t *truncated, const uint8_t *episode_start) {
  CHECK_CTX(c);
  if (!frames || !rewards || !terminated || !truncated || !episode_start)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  if (kind != ALEPPO_FRAMES_84 && kind != ALEPPO_FRAMES_RAW_PAIR)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "unknown frame kind");
  if (c->t >= c->T)
    return set_err(c, ALEPPO_ERR_RUNTIME, "rollout buffer is full: call aleppo_finish_rollout");
  // No per-slot upload: the scalars of rollout.cc:212-227 are packed into a pinned host record and reach the
  // device in ONE copy at finish_rollout (only GAE reads them); the episode-start flags ingest needs now
  // travel as a kernel-argument bitmask.
  const int E = c->E;
  uint8_t *rec = c->h_rec + (size_t)c->t * c->step_rec_bytes;
  std::memcpy(rec, rewards, (size_t)E * 4);
  std::memcpy(rec + 4 * (size_t)E, terminated, E);
  std::memcpy(rec + 5 * (size_t)E, truncated, E);
  std::memcpy(rec + 6 * (size_t)E, episode_start, E);
  StartBits sb{};
  for (int e = 0; e < E; ++e)
    if (episode_start[e])
      sb.w[e >> 5] |= 1u << (e & 31);
  const uint8_t *df = nullptr;
  if (location == ALEPPO_HOST)
    HIPCHK(c, hipEventSynchronize(c->ev_tmp)); // frame staging reuse guard
  int rc = upload_frames(c, frames, kind, location, &df);
  if (rc)
    return rc;
  rc = step_enqueue(c, df, kind, location, &sb, nullptr, c->t);
  if (rc)
    return rc;
  HIPCHK(c, hipGetLastError());
  if (location == ALEPPO_HOST)
    HIPCHK(c, hipEventRecord(c->ev_tmp, c->stream));
  c->t++;
  rec_tick(c, ALEPPO_REC_ROLLOUT);
  return ALEPPO_OK;
}
// Park the main stream: everything enqueued after this runs once the host has stored a number >= the returned sequence
// number into the release word (gate_kernel; it gives up after gate_timeout_ticks and reports, see check_gate).
static int gate_enqueue(aleppo_ctx *c) {
  unsigned long long *go_dev = nullptr;
  HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void **>(&go_dev), c->h_go, 0));
  launch_gate(c->stream, go_dev, c->go_seq + 1, c->gate_timeout_ticks);
  HIPCHK(c, hipGetLastError());
  c->go_seq++; // (only once the gate is on the stream: an error above leaves nothing to release)
  return ALEPPO_OK;
}
static inline void gate_release(aleppo_ctx *c) { __atomic_store_n(c->h_go, c->go_seq, __ATOMIC_RELEASE); }

// Live loops one slot ahead (the replay loop below does the same with a recorded trace): see include/aleppo.h.
extern "C" int aleppo_arm_step(aleppo_ctx *c, const uint8_t *frames, int kind, const uint8_t *episode_start_mapped,
                               const float *noise_next) {
  CHECK_CTX(c);
  if (!frames || !episode_start_mapped)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  if (kind != ALEPPO_FRAMES_84 && kind != ALEPPO_FRAMES_RAW_PAIR)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "unknown frame kind");
  if (c->t >= c->T)
    return set_err(c, ALEPPO_ERR_RUNTIME, "rollout buffer is full: call aleppo_finish_rollout");
  if (c->prof_on || c->dbg_no_publish)
    return set_err(c, ALEPPO_ERR_RUNTIME, "aleppo_arm_step is not available while per-kernel profiling is on");
  const uint8_t *df = nullptr;
  int rc = upload_frames(c, frames, kind, ALEPPO_HOST_MAPPED, &df);
  if (rc)
    return rc;
  void *sdev = nullptr;
  if (hipHostGetDevicePointer(&sdev, const_cast<uint8_t *>(episode_start_mapped), 0) != hipSuccess || !sdev)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "episode_start_mapped must lie in mapped page-locked host memory (aleppo_host_alloc)");
  rc = gate_enqueue(c);
  if (rc)
    return rc;
  rc = step_enqueue(c, df, kind, ALEPPO_HOST_MAPPED, nullptr, episode_start_mapped, c->t);
  if (rc == ALEPPO_OK && c->t + 1 < c->T) {
    rc = act_enqueue(c, noise_next, c->t + 1);
    c->act_queued_slot = c->t + 1;
    c->act_queued_ticket = c->ticket;
  }
  if (rc || hipGetLastError() != hipSuccess) {
    // part of the slot is on the stream behind the gate and must not run on frames that do not exist yet: the context
    // is failed (sticky), the gate released so that the stream drains (the caller's buffers stay referenced until
    // aleppo_destroy)
    const std::string why = rc ? c->err : std::string("a launch failed");
    return fail_ctx(c, rc ? rc : ALEPPO_ERR_HIP, "aleppo_arm_step: " + why);
  }
  c->armed = true;
  c->armed_start = episode_start_mapped;
  return ALEPPO_OK;
}
extern "C" int aleppo_release_step(aleppo_ctx *c, const float *rewards, const uint8_t *terminated,
                                   const uint8_t *truncated) {
  CHECK_CTX_ANY(c);
  if (!c->armed)
    return set_err(c, ALEPPO_ERR_RUNTIME, "aleppo_release_step without an armed step");
  if (!rewards || !terminated || !truncated) // (checked while still armed: the caller can repeat the call)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_gate(c)) // the gate gave up before this release: the slot already ran without the frames
    return rc;
  // the frames and the episode-start bytes are in place: let the stream go FIRST, the bookkeeping is off its path
  std::atomic_thread_fence(std::memory_order_release);
  gate_release(c);
  c->armed = false;
  const int E = c->E;
  uint8_t *rec = c->h_rec + (size_t)c->t * c->step_rec_bytes; // uploaded at finish_rollout
  std::memcpy(rec, rewards, (size_t)E * 4);
  std::memcpy(rec + 4 * (size_t)E, terminated, E);
  std::memcpy(rec + 5 * (size_t)E, truncated, E);
  std::memcpy(rec + 6 * (size_t)E, c->armed_start, E);
  c->t++;
  rec_tick(c, ALEPPO_REC_ROLLOUT);
  return ALEPPO_OK;
}
extern "C" int aleppo_replay_rollout(aleppo_ctx *c, const uint8_t *frames, int kind, int location,
                                     size_t slot_stride_bytes, const float *rewards, const uint8_t *terminated,
                                     const uint8_t *truncated, const uint8_t *episode_start, const float *noise) {
  CHECK_CTX(c);
  if (!frames || !rewards || !terminated || !truncated || !episode_start)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null argument");
  if (location != ALEPPO_DEVICE && location != ALEPPO_HOST_MAPPED)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "replay_rollout: frames must be ALEPPO_DEVICE or ALEPPO_HOST_MAPPED");
  if (c->t != 0)
    return set_err(c, ALEPPO_ERR_RUNTIME, "replay_rollout needs an empty rollout buffer");
  const size_t E = (size_t)c->E;
  // rollout.cc:198-278 with the emulator replaced by the recorded trace.  The stream runs ONE slot ahead of the host:
  // slot t + 1's kernels (ingest of the frames the emulator produces from action t, convolutions, fc, head) are enqueued
  // while slot t is still on the GPU, behind a gate (gate_kernel) on a pinned word that the host writes once it HAS
  // slot t's actions (and, with a live emulator, the frames).  The hand-off keeps its order - the GPU never touches slot
  // t + 1's frames before the host has seen action t - but the next slot starts ~1 us after the host's store instead of
  // a kernel-launch latency after it (micro-benchmark tests/tools/waitvalue.hip: 3.7 vs 6.7 us per ping-pong).
  static const bool gated_env = [] {
    const char *e = getenv("ALEPPO_REPLAY_GATED");
    return !e || atoi(e) != 0;
  }();
  const bool gated = gated_env && !c->prof_on && !c->dbg_no_publish;
  auto noise_at = [&](int t) { return noise ? noise + (size_t)t * E * c->A : nullptr; };
  int rc = act_enqueue(c, noise_at(0), 0);
  if (rc)
    return rc;
  for (int t = 0; t < c->T; ++t) {
    const long long ticket_t = c->ticket; // of act(t), enqueued above / in the previous iteration
    if (gated) {
      rc = gate_enqueue(c); // (nothing of this slot is behind a gate yet: an ordinary error)
      if (rc)
        return rc;
    } else {
      rc = act_wait(c, ticket_t);
      if (rc)
        return rc;
    }
    rc = aleppo_step(c, frames + (size_t)t * slot_stride_bytes, kind, location, rewards + (size_t)t * E,
                     terminated + (size_t)t * E, truncated + (size_t)t * E, episode_start + (size_t)t * E);
    if (rc == ALEPPO_OK && t + 1 < c->T)
      rc = act_enqueue(c, noise_at(t + 1), t + 1);
    if (gated) {
      if (rc) // a slot is half enqueued behind the gate: see aleppo_arm_step
        return fail_ctx(c, rc, "aleppo_replay_rollout: " + c->err);
      rc = act_wait(c, ticket_t, /*stream_parked=*/true); // the host has slot t's actions: the emulator would step now
      if (rc)
        return c->failed ? rc : fail_ctx(c, rc, "aleppo_replay_rollout: " + c->err);
      gate_release(c);            // ... and hand over slot t + 1's frames
    } else if (rc) {
      return rc;
    }
  }
  return ALEPPO_OK;
}
extern "C" int aleppo_set_gray_lut(aleppo_ctx *c, const uint8_t *lut256) {
  CHECK_CTX(c);
  if (!lut256)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "null lut");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, copy_sync(c, c->lut, lut256, 256, hipMemcpyHostToDevice));
  return ALEPPO_OK;
}

// ALEPPO_OPT_REWARD_SCALE: one device allocation, made on first use and kept where it is until aleppo_destroy - the
// state block, the two running-return arrays (state / scan output), the scan's partials and the all-reduce's sums.
namespace aleppo {
const double RS_INITIAL[RS_BLOCK] = {1e-4, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0}; // gym's RunningMeanStd; s = 1
int ensure_rs_storage(aleppo_ctx *c) {
  if (c->rs_blk)
    return ALEPPO_OK;
  const size_t E = (size_t)c->E, doubles = RS_BLOCK + 2 * E + (size_t)rs_blocks(c->E) * 4 + 4;
  double *blk = nullptr;
  HIPCHK(c, dalloc(c, &blk, doubles * sizeof(double))); // (zeroed: G = 0)
  HIPCHK(c, copy_sync(c, blk, RS_INITIAL, sizeof(RS_INITIAL), hipMemcpyHostToDevice));
  c->rs_blk = blk;
  c->rs_g[0] = blk + RS_BLOCK;
  c->rs_g[1] = c->rs_g[0] + E;
  c->rs_part = c->rs_g[1] + E;
  c->rs_cur = 0;
  return ALEPPO_OK;
}
bool rs_state_valid(const double stats[3]) {
  return std::isfinite(stats[0]) && std::isfinite(stats[1]) && std::isfinite(stats[2]) && stats[0] > 0.0 &&
         stats[2] >= 0.0;
}
} // namespace aleppo

extern "C" int aleppo_finish_rollout(aleppo_ctx *c, const float *noise) {
  CHECK_CTX(c);
  c->act_queued_slot = -1;
  if (c->t != c->T)
    return set_err(c, ALEPPO_ERR_RUNTIME, "Buffer is not full, cannot compute GAE."); // buffer.cc:64-65
  if (int rcg = check_gate(c))
    return rcg;
  const int E = c->E, T = c->T, A = c->A;
  const bool rs_on = c->reward_scale;
  const bool rs_dp = rs_on && (c->world > 1 || (c->nccl_comm && c->force_comm));
  if (rs_on) {
    if (c->world > 1 && !c->nccl_comm)
      return set_err(c, ALEPPO_ERR_RUNTIME, "world_size > 1 but aleppo_comm_init was not called");
    if (int rcs = ensure_rs_storage(c))
      return rcs;
  }
  // extra selector call on the post-rollout observation: its values bootstrap slot T-1, its sample is
  // discarded but advances the RNG stream like the reference (rollout.cc:268-270)
  int rc = do_act(c, noise, T, rp(c, c->logits_tm, (size_t)T * E * A), rp(c, c->values_tm, (size_t)T * E),
                  c->actions_tm + (size_t)T * E, false);
  if (rc)
    return rc;
  if (!c->rec_on_device) // (aleppo_env_rollout's records are where GAE reads them already)
    HIPCHK(c, hipMemcpyAsync(c->step_rec, c->h_rec, c->step_rec_bytes * T, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_err, 0, 4, c->stream));
  if (rs_on) { // ALEPPO_OPT_REWARD_SCALE: scan -> moments -> [all-reduce] -> merge and scale -> GAE on the scaled rewards
    double *const sums = c->rs_part + (size_t)rs_blocks(E) * 4;
    prof_begin(c, ALEPPO_K_GAE);
    launch_rs_scan(c->stream, c->step_rec, c->step_rec_bytes, c->rs_g[c->rs_cur], c->rs_g[c->rs_cur ^ 1], c->rs_part,
                   c->d_err, E, T, c->cfg.gamma);
    launch_rs_reduce(c->stream, c->rs_part, rs_blocks(E), rs_dp ? sums : nullptr, c->rs_blk, c->d_err);
    if (rs_dp) {
      NCCLCHK(c, ncclAllReduce(sums, sums, 3, ncclDouble, ncclSum, static_cast<ncclComm_t>(c->nccl_comm), c->stream));
      launch_rs_finalise(c->stream, sums, c->rs_blk, c->d_err);
    }
    launch_gae_scaled(c->stream, c->step_rec, c->step_rec_bytes, c->values_tm, c->logits_tm, c->actions_tm, c->adv_n,
                      c->ret_n, c->oldlp_n, c->act_n, c->mask_n, c->d_err, E, T, A, c->cfg.gamma, c->cfg.lambda, c->rs_blk,
                      c->reward_scale_clip, c->rt16);
    prof_end(c, ALEPPO_K_GAE);
  } else {
    prof_begin(c, ALEPPO_K_GAE);
    launch_gae(c->stream, c->step_rec, c->step_rec_bytes, c->values_tm, c->logits_tm, c->actions_tm, c->adv_n, c->ret_n,
               c->oldlp_n, c->act_n, c->mask_n, c->d_err, E, T, A, c->cfg.gamma, c->cfg.lambda, true, c->rt16);
    prof_end(c, ALEPPO_K_GAE);
  }
  if (c->cfg.advantage_norm) {
    launch_adv_norm(c->stream, c->adv_n, c->mask_n, c->adv_stats, c->N, 0, c->rt16);
    if ((c->world > 1 || c->force_comm) && c->nccl_comm)
      NCCLCHK(c, ncclAllReduce(c->adv_stats, c->adv_stats, 3, ncclFloat, ncclSum,
                               static_cast<ncclComm_t>(c->nccl_comm), c->stream));
    launch_adv_norm(c->stream, c->adv_n, c->mask_n, c->adv_stats, c->N, 1, c->rt16);
  }
  HIPCHK(c, hipMemcpyAsync(c->h_err, c->d_err, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rcg = check_gate(c)) // (the last armed slot's gate may have given up while the stream drained)
    return rcg;
  c->t = 0;
  c->rec_on_device = false;
  c->pre_acted = -1;
  c->need_carry = true;
  c->batch_n = c->N;
  c->caller_batch = false;
  c->val_src = Ctx::VAL_ROLLOUT; // (values_tm; any values supplied for a caller batch are forgotten)
  c->fresh_valid = false;        // (aleppo_refresh_advantages' plane belongs to the batch this one replaces)
  c->batch_refused = *c->h_err != 0;
  if (rs_on && !*c->h_err)
    c->rs_cur ^= 1; // the scan's output is the running return now (a refused rollout leaves the state as it was)
  if (*c->h_err)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "Episode starts, terminals, and truncations must be mutually exclusive."); // gae.cc:49-53
  return ALEPPO_OK;
}

// ALEPPO_OPT_REWARD_SCALE's part of a checkpoint: the running statistics and the per-environment running returns
extern "C" int aleppo_export_reward_scale(aleppo_ctx *c, double stats[3], double *returns, size_t num_envs) {
  CHECK_CTX(c);
  if (!stats || !returns)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "export_reward_scale: null argument");
  if (num_envs != (size_t)c->E)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "export_reward_scale: num_envs is not the context's");
  if (int rc = ensure_rs_storage(c))
    return rc;
  HIPCHK(c, hipMemcpyAsync(stats, c->rs_blk, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, copy_sync(c, returns, c->rs_g[c->rs_cur], num_envs * sizeof(double), hipMemcpyDeviceToHost));
  return ALEPPO_OK;
}
extern "C" int aleppo_import_reward_scale(aleppo_ctx *c, const double stats[3], const double *returns,
                                          size_t num_envs) {
  CHECK_CTX(c);
  if (!stats || !returns)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "import_reward_scale: null argument");
  if (num_envs != (size_t)c->E)
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "import_reward_scale: num_envs is not the context's");
  if (!rs_state_valid(stats))
    return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT,
                   "import_reward_scale: count must be finite and > 0, mean finite, var finite and >= 0");
  for (size_t e = 0; e < num_envs; ++e)
    if (!std::isfinite(returns[e]))
      return set_err(c, ALEPPO_ERR_INVALID_ARGUMENT, "import_reward_scale: a running return is not finite");
  if (int rc = ensure_rs_storage(c))
    return rc;
  // (the scale, the batch count and the clip counter describe the last scaled rollout: they are not part of the state)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyAsync(c->rs_blk, stats, 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, copy_sync(c, c->rs_g[c->rs_cur], returns, num_envs * sizeof(double), hipMemcpyHostToDevice));
  return ALEPPO_OK;
}
