// rec_capture.hpp - the capture kernel of the episode recorders (include/aleppo.h: aleppo_rec_open / aleppo_rec_read): one
// launch per recorded step of a source, enqueued directly behind that step's ingest, copies ONE environment's (or lane's)
// frame, newest observation plane, logits and step metadata into row r of the recorder's planes.  The host knows r when
// it enqueues - every step of a source takes exactly one row - so the arguments are finished pointers: no device-side
// cursor, no header, no atomics.  The game (env_slot) is env_synth.hpp's; nothing of it is restated here.
#pragma once
#include "env_synth.hpp"

namespace aleppo {

// What one launch reads and writes; every pointer already addresses the recorded index's data and row r.  A plane that
// is not part of the recorder's content has frame_dst / obs_dst == nullptr and is neither read nor written.
struct RecCaptureArgs {
  const uint8_t *frame_src;     // the index's part of the frame buffer as the environment kernel left it (16-byte aligned)
  uint8_t *frame_dst;           // row r of the frames plane, 7056 or 67200 bytes
  const uint32_t *stack;        // the index's packed stack AFTER the ingest [7056]: byte 0 of each u32 is the newest frame
  uint8_t *obs_dst;             // row r of the observation plane, 7056 bytes
  const void *logits;           // RT [A] (float, or IEEE half with rt16) of this step's acting decision
  const void *value;            // RT [1]
  const int *action;            // the int32 the head wrote
  const aleppo_env_state *in;   // the index's state BEFORE this step (intact until the next step's environment kernel)
  float *logits_dst;            // row r of the logits plane [A]
  aleppo_rec_step *step_dst;    // row r of the steps plane
  uint64_t ordinal, max_steps;
  float max_return;
  int A, rt16;
};

#ifdef __HIPCC__
static_assert(sizeof(aleppo_rec_step) == 32, "aleppo_rec_step is two 16-byte stores");
// Grid (parts) workgroups of 256: the frame's 16-byte words (441, or 4200 for a raw pair) are shared out over all parts
// the way env_render shares out its stores (ENV_RAW_PARTS parts for a raw pair, whose 67 KB would otherwise be copied by
// one CU; 1 otherwise); part 0 also does the observation plane - each lane loads four u32x4 of the stack, packs their
// sixteen low bytes and stores them as one 16-byte word - and the metadata: the logits and the value widened as
// aleppo_read_batch widens them, and env_slot applied to a COPY of the IN state with the head's action, which yields the
// reward, the flags, lives and game_over of this step exactly as the environment kernel computed them.  No LDS, no
// barrier, no scratch; every byte of a row is written exactly once.
template <bool RAW> __global__ __launch_bounds__(256) void rec_capture_kernel(const RecCaptureArgs a) {
  const int tid = threadIdx.x, part = blockIdx.x;
  if (a.frame_dst) {
    constexpr int FRAME16 = RAW ? 2 * 210 * 160 / 16 : 84 * 84 / 16;
    const env_u32x4 *src = reinterpret_cast<const env_u32x4 *>(a.frame_src);
    env_u32x4 *dst = reinterpret_cast<env_u32x4 *>(a.frame_dst);
    for (int c = part * 256 + tid; c < FRAME16; c += 256 * gridDim.x)
      dst[c] = src[c];
  }
  if (part != 0)
    return;
  if (a.obs_dst) {
    constexpr int OBS16 = 84 * 84 / 16; // 441 words of 16 pixels
    const env_u32x4 *src = reinterpret_cast<const env_u32x4 *>(a.stack);
    env_u32x4 *dst = reinterpret_cast<env_u32x4 *>(a.obs_dst);
    for (int c = tid; c < OBS16; c += 256) {
      env_u32x4 v;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const env_u32x4 p = src[c * 4 + w];
        v[w] = (p[0] & 255u) | ((p[1] & 255u) << 8) | ((p[2] & 255u) << 16) | (p[3] << 24);
      }
      dst[c] = v;
    }
  }
  if (tid < a.A)
    a.logits_dst[tid] = a.rt16 ? (float)static_cast<const _Float16 *>(a.logits)[tid] : static_cast<const float *>(a.logits)[tid];
  if (tid == 0) {
    aleppo_env_state s = *a.in;
    const int action = *a.action;
    const EnvSlotOut o = env_slot(s, action, a.max_steps, a.max_return);
    aleppo_rec_step st;
    st.ordinal = a.ordinal;
    st.action = action;
    st.reward = o.reward;
    st.value = a.rt16 ? (float)*static_cast<const _Float16 *>(a.value) : *static_cast<const float *>(a.value);
    st.start = o.start;
    st.terminated = o.term;
    st.truncated = o.trunc;
    st.game_over = (o.term || o.trunc) && s.game_over;
    st.lives = s.lives;
    st.reserved = 0;
    *a.step_dst = st;
  }
}
#endif

} // namespace aleppo
