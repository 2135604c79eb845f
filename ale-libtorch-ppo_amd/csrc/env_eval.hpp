// env_eval.hpp - the environment kernel of the device-resident evaluation (include/aleppo.h: aleppo_eval_env_run): one
// agent step of every evaluation lane's SyntheticAtari, and its frame.  The game (env_slot), the pixels and the render
// loops (env_render) are env_synth.hpp's; nothing of the game is restated here.
#pragma once
#include "env_synth.hpp"

namespace aleppo {

#ifdef __HIPCC__
// Grid and work split as env_step_kernel's: lane l is blockIdx.x, its frame is shared out over gridDim.y workgroups
// (ENV_RAW_PARTS for a raw pair, 1 for an 84x84 frame); every thread recomputes the game logic from the state of the
// previous step (in), and thread 0 of part 0 writes the new state to the OTHER state array.  What differs is what that
// thread writes besides: no step record - an evaluation has none - but the start-at-entry byte where the ingest that
// follows reads it, and the four log entries of this step (row s of the [S][L] planes; zeros where nothing ended).
// actions: the int32 actions eval_head_kernel wrote for this step (ignored by a lane that starts an episode).
template <bool RAW>
__global__ __launch_bounds__(256) void eval_env_step_kernel(const aleppo_env_state *__restrict__ in,
                                                             aleppo_env_state *__restrict__ out, const int *__restrict__ actions,
                                                             uint8_t *__restrict__ frames, uint8_t *__restrict__ start,
                                                             float *__restrict__ log_ep_ret, uint32_t *__restrict__ log_ep_len,
                                                             float *__restrict__ log_game_ret,
                                                             uint32_t *__restrict__ log_game_len, uint64_t max_steps,
                                                             float max_return) {
  const int l = blockIdx.x;
  aleppo_env_state s = in[l];
  const EnvSlotOut o = env_slot(s, actions[l], max_steps, max_return);
  if (threadIdx.x == 0 && blockIdx.y == 0) {
    out[l] = s;
    start[l] = o.start;
    log_ep_ret[l] = o.ep_ret;
    log_ep_len[l] = o.ep_len;
    log_game_ret[l] = o.game_ret;
    log_game_len[l] = o.game_len;
  }
  env_render<RAW>(frames, l, s);
}
#endif

} // namespace aleppo
