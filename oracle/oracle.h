/* TEST INFRASTRUCTURE - NOT PRODUCT CODE.
 * CPU restatement (plain C) of the reference's hot-path algorithm.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library; the
 * product path (ale-libtorch-ppo_amd/, include/aleppo.h) never links or calls it.
 *
 * Parity status: PINNED.  Checked by tests/test_oracle.py against (i) the six known-answer
 * cases of the reference's test/ai/gae-test.cc, (ii) the constant-preservation cases of
 * test/ai/vision-test.cc and (iii) tests/golden/ref_golden.npz = outputs of the reference's own
 * compiled gae.cc / buffer.cc / ppo/losses.cc / ppo/train.{h,cc} (oracle/_ref, built from
 * /root/reference by oracle/build_ref.sh; fixtures packed by oracle/make_golden.py).
 *
 * All tensors use the REFERENCE's layouts: env-major [E,T], observations NCHW uint8
 * [N,4,84,84], parameters flat in libtorch parameters() order
 *   conv1.w[32,4,8,8] conv1.b[32] conv2.w[64,32,4,4] conv2.b[64] conv3.w[64,64,3,3] conv3.b[64]
 *   fc.w[H,3136] fc.b[H] action.w[A,H] action.b[A] value.w[1,H] value.b[1]
 */
#ifndef ALEPPO_ORACLE_H
#define ALEPPO_ORACLE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

size_t oracle_param_count(int H, int A);
/* offsets[13]: start of each of the 12 tensors + total */
void oracle_param_offsets(int H, int A, size_t *offsets);

/* src/ai/gae.cc:4-80.  returns 0, or -1 if start/terminal/truncation overlap (the reference throws) */
int oracle_gae(float *adv, const float *rewards, const float *values, const float *next_values,
               const uint8_t *terminals, const uint8_t *truncations, const uint8_t *episode_starts, int E, int T,
               float gamma, float lambda);
/* src/ai/buffer.cc:58-77: clamp rewards in place, gae, returns = adv + values, masks = !starts */
int oracle_buffer_get(float *rewards, const float *values, const float *next_values, const uint8_t *terminals,
                      const uint8_t *truncations, const uint8_t *episode_starts, float *adv, float *returns,
                      uint8_t *masks, int E, int T, float gamma, float lambda);
/* src/ai/rollout.cc:184-196 on obs [E,S,84,84] */
void oracle_update_observations(uint8_t *obs, const uint8_t *frames, const uint8_t *start, int E, int S);
/* src/ai/vision.cc:8-32: interpolate(mode=area) == adaptive average pooling */
void oracle_area_resize_f32(const float *in, float *out, int N, int IH, int IW, int OH, int OW);
/* src/ai/vision.cc:51,71-84: [N,3,P] -> [N,P] */
void oracle_rgb_to_gray(const float *rgb, float *out, int N, int P);
/* device preprocessing spec: per frame lut -> area 210x160->84x84 -> rint -> u8,
 * then max over the nframes frames (src/ai/environment/max_and_skip.cc:33-42). lut may be NULL. */
void oracle_preprocess_u8(const uint8_t *raw, const uint8_t *lut, uint8_t *out, int E, int nframes);

/* src/ai/ppo/losses.cc:45-47 */
void oracle_log_softmax(const float *logits, float *out, int B, int A);
void oracle_softmax(const float *logits, float *out, int B, int A);
/* src/bin/train.cc:374-375: multinomial(probs,1,true) == argmax(p/q), q~Exp(1), first max wins */
void oracle_sample(const float *probs, const float *q, int64_t *actions, int E, int A);

/* src/bin/train.cc:255-265.  acts (optional) receives the saved activations used by backward:
 * per sample x0[4*84*84] a1[32*400] a2[64*81] a3[3136] h[H] */
size_t oracle_acts_per_sample(int H);
void oracle_net_forward(const float *params, int H, int A, const uint8_t *obs, int N, float *logits, float *values,
                        float *acts);
/* gradients of sum_i (dlogits_i . logits_i + dvalues_i * value_i) wrt params, accumulated into grads (zeroed first) */
void oracle_net_backward(const float *params, int H, int A, int N, const float *acts, const float *dlogits,
                         const float *dvalues, float *grads);

/* src/ai/ppo/losses.cc:4-43 forward, closed-form backward.  n_mask <= 0: use sum(masks).
 * per-sample outputs may be NULL.  returns the scalar loss. */
float oracle_ppo_loss(const float *logits, const float *old_logp, const int64_t *actions, const float *adv,
                      const float *values, const float *returns, const uint8_t *masks, int B, int A, float clip,
                      float c_v, float c_e, float n_mask, float *clipped, float *value_losses, float *entropies,
                      float *total_losses, float *ratio, float *dlogits, float *dvalues);

/* src/ai/ppo/train.cc:12-46: returns the pre-clip total norm, scales grads in place */
float oracle_clip_grad_norm(float *grads, int H, int A, float max_norm);
/* torch::optim::Adam step (src/bin/train.cc:360-362), step counts from 1 */
void oracle_adam_step(float *p, const float *g, float *m, float *v, size_t n, double lr, double beta1, double beta2,
                      double eps, int64_t step);

/* src/ai/ppo/train.h:114-157: epochs x M contiguous minibatches.  out arrays sized
 * loss[epochs*M], grad_norm[epochs*M], per-sample [epochs*M*B] (may be NULL). */
int oracle_train(float *params, float *adam_m, float *adam_v, int64_t *adam_step, int H, int A, const uint8_t *obs,
                 const int64_t *actions, const float *old_logp, const float *adv, const float *returns,
                 const uint8_t *masks, int N, int epochs, int M, double lr, float clip, float c_v, float c_e,
                 float max_norm, float *loss, float *grad_norm, float *total_losses, float *ratio, float *entropies,
                 float *value_losses, float *clipped, float *last_grads);
/* ---------------------------------------------------------------- bf16 emulation
 * mode ORACLE_FP32 (0): the functions above, bit for bit.  ORACLE_BF16 (1): the exact model of the bf16 update /
 * acting path - operands rounded to bf16 (round-to-nearest-even, the device's (__bf16) casts) where the device STORES
 * bf16 and nowhere else, every sum before a rounding point taken in double, results kept as fp32.  ORACLE_BF16_F32SUM
 * (2): the same rounding points with sequential fp32 sums - a second summation order, used only to measure how far
 * summation order alone moves the results (the floor under the GPU bounds, tests/test_oracle_bf16.py).
 *
 * Rounding points, checked against the kernels of every route (paths below ale-libtorch-ppo_amd/csrc/):
 *
 *  quantity              | device storage / arithmetic                                  | emulation
 *  ----------------------+--------------------------------------------------------------+---------------------------
 *  conv1-3, fc weights   | bf16 compute copy of the fp32 master: cast_params_kernel      | W_b = bf16(W)
 *                        | kernels.hip:1270-1273, adam_kernel kernels.hip:1206 / 1232;  |
 *                        | dgrad layouts W3d / W2d kernels.hip:1284 / 1289, WfcT        |
 *                        | kernels.hip:1301 - all (T) casts of the same fp32 value      |
 *  biases, action/value  | fp32: load_bias conv_patch.hpp:474, EpiBiasAct gemm.hpp:196, | no rounding
 *  heads                 | fwd_fused W.br conv_fwd_fused.hpp:167; head_train_kernel     |
 *                        | kernels.hip:713-724 and act_head.hpp's head_dot              |
 *                        | read fp32 Wh / bh                                            |
 *  observations          | u8, widened exactly (gemm.hpp:55-75); 1/255 is conv1's fp32  | x = byte value;
 *                        | epilogue scale (conv_fwd_fused.hpp:306, conv_patch_launch.hip:| a1 = bf16(relu(S/255 + b1))
 *                        | 69, conv_patch.hpp:656, gemm_launch.hip:36) and the scale of  | dW1 = (1/255) sum dz1_b x
 *                        | conv1's weight-gradient slabs (conv1_wgrad.hpp:239,          |
 *                        | conv_bwd_fused.hpp:539, gemm_launch.hip:428)                 |
 *  a1, a2, a3            | bf16 after scale, bias, ReLU: fused conv_fwd_fused.hpp:167;  | bf16(relu(S*scale + b))
 *                        | three launches conv_patch.hpp:357-360; acting                |
 *                        | conv_patch.hpp:504-505; generic gemm.hpp:196-199             |
 *  h (fc output)         | fp32 split-K slabs summed in head_train_kernel               | none (fp32)
 *                        | kernels.hip:666-673 / act_head.hpp's head_hidden             |
 *  logits, value, loss,  | fp32 (kernels.hip:710-790)                                   | none; the loss and its
 *  planes, dlogits/dvalue|                                                              | gradient are oracle_ppo_loss
 *  dh                    | bf16: head_train_kernel kernels.hip:822 `dr[i] = (T)d[i]`    | dh_b = bf16(Wh^T dz)
 *  dz3                   | bf16 gated by the stored bf16 a3 > 0: pipelined fc dgrad     | bf16((a3 > 0) Wfc_b^T dh_b)
 *                        | gemm_pipe.hpp:302-310; small-tile / generic EpiDgrad         |
 *                        | gemm.hpp:250-252                                             |
 *  dz2                   | bf16 gated by a2 > 0: conv3_dgrad_tile_kernel                | bf16((a2 > 0) W3_b^T dz3_b)
 *                        | conv3_tile.hpp:131-143; patch dgrad conv_patch.hpp:372-379;  |
 *                        | generic gemm.hpp:250-252                                     |
 *  dz1                   | bf16 gated by a1 > 0: fused tail (LDS only)                  | bf16((a1 > 0) W2_b^T dz2_b)
 *                        | conv_bwd_fused.hpp:313-321; three launches                   |
 *                        | conv_patch.hpp:372-379; generic gemm.hpp:250-252             |
 *  conv / fc weight and  | fp32 accumulation of the bf16 operands into fp32 slabs; the  | double sums of the rounded
 *  bias gradients        | bias gradient is the column sum of the SAME bf16 dz operand  | dz / dh (bias included)
 *                        | on every route: gemm_tn_kernel gemm.hpp:479 / 636, patch     |
 *                        | wgrad conv_patch.hpp:893 / 953, conv1 wgrad                  |
 *                        | conv1_wgrad.hpp:191, fused tail conv_bwd_fused.hpp:483       |
 *  head weight / bias    | fp32 from the fp32 dz and fp32 h: kernels.hip:817 / 834      | none
 *  gradients             |                                                              |
 *  clip, Adam, masters   | fp32                                                         | unchanged (mode-free)
 *
 * Every route - fused / three-launch forward, fused / three-launch backward tail, pipelined / small-tile fc, patch /
 * generic convs, shuffled / contiguous minibatches - rounds at the same points, so one model covers all of them: no
 * per-route switch is needed (the sweep in tests/test_gpu_bf16_emulated.py checks each against this model).
 * Activations saved for the backward pass (acts) hold x0 as raw byte values in the emulated modes. */
#define ORACLE_FP32 0
#define ORACLE_BF16 1
#define ORACLE_BF16_F32SUM 2
void oracle_round_bf16(const float *in, float *out, size_t n);
void oracle_net_forward_ex(const float *params, int H, int A, const uint8_t *obs, int N, float *logits, float *values,
                           float *acts, int mode);
void oracle_net_backward_ex(const float *params, int H, int A, int N, const float *acts, const float *dlogits,
                            const float *dvalues, float *grads, int mode);
/* the same, and (dacts != NULL) what the backward pass stores on its way: per sample [H + 3136 + 5184 + 12800] floats =
 * dh, dz3, dz2, dz1 in the reference's tensor order (NCHW), after the gates (and, in the emulated modes, the roundings) */
void oracle_net_backward_stored(const float *params, int H, int A, int N, const float *acts, const float *dlogits,
                                const float *dvalues, float *grads, float *dacts, int mode);
int oracle_train_ex(float *params, float *adam_m, float *adam_v, int64_t *adam_step, int H, int A, const uint8_t *obs,
                    const int64_t *actions, const float *old_logp, const float *adv, const float *returns,
                    const uint8_t *masks, int N, int epochs, int M, double lr, float clip, float c_v, float c_e,
                    float max_norm, float *loss, float *grad_norm, float *total_losses, float *ratio, float *entropies,
                    float *value_losses, float *clipped, float *last_grads, int mode);
/* advantage normalisation over unmasked samples - an extension with NO reference counterpart:
 * PARITY UNPINNED, see oracle.c.  returns the unmasked count. */
long oracle_adv_norm(float *adv, const uint8_t *masks, long n);
int oracle_num_threads(void);
#ifdef __cplusplus
}
#endif
#endif
