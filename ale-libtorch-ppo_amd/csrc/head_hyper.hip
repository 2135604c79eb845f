// head_hyper.hip - the PPO head training kernel's entry points that read the clip range, the value-clip range and the
// two loss coefficients from a device block (ALEPPO_OPT_CLIP_PARAM, ALEPPO_OPT_VALUE_CLIP_RANGE,
// ALEPPO_OPT_VALUE_LOSS_COEF, ALEPPO_OPT_ENTROPY_COEF) instead of kernel arguments: a captured update follows values
// changed between calls.  Same text as the default entry points of kernels.hip (head_train_entry.inc over
// head_train_body.inc) - same expressions in the same order, so the same bits for the same numbers; the block is
// read once per workgroup, one 16-byte load beside the mask count.  A translation unit of its own: the 96
// instantiations compile next to kernels.hip's.
#include "head_train.hpp"

namespace aleppo {

#define HEAD_KERNEL head_train_dev_kernel
#define HEAD_ADVN_KERNEL head_train_advn_dev_kernel
#define HEAD_KL_KERNEL head_train_kl_dev_kernel
#define HEAD_LAUNCH launch_head_train_dev
#define HEAD_HP_T const float *__restrict__
#define HEAD_HYPER_LOAD                                                                                                \
  const f32x4 hpv = *reinterpret_cast<const f32x4 *>(hp);                                                              \
  const float hp_clip = hpv[HYPER_CLIP], hp_vclip = hpv[HYPER_VCLIP], hp_cv = hpv[HYPER_CV], hp_ce = hpv[HYPER_CE];
#include "head_train_entry.inc"

} // namespace aleppo
