// head_train_body.inc - the body of the PPO head training kernel, included by the three __global__ entry points of
// head_train.hip: head_train_kernel (ADVN = false), head_train_advn_kernel (ADVN = true, ALEPPO_OPT_ADV_NORM_MINIBATCH),
// head_train_kl_kernel (KLPEN = true, ALEPPO_OPT_KL_PENALTY; there `advs` may be null, which leaves the advantages as
// stored).  The text is shared this way, not through a __device__ function, because inlining a function changed the
// register allocation of the default kernels (AMAX = 18: 336 instead of 402 VGPRs); included into the kernel, the
// ADVN = KLPEN = false instantiations compile to the same code as before the options existed.
// In scope: the template parameters T, AMAX, RT, VCLIP, the kernel arguments, `constexpr bool ADVN`, `constexpr bool
// KLPEN`, `advs`, `klb` (the device word holding beta) and `ps_kle` (the per-sample exact-KL plane).
  constexpr int A1 = AMAX + 1, HPL = 8; // H <= 512: 8 hidden units per lane
  constexpr int NWV = head_waves(AMAX, KLPEN); // waves per workgroup
  // Every variant adds the rows' weight gradients in the order of the option-off kernel, whose NVW waves each sum
  // rows wave, wave + NVW, ... and whose partials are then added in wave order.  A variant with fewer waves (the KL
  // penalty at AMAX = 10) runs NPASS passes: in pass p wave w does the rows of the option-off kernel's wave
  // w + p * NWV, and the reduction after each pass continues the running sum in the slab, so the bits are the same.
  constexpr int NVW = head_waves(AMAX, false), NPASS = NVW / NWV;
  extern __shared__ float smem[];
  float *sW = smem;                    // [(A+1)][H]
  float *sAcc = smem + (size_t)A1 * H; // [(A+1)][H] cross-wave wgrad accumulator
  float *sB = sAcc + (size_t)(A1 > NWV ? A1 : NWV) * H; // [NVW][A1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long rows_per_blk = (B + gridDim.x - 1) / gridDim.x;
  const long row0 = (long)blockIdx.x * rows_per_blk, row1 = min(B, row0 + rows_per_blk);
  // Everything a row needs (h, action, advantage, return, mask and ALL A old log-probs, so that nothing is a
  // dependent load) is fetched ONE ROW AHEAD: a row's memory round trips hide behind the previous row's math.
  // The first row's loads are issued before the weight staging below.
  float hnext[HPL], olp_n[AMAX], adv_n = 0.f, ret_n = 0.f, vold_n = 0.f;
  int act_n = 0;
  bool mask_n = false;
  auto fetch = [&](long r) {
    const bool ok = r < row1;
    // lane l owns hidden units 4l .. 4l+3 and H/2 + 4l .. H/2 + 4l+3 (H % 8 == 0): 16-byte loads instead of scalar
    // ones, and consecutive lanes touch consecutive 16-byte pieces (coalesced; conflict-free LDS reads of the weights)
#pragma unroll
    for (int i = 0; i < HPL; ++i)
      hnext[i] = 0.f;
    if (ok && lane * 8 < H) // h arrives as `hparts` split-K partial slabs [hparts][B][H] (slab 0 carries the bias)
      add_h_slabs(h, hparts, B, r, H, lane, hnext);
#pragma unroll
    for (int a = 0; a < AMAX; ++a)
      olp_n[a] = (ok && a < A) ? (float)oldlp[(size_t)r * A + a] : 0.f;
    act_n = ok ? act[r] : 0;
    adv_n = ok ? (float)adv[r] : 0.f;
    ret_n = ok ? (float)ret[r] : 0.f;
    if constexpr (VCLIP)
      vold_n = ok ? (float)vold[r] : 0.f;
    mask_n = ok ? mask[r] != 0 : false;
  };
  fetch(row0 + wave);
  for (int i = tid; i < (A + 1) * H; i += 64 * NWV)
    sW[i] = Wh[i];
  __syncthreads();
  const float inv_nm = 1.0f / mask_count[0];
  // the clip range, the value-clip range and the two loss coefficients: slots 0-3 of the device block, one 16-byte load
  const f32x4 hpv = *reinterpret_cast<const f32x4 *>(hp);
  const float hp_clip = hpv[HYPER_CLIP], hp_vclip = hpv[HYPER_VCLIP], hp_cv = hpv[HYPER_CV], hp_ce = hpv[HYPER_CE];
  float kl_beta = 0.f;
  if constexpr (KLPEN)
    kl_beta = klb[0]; // ALEPPO_OPT_KL_COEF: a device value, so that a graph replay follows a beta changed between calls
  float adv_mean = 0.f, adv_inv = 1.f;
  if constexpr (KLPEN) {
    if (advs) { // (null: mean 0, scale 1, and (a - 0) * 1 is a exactly)
      adv_mean = advs[0];
      adv_inv = advs[1];
    }
  } else if constexpr (ADVN) {
    adv_mean = advs[0];
    adv_inv = advs[1];
  }
  float gW[A1][HPL], gb[A1];
#ifdef HEAD_TRAIN_PASSES // (only head_train_kl_kernel: the other entry points keep their single pass as it was)
  for (int pass = 0; pass < NPASS; ++pass) {
    const int vw = wave + pass * NWV; // the option-off kernel's wave this pass stands in for (NPASS = 1: this wave)
    if (pass > 0)
      fetch(row0 + vw);
#else
  {
    static_assert(NPASS == 1, "fewer waves than the option-off kernel need HEAD_TRAIN_PASSES");
    constexpr int pass = 0;
    const int vw = wave;
#endif
#pragma unroll
    for (int a = 0; a < A1; ++a) {
      gb[a] = 0.f;
#pragma unroll
      for (int i = 0; i < HPL; ++i)
        gW[a][i] = 0.f;
    }
    for (long row = row0 + vw; row < row1; row += NVW) {
      float hv[HPL], olp_c[AMAX];
#pragma unroll
      for (int i = 0; i < HPL; ++i)
        hv[i] = hnext[i];
#pragma unroll
      for (int a = 0; a < AMAX; ++a)
        olp_c[a] = olp_n[a];
      const int ai = act_n;
      const float advi = ADVN ? (adv_n - adv_mean) * adv_inv : adv_n, reti = ret_n, voldi = vold_n;
      const bool maski = mask_n;
      fetch(row + NVW); // next row of this wave
      float z[A1];
#pragma unroll
      for (int a = 0; a < A1; ++a) {
        float s = 0.f;
        if (a <= A) {
          if (lane * 8 < H) {
            const f32x4 w0 = *reinterpret_cast<const f32x4 *>(sW + a * H + lane * 4);
            const f32x4 w1 = *reinterpret_cast<const f32x4 *>(sW + a * H + H / 2 + lane * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i)
              s += hv[i] * w0[i];
#pragma unroll
            for (int i = 0; i < 4; ++i)
              s += hv[4 + i] * w1[i];
          }
          s = wave_sum(s) + bh[a];
        }
        z[a] = s;
      }
      // every lane now holds logits z[0..A-1] and the value z[A]
      const float value = [&] {
        float v = 0.f;
#pragma unroll
        for (int a = 0; a < A1; ++a)
          if (a == A)
            v = z[a];
        return v;
      }();
      float mx = -3.0e38f;
#pragma unroll
      for (int a = 0; a < AMAX; ++a)
        if (a < A)
          mx = fmaxf(mx, z[a]);
      float se = 0.f;
#pragma unroll
      for (int a = 0; a < AMAX; ++a)
        if (a < A)
          se += expf(z[a] - mx);
      const float lse = mx + logf(se);
      float lp[AMAX], p[AMAX], ent = 0.f, lpa = 0.f, olpa = 0.f;
#pragma unroll
      for (int a = 0; a < AMAX; ++a) {
        lp[a] = 0.f;
        p[a] = 0.f;
        if (a < A) {
          lp[a] = z[a] - lse;            // losses.cc:45-47
          p[a] = expf(lp[a]);
          ent += p[a] * lp[a];           // losses.cc:41-43
          if (a == ai) {
            lpa = lp[a];
            olpa = olp_c[a];
          }
        }
      }
      ent = -ent;
      // ALEPPO_OPT_KL_PENALTY: S = sum q_a and the exact KL(pi_old || pi) = sum q_a (olp_a - lp_a), q_a = exp(olp_a)
      // (written as exp(olp) where it is used, with no second [AMAX] array; the registers it takes are why the
      // penalty's AMAX = 10 variants run 4 waves per workgroup: head_waves in head_train.hpp)
      float kl_s = 0.f, kl = 0.f;
      if constexpr (KLPEN) {
#pragma unroll
        for (int a = 0; a < AMAX; ++a)
          if (a < A) {
            const float q = expf(olp_c[a]);
            kl_s += q;
            kl += q * (olp_c[a] - lp[a]);
          }
      }
      const float logr = lpa - olpa;
      const float rho = expf(logr);                                        // losses.cc:33
      const float crho = fminf(fmaxf(rho, 1.0f - hp_clip), 1.0f + hp_clip); // losses.cc:34-35
      const float un = rho * advi, cl = crho * advi;
      const float obj = fminf(un, cl);                                     // losses.cc:38
      const float dv = value - reti;
      float lv, dvg; // value loss and its derivative in v (before the mask and c_v)
      if constexpr (VCLIP) { // aleppo.h ALEPPO_OPT_VALUE_CLIP: a select, so that inside the range vc IS value
        const float d = value - voldi;
        const float vc = fabsf(d) <= hp_vclip ? value : voldi + copysignf(hp_vclip, d);
        const float dc = vc - reti;
        const float lu = dv * dv, lc = dc * dc;
        lv = 0.5f * fmaxf(lu, lc);
        dvg = lu >= lc ? dv : 0.f; // ties: the unclipped branch; the clipped one is flat in v
      } else {
        lv = 0.5f * (dv * dv);                                             // losses.cc:15
        dvg = dv;
      }
      float Ltot = -obj + hp_cv * lv - hp_ce * ent;                      // losses.cc:17-18
      if constexpr (KLPEN) {
        if (kl_beta != 0.f) // (a branch, not + 0 * KL: beta = 0 leaves every number of the option-off kernel as it was)
          Ltot += kl_beta * kl;
      }
      const float m = maski ? inv_nm : 0.f;                                // losses.cc:19 masked mean
      const bool active = advi >= 0.f ? (rho <= 1.0f + hp_clip) : (rho >= 1.0f - hp_clip);
      const float gs = active ? -rho * advi : 0.f;
      float dz[A1];
#pragma unroll
      for (int a = 0; a < A1; ++a) {
        dz[a] = 0.f;
        if (a < A && a < AMAX)
          dz[a] = m * (gs * ((a == ai ? 1.0f : 0.0f) - p[a < AMAX ? a : 0]) +
                       hp_ce * p[a < AMAX ? a : 0] * (lp[a < AMAX ? a : 0] + ent));
        if (a == A)
          dz[a] = m * hp_cv * dvg;
      }
      if constexpr (KLPEN) {
        if (kl_beta != 0.f) { // d(beta KL)/dz_j = beta (p_j S - q_j): S, not 1, the exact derivative when sum q != 1
          const float mk = m * kl_beta;
#pragma unroll
          for (int a = 0; a < AMAX; ++a)
            if (a < A)
              dz[a] += mk * (p[a] * kl_s - expf(olp_c[a]));
        }
      }
      if (lane == 0) {
        ps_total[row] = Ltot;
        ps_clipped[row] = obj;
        ps_value[row] = lv;
        ps_entropy[row] = ent;
        ps_ratio[row] = rho;
        ps_kl[row] = (rho - 1.0f) - logr;                                  // approx-KL (k3 estimator)
        ps_cf[row] = fabsf(rho - 1.0f) > hp_clip ? 1.0f : 0.0f;           // clip fraction (strict)
        if constexpr (KLPEN)
          ps_kle[row] = kl;                                                // exact KL (ALEPPO_M_KL)
        if (logits_out) {
#pragma unroll
          for (int a = 0; a < AMAX; ++a)
            if (a < A)
              logits_out[(size_t)row * A + a] = z[a];
          values_out[row] = value;
        }
      }
      // head dgrad: dh = sum_a dz[a] * W[a][:]   and wgrad partial: gW[a][:] += dz[a] * h
      if (lane * 8 < H) {
        float d[HPL];
#pragma unroll
        for (int i = 0; i < HPL; ++i)
          d[i] = 0.f;
#pragma unroll
        for (int a = 0; a < A1; ++a)
          if (a <= A) {
            const f32x4 w0 = *reinterpret_cast<const f32x4 *>(sW + a * H + lane * 4);
            const f32x4 w1 = *reinterpret_cast<const f32x4 *>(sW + a * H + H / 2 + lane * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              d[i] += dz[a] * w0[i];
              d[4 + i] += dz[a] * w1[i];
            }
#pragma unroll
            for (int i = 0; i < HPL; ++i)
              gW[a][i] += dz[a] * hv[i];
          }
        T dr[HPL];
#pragma unroll
        for (int i = 0; i < HPL; ++i)
          dr[i] = (T)d[i];
        T *dst = dh + (size_t)row * H + lane * 4;
        if constexpr (sizeof(T) == 2) {
          *reinterpret_cast<u32x2 *>(dst) = reinterpret_cast<const u32x2 *>(dr)[0];
          *reinterpret_cast<u32x2 *>(dst + H / 2) = reinterpret_cast<const u32x2 *>(dr)[1];
        } else {
          *reinterpret_cast<u32x4 *>(dst) = reinterpret_cast<const u32x4 *>(dr)[0];
          *reinterpret_cast<u32x4 *>(dst + H / 2) = reinterpret_cast<const u32x4 *>(dr)[1];
        }
      }
#pragma unroll
      for (int a = 0; a < A1; ++a)
        gb[a] += dz[a];
    }
    // deterministic cross-wave reduction, one head row at a time: every wave writes its partial of row a, then
    // thread j adds the NWV partials of column j in fixed order and stores the workgroup's slab entry
    float *sPart = sAcc; // [NWV][H] (reuses the accumulator region: (A+1)*H >= ... is not needed, H*NWV floats)
    float *ow = slab_w + (size_t)blockIdx.x * (A + 1) * H;
#pragma unroll
    for (int a = 0; a < A1; ++a) {
      if (a <= A) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < HPL; ++i) {
          const int j = (i < 4 ? 0 : H / 2) + lane * 4 + (i & 3);
          if (lane * 8 < H)
            sPart[wave * H + j] = gW[a][i];
        }
        if (lane == 0)
          sB[vw * A1 + a] = gb[a];
        __syncthreads();
        for (int j = tid; j < H; j += 64 * NWV) {
          float sum = pass > 0 ? ow[a * H + j] : 0.f; // (the running sum of the earlier passes' waves)
#pragma unroll
          for (int w = 0; w < NWV; ++w)
            sum += sPart[w * H + j];
          ow[a * H + j] = sum;
        }
      }
    }
  }
  __syncthreads();
  if (tid <= A) {
    float sb = 0.f;
#pragma unroll
    for (int w = 0; w < NVW; ++w)
      sb += sB[w * A1 + tid];
    slab_b[(size_t)blockIdx.x * (A + 1) + tid] = sb;
  }
