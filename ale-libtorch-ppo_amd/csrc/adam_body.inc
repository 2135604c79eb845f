// adam_body.inc - the body of the norm-clip + Adam kernel (kernels.hip), included by its two __global__ entry points:
// adam_kernel (max_norm a kernel argument) and adam_dev_kernel (max_norm read from the device block of
// ALEPPO_OPT_MAX_GRAD_NORM, so that a captured update follows it).  In scope: T, the kernel arguments and `max_norm`.
  __shared__ float s4[4];
  __shared__ float tile[64][65];
  float s = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 256)
    s += partials[i];
  s = block_sum_256(s, s4);
  const float norm = sqrtf(s);
  float coef = max_norm / (norm + 1e-6f); // train.cc:39
  coef = fminf(coef, 1.0f);               // train.cc:40-41
  if (blockIdx.x == 0 && threadIdx.x == 0 && grad_norm_out)
    *grad_norm_out = norm;                // pre-clip norm is what the reference reports (Q9)
  // lr / (1 - beta1^t) and sqrt(1 - beta2^t) of THIS optimizer step: device scalars (a captured hipGraph of the update
  // follows the annealed rate and the step count; the reference's captured graph bakes both, train.h:163-195)
  const AdamScalars a{coef, sched[0], sched[1], beta1, beta2, 1.0f - beta1, 1.0f - beta2, eps};
  const int ntile = tl.first[3];
  if ((int)blockIdx.x < ntile) { // a 64-row tile of Wfc / W3 / W2
    const int t = blockIdx.x;
    long src;      // flat index of tile element (0, 0)
    int rs, rows, cols;
    T *dst;        // transposed element (c, r) at dst[c * ds + r]
    int ds;
    if (t < tl.first[1]) {          // Wfc[o][j] -> WfcT[j][o]: tile (o-block, j-block of 64; 3136 = 49 * 64)
      const int ob = t / 49, jb = t - ob * 49;
      rs = FC_IN;
      rows = min(64, tl.H - ob * 64);
      cols = 64;
      src = tl.off[0] + (long)ob * 64 * FC_IN + jb * 64;
      dst = WfcT + (long)jb * 64 * tl.H + ob * 64;
      ds = tl.H;
    } else if (t < tl.first[2]) {   // W3[oc][tap][c] -> W3d[c][tap][oc]: one tile per tap
      const int tap = t - tl.first[1];
      rs = 576;
      rows = 64;
      cols = 64;
      src = tl.off[1] + tap * 64;
      dst = W3d + tap * 64;
      ds = 576;
    } else {                        // W2[oc][(kh,kw)][c] -> W2d[class][c][(ab)][oc]: one 64 x 32 tile per (kh, kw)
      const int k = t - tl.first[2], kh = k >> 2, kw = k & 3;
      const int cls = (kh & 1) * 2 + (kw & 1), ab = (kh >> 1) * 2 + (kw >> 1);
      rs = 512;
      rows = 64;
      cols = 32;
      src = tl.off[2] + k * 32;
      dst = W2d + cls * (32 * 256) + ab * 64;
      ds = 256;
    }
    const int c = threadIdx.x & 63, r4 = threadIdx.x >> 6;
    if (c < cols) {
      // all 64 loads of a thread's 16 elements are issued before the first store (P / M1 / M2 are read and written through
      // the same pointers, so the compiler may not hoist them itself; a dependent load-compute-store chain per element made
      // this kernel latency-bound: 23 vs 13 us)
      float g[16], m1[16], m2[16], p0[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int r = r4 + 4 * k;
        const long i = src + (long)(r < rows ? r : 0) * rs + c;
        g[k] = G[i];
        m1[k] = M1[i];
        m2[k] = M2[i];
        p0[k] = P[i];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int r = r4 + 4 * k;
        if (r < rows) {
          const long i = src + (long)r * rs + c;
          const float gg = g[k] * a.coef;
          const float m = m1[k] * a.beta1 + a.omb1 * gg;
          const float v = m2[k] * a.beta2 + a.omb2 * (gg * gg);
          const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
          const float p = p0[k] - a.step_size * (m / denom);
          M1[i] = m;
          M2[i] = v;
          P[i] = p;
          if (Gs)
            Gs[i] = gg;
          if (Pc)
            Pc[i] = (T)p;
          tile[r][c] = p;
        }
      }
    }
    __syncthreads();
    const int r = threadIdx.x & 63, c4 = threadIdx.x >> 6;
    if (r < rows)
      for (int cc = c4; cc < cols; cc += 4)
        dst[(long)cc * ds + r] = (T)tile[r][cc];
    return;
  }
  // everything else, flat: index k of the compacted space of the (at most four) ranges between the tiled tensors
  const long stride = (long)(gridDim.x - ntile) * 256;
  for (long k = (long)((int)blockIdx.x - ntile) * 256 + threadIdx.x; k < n_flat; k += stride) {
    long i = k;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (i < fr.len[q]) {
        i += fr.begin[q];
        break;
      }
      i -= fr.len[q];
    }
    const float p = adam_element(i, P, G, Gs, M1, M2, a);
    if (Pc)
      Pc[i] = (T)p;
  }
