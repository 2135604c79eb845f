/* TEST INFRASTRUCTURE - NOT PRODUCT CODE.  The bf16 emulation of oracle.c (see the rounding-point table in oracle.h).
 * Included twice by oracle.c: with ACC = double (ORACLE_BF16, the exact bf16 model: every pre-rounding sum in double)
 * and with ACC = float (ORACLE_BF16_F32SUM: the same rounding points, sequential fp32 sums - only used to measure how
 * far a summation order alone moves the results).  EMU(name) appends the accumulator's suffix. */

/* out[oc][p] = bf16(relu(scale * sum_k w[oc][k] cols[k][p] + b[oc])) - the conv epilogues */
static void EMU(conv_fwd)(const float *w, const float *b, const float *cols, int OC, int Kd, int P, float scale,
                          float *out, ACC *acc) {
  for (int oc = 0; oc < OC; ++oc) {
    for (int p = 0; p < P; ++p)
      acc[p] = 0;
    for (int k = 0; k < Kd; ++k) {
      const ACC wk = w[(size_t)oc * Kd + k];
      const float *c = cols + (size_t)k * P;
      for (int p = 0; p < P; ++p)
        acc[p] += wk * (ACC)c[p];
    }
    for (int p = 0; p < P; ++p) {
      const ACC v = acc[p] * (ACC)scale + (ACC)b[oc];
      out[(size_t)oc * P + p] = bf16r(v > 0 ? (float)v : 0.0f);
    }
  }
}

/* pb: params with the conv and fc weights rounded to bf16 (heads and biases fp32).  acts as in oracle_net_forward,
 * except x0 holds the raw byte values (the 1/255 is conv1's epilogue scale and its weight gradient's scale). */
static void EMU(forward_one)(const float *pb, const size_t *po, int H, int A, const uint8_t *obs, float *logits,
                             float *value, float *acts, float *cols, ACC *acc) {
  float *x0 = acts, *a1 = x0 + X0, *a2 = a1 + A1, *a3 = a2 + A2, *h = a3 + A3;
  for (int i = 0; i < X0; ++i)
    x0[i] = (float)obs[i];
  im2col(x0, 4, 84, 84, 8, 4, 20, 20, cols);
  EMU(conv_fwd)(pb + po[0], pb + po[1], cols, 32, 256, 400, 1.0f / 255.0f, a1, acc);
  im2col(a1, 32, 20, 20, 4, 2, 9, 9, cols);
  EMU(conv_fwd)(pb + po[2], pb + po[3], cols, 64, 512, 81, 1.0f, a2, acc);
  im2col(a2, 64, 9, 9, 3, 1, 7, 7, cols);
  EMU(conv_fwd)(pb + po[4], pb + po[5], cols, 64, 576, 49, 1.0f, a3, acc);
  for (int o = 0; o < H; ++o) { /* h: fp32, no rounding, no relu */
    const float *w = pb + po[6] + (size_t)o * A3;
    ACC s = 0;
    for (int j = 0; j < A3; ++j)
      s += (ACC)w[j] * (ACC)a3[j];
    h[o] = (float)(s + (ACC)pb[po[7] + o]);
  }
  for (int a = 0; a <= A; ++a) { /* heads: fp32 weights, fp32 outputs */
    const float *w = pb + (a < A ? po[8] + (size_t)a * H : po[10]);
    ACC s = 0;
    for (int j = 0; j < H; ++j)
      s += (ACC)w[j] * (ACC)h[j];
    const float z = (float)(s + (ACC)pb[a < A ? po[9] + a : po[11]]);
    if (a < A)
      logits[a] = z;
    else
      *value = z;
  }
}

/* dW[oc][k] += sum_p dz[oc][p] cols[k][p];  db[oc] += sum_p dz[oc][p]  (dz already bf16: bias from the rounded dz) */
static void EMU(conv_wgrad)(const float *dz, const float *cols, int OC, int Kd, int P, ACC *dw, ACC *db) {
  for (int oc = 0; oc < OC; ++oc) {
    const float *d = dz + (size_t)oc * P;
    for (int p = 0; p < P; ++p)
      db[oc] += (ACC)d[p];
    for (int k = 0; k < Kd; ++k) {
      const float *c = cols + (size_t)k * P;
      ACC s = dw[(size_t)oc * Kd + k];
      for (int p = 0; p < P; ++p)
        s += (ACC)d[p] * (ACC)c[p];
      dw[(size_t)oc * Kd + k] = s;
    }
  }
}

/* dz_in = bf16((act > 0) * col2im(sum_oc w[oc][k] dz[oc][p])) */
static void EMU(conv_dgrad)(const float *w, const float *dz, int OC, int Kd, int P, int C, int IH, int IW, int K,
                            int S, int OH, int OW, const float *act, ACC *dcols, ACC *din, float *out) {
  for (size_t i = 0; i < (size_t)Kd * P; ++i)
    dcols[i] = 0;
  for (int oc = 0; oc < OC; ++oc) {
    const float *d = dz + (size_t)oc * P;
    for (int k = 0; k < Kd; ++k) {
      const ACC wk = w[(size_t)oc * Kd + k];
      ACC *c = dcols + (size_t)k * P;
      for (int p = 0; p < P; ++p)
        c[p] += wk * (ACC)d[p];
    }
  }
  const int n = C * IH * IW;
  for (int i = 0; i < n; ++i)
    din[i] = 0;
  for (int c = 0; c < C; ++c)
    for (int kh = 0; kh < K; ++kh)
      for (int kw = 0; kw < K; ++kw) {
        const ACC *row = dcols + (size_t)((c * K + kh) * K + kw) * OH * OW;
        for (int oy = 0; oy < OH; ++oy)
          for (int ox = 0; ox < OW; ++ox)
            din[((size_t)c * IH + oy * S + kh) * IW + ox * S + kw] += row[oy * OW + ox];
      }
  for (int i = 0; i < n; ++i)
    out[i] = act[i] > 0.0f ? bf16r((float)din[i]) : 0.0f;
}

static void EMU(backward_one)(const float *pb, const size_t *po, int H, int A, const float *acts, const float *dlogits,
                              float dvalue, ACC *g, float *cols, ACC *dcols, ACC *din, float *scratch) {
  const float *x0 = acts, *a1 = x0 + X0, *a2 = a1 + A1, *a3 = a2 + A2, *h = a3 + A3;
  float *dh = scratch, *dz3 = dh + H, *dz2 = dz3 + A3, *dz1 = dz2 + A2;
  /* heads (fp32 operands): weight / bias gradients from the fp32 dz, dh = bf16(Wh^T dz) */
  for (int j = 0; j < H; ++j) {
    ACC s = (ACC)dvalue * (ACC)pb[po[10] + j];
    for (int a = 0; a < A; ++a)
      s += (ACC)dlogits[a] * (ACC)pb[po[8] + (size_t)a * H + j];
    dh[j] = bf16r((float)s);
  }
  for (int a = 0; a <= A; ++a) {
    const ACC d = a < A ? dlogits[a] : dvalue;
    ACC *gw = g + (a < A ? po[8] + (size_t)a * H : po[10]);
    for (int j = 0; j < H; ++j)
      gw[j] += d * (ACC)h[j];
    g[a < A ? po[9] + a : po[11]] += d;
  }
  /* fc: weight / bias gradients from the bf16 dh; dz3 = bf16((a3 > 0) * Wfc_b^T dh_b) */
  ACC *da3 = din;
  for (int j = 0; j < A3; ++j)
    da3[j] = 0;
  for (int o = 0; o < H; ++o) {
    const ACC d = dh[o];
    const float *w = pb + po[6] + (size_t)o * A3;
    ACC *gw = g + po[6] + (size_t)o * A3;
    for (int j = 0; j < A3; ++j) {
      da3[j] += d * (ACC)w[j];
      gw[j] += d * (ACC)a3[j];
    }
    g[po[7] + o] += d;
  }
  for (int j = 0; j < A3; ++j)
    dz3[j] = a3[j] > 0.0f ? bf16r((float)da3[j]) : 0.0f;
  /* conv3 */
  im2col(a2, 64, 9, 9, 3, 1, 7, 7, cols);
  EMU(conv_wgrad)(dz3, cols, 64, 576, 49, g + po[4], g + po[5]);
  EMU(conv_dgrad)(pb + po[4], dz3, 64, 576, 49, 64, 9, 9, 3, 1, 7, 7, a2, dcols, din, dz2);
  /* conv2 */
  im2col(a1, 32, 20, 20, 4, 2, 9, 9, cols);
  EMU(conv_wgrad)(dz2, cols, 64, 512, 81, g + po[2], g + po[3]);
  EMU(conv_dgrad)(pb + po[2], dz2, 64, 512, 81, 32, 20, 20, 4, 2, 9, 9, a1, dcols, din, dz1);
  /* conv1 (x0 = raw bytes: the 1/255 is applied to the summed weight gradient) */
  im2col(x0, 4, 84, 84, 8, 4, 20, 20, cols);
  EMU(conv_wgrad)(dz1, cols, 32, 256, 400, g + po[0], g + po[1]);
}

static void EMU(net_forward)(const float *params, int H, int A, const uint8_t *obs, int N, float *logits,
                             float *values, float *acts) {
  size_t po[13];
  oracle_param_offsets(H, A, po);
  const size_t aps = oracle_acts_per_sample(H);
  float *pb = bf16_compute_copy(params, po);
#pragma omp parallel
  {
    float *cols = (float *)malloc(sizeof(float) * COLS_MAX);
    ACC *acc = (ACC *)malloc(sizeof(ACC) * 400);
    float *tmp = acts ? NULL : (float *)malloc(sizeof(float) * aps);
#pragma omp for schedule(static)
    for (int n = 0; n < N; ++n)
      EMU(forward_one)(pb, po, H, A, obs + (size_t)n * X0, logits + (size_t)n * A, values + n,
                       acts ? acts + (size_t)n * aps : tmp, cols, acc);
    free(cols);
    free(acc);
    free(tmp);
  }
  free(pb);
}

static void EMU(net_backward)(const float *params, int H, int A, int N, const float *acts, const float *dlogits,
                              const float *dvalues, float *grads, float *dacts) {
  size_t po[13];
  oracle_param_offsets(H, A, po);
  const size_t np = po[12], aps = oracle_acts_per_sample(H);
  const int nt = oracle_num_threads();
  float *pb = bf16_compute_copy(params, po);
  ACC *part = (ACC *)calloc((size_t)nt * np, sizeof(ACC));
#pragma omp parallel num_threads(nt)
  {
#ifdef _OPENMP
    const int tid = omp_get_thread_num();
#else
    const int tid = 0;
#endif
    float *cols = (float *)malloc(sizeof(float) * COLS_MAX);
    ACC *dcols = (ACC *)malloc(sizeof(ACC) * COLS_MAX);
    ACC *din = (ACC *)malloc(sizeof(ACC) * A1);
    const size_t dps = (size_t)H + A3 + A2 + A1; /* dacts: as oracle_net_backward_stored (the scratch, kept) */
    float *scratch = (float *)malloc(sizeof(float) * dps);
#pragma omp for schedule(static)
    for (int n = 0; n < N; ++n)
      EMU(backward_one)(pb, po, H, A, acts + (size_t)n * aps, dlogits + (size_t)n * A, dvalues[n],
                        part + (size_t)tid * np, cols, dcols, din, dacts ? dacts + (size_t)n * dps : scratch);
    free(cols);
    free(dcols);
    free(din);
    free(scratch);
  }
  for (size_t i = 0; i < np; ++i) { /* fixed thread order -> deterministic for a fixed thread count */
    ACC s = 0;
    for (int t = 0; t < nt; ++t)
      s += part[(size_t)t * np + i];
    if (i < po[1])
      s *= (ACC)(1.0f / 255.0f); /* conv1's weight gradient: the epilogue scale of its slabs */
    grads[i] = (float)s;
  }
  free(part);
  free(pb);
}
