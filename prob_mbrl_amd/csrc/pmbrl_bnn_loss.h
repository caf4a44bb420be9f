// The loss sections of the BNN training step, the text of both kernel forms (pm_bnn_fwd_bwd, pmbrl_bnn.h; pm_bnn_fwd_bwd_spill,
// pmbrl_bnn_spill.h): included INSIDE the kernel body, behind the head GEMM.  As a function the sections changed the resident
// instances' register allocation (tools/kernel_diff.py); as text they compile to what they were.  Reads of the enclosing
// scope: A (BnnArgs), G1 (the head outputs [16][LD]), G0 (out: the gradient wrt them), red (PM_NT floats), R = 16, LD, nl, wg,
// row0, nvalid, tid.  Also writes the dW stash gT[nl - 1], part_loss and row_lp.  Contains barriers; the kernel syncs after.
  // ---- mixture negative log-likelihood (losses.py:40-64; head parametrisation models/densities.py:173-207):
  //      ll = logsumexp_c [log_softmax(logit / T)_c - sum_d lsc_dc - D/2 log 2 pi - 1/2 sum_d t_dc^2]
  if (A.gmm_n > 1) {
    const int n = A.gmm_n, D = A.n_out, nD = n * D, W16 = A.nt[nl] * 16;
    float* gst = A.gT[nl - 1] + (size_t)wg * W16 * 16;
    __shared__ float s_resp[16][PMBRL_MAX_COMP], s_sm[16][PMBRL_MAX_COMP], s_temp[16], s_ll[16];
    // responsibilities: one thread per row (n <= 8, D <= 64: a few hundred flops)
    if (tid < R) {
      const int r = tid;
      float ll = 0.f;
      if (r < nvalid) {
        const float* o = G1 + r * LD;
        const float* y = A.Y + (size_t)A.idx[row0 + r] * D;
        const float temp = 0.1f + softplusf(o[2 * nD + n]);
        float lg[PMBRL_MAX_COMP], lp[PMBRL_MAX_COMP], mx = -3.0e38f;
        for (int c = 0; c < n; ++c) { lg[c] = o[2 * nD + c] / temp; mx = fmaxf(mx, lg[c]); }
        float se = 0.f;
        for (int c = 0; c < n; ++c) se += expf(lg[c] - mx);
        const float lse = mx + logf(se);
        float mxp = -3.0e38f;
        for (int c = 0; c < n; ++c) {
          float sls = 0.f, sq = 0.f;
          for (int d = 0; d < D; ++d) {
            const float lsc = -softplusf(-o[nD + d * n + c] + A.mls) + A.mls;
            const float t = (o[d * n + c] - y[d]) * expf(-lsc);
            sls += lsc;
            sq = fmaf(t, t, sq);
          }
          lp[c] = (lg[c] - lse) + (-(float)D * 0.9189385332046727f - sls) - 0.5f * sq;
          s_sm[r][c] = expf(lg[c] - lse);
          mxp = fmaxf(mxp, lp[c]);
        }
        float sp = 0.f;
        for (int c = 0; c < n; ++c) sp += expf(lp[c] - mxp);
        ll = mxp + logf(sp);
        for (int c = 0; c < n; ++c) s_resp[r][c] = expf(lp[c] - ll);
        s_temp[r] = temp;
      }
      s_ll[r] = ll;
    }
    __syncthreads();
    float lsum = 0.f;
    for (int i = tid; i < R * W16; i += PM_NT) {
      const int r = i / W16, j = i - r * W16;
      float gval = 0.f;
      if (r < nvalid && j <= 2 * nD + n) {
        const float* o = G1 + r * LD;
        const float rw = (A.row_w ? A.row_w[row0 + r] : 1.f) * A.inv_M;
        if (j < 2 * nD) {
          const int jj = j < nD ? j : j - nD, d = jj / n, c = jj - d * n;
          const float ls = o[nD + jj];
          const float lsc = -softplusf(-ls + A.mls) + A.mls;
          const float sd = expf(-lsc);
          const float t = (o[jj] - A.Y[(size_t)A.idx[row0 + r] * D + d]) * sd;
          gval = j < nD ? rw * s_resp[r][c] * t * sd : rw * s_resp[r][c] * (1.f - t * t) * sigmoidf(A.mls - ls);
        } else if (j < 2 * nD + n) {
          const int c = j - 2 * nD;
          gval = -rw * (s_resp[r][c] - s_sm[r][c]) / s_temp[r];
        } else {
          float a = 0.f;
          for (int c = 0; c < n; ++c) a += (s_resp[r][c] - s_sm[r][c]) * o[2 * nD + c];
          gval = rw * a * sigmoidf(o[2 * nD + n]) / (s_temp[r] * s_temp[r]);
        }
        if (j == 0) lsum -= (A.row_w ? A.row_w[row0 + r] : 1.f) * s_ll[r];
      }
      G0[r * LD + j] = gval;
      gst[(size_t)j * 16 + r] = gval;
    }
    red[tid] = lsum;
    __syncthreads();
    for (int o = PM_NT / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) A.part_loss[wg] = red[0];
    if (A.row_lp && tid < nvalid) A.row_lp[row0 + tid] = s_ll[tid];
  } else
  // ---- Gaussian negative log-likelihood and its gradient wrt the head outputs
  {
    const int n = A.n_out;
    float* gst = A.gT[nl - 1] + (size_t)wg * A.nt[nl] * 16 * 16;
    float lsum = 0.f;
    __shared__ float rowlp[16];
    if (tid < 16) rowlp[tid] = 0.f;
    __syncthreads();
    for (int i = tid; i < R * A.nt[nl] * 16; i += PM_NT) {
      const int r = i / (A.nt[nl] * 16), j = i - r * (A.nt[nl] * 16);
      float gval = 0.f;
      if (r < nvalid && j < 2 * n) {
        const int d = j < n ? j : j - n;
        const float mu = G1[r * LD + d];
        const float ls = G1[r * LD + n + d];
        if (A.mse) {
          // torch.nn.functional.mse_loss: mean over the M x n entries
          const float dl = mu - A.Y[(size_t)A.idx[row0 + r] * n + d];
          if (j < n) {
            gval = 2.f * dl * A.inv_M / (float)n;
            lsum += dl * dl / (float)n;
          }
        } else {
        const float lsc = -softplusf(-ls + A.mls) + A.mls;
        const float s = expf(-lsc);
        const float t = (mu - A.Y[(size_t)A.idx[row0 + r] * n + d]) * s;
        const float rw = A.row_w ? A.row_w[row0 + r] : 1.f;
        if (j < n) {
          gval = rw * t * s * A.inv_M;
          const float nl_d = 0.5f * t * t + lsc + 0.9189385332046727f;   // + 1/2 log(2 pi)
          lsum += rw * nl_d;
          if (A.row_lp) atomicAdd(&rowlp[r], -nl_d);
        } else {
          gval = rw * (1.f - t * t) * sigmoidf(A.mls - ls) * A.inv_M;
        }
        }
      }
      G0[r * LD + j] = gval;
      gst[(size_t)j * 16 + r] = gval;
    }
    red[tid] = lsum;
    __syncthreads();
    for (int o = PM_NT / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) A.part_loss[wg] = red[0];
    if (A.row_lp && tid < nvalid) A.row_lp[row0 + tid] = rowlp[tid];
  }
