// Stand-alone evaluation of one Bayesian MLP + diagonal-Gaussian head on B independent rows
// (include/pmbrl.h: pmbrl_mlp_forward; reference: models/core.py:169-187, 221-248, 265-303,
// models/densities.py:87-121).  Same MFMA tile routines and fragment-packed weights as the
// rollout kernels; a workgroup (PM_NW waves) owns 16 rows and walks the layers through two LDS
// activation buffers.  This is the acting / model-evaluation path (a handful of rows per call),
// not a throughput kernel.
#pragma once
#include "pmbrl_dev.h"

struct MlpArgs {
  int B, nl, LD, n_out;
  int dim[PM_MAXL + 1], nt[PM_MAXL + 1];
  const float* wf[PM_MAXL];
  const float* bias[PM_MAXL];
  const uint16_t* mask[PM_MAXL];    // bit rows [B][nt[l+1]] or nullptr
  float keep[PM_MAXL];
  const float *x, *z, *in_shift, *in_iscale, *out_scale, *out_shift, *sq_scale, *sq_bias;
  float mls;
  float *sample, *mean, *log_std;
  int act;                          // PMBRL_ACT_* per hidden layer (pm_act_code); 0: every layer is ReLU
};

// The same with this layer's activation (pm_act; act = its PMBRL_ACT_* code): h = act(v) * mask / keep, and -- d_out
// given, the input gradient's recomputed forward -- act'(v) * mask / keep next to it.  Padded units (width .. nt * 16),
// rows past nvalid and masked units are 0 in both, whatever act(0) is (PMBRL_ACT_EXP: 1).
struct EpiMlpAct {
  const float* bias;
  const uint16_t* mask;
  float keep;
  float* lds_out;
  float* d_out;
  int ld, row0, nvalid, nt, lane, act, width;
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) {
    const int g = lane >> 4;
    const int lrow = rt * 16 + (lane & 15);
    const int f0 = ot * 16 + 4 * g;
    const f32x4 b = ldg4(bias + f0);
    unsigned nib = lrow < nvalid ? 0xFu : 0u;
    if (mask && lrow < nvalid) nib = ((unsigned)mask[(size_t)(row0 + lrow) * nt + ot] >> (4 * g)) & 0xFu;
    f32x4 h, d;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float hv, dv;
      pm_act(act, acc[r] + b[r], f0 + r, width, hv, dv);
      const bool m = ((nib >> r) & 1u) && f0 + r < width;
      h[r] = m ? (keep == 1.f ? hv : hv / keep) : 0.f;
      d[r] = m ? (keep == 1.f ? dv : dv / keep) : 0.f;
    }
    *reinterpret_cast<f32x4*>(lds_out + lrow * ld + f0) = h;
    if (d_out) *reinterpret_cast<f32x4*>(d_out + lrow * ld + f0) = d;
  }
};

struct EpiMlpHidden {
  const float* bias;
  const uint16_t* mask;
  float keep;
  float* lds_out;
  int ld, row0, nvalid, nt, lane;
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) {
    const int g = lane >> 4;
    const int lrow = rt * 16 + (lane & 15);
    const int f0 = ot * 16 + 4 * g;
    const f32x4 b = ldg4(bias + f0);
    unsigned nib = 0xFu;
    if (mask) {
      unsigned mw = 0;
      if (lrow < nvalid) mw = mask[(size_t)(row0 + lrow) * nt + ot];
      nib = (mw >> (4 * g)) & 0xFu;
    }
    f32x4 h;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = acc[r] + b[r];
      const bool a = ((nib >> r) & 1u) && (v > 0.f);
      h[r] = a ? (keep == 1.f ? v : v / keep) : 0.f;
    }
    *reinterpret_cast<f32x4*>(lds_out + lrow * ld + f0) = h;
  }
};

// ---------------------------------------------------------------------------
// layer norm (pmbrl_mlp_layer_norm; models/core.py:56-58): hidden layer l with gamma[l] != nullptr normalises the row of
// v = h W^T + b over the layer's true width before the activation.  The GEMM's epilogue stores v (EpiMlpLnPre), and
// behind the barrier a row pass (pm_mlp_ln_rows) does the rest in place: a wave owns rows wid, wid + PM_NW of the tile,
// a lane the units lane, lane + 64, ..., and the row sums meet by a butterfly over the wave's lanes -- a fixed order.
// The LN instances of the three kernels are compile-time (template <bool LN>); the <false> instances are the kernels as
// they were.
// ---------------------------------------------------------------------------
struct MlpLnArgs {
  const float* gamma[PM_MAXL];     // [dim[l + 1]] of hidden layer l, or null: no layer norm
  const float* beta[PM_MAXL];
  float eps[PM_MAXL];
  int z_idx[PM_MAXL];              // which zhat buffer (the backward kernels)
  size_t g_off[PM_MAXL];           // offset of the layer's [d gamma | d beta] in grad_ln
  float* slab;                     // [gridDim.x][n_ln] or null (pm_mlp_bwdp_kernel)
  size_t n_ln;
};

// v = acc + b, exact zeros in rows >= nvalid and columns >= width
struct EpiMlpLnPre {
  const float* bias;
  float* lds_out;
  int ld, nvalid, lane, width;
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) {
    const int g = lane >> 4;
    const int lrow = rt * 16 + (lane & 15);
    const int f0 = ot * 16 + 4 * g;
    const f32x4 b = ldg4(bias + f0);
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (lrow < nvalid && f0 + r < width) ? acc[r] + b[r] : 0.f;
    *reinterpret_cast<f32x4*>(lds_out + lrow * ld + f0) = v;
  }
};

__device__ __forceinline__ float pm_wave_sum(float s) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
  return s;
}

// where 1 / sqrt(var + eps) of a row sits: the first of the 8 spare columns of its zhat row (LD = widest layer + 8)
#define PM_LN_RSTD(ld) ((ld) - 8)

// The row pass of a layer-norm layer.  V [16][ld]: v in, h = act(y) * mask / keep out.  Next to it, each where its
// buffer is given: D = act'(y) * mask / keep, Z = zhat (and the row's rstd), Q = a probs (1 - probs) / temp of a
// train-mode concrete layer (a = act(y) before the mask; EpiMlpConcFwd).  Rows >= nvalid and columns >= width: exact
// zeros in all of them.
struct MlpLnRows {
  const float *gamma, *beta;
  float eps;
  const uint16_t* mask;
  float keep;
  int act, width, nt;
  float *V, *D, *Z;
  const float *u, *logit;          // (Q given)
  float temp;
  float* Q;
};
__device__ __forceinline__ void pm_mlp_ln_rows(const MlpLnRows& p, int ld, int row0, int nvalid, int wid, int lane) {
  const int W16 = p.nt * 16;
  for (int r = wid; r < 16; r += PM_NW) {
    float* v = p.V + r * ld;
    float* d = p.D ? p.D + r * ld : nullptr;
    float* z = p.Z ? p.Z + r * ld : nullptr;
    float* q = p.Q ? p.Q + r * ld : nullptr;
    float mu = 0.f, rstd = 0.f;
    if (r < nvalid) {
      float s = 0.f;
      for (int j = lane; j < p.width; j += 64) s += v[j];
      mu = pm_wave_sum(s) / (float)p.width;
      float ss = 0.f;
      for (int j = lane; j < p.width; j += 64) {
        const float c = v[j] - mu;
        ss += c * c;
      }
      rstd = 1.f / sqrtf(pm_wave_sum(ss) / (float)p.width + p.eps);
    }
    for (int j = lane; j < W16; j += 64) {
      float hv = 0.f, dv = 0.f, zv = 0.f, qv = 0.f;
      if (r < nvalid && j < p.width) {
        zv = (v[j] - mu) * rstd;
        float a, da;
        pm_act(p.act, p.gamma[j] * zv + p.beta[j], j, p.width, a, da);
        bool m = true;
        if (p.mask) m = ((unsigned)p.mask[(size_t)(row0 + r) * p.nt + (j >> 4)] >> (j & 15)) & 1u;
        if (m) {
          hv = p.keep == 1.f ? a : a / p.keep;
          dv = p.keep == 1.f ? da : da / p.keep;
        }
        if (q) {
          const float uu = p.u[(size_t)(row0 + r) * p.width + j];
          const float c = p.logit[j] + logf((uu + 1e-7f) / (1.f - (uu - 1e-7f)));
          const float e = expf(-fabsf(c / p.temp));
          qv = a * (e / ((1.f + e) * (1.f + e))) / p.temp;
        }
      }
      v[j] = hv;
      if (d) d[j] = dv;
      if (z) z[j] = zv;
      if (q) q[j] = qv;
    }
    if (z && lane == 0) z[PM_LN_RSTD(ld)] = rstd;
  }
}

// The backward's row pass: G [16][ld] holds g_y (what the dX epilogue left), and becomes
//   g_v = rstd (g_zhat - mean_j g_zhat - zhat mean_j (g_zhat zhat)),   g_zhat = g_y gamma
// in place.  Rows >= nvalid hold zeros in G and Z (rstd 0) and stay zeros; columns >= width are not touched.
__device__ __forceinline__ void pm_mlp_ln_bwd_rows(float* G, const float* Z, const float* gamma, int width, int ld,
                                                   int wid, int lane) {
  for (int r = wid; r < 16; r += PM_NW) {
    float* g = G + r * ld;
    const float* z = Z + r * ld;
    const float rstd = z[PM_LN_RSTD(ld)];
    float s1 = 0.f, s2 = 0.f;
    for (int j = lane; j < width; j += 64) {
      const float gz = g[j] * gamma[j];
      s1 += gz;
      s2 += gz * z[j];
    }
    s1 = pm_wave_sum(s1) / (float)width;
    s2 = pm_wave_sum(s2) / (float)width;
    for (int j = lane; j < width; j += 64) g[j] = rstd * (g[j] * gamma[j] - s1 - z[j] * s2);
  }
}

// slab[d gamma | d beta] (+)= column sums over the tile's valid rows of g_y zhat | g_y, as pm_mlp_accum_dw sums db
__device__ __forceinline__ void pm_mlp_ln_accum(const float* G, const float* Z, int ld, int width, float* dgb, bool first,
                                                int nvalid, int tid) {
  for (int o = tid; o < width; o += PM_NT) {
    float sg = first ? 0.f : dgb[o], sb = first ? 0.f : dgb[width + o];
    for (int r = 0; r < nvalid; ++r) {
      const float gy = G[r * ld + o];
      sg += gy * Z[r * ld + o];
      sb += gy;
    }
    dgb[o] = sg;
    dgb[width + o] = sb;
  }
}

struct MlpLnFwdArgs : MlpArgs {
  MlpLnArgs ln;
};
template <bool LN> struct MlpFwdSel { typedef MlpArgs type; };
template <> struct MlpFwdSel<true> { typedef MlpLnFwdArgs type; };

// LN: some hidden layers are layer-normalised (MlpLnFwdArgs); <false> is pmbrl_mlp_forward's kernel as it always was
template <bool LN>
__global__ __launch_bounds__(PM_NT, 1) void pm_mlp_fwd_kernel(const typename MlpFwdSel<LN>::type A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = 16;
  const MlpLnArgs* Ln = nullptr;
  if constexpr (LN) Ln = &A.ln;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * R;
  const int nvalid = min(R, A.B - row0);
  const int LD = A.LD;
  float* X = smem;
  float* Y = smem + (size_t)R * LD;
  float* part = smem + 2 * (size_t)R * LD;
  const int K0 = A.dim[0];
  for (int i = tid; i < R * A.nt[0] * 16; i += PM_NT) {
    const int r = i / (A.nt[0] * 16), k = i - r * (A.nt[0] * 16);
    float v = 0.f;
    if (r < nvalid && k < K0) {
      v = A.x[(size_t)(row0 + r) * K0 + k];
      if (A.in_shift) v = (v - A.in_shift[k]) * A.in_iscale[k];
    }
    X[r * LD + k] = v;
  }
  __syncthreads();
  for (int l = 0; l < A.nl - 1; ++l) {
    if constexpr (LN) {
      if (Ln->gamma[l]) {
        EpiMlpLnPre e{A.bias[l], Y, LD, nvalid, lane, A.dim[l + 1]};
        gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], X, LD, wid, lane, e);
        __syncthreads();
        const MlpLnRows p{Ln->gamma[l], Ln->beta[l], Ln->eps[l], A.mask[l], A.keep[l], pm_act_code(A.act, l), A.dim[l + 1],
                          A.nt[l + 1], Y, nullptr, nullptr, nullptr, nullptr, 1.f, nullptr};
        pm_mlp_ln_rows(p, LD, row0, nvalid, wid, lane);
        __syncthreads();
        float* t = X; X = Y; Y = t;
        continue;
      }
    }
    if (A.act != PMBRL_ACT_RELU) {
      EpiMlpAct e{A.bias[l], A.mask[l], A.keep[l], Y, nullptr, LD, row0, nvalid, A.nt[l + 1], lane, pm_act_code(A.act, l), A.dim[l + 1]};
      gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], X, LD, wid, lane, e);
    } else {
      EpiMlpHidden e{A.bias[l], A.mask[l], A.keep[l], Y, LD, row0, nvalid, A.nt[l + 1], lane};
      gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], X, LD, wid, lane, e);
    }
    __syncthreads();
    float* t = X; X = Y; Y = t;
  }
  gemm_narrow<1>(A.wf[A.nl - 1], A.nt[A.nl], A.nt[A.nl - 1], A.bias[A.nl - 1], X, Y, LD, part, wid, lane, tid);
  const int n = A.n_out;
  for (int i = tid; i < nvalid * n; i += PM_NT) {
    const int r = i / n, j = i - r * n;
    float mu = Y[r * LD + j];
    float ls = Y[r * LD + n + j];
    ls = -softplusf(-ls + A.mls) + A.mls;            // models/densities.py:97-98
    if (A.out_scale) {
      ls += logf(A.out_scale[j]);
      mu = mu * A.out_scale[j] + A.out_shift[j];
    }
    const size_t o = (size_t)(row0 + r) * n + j;
    float s = mu;
    if (A.z) s = mu + A.z[o] * expf(ls);
    if (A.sq_scale) s = A.sq_scale[j] * tanhf(s) + A.sq_bias[j];
    if (A.sample) A.sample[o] = s;
    if (A.mean) A.mean[o] = mu;
    if (A.log_std) A.log_std[o] = ls;
  }
}

// ---------------------------------------------------------------------------
// gradient of the outputs of pm_mlp_fwd_kernel with respect to its INPUT rows (the network is
// constant): what autograd needs when a stand-alone network sits inside a differentiable
// computation, e.g. the terminal value V(x_H) of algorithms/mc_pilco.py:136-140.  The forward
// is recomputed in the same launch (layer inputs stay in LDS), then the dX chain runs back.
// ---------------------------------------------------------------------------
struct MlpBwdArgs {
  MlpArgs f;                       // the forward's arguments (outputs unused)
  const float* wb[PM_MAXL];        // transposed fragments
  const float *g_sample, *g_mean, *g_log_std;   // [B][n_out], any may be null
  float* grad_x;                   // [B][n_in]
};

struct EpiMlpBwd {
  const float* h_in;               // that layer's output (zero where masked / inactive)
  float inv_keep;
  float* g_out;
  int ld, lane;
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) {
    const int g = lane >> 4, lrow = lane & 15;
    const int f0 = ot * 16 + 4 * g;
    const f32x4 h = *reinterpret_cast<const f32x4*>(h_in + lrow * ld + f0);
    f32x4 gp;
#pragma unroll
    for (int r = 0; r < 4; ++r) gp[r] = h[r] > 0.f ? acc[r] * inv_keep : 0.f;
    *reinterpret_cast<f32x4*>(g_out + lrow * ld + f0) = gp;
  }
};

// ... an activation other than ReLU: g_pre = acc * d with d = act'(v) * mask / keep from the recomputed forward (the
// layer's OUTPUT does not give SiLU's derivative).  d of hidden layer l - 1 lives where the input of layer l - 2 was -- dead
// once layer l - 2 has run -- and the first hidden layer's in one more buffer (pm_mlp_bwd_lds_floats).
struct EpiMlpBwdAct {
  const float* d_in;
  float* g_out;
  int ld, lane;
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) {
    const int g = lane >> 4, lrow = lane & 15;
    const int f0 = ot * 16 + 4 * g;
    const f32x4 d = *reinterpret_cast<const f32x4*>(d_in + lrow * ld + f0);
    f32x4 gp;
#pragma unroll
    for (int r = 0; r < 4; ++r) gp[r] = d[r] != 0.f ? acc[r] * d[r] : 0.f;
    *reinterpret_cast<f32x4*>(g_out + lrow * ld + f0) = gp;
  }
};

// the 16 input rows of a tile, normalised, zero beyond the valid rows and the true width
__device__ __forceinline__ void pm_mlp_load_rows(const MlpArgs& A, float* H, int row0, int nvalid, int tid) {
  const int K0 = A.dim[0], LD = A.LD;
  for (int i = tid; i < 16 * A.nt[0] * 16; i += PM_NT) {
    const int r = i / (A.nt[0] * 16), k = i - r * (A.nt[0] * 16);
    float v = 0.f;
    if (r < nvalid && k < K0) {
      v = A.x[(size_t)(row0 + r) * K0 + k];
      if (A.in_shift) v = (v - A.in_shift[k]) * A.in_iscale[k];
    }
    H[r * LD + k] = v;
  }
}

// gradient wrt the raw head outputs [mu | log_std] (`raw`, from the recomputed forward) into `g`: exact zeros in the
// rows past the valid ones and the columns past 2 n_out
__device__ __forceinline__ void pm_mlp_head_grad(const MlpBwdArgs& B, const float* raw, float* g, int row0, int nvalid,
                                                 int tid) {
  const MlpArgs& A = B.f;
  const int LD = A.LD;
  const int n = A.n_out, W16 = A.nt[A.nl] * 16;
  for (int i = tid; i < 16 * W16; i += PM_NT) {
    const int r = i / W16, j = i - r * W16;
    float gv = 0.f;
    if (r < nvalid && j < 2 * n) {
      const int d = j < n ? j : j - n;
      const size_t o = (size_t)(row0 + r) * n + d;
      const float mu0 = raw[r * LD + d], ls0 = raw[r * LD + n + d];
      float ls = -softplusf(-ls0 + A.mls) + A.mls;
      float mu = mu0, osc = 1.f;
      if (A.out_scale) {
        osc = A.out_scale[d];
        ls += logf(osc);
        mu = mu0 * osc + A.out_shift[d];
      }
      const float zz = A.z ? A.z[o] : 0.f;
      const float e = expf(ls);
      float gs = B.g_sample ? B.g_sample[o] : 0.f;
      if (A.sq_scale && B.g_sample) {
        const float th = tanhf(mu + zz * e);
        gs *= A.sq_scale[d] * (1.f - th * th);
      }
      if (j < n) gv = (gs + (B.g_mean ? B.g_mean[o] : 0.f)) * osc;
      else gv = (gs * zz * e + (B.g_log_std ? B.g_log_std[o] : 0.f)) * sigmoidf(A.mls - ls0);
    }
    g[r * LD + j] = gv;
  }
}

__host__ __device__ inline size_t pm_mlp_bwd_lds_floats(int nl, int LD, int act = 0, int n_ln = 0) {
  // H[0..nl-1], two gradient buffers, K-split scratch; act != ReLU: the first hidden layer's derivatives; one zhat
  // buffer per layer-norm layer (pmbrl_mlp_grad_input_ln)
  return ((size_t)nl + 2 + (act ? 1 : 0) + n_ln) * 16 * LD + (size_t)PM_NW * PM_KS_NT * 256;
}

struct MlpLnBwdArgs {
  MlpBwdArgs b;
  MlpLnArgs ln;
};
template <bool LN> struct MlpBwdSel { typedef MlpBwdArgs type; };
template <> struct MlpBwdSel<true> { typedef MlpLnBwdArgs type; };
__device__ __forceinline__ const MlpBwdArgs& pm_bwd_of(const MlpBwdArgs& a) { return a; }
__device__ __forceinline__ const MlpBwdArgs& pm_bwd_of(const MlpLnBwdArgs& a) { return a.b; }
__device__ __forceinline__ const MlpLnArgs* pm_ln_of(const MlpBwdArgs&) { return nullptr; }
__device__ __forceinline__ const MlpLnArgs* pm_ln_of(const MlpLnBwdArgs& a) { return &a.ln; }

// LN: as pm_mlp_fwd_kernel's; the recomputed forward also leaves zhat and rstd of every layer-norm layer in a buffer of
// its own, and the dX chain turns g_y into g_v behind each dX GEMM (pm_mlp_ln_bwd_rows)
template <bool LN>
__global__ __launch_bounds__(PM_NT, 1) void pm_mlp_bwdx_kernel(const typename MlpBwdSel<LN>::type BB) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = 16;
  const MlpBwdArgs& B = pm_bwd_of(BB);
  const MlpLnArgs* Ln = pm_ln_of(BB);
  const MlpArgs& A = B.f;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * R;
  const int nvalid = min(R, A.B - row0);
  const int LD = A.LD, nl = A.nl;
  float* H = smem;                                   // [nl][16][LD]
  float* G0 = H + (size_t)nl * R * LD;
  float* G1 = G0 + (size_t)R * LD;
  float* part = G1 + (size_t)R * LD;
  const bool smooth = A.act != PMBRL_ACT_RELU;
  float* D0 = part + (size_t)PM_NW * PM_KS_NT * 256;   // (smooth only: pm_mlp_bwd_lds_floats)
  // derivatives of hidden layer l (the output of Linear l): D0 for l = 0, else the dead input buffer of Linear l - 1
  auto dbuf = [&](int l) { return l == 0 ? D0 : H + (size_t)(l - 1) * R * LD; };
  const int K0 = A.dim[0];
  float* Z = D0 + (smooth ? (size_t)R * LD : 0);      // (LN only) [layer-norm layers][16][LD]
  pm_mlp_load_rows(A, H, row0, nvalid, tid);
  __syncthreads();
  for (int l = 0; l < nl - 1; ++l) {
    if constexpr (LN) {
      if (Ln->gamma[l]) {
        float* Hn = H + (size_t)(l + 1) * R * LD;
        EpiMlpLnPre e{A.bias[l], Hn, LD, nvalid, lane, A.dim[l + 1]};
        gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], H + (size_t)l * R * LD, LD, wid, lane, e);
        __syncthreads();
        const MlpLnRows p{Ln->gamma[l], Ln->beta[l], Ln->eps[l], A.mask[l], A.keep[l], pm_act_code(A.act, l), A.dim[l + 1],
                          A.nt[l + 1], Hn, smooth ? dbuf(l) : nullptr, Z + (size_t)Ln->z_idx[l] * R * LD, nullptr, nullptr,
                          1.f, nullptr};
        pm_mlp_ln_rows(p, LD, row0, nvalid, wid, lane);
        __syncthreads();
        continue;
      }
    }
    if (smooth) {
      EpiMlpAct e{A.bias[l], A.mask[l], A.keep[l], H + (size_t)(l + 1) * R * LD, dbuf(l), LD, row0, nvalid, A.nt[l + 1],
                  lane, pm_act_code(A.act, l), A.dim[l + 1]};
      gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], H + (size_t)l * R * LD, LD, wid, lane, e);
    } else {
      EpiMlpHidden e{A.bias[l], A.mask[l], A.keep[l], H + (size_t)(l + 1) * R * LD, LD, row0, nvalid, A.nt[l + 1], lane};
      gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], H + (size_t)l * R * LD, LD, wid, lane, e);
    }
    __syncthreads();
  }
  gemm_narrow<1>(A.wf[nl - 1], A.nt[nl], A.nt[nl - 1], A.bias[nl - 1], H + (size_t)(nl - 1) * R * LD, G1, LD, part,
                 wid, lane, tid);
  pm_mlp_head_grad(B, G1, G0, row0, nvalid, tid);
  __syncthreads();
  float* Gin = G0;
  float* Gout = G1;
  for (int l = nl - 1; l >= 1; --l) {
    if (smooth) {
      EpiMlpBwdAct e{dbuf(l - 1), Gout, LD, lane};
      gemm_tiles<1>(B.wb[l], A.nt[l], A.nt[l + 1], Gin, LD, wid, lane, e);
    } else {
      EpiMlpBwd e{H + (size_t)l * R * LD, 1.f / A.keep[l - 1], Gout, LD, lane};
      gemm_tiles<1>(B.wb[l], A.nt[l], A.nt[l + 1], Gin, LD, wid, lane, e);
    }
    __syncthreads();
    if constexpr (LN) {
      if (Ln->gamma[l - 1]) {                          // Gout = g_y of hidden layer l - 1 -> g_v
        pm_mlp_ln_bwd_rows(Gout, Z + (size_t)Ln->z_idx[l - 1] * R * LD, Ln->gamma[l - 1], A.dim[l], LD, wid, lane);
        __syncthreads();
      }
    }
    float* t = Gin; Gin = Gout; Gout = t;
  }
  // first layer: d / d x_in, then the input normalisation
  {
    EpiPlain e{nullptr, Gout, LD, lane};
    gemm_tiles<1>(B.wb[0], A.nt[0], A.nt[1], Gin, LD, wid, lane, e);
    __syncthreads();
    for (int i = tid; i < nvalid * K0; i += PM_NT) {
      const int r = i / K0, k = i - r * K0;
      float v = Gout[r * LD + k];
      if (A.in_iscale) v *= A.in_iscale[k];
      B.grad_x[(size_t)(row0 + r) * K0 + k] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// gradient with respect to the PARAMETERS as well (pmbrl_mlp_backward): pm_mlp_bwdx_kernel's recomputed forward and dX
// chain, and at every Linear l -- while G_l (gradient at its output) and H_l (its input) both sit in LDS --
//   dW_l += G_l^T H_l   (v_mfma_f32_16x16x4_f32 with the tile's 16 ROWS as K: four issues per 16 x 16 tile of dW_l)
//   db_l += sum_r G_l[r]
// The weight gradient reads every H_l, so the derivatives of a Tanh / SiLU layer cannot live in a dead H buffer as they
// do above: they get buffers of their own (pm_mlp_bwdp_lds_floats).  The grid is capped (PMBRL_MLP_BWD_MAX_BLOCKS): a
// workgroup strides over its tiles and adds into its own slab [n_params] of the workspace -- the same lane adds to the
// same address in program order, the first tile stores instead of adding -- and pm_mlp_bwd_reduce_kernel sums the slabs
// in slab order.  No atomics anywhere: the result is the same bits call after call.
// ---------------------------------------------------------------------------
struct MlpBwdPArgs {
  MlpBwdArgs b;                    // grad_x may be null here
  float* slab;                     // [gridDim.x][n_params] or null (no parameter gradient wanted)
  size_t n_params;
  size_t w_off[PM_MAXL], b_off[PM_MAXL];   // offsets of W_l [out][in] and b_l in the flat parameter order
};

__host__ __device__ inline size_t pm_mlp_bwdp_lds_floats(int nl, int LD, int act, int n_conc = 0, int n_ln = 0) {
  // H[0..nl-1], two gradient buffers, K-split scratch; act != ReLU: one derivative buffer per hidden layer; one Q buffer
  // per train-mode concrete-dropout layer (pmbrl_mlp_backward_concrete); one zhat buffer per layer-norm layer
  // (pmbrl_mlp_backward_ln).  Two hidden layers of 200 (LD = 216, 13 824 B a buffer, 24 KB scratch) against 160 KB:
  // ReLU + 2 LN + 2 concrete is 9 buffers = 148 992 B and fits, Tanh / SiLU + 2 LN + 2 concrete is 11 = 176 640 B and does
  // not; Tanh + 2 LN + 1 concrete (10 = 162 816 B) still fits (the table in include/pmbrl.h).
  return ((size_t)nl + 2 + (act ? nl - 1 : 0) + n_conc + n_ln) * 16 * LD + (size_t)PM_NW * PM_KS_NT * 256;
}

// ---------------------------------------------------------------------------
// train-mode concrete dropout (pmbrl_mlp_backward_concrete; models/modules.py:102-118,151-153): the mask of layer l is
// a hard Bernoulli sample of probs = sigmoid(c / temp), c = logit_p[j] + log((u + 1e-7) / (1 - (u - 1e-7))), and the
// backward goes through probs:  d logit_p[j] += sum_r gh[r][j] a[r][j] probs (1 - probs) / temp  with a the activation
// BEFORE the mask and gh the gradient at the layer's output before the mask -- both at dropped units too.  The
// recomputed forward leaves Q = a probs (1 - probs) / temp in a buffer of its own, the dX chain multiplies its
// accumulator (gh) by it and sums the tile's 16 rows.
// ---------------------------------------------------------------------------
struct MlpConcArgs {
  const float* u[PM_MAXL];         // [B][dim[l + 1]] uniform noise of hidden layer l, or null: not a concrete layer
  const float* logit[PM_MAXL];     // [dim[l + 1]]
  float temp[PM_MAXL];
  int q_idx[PM_MAXL];              // which Q buffer
  size_t g_off[PM_MAXL];           // offset of the layer's logits in the gradient
  float* slab;                     // [gridDim.x][n_logit]
  size_t n_logit;
};

// the base epilogue of the recomputed forward, and Q next to it: exact zeros in rows >= nvalid and columns >= width
template <class Base>
struct EpiMlpConcFwd {
  Base base;
  const float *bias, *u, *logit;
  float temp;
  float* q_out;
  int ld, row0, nvalid, lane, act, width;
  bool smooth;
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) {
    base(ot, rt, acc);
    const int g = lane >> 4;
    const int lrow = rt * 16 + (lane & 15);
    const int f0 = ot * 16 + 4 * g;
    const f32x4 b = ldg4(bias + f0);
    f32x4 q;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = f0 + r;
      float qv = 0.f;
      if (lrow < nvalid && j < width) {
        const float v = acc[r] + b[r];
        float a = v > 0.f ? v : 0.f, d;
        if (smooth) pm_act(act, v, j, width, a, d);
        const float uu = u[(size_t)(row0 + lrow) * width + j];
        const float c = logit[j] + logf((uu + 1e-7f) / (1.f - (uu - 1e-7f)));
        // probs (1 - probs) = e / (1 + e)^2 with e = exp(-|c / temp|): no overflow, an exact 0 once probs saturates
        const float e = expf(-fabsf(c / temp));
        qv = a * (e / ((1.f + e) * (1.f + e))) / temp;
      }
      q[r] = qv;
    }
    *reinterpret_cast<f32x4*>(q_out + lrow * ld + f0) = q;
  }
};

// the base epilogue of the dX chain (acc = gh), and gl[j] (+)= sum over the tile's rows of gh Q: a lane holds one row
// and four units, so the 16 rows meet by a butterfly over the lanes of a 16-lane group -- a fixed order -- and lane 0 of
// the group owns the four addresses: the first tile stores, later tiles add in program order
template <class Base>
struct EpiMlpConcBwd {
  Base base;
  const float* q_in;
  float* gl;
  bool first;
  int ld, lane, width;
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) {
    base(ot, rt, acc);
    const int g = lane >> 4, lrow = lane & 15;
    const int f0 = ot * 16 + 4 * g;
    const f32x4 q = *reinterpret_cast<const f32x4*>(q_in + lrow * ld + f0);
    f32x4 s;
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = acc[r] * q[r];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) s[r] += __shfl_xor(s[r], o);
    }
    if (lrow == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (f0 + r < width) gl[f0 + r] = first ? s[r] : gl[f0 + r] + s[r];
    }
  }
};

// slab[W_l] (+)= G^T H and slab[b_l] (+)= column sums of G; G, H: [16][LD] in LDS, rows >= nvalid read as exact zeros
__device__ __forceinline__ void pm_mlp_accum_dw(const float* G, const float* H, int ld, int n_out, int n_in, float* dW,
                                                float* db, bool first, int nvalid, int wid, int lane, int tid) {
  const int c = lane & 15, g = lane >> 4;
  const int n_ot = (n_out + 15) >> 4, n_it = (n_in + 15) >> 4;
  for (int t = wid; t < n_ot * n_it; t += PM_NW) {
    const int ot = t / n_it, it = t - ot * n_it;
    const int o0 = ot * 16 + 4 * g, i = it * 16 + c;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!first && i < n_in) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (o0 + r < n_out) acc[r] = dW[(size_t)(o0 + r) * n_in + i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 4 * j + g;                       // K index g of issue j
      const bool v = row < nvalid;
      const float a = v ? G[row * ld + ot * 16 + c] : 0.f;
      const float b = v ? H[row * ld + it * 16 + c] : 0.f;
      acc = mfma4(a, b, acc);                          // D[i = out feature 4 g + r][j = in feature c]
    }
    if (i < n_in) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (o0 + r < n_out) dW[(size_t)(o0 + r) * n_in + i] = acc[r];
    }
  }
  for (int o = tid; o < n_out; o += PM_NT) {
    float s = first ? 0.f : db[o];
    for (int r = 0; r < nvalid; ++r) s += G[r * ld + o];
    db[o] = s;
  }
}

struct MlpBwdCArgs {
  MlpBwdPArgs p;
  MlpConcArgs c;
};
struct MlpBwdLArgs {               // a layer-norm call: c is all zeros where no layer is concrete
  MlpBwdPArgs p;
  MlpConcArgs c;
  MlpLnArgs ln;
};
template <bool CONC, bool LN> struct MlpBwdPSel { typedef MlpBwdPArgs type; };
template <> struct MlpBwdPSel<true, false> { typedef MlpBwdCArgs type; };
template <bool CONC> struct MlpBwdPSel<CONC, true> { typedef MlpBwdLArgs type; };
__device__ __forceinline__ const MlpBwdPArgs& pm_bwdp_of(const MlpBwdPArgs& a) { return a; }
__device__ __forceinline__ const MlpBwdPArgs& pm_bwdp_of(const MlpBwdCArgs& a) { return a.p; }
__device__ __forceinline__ const MlpBwdPArgs& pm_bwdp_of(const MlpBwdLArgs& a) { return a.p; }
__device__ __forceinline__ const MlpConcArgs* pm_conc_of(const MlpBwdPArgs&) { return nullptr; }
__device__ __forceinline__ const MlpConcArgs* pm_conc_of(const MlpBwdCArgs& a) { return &a.c; }
__device__ __forceinline__ const MlpConcArgs* pm_conc_of(const MlpBwdLArgs& a) { return &a.c; }
__device__ __forceinline__ const MlpLnArgs* pm_ln_of(const MlpBwdPArgs&) { return nullptr; }
__device__ __forceinline__ const MlpLnArgs* pm_ln_of(const MlpBwdCArgs&) { return nullptr; }
__device__ __forceinline__ const MlpLnArgs* pm_ln_of(const MlpBwdLArgs& a) { return &a.ln; }

// CONC: some hidden layers are train-mode concrete dropout (MlpBwdCArgs); LN: some are layer-normalised (MlpBwdLArgs;
// z_idx counts on from the Q buffers).  <false, false> is pmbrl_mlp_backward's kernel as it always was, <true, false>
// pmbrl_mlp_backward_concrete's.
template <bool CONC, bool LN>
__global__ __launch_bounds__(PM_NT, 1) void pm_mlp_bwdp_kernel(const typename MlpBwdPSel<CONC, LN>::type PP) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = 16;
  const MlpBwdPArgs& P = pm_bwdp_of(PP);
  const MlpConcArgs* Cc = pm_conc_of(PP);
  const MlpLnArgs* Ln = pm_ln_of(PP);
  const MlpBwdArgs& B = P.b;
  const MlpArgs& A = B.f;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int LD = A.LD, nl = A.nl;
  float* H = smem;                                   // [nl][16][LD]
  float* G0 = H + (size_t)nl * R * LD;
  float* G1 = G0 + (size_t)R * LD;
  float* part = G1 + (size_t)R * LD;
  const bool smooth = A.act != PMBRL_ACT_RELU;
  float* D = part + (size_t)PM_NW * PM_KS_NT * 256;  // (smooth only) [nl - 1][16][LD]: act' of hidden layer l
  float* slab = P.slab ? P.slab + (size_t)blockIdx.x * P.n_params : nullptr;
  float* Q = nullptr;                                // (CONC) [concrete layers][16][LD]
  float* lslab = nullptr;
  if constexpr (CONC) {
    Q = D + (smooth ? (size_t)(nl - 1) * R * LD : 0);
    lslab = Cc->slab + (size_t)blockIdx.x * Cc->n_logit;
  }
  float* Z = nullptr;                                // (LN) [Q buffers, then layer-norm layers][16][LD]
  float* nslab = nullptr;
  if constexpr (LN) {
    Z = D + (smooth ? (size_t)(nl - 1) * R * LD : 0);
    if (Ln->slab) nslab = Ln->slab + (size_t)blockIdx.x * Ln->n_ln;
  }
  const int K0 = A.dim[0];
  const int n_tiles = (A.B + R - 1) / R;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int row0 = tile * R;
    const int nvalid = min(R, A.B - row0);
    const bool first = tile == (int)blockIdx.x;
    pm_mlp_load_rows(A, H, row0, nvalid, tid);
    __syncthreads();
    for (int l = 0; l < nl - 1; ++l) {
      bool conc = false;
      if constexpr (CONC) conc = Cc->u[l] != nullptr;
      if constexpr (LN) {
        if (Ln->gamma[l]) {
          float* Hn = H + (size_t)(l + 1) * R * LD;
          EpiMlpLnPre e{A.bias[l], Hn, LD, nvalid, lane, A.dim[l + 1]};
          gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], H + (size_t)l * R * LD, LD, wid, lane, e);
          __syncthreads();
          MlpLnRows p{Ln->gamma[l], Ln->beta[l], Ln->eps[l], A.mask[l], A.keep[l], pm_act_code(A.act, l), A.dim[l + 1],
                      A.nt[l + 1], Hn, smooth ? D + (size_t)l * R * LD : nullptr, Z + (size_t)Ln->z_idx[l] * R * LD, nullptr,
                      nullptr, 1.f, nullptr};
          if constexpr (CONC) {
            if (conc) {
              p.u = Cc->u[l];
              p.logit = Cc->logit[l];
              p.temp = Cc->temp[l];
              p.Q = Q + (size_t)Cc->q_idx[l] * R * LD;
            }
          }
          pm_mlp_ln_rows(p, LD, row0, nvalid, wid, lane);
          __syncthreads();
          continue;
        }
      }
      if (smooth) {
        EpiMlpAct e{A.bias[l], A.mask[l], A.keep[l], H + (size_t)(l + 1) * R * LD, D + (size_t)l * R * LD, LD, row0,
                    nvalid, A.nt[l + 1], lane, pm_act_code(A.act, l), A.dim[l + 1]};
        if (conc) {
          EpiMlpConcFwd<EpiMlpAct> ec{e, A.bias[l], Cc->u[l], Cc->logit[l], Cc->temp[l], Q + (size_t)Cc->q_idx[l] * R * LD,
                                      LD, row0, nvalid, lane, pm_act_code(A.act, l), A.dim[l + 1], true};
          gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], H + (size_t)l * R * LD, LD, wid, lane, ec);
        } else {
          gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], H + (size_t)l * R * LD, LD, wid, lane, e);
        }
      } else {
        EpiMlpHidden e{A.bias[l], A.mask[l], A.keep[l], H + (size_t)(l + 1) * R * LD, LD, row0, nvalid, A.nt[l + 1], lane};
        if (conc) {
          EpiMlpConcFwd<EpiMlpHidden> ec{e, A.bias[l], Cc->u[l], Cc->logit[l], Cc->temp[l],
                                         Q + (size_t)Cc->q_idx[l] * R * LD, LD, row0, nvalid, lane, PMBRL_ACT_RELU,
                                         A.dim[l + 1], false};
          gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], H + (size_t)l * R * LD, LD, wid, lane, ec);
        } else {
          gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], H + (size_t)l * R * LD, LD, wid, lane, e);
        }
      }
      __syncthreads();
    }
    gemm_narrow<1>(A.wf[nl - 1], A.nt[nl], A.nt[nl - 1], A.bias[nl - 1], H + (size_t)(nl - 1) * R * LD, G1, LD, part,
                   wid, lane, tid);
    pm_mlp_head_grad(B, G1, G0, row0, nvalid, tid);
    __syncthreads();
    float* Gin = G0;
    float* Gout = G1;
    for (int l = nl - 1; l >= 0; --l) {
      // Gin = G_l, the gradient at Linear l's output
      if (slab)
        pm_mlp_accum_dw(Gin, H + (size_t)l * R * LD, LD, A.dim[l + 1], A.dim[l], slab + P.w_off[l], slab + P.b_off[l], first,
                        nvalid, wid, lane, tid);
      if (l == 0) break;
      bool conc = false;                               // is hidden layer l - 1, whose gh this GEMM forms, concrete?
      if constexpr (CONC) conc = Cc->u[l - 1] != nullptr;
      if (smooth) {
        EpiMlpBwdAct e{D + (size_t)(l - 1) * R * LD, Gout, LD, lane};
        if (conc) {
          EpiMlpConcBwd<EpiMlpBwdAct> ec{e, Q + (size_t)Cc->q_idx[l - 1] * R * LD, lslab + Cc->g_off[l - 1], first, LD,
                                         lane, A.dim[l]};
          gemm_tiles<1>(B.wb[l], A.nt[l], A.nt[l + 1], Gin, LD, wid, lane, ec);
        } else {
          gemm_tiles<1>(B.wb[l], A.nt[l], A.nt[l + 1], Gin, LD, wid, lane, e);
        }
      } else {
        EpiMlpBwd e{H + (size_t)l * R * LD, 1.f / A.keep[l - 1], Gout, LD, lane};
        if (conc) {
          EpiMlpConcBwd<EpiMlpBwd> ec{e, Q + (size_t)Cc->q_idx[l - 1] * R * LD, lslab + Cc->g_off[l - 1], first, LD, lane,
                                      A.dim[l]};
          gemm_tiles<1>(B.wb[l], A.nt[l], A.nt[l + 1], Gin, LD, wid, lane, ec);
        } else {
          gemm_tiles<1>(B.wb[l], A.nt[l], A.nt[l + 1], Gin, LD, wid, lane, e);
        }
      }
      __syncthreads();
      if constexpr (LN) {
        if (Ln->gamma[l - 1]) {                        // Gout = g_y of hidden layer l - 1: d gamma, d beta, then -> g_v
          const float* Zl = Z + (size_t)Ln->z_idx[l - 1] * R * LD;
          if (nslab) {
            pm_mlp_ln_accum(Gout, Zl, LD, A.dim[l], nslab + Ln->g_off[l - 1], first, nvalid, tid);
            __syncthreads();
          }
          pm_mlp_ln_bwd_rows(Gout, Zl, Ln->gamma[l - 1], A.dim[l], LD, wid, lane);
          __syncthreads();
        }
      }
      float* t = Gin; Gin = Gout; Gout = t;
    }
    if (B.grad_x) {
      // first layer: d / d x_in, then the input normalisation
      EpiPlain e{nullptr, Gout, LD, lane};
      gemm_tiles<1>(B.wb[0], A.nt[0], A.nt[1], Gin, LD, wid, lane, e);
      __syncthreads();
      for (int i = tid; i < nvalid * K0; i += PM_NT) {
        const int r = i / K0, k = i - r * K0;
        float v = Gout[r * LD + k];
        if (A.in_iscale) v *= A.in_iscale[k];
        B.grad_x[(size_t)(row0 + r) * K0 + k] = v;
      }
    }
    __syncthreads();                                 // the next tile overwrites H and the gradient buffers
  }
}


// the launches of the layer-norm instances (pmbrl_mlp_ln.hip, the one object that compiles them); 0 or a pmbrl error code
int pm_mlp_ln_launch_fwd(hipStream_t s, int n_blocks, size_t lds, const MlpLnFwdArgs& a);
int pm_mlp_ln_launch_bwdx(hipStream_t s, int n_blocks, size_t lds, const MlpLnBwdArgs& a);
int pm_mlp_ln_launch_bwdp(hipStream_t s, int n_blocks, size_t lds, const MlpBwdLArgs& a, bool conc);
