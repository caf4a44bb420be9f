// What both kernel forms of the BNN training step are made of (pmbrl_bnn.h: pm_bnn_fwd_bwd, every layer resident in LDS;
// pmbrl_bnn_spill.h: pm_bnn_fwd_bwd_spill, one layer's working set in LDS): the argument record, the epilogues of the forward
// and the backward GEMMs and the LDS maps; the loss sections are pmbrl_bnn_loss.h, text both bodies include.  One
// definition each, so that the two forms cannot drift apart: at a shape both accept they give the same bits.
#pragma once

#include "pmbrl_dev.h"

struct BnnArgs {
  int M, nl, LD, n_out, nwg, n_in, sum_h;
  int dim[PM_MAXL + 1], nt[PM_MAXL + 1];
  const float* wf[PM_MAXL];
  const float* wb[PM_MAXL];
  const float* bias[PM_MAXL];
  const float* logit_p[PM_MAXL];   // hidden layer l: [dim[l+1]] or nullptr (no dropout)
  const float* u[PM_MAXL];         // [M][dim[l+1]] uniform noise of the concrete relaxation
  const float* bvar[PM_MAXL];      // [M][dim[l+1]] uniform variate of the Bernoulli draw (hard = bvar < probs)
  float inv_temp[PM_MAXL];
  int lp_off[PM_MAXL];             // offset of layer l's logits in the concatenated logit vector
  const float *X, *Y;              // normalised dataset [N][n_in], [N][n_out]
  const int* idx;                  // [M] minibatch rows
  float mls, inv_M;
  int mse;                         // loss: mean squared error of the mean head instead of the Gaussian NLL
  int gmm_n;                       // > 1: mixture-of-Gaussians NLL, head = [n D means | n D log-stds | n logits | log-T]
  const float* row_w;              // [M] per-row weight of the log-likelihood (importance sampling) or nullptr
  float* row_lp;                   // [M] out: per-row log-likelihood (unweighted) or nullptr
  float* actT[PM_MAXL];            // stash: input of layer l   [wg][nt[l]*16][16]
  float* gT[PM_MAXL];              // stash: grad wrt pre-activation of layer l [wg][nt[l+1]*16][16]
  float* part_lp;                  // [nwg][sum_h]
  float* part_loss;                // [nwg]
  // u / bvar drawn inside the kernel (pmbrl_bnn_train_steps without recorded draws): Philox keyed by the caller's seed,
  // counter = (minibatch row, feature quad, hidden layer | stream << 8, step)
  int rng;
  unsigned rng_k0, rng_k1, rng_step;
  long long* prof;                 // debugging: cycle stamps of workgroup 0 (nullptr: none)
  int act;                         // PMBRL_ACT_* per hidden layer, pm_act_code (pm_bnn_fwd_bwd<true> when not 0 = all ReLU)
  // fixed-rate Bernoulli dropout behind hidden layer l (pm_bnn_fwd_bwd<., true>): the units' keep probabilities
  // [nt[l+1] * 16] (a scalar rate is stored once per unit), nullptr for a layer of another kind.  m = bvar < p_j.
  const float* keep[PM_MAXL];
};

// 1 / x to an ulp or two: v_rcp_f32 and one Newton step
__device__ __forceinline__ float pm_fast_rcp(float d) {
  const float r = __builtin_amdgcn_rcpf(d);
  return __builtin_fmaf(__builtin_fmaf(-d, r, 1.f), r, r);
}

// hidden layer forward: out = relu(acc + b) * hard ;  q = relu(.) * d mask / d logit_p
// ACT: out = act(acc + b) * hard, q = act(.) * d mask / d logit_p, and d_out = act'(acc + b) * hard for the backward pass
// (pm_act; act = this layer's PMBRL_ACT_* code).  The ReLU instance is what it was.  Padded units and rows past nvalid
// are forced to 0 in out, q and d_out after the activation, whatever act(0) is (PMBRL_ACT_EXP: 1).
// BERN (plans with a Bernoulli layer; keep != nullptr marks one): m = bvar < p_j, out = act(acc + b) * m / p_j -- divided as
// BDropout.forward divides, per unit -- q = 0 (there is no logit), d_out = act'(acc + b) * m / p_j.
template <bool ACT = false, bool BERN = false>
struct EpiBnnFwd {
  int act;
  float* d_out;
  const float* bias;
  const float* logit_p;
  const float* keep;
  const float *u, *bvar;
  float inv_temp;
  float *h_out, *q_out, *stash;
  int ld, row0, nvalid, width, lane;
  int rng;                       // 1: u / bvar from the generator (rk0, rk1, rstep; rlayer = this hidden layer)
  unsigned rk0, rk1, rstep, rlayer;
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) {
    const int g = lane >> 4, lrow = lane & 15;
    const int f0 = ot * 16 + 4 * g;
    const f32x4 b = ldg4(bias + f0);
    f32x4 h, q, dd;
    unsigned ru[4] = {0u, 0u, 0u, 0u}, rv[4] = {0u, 0u, 0u, 0u};
    if (rng && logit_p) {      // 24-bit uniforms in [0, 1), what torch.rand gives a float tensor
      pm_philox((unsigned)(row0 + lrow), (unsigned)(f0 >> 2), rlayer, rstep, rk0, rk1, ru);
      pm_philox((unsigned)(row0 + lrow), (unsigned)(f0 >> 2), rlayer | 0x100u, rstep, rk0, rk1, rv);
    }
    f32x4 kp = {1.f, 1.f, 1.f, 1.f};
    if constexpr (BERN) {
      if (keep) {
        kp = ldg4(keep + f0);
        if (rng) pm_philox((unsigned)(row0 + lrow), (unsigned)(f0 >> 2), rlayer | 0x100u, rstep, rk0, rk1, rv);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = f0 + r;
      float v, dv = 0.f;
      if constexpr (ACT) pm_act(act, acc[r] + b[r], f, width, v, dv);
      else v = fmaxf(acc[r] + b[r], 0.f);
      float hv = v, qv = 0.f;
      if (logit_p && f < width && lrow < nvalid) {
        const size_t o = (size_t)(row0 + lrow) * width + f;
        const float uu = rng ? (float)(ru[r] >> 8) * (1.0f / 16777216.0f) : u[o];
        // the logistic noise and the keep probability on the hardware's log2 / exp2 / reciprocal (1 ulp each, what the
        // library routines wrap in range handling this argument range does not need: u in [0, 1), the exponent clamped
        // so that the reciprocal never sees an infinity): 12.2 k -> 9.3 k cycles for the 5 -> 200 layer's 13 tile
        // epilogues, 19.6 k -> 17.9 k for the 200 -> 200 layer's -- the epilogues are instruction issue, four tiles a SIMD.
        // (Staging bias and logits in LDS at the head of the kernel, so that the epilogues load nothing from memory, was
        //  measured with it: the staging cost what the epilogues gained; not kept.)
        const float cp = logit_p[f] + 0.6931471805599453f * (__builtin_amdgcn_logf(uu + 1e-7f) - __builtin_amdgcn_logf(1.f - (uu - 1e-7f)));
        const float pr = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fminf(-1.4426950408889634f * (cp * inv_temp), 80.f)));
        const bool hard = (rng ? (float)(rv[r] >> 8) * (1.0f / 16777216.0f) : bvar[o]) < pr;
        hv = hard ? v : 0.f;
        qv = v * pr * (1.f - pr) * inv_temp;
        if (!hard) dv = 0.f;
      }
      if constexpr (BERN) {
        if (keep && f < width && lrow < nvalid) {
          const size_t o = (size_t)(row0 + lrow) * width + f;
          const bool hard = (rng ? (float)(rv[r] >> 8) * (1.0f / 16777216.0f) : bvar[o]) < kp[r];
          hv = hard ? v / kp[r] : 0.f;
          dv = hard ? dv / kp[r] : 0.f;
        }
      }
      if (f >= width || lrow >= nvalid) { hv = 0.f; qv = 0.f; dv = 0.f; }
      h[r] = hv;
      q[r] = qv;
      dd[r] = dv;
    }
    *reinterpret_cast<f32x4*>(h_out + lrow * ld + f0) = h;
    *reinterpret_cast<f32x4*>(q_out + lrow * ld + f0) = q;
    if constexpr (ACT) *reinterpret_cast<f32x4*>(d_out + lrow * ld + f0) = dd;
#pragma unroll
    for (int r = 0; r < 4; ++r) stash[(size_t)(f0 + r) * 16 + lrow] = h[r];
  }
};

// backward through hidden layer l-1's output: acc = dL/d out ; gq = acc * q (dropout-logit term),
// g_pre = out > 0 ? acc : 0
// (ACT: g_pre = acc * d, h_in = the d_out of EpiBnnFwd<true>)
// BERN, behind a Bernoulli layer (keep != nullptr): out = relu(.) m / p_j, so g_pre = out > 0 ? acc / p_j : 0 (the ACT
// instances carry m / p_j in d already)
template <bool ACT = false, bool BERN = false>
struct EpiBnnBwd {
  const float *h_in, *q_in;   // out and q of that layer
  const float* keep;
  float *g_out, *gq_out, *stash;
  int ld, lane;
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) {
    const int g = lane >> 4, lrow = lane & 15;
    const int f0 = ot * 16 + 4 * g;
    const f32x4 h = *reinterpret_cast<const f32x4*>(h_in + lrow * ld + f0);
    const f32x4 q = *reinterpret_cast<const f32x4*>(q_in + lrow * ld + f0);
    f32x4 gp, gq;
    f32x4 kp = {1.f, 1.f, 1.f, 1.f};
    if constexpr (BERN && !ACT) {
      if (keep) kp = ldg4(keep + f0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (ACT) gp[r] = h[r] != 0.f ? acc[r] * h[r] : 0.f;
      else if constexpr (BERN) gp[r] = h[r] > 0.f ? (keep ? acc[r] / kp[r] : acc[r]) : 0.f;
      else gp[r] = h[r] > 0.f ? acc[r] : 0.f;
      gq[r] = acc[r] * q[r];
    }
    *reinterpret_cast<f32x4*>(g_out + lrow * ld + f0) = gp;
    *reinterpret_cast<f32x4*>(gq_out + lrow * ld + f0) = gq;
#pragma unroll
    for (int r = 0; r < 4; ++r) stash[(size_t)(f0 + r) * 16 + lrow] = gp[r];
  }
};

// (A GEMM variant that requests ALL of a wave's weight fragments of a layer at once was measured: pm_bnn_fwd_bwd 27.7 ->
//  34.3 us -- the first MFMA then waits for 32 loads where gemm_tiles starts on four; the layer chain is not what bounds it.)
__host__ __device__ inline size_t pm_bnn_lds_floats(int nl, int LD, int act = 0) {
  // H[0..nl-1], Q[0..nl-2], two gradient buffers, one gq buffer, K-split scratch, loss scratch; an activation other than
  // ReLU: one more buffer, the first hidden layer's derivatives (those of hidden layer l >= 1 go where the input of
  // Linear l - 1 was: the dW stash has it, and the backward pass of these instances does not read H)
  return ((size_t)nl + (nl - 1) + 3 + (act ? 1 : 0)) * 16 * LD + (size_t)PM_NW * PM_KS_NT * 256 + PM_NT;
}

// The spill form's map: three [16][LD] buffers, whatever the depth, the activations and the dropout kinds.  Forward: layer l
// reads buffer l & 1 and writes the other; the head reads the last of them and writes buffer 2; the loss sections read
// buffer 2 and write the head's gradient where the input of the last hidden layer was.  Backward: that buffer and buffer 2
// are the gradient ping-pong, the buffer the head read is GQ.  Behind them the K-split scratch and the loss scratch.
__host__ __device__ inline size_t pm_bnn_spill_lds_floats(int LD) {
  return (size_t)3 * 16 * LD + (size_t)PM_NW * PM_KS_NT * 256 + PM_NT;
}
// ... and what the loss sections declare on top of either map (the mixture's responsibilities: 2 x [16][PMBRL_MAX_COMP] +
// 2 x [16] floats; the Gaussian's row sums), rounded up: the spill form's plan counts it against the 160 KB
#define PM_BNN_LDS_STATIC 2048
// What the backward pass needs of hidden layer l beside the dW stashes, per workgroup, in HBM: two [16][LD] blocks, row-major
// with the LDS buffers' own leading dimension -- the epilogues address them as they address LDS, 16 bytes a lane.
// Block 0: the layer's output (ReLU instances) or act' x mask (ACT instances), block 1: q.
struct BnnSpillArgs : BnnArgs {
  float* hq;                       // [nwg][nl - 1][2][16][LD]
};
__host__ __device__ inline size_t pm_bnn_spill_stash_floats(int nwg, int nl, int LD) {
  return (size_t)nwg * (nl - 1) * 2 * 16 * LD;
}
// the spill form's instances and their launcher are pmbrl_bnn_spill.hip's
// (the instance's dynamic LDS limit, raised once to the most any spill plan asks for: plans of several sizes share an instance)
hipError_t pm_bnn_spill_prepare(int act, int bern);
void pm_bnn_spill_launch(const BnnSpillArgs& A, int act, int bern, size_t lds_bytes, hipStream_t s);
