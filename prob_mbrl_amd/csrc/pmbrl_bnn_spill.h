// The spill form of the BNN training step (pmbrl_bnn.h has the resident one): networks whose layers do not all fit in LDS
// at once.  As there, a workgroup (PM_NW waves) owns 16 minibatch rows and runs forward, loss and backward in one launch,
// with the same GEMM routines, the same epilogues (pmbrl_bnn_parts.h) and loss sections (pmbrl_bnn_loss.h) in the same order -- so
// the same bits.  What differs is where a layer's values wait for the backward pass: LDS holds three [16][LD] buffers
// (pm_bnn_spill_lds_floats), the forward pass ping-pongs between two of them, and what EpiBnnBwd reads of hidden layer l
// -- its output or act' x mask, and q -- goes to the workgroup's own blocks of BnnSpillArgs::hq in HBM, written by
// EpiBnnFwd through the pointers that are LDS buffers in the resident form.  The dW stashes actT / gT are written as
// there, so everything behind the kernel (the dW block kernel, pm_bnn_finish, pm_bnn_tail) serves both forms.
#pragma once
#include "pmbrl_bnn_parts.h"

template <bool ACT = false, bool BERN = false>
__global__ __launch_bounds__(PM_NT, 1) void pm_bnn_fwd_bwd_spill(const BnnSpillArgs A) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wg = blockIdx.x;
  const int row0 = wg * R;
  const int nvalid = min(R, A.M - row0);
  const int LD = A.LD, nl = A.nl;
  auto buf = [&](int i) { return smem + (size_t)i * R * LD; };      // the three buffers
  float* part = smem + (size_t)3 * R * LD;
  float* red = part + (size_t)PM_NW * PM_KS_NT * 256;
  // this workgroup's blocks of hidden layer l: out / act' x mask, then q
  float* hq = A.hq + (size_t)wg * (nl - 1) * 2 * R * LD;
  auto hblk = [&](int l) { return hq + (size_t)(2 * l) * R * LD; };
  auto qblk = [&](int l) { return hq + (size_t)(2 * l + 1) * R * LD; };
#define BNN_SPILL_STAMP(i) do { if (A.prof && wg == 0 && tid == 0) A.prof[i] = (long long)__builtin_readcyclecounter(); } while (0)
  BNN_SPILL_STAMP(0);

  // ---- gather the minibatch rows (+ dW stash of the first layer's input)
  {
    const int K16 = A.nt[0] * 16;
    float* st = A.actT[0] + (size_t)wg * K16 * 16;
    float* H0 = buf(0);
    for (int i = tid; i < R * K16; i += PM_NT) {
      const int k = i / R, r = i - k * R;
      float v = 0.f;
      if (r < nvalid && k < A.n_in) v = A.X[(size_t)A.idx[row0 + r] * A.n_in + k];
      H0[r * LD + k] = v;
      st[(size_t)k * 16 + r] = v;
    }
  }
  __syncthreads();
  BNN_SPILL_STAMP(1);
  // ---- forward: layer l from buffer l & 1 into the other; q and (ACT) act' x mask straight to the workgroup's blocks
  for (int l = 0; l < nl - 1; ++l) {
    float* out = buf((l + 1) & 1);
    EpiBnnFwd<ACT, BERN> e{pm_act_code(A.act, l), ACT ? hblk(l) : nullptr, A.bias[l], A.logit_p[l], BERN ? A.keep[l] : nullptr, A.u[l], A.bvar[l], A.inv_temp[l],
                out, qblk(l),
                A.actT[l + 1] + (size_t)wg * A.nt[l + 1] * 16 * 16, LD, row0, nvalid, A.dim[l + 1], lane,
                A.rng, A.rng_k0, A.rng_k1, A.rng_step, (unsigned)l};
    gemm_tiles<1>(A.wf[l], A.nt[l + 1], A.nt[l], buf(l & 1), LD, wid, lane, e);
    __syncthreads();
    if constexpr (!ACT) {
      // the ReLU instances' backward pass reads the layer's output itself: the tiles the epilogue wrote, 16 bytes a lane
      // (nothing writes `out` before the barrier behind the next layer)
      const int q4 = A.nt[l + 1] * 4;
      float* hb = hblk(l);
      for (int i = tid; i < R * q4; i += PM_NT) {
        const int r = i / q4, c = (i - r * q4) * 4;
        *reinterpret_cast<f32x4*>(hb + r * LD + c) = *reinterpret_cast<const f32x4*>(out + r * LD + c);
      }
    }
    BNN_SPILL_STAMP(2 + l);
  }
  float* Gin = buf(nl & 1);             // the head's gradient: where the input of the last hidden layer was
  float* Gout = buf(2);                 // the head's outputs, then the gradient pong
  float* GQ = buf((nl - 1) & 1);        // the head's input, then the dropout-logit terms
  gemm_narrow<1>(A.wf[nl - 1], A.nt[nl], A.nt[nl - 1], A.bias[nl - 1], GQ, Gout, LD, part, wid, lane, tid);
  BNN_SPILL_STAMP(10);
  // ---- the likelihood (mixture, Gaussian or squared error) and its gradient wrt the head outputs: G1 -> G0
  {
    const float* G1 = Gout;
    float* G0 = Gin;
#include "pmbrl_bnn_loss.h"
  }
  __syncthreads();
  BNN_SPILL_STAMP(11);
  // ---- backward: dX chain, dropout-logit terms, G stash; h / d and q of a layer from the workgroup's blocks
  for (int l = nl - 1; l >= 1; --l) {
    EpiBnnBwd<ACT, BERN> e{hblk(l - 1), qblk(l - 1), BERN ? A.keep[l - 1] : nullptr, Gout, GQ,
                A.gT[l - 1] + (size_t)wg * A.nt[l] * 16 * 16, LD, lane};
    gemm_tiles<1>(A.wb[l], A.nt[l], A.nt[l + 1], Gin, LD, wid, lane, e);
    __syncthreads();
    if (A.logit_p[l - 1]) {
      float* pl = A.part_lp + (size_t)wg * A.sum_h + A.lp_off[l - 1];
      for (int f = tid; f < A.dim[l]; f += PM_NT) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) s += GQ[r * LD + f];
        pl[f] = s;
      }
    }
    __syncthreads();
    BNN_SPILL_STAMP(12 + (nl - 1 - l));
    float* t = Gin; Gin = Gout; Gout = t;
  }
  BNN_SPILL_STAMP(20);
#undef BNN_SPILL_STAMP
}
