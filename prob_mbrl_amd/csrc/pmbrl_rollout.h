// Fused H-step rollout kernels: one workgroup owns `rows_per_wg` particle rows
// for ALL time steps (rows are independent except inside a moment-matching
// group, and a workgroup always owns whole groups), so the whole rollout is ONE
// launch with no grid-wide synchronisation.  The particle state never leaves
// LDS between steps; HBM sees only the trajectory outputs and the stashes the
// backward sweep / dW GEMM consume.
#pragma once
#include "pmbrl_dev.h"
#include "pmbrl_mm.h"
#include "pmbrl_gsplit.h"
#include "pmbrl_wide.h"

// ---------------------------------------------------------------------------
// epilogues
// ---------------------------------------------------------------------------
// hidden layer, forward:  h = relu(acc + b) * mask / keep     (models/modules.py:46-61,120-160)
// NP = 0: fp32 rows out (leading dimension ld floats); NP = 2: two piece planes (pmbrl_gsplit.h; ld in 16-bit
// elements, R rows per plane; F16: fp16 pieces with range check into *ovf)
template <int NP = 0, bool F16 = false, int R = 0>
struct EpiHiddenFwdT {
  const float* bias;
  const uint16_t* mask;   // [B][nt]
  uint16_t* abits;        // [B][nt] slice of step t
  float keep;
  float* lds_out;
  float* stash;           // feature-major block [nt*16][Rw] or nullptr
  int ld, Rw, row0, nvalid, nt, lane;
  int* ovf;
  // the epilogue's operands from HBM / L2 (bias, dropout bits): fetched by the split-operand GEMMs when a tile
  // group STARTS, so that the round trip hides behind the group's MFMAs
  struct Pre {
    f32x4 b;
    unsigned mw;
  };
  __device__ __forceinline__ Pre pre(int ot, int rt) const {
    const int g = lane >> 4;
    const int lrow = rt * 16 + (lane & 15);
    Pre p;
    p.b = ldg4(bias + ot * 16 + 4 * g);
    p.mw = 0;
    if (lrow < nvalid) p.mw = mask[(size_t)(row0 + lrow) * nt + ot];
    return p;
  }
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) { (*this)(ot, rt, acc, pre(ot, rt)); }
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc, const Pre& pr) {
    const int g = lane >> 4;
    const int lrow = rt * 16 + (lane & 15);
    const int f0 = ot * 16 + 4 * g;
    const f32x4 b = pr.b;
    const bool valid = lrow < nvalid;
    const unsigned nib = (pr.mw >> (4 * g)) & 0xFu;
    f32x4 h;
    unsigned act = 0;
    // (fp32 form: the reference's division, x / p; split form: a multiply -- the product is not bit-exact anyway
    //  and four IEEE divisions are a third of this epilogue's instructions)
    const float ik = NP > 0 ? 1.f / keep : 1.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = acc[r] + b[r];
      const bool a = ((nib >> r) & 1u) && (v > 0.f);
      if constexpr (NP > 0) h[r] = a ? v * ik : 0.f;
      else h[r] = a ? (keep == 1.f ? v : v / keep) : 0.f;
      act |= (a ? 1u : 0u) << r;
    }
    if constexpr (NP > 0) {
      pm_store_planes<NP, R, F16>(lds_out, (unsigned)ld, (unsigned)lrow, (unsigned)f0, h);
      // the K padding up to the next K32 block (the buffer held fp32 rows / partial tiles before: any bits)
      if (ot == nt - 1 && (nt & 1))
        pm_store_planes<NP, R, F16>(lds_out, (unsigned)ld, (unsigned)lrow, (unsigned)f0 + 16u, f32x4{0.f, 0.f, 0.f, 0.f});
      if constexpr (F16) {
        // an activation out of fp16's range (h >= 0 here); a WEIGHT out of range -- it would pack to inf, inf x 0 is
        // NaN, and a NaN pre-activation vanishes in the ReLU -- is caught when the weights are packed (A.wflag)
        if (fmaxf(fmaxf(h[0], h[1]), fmaxf(h[2], h[3])) > 65504.f) *ovf = 1;
      }
    } else {
      *reinterpret_cast<f32x4*>(lds_out + lrow * ld + f0) = h;
    }
#ifndef PM_EXP_GS_NOSTASH
    if (stash) {
#pragma unroll
      for (int r = 0; r < 4; ++r) __builtin_nontemporal_store(h[r], stash + (size_t)(f0 + r) * Rw + lrow);   // write-once stream: keep the weights in L2
    }
#endif
#ifndef PM_EXP_GS_NOABITS
    unsigned w16 = act << (4 * g);
    w16 |= __shfl_xor(w16, 16);
    w16 |= __shfl_xor(w16, 32);
    if (g == 0 && valid) abits[(size_t)(row0 + lrow) * nt + ot] = (uint16_t)w16;
#endif
  }
};

// hidden layer, backward: g_pre = active ? acc / keep : 0
template <int NP = 0, int R = 0>
struct EpiHiddenBwdT {
  const uint16_t* abits;  // [B][nt] slice of step t
  float keep;
  float* lds_out;
  float* stash;           // gT block or nullptr
  int ld, Rw, row0, nvalid, nt, lane;
  struct Pre {
    unsigned mw;
  };
  __device__ __forceinline__ Pre pre(int ot, int rt) const {
    const int lrow = rt * 16 + (lane & 15);
    Pre p;
    p.mw = 0;
    if (lrow < nvalid) p.mw = abits[(size_t)(row0 + lrow) * nt + ot];
    return p;
  }
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) { (*this)(ot, rt, acc, pre(ot, rt)); }
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc, const Pre& pr) {
    const int g = lane >> 4;
    const int lrow = rt * 16 + (lane & 15);
    const int f0 = ot * 16 + 4 * g;
    const unsigned nib = (pr.mw >> (4 * g)) & 0xFu;
    f32x4 h;
    const float ik = NP > 0 ? 1.f / keep : 1.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (NP > 0) h[r] = ((nib >> r) & 1u) ? acc[r] * ik : 0.f;
      else h[r] = ((nib >> r) & 1u) ? (keep == 1.f ? acc[r] : acc[r] / keep) : 0.f;
    }
    if constexpr (NP > 0) {
      pm_store_planes<NP, R, false>(lds_out, (unsigned)ld, (unsigned)lrow, (unsigned)f0, h);
      if (ot == nt - 1 && (nt & 1))
        pm_store_planes<NP, R, false>(lds_out, (unsigned)ld, (unsigned)lrow, (unsigned)f0 + 16u, f32x4{0.f, 0.f, 0.f, 0.f});
    } else {
      *reinterpret_cast<f32x4*>(lds_out + lrow * ld + f0) = h;
    }
    if (stash) {
#pragma unroll
      for (int r = 0; r < 4; ++r) __builtin_nontemporal_store(h[r], stash + (size_t)(f0 + r) * Rw + lrow);   // write-once stream: keep the weights in L2
    }
  }
};

// Hidden layers of a plan with a network that is not ReLU (pmbrl_mlp::act; the kernels' ACT instances).  Forward:
//   h = act(acc + b) * mask / keep,   dact = act'(acc + b) * mask / keep
// dact ([B][nt * 16] floats of step t, in the workspace region the activity bits of a ReLU plan have) is all the adjoint
// needs of the layer: g_pre = acc * dact.  tanh' could be had from the stashed h, SiLU's cannot (it is not monotone),
// and the dynamics layers have no stash of h at all: one form for every activation, a ReLU layer or network of a mixed
// plan included (dact = mask / keep where the pre-activation is positive; PMBRL_ACT_NONE: dact = mask / keep).  `act` is
// THIS layer's code (pm_act_code of RolloutArgs::pol_acts / dyn_acts).  Padded units (width .. nt * 16), rows past
// nvalid (their mask word is read as 0) and masked units get h = 0 and dact = 0 whatever act(0) and act'(0) are --
// PMBRL_ACT_EXP has act(0) = 1 -- so the LDS operand of the next layer, the stash the dW GEMM reads and dact hold zeros
// there.
template <int NP = 0, bool F16 = false, int R = 0>
struct EpiActFwdT {
  const float* bias;
  const uint16_t* mask;   // [B][nt]
  float* dact;            // [B][nt * 16] slice of step t
  float keep;
  float* lds_out;
  float* stash;           // feature-major block [nt*16][Rw] or nullptr
  int ld, Rw, row0, nvalid, nt, lane, act, width;
  int* ovf;
  typedef typename EpiHiddenFwdT<NP, F16, R>::Pre Pre;
  __device__ __forceinline__ Pre pre(int ot, int rt) const {
    const int g = lane >> 4;
    const int lrow = rt * 16 + (lane & 15);
    Pre p;
    p.b = ldg4(bias + ot * 16 + 4 * g);
    p.mw = 0;
    if (lrow < nvalid) p.mw = mask[(size_t)(row0 + lrow) * nt + ot];
    return p;
  }
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) { (*this)(ot, rt, acc, pre(ot, rt)); }
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc, const Pre& pr) {
    const int g = lane >> 4;
    const int lrow = rt * 16 + (lane & 15);
    const int f0 = ot * 16 + 4 * g;
    const unsigned nib = (pr.mw >> (4 * g)) & 0xFu;   // (rows past the batch: no bit set)
    f32x4 h, dd;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float hv, dv;
      pm_act(act, acc[r] + pr.b[r], f0 + r, width, hv, dv);
      const bool m = ((nib >> r) & 1u) && f0 + r < width;
      // (the reference's division, x / p)
      h[r] = m ? (keep == 1.f ? hv : hv / keep) : 0.f;
      dd[r] = m ? (keep == 1.f ? dv : dv / keep) : 0.f;
    }
    if constexpr (NP > 0) {
      pm_store_planes<NP, R, F16>(lds_out, (unsigned)ld, (unsigned)lrow, (unsigned)f0, h);
      if (ot == nt - 1 && (nt & 1))
        pm_store_planes<NP, R, F16>(lds_out, (unsigned)ld, (unsigned)lrow, (unsigned)f0 + 16u, f32x4{0.f, 0.f, 0.f, 0.f});
      if constexpr (F16) {
        // (SiLU is unbounded above; a NaN pre-activation stays a NaN here and ends the rollout at this step)
        if (fmaxf(fmaxf(fabsf(h[0]), fabsf(h[1])), fmaxf(fabsf(h[2]), fabsf(h[3]))) > 65504.f) *ovf = 1;
      }
    } else {
      *reinterpret_cast<f32x4*>(lds_out + lrow * ld + f0) = h;
    }
    if (stash) {
#pragma unroll
      for (int r = 0; r < 4; ++r) __builtin_nontemporal_store(h[r], stash + (size_t)(f0 + r) * Rw + lrow);
    }
    if (lrow < nvalid) *reinterpret_cast<f32x4*>(dact + ((size_t)(row0 + lrow) * nt + ot) * 16 + 4 * g) = dd;
  }
};

// ... backward: g_pre = acc * dact (zero where dact is: a dropped, padded or saturated unit passes no NaN on)
template <int NP = 0, int R = 0>
struct EpiActBwdT {
  const float* dact;      // [B][nt * 16] slice of step t
  float* lds_out;
  float* stash;           // gT block or nullptr
  int ld, Rw, row0, nvalid, nt, lane;
  struct Pre {
    f32x4 d;
  };
  __device__ __forceinline__ Pre pre(int ot, int rt) const {
    const int lrow = rt * 16 + (lane & 15);
    Pre p;
    p.d = f32x4{0.f, 0.f, 0.f, 0.f};
    if (lrow < nvalid) p.d = ldg4(dact + ((size_t)(row0 + lrow) * nt + ot) * 16 + 4 * (lane >> 4));
    return p;
  }
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc) { (*this)(ot, rt, acc, pre(ot, rt)); }
  __device__ __forceinline__ void operator()(int ot, int rt, f32x4 acc, const Pre& pr) {
    const int g = lane >> 4;
    const int lrow = rt * 16 + (lane & 15);
    const int f0 = ot * 16 + 4 * g;
    f32x4 h;
#pragma unroll
    for (int r = 0; r < 4; ++r) h[r] = pr.d[r] != 0.f ? acc[r] * pr.d[r] : 0.f;
    if constexpr (NP > 0) {
      pm_store_planes<NP, R, false>(lds_out, (unsigned)ld, (unsigned)lrow, (unsigned)f0, h);
      if (ot == nt - 1 && (nt & 1))
        pm_store_planes<NP, R, false>(lds_out, (unsigned)ld, (unsigned)lrow, (unsigned)f0 + 16u, f32x4{0.f, 0.f, 0.f, 0.f});
    } else {
      *reinterpret_cast<f32x4*>(lds_out + lrow * ld + f0) = h;
    }
    if (stash) {
#pragma unroll
      for (int r = 0; r < 4; ++r) __builtin_nontemporal_store(h[r], stash + (size_t)(f0 + r) * Rw + lrow);
    }
  }
};

// ---------------------------------------------------------------------------
// reward (envs/<env>/env.py:*Reward.forward); one thread per row
// ---------------------------------------------------------------------------
__device__ inline float reward_row(const RewardDev* __restrict__ rw, const float* x, int D,
                                   const float* a, int U, float* delta_out) {
  float phi[PMBRL_MAX_DIM];
  int De;
  if (rw->expand) {
    const int no = rw->n_other, na = rw->n_angle;
    for (int i = 0; i < no; ++i) phi[i] = x[rw->other_dims[i]];
    for (int j = 0; j < na; ++j) {
      const float th = x[rw->angle_dims[j]];
      phi[no + j] = sinf(th);
      phi[no + na + j] = cosf(th);
    }
    De = no + 2 * na;
  } else {
    for (int i = 0; i < D; ++i) phi[i] = x[i];
    De = D;
  }
  const int k = rw->k;
  float delta[PMBRL_MAX_TIP];
  for (int i = 0; i < k; ++i) {
    float s = 0.f;
    for (int j = 0; j < De; ++j) s = fmaf(phi[j], rw->C[i * De + j], s);
    delta[i] = s - rw->tt[i];
    if (delta_out) delta_out[i] = delta[i];
  }
  float cost = 0.f;
  for (int i = 0; i < k; ++i) {
    float s = 0.f;
    for (int j = 0; j < k; ++j) s = fmaf(delta[j], rw->Q[j * k + i], s);
    cost = fmaf(s, delta[i], cost);
  }
  for (int i = 0; i < U; ++i) {
    float s = 0.f;
    for (int j = 0; j < U; ++j) s = fmaf(a[j], rw->R[j * U + i], s);
    cost = fmaf(s, a[i], cost);
  }
  cost *= rw->w;
  return rw->kind == PMBRL_REWARD_EXP ? expf(-cost) : -cost;
}

// adjoint of reward_row: adds d r / d x into gx[D], writes d r / d a into ga[U],
// both scaled by the upstream gr.
__device__ inline void reward_row_bwd(const RewardDev* __restrict__ rw, const float* x, int D,
                                      const float* a, int U, float r, float gr, float* gx,
                                      float* ga) {
  float delta[PMBRL_MAX_TIP];
  (void)reward_row(rw, x, D, a, U, delta);   // recompute delta (cheap)
  const float gc = (rw->kind == PMBRL_REWARD_EXP ? -gr * r : -gr) * rw->w;
  const int k = rw->k;
  const int De = rw->expand ? rw->n_other + 2 * rw->n_angle : D;
  float gdelta[PMBRL_MAX_TIP];
  for (int i = 0; i < k; ++i) {
    float s = 0.f;
    for (int j = 0; j < k; ++j) s = fmaf(delta[j], rw->QQ[j * k + i], s);
    gdelta[i] = gc * s;
  }
  for (int i = 0; i < U; ++i) {
    float s = 0.f;
    for (int j = 0; j < U; ++j) s = fmaf(a[j], rw->RR[j * U + i], s);
    ga[i] = gc * s;
  }
  float gphi[PMBRL_MAX_DIM];
  for (int j = 0; j < De; ++j) {
    float s = 0.f;
    for (int i = 0; i < k; ++i) s = fmaf(gdelta[i], rw->C[i * De + j], s);
    gphi[j] = s;
  }
  if (rw->expand) {
    const int no = rw->n_other, na = rw->n_angle;
    for (int i = 0; i < no; ++i) gx[rw->other_dims[i]] += gphi[i];
    for (int j = 0; j < na; ++j) {
      const float th = x[rw->angle_dims[j]];
      gx[rw->angle_dims[j]] += gphi[no + j] * cosf(th) - gphi[no + na + j] * sinf(th);
    }
  } else {
    for (int i = 0; i < D; ++i) gx[i] += gphi[i];
  }
}

// ---------------------------------------------------------------------------
// LDS carve-up: the pointers of the map (pm_lds_map, pmbrl_lds_map.h), which also gives the host the launch's size.
// ---------------------------------------------------------------------------
// moment-matching noise addressing: cyclic PEGASUS buffer or fresh rows per step
__device__ __forceinline__ const float* pm_zbase(const float* z, int ld, int t, int Bg, int flags) {
  return (flags & PMBRL_FLAG_ZMM_PER_STEP) ? z + (size_t)t * Bg * ld : z;
}
__device__ __forceinline__ int pm_zrow0(int t, int row, int flags) {
  return (flags & PMBRL_FLAG_ZMM_PER_STEP) ? row : t + row;
}

struct LdsMap {
  float *bufA, *bufB, *xa, *xb, *av, *gad, *rr, *gr, *part, *tbl;
  double* mm;
};
// ip: in-place layers (gemm_layer_inplace_s) -- ONE activation buffer, narrow GEMM outputs at column PM_IP_NOFF of it
__device__ inline LdsMap pm_lds_carve(float* base, int R, int LD, int D, int U, int RT, bool ip = false) {
  const PmLdsMapT<float*> o = pm_lds_map(base, R, LD, D, U, RT, 0, ip);
  LdsMap m;
  m.bufA = o.bufA; m.bufB = o.bufB; m.xa = o.xa; m.xb = o.xb;
  m.av = o.av; m.gad = o.gad; m.rr = o.rr; m.gr = o.gr;
  m.part = o.has_part ? o.part : nullptr;
  m.tbl = o.tbl;
  m.mm = reinterpret_cast<double*>(o.mm);
  return m;
}

// the sweeps (pmbrl_rollout_sweeps.h says why twice)
#define PM_SWEEP_FWD pm_rollout_fwd
#define PM_SWEEP_BWD pm_rollout_bwd
#define PM_SWEEP_LR 0
#include "pmbrl_rollout_sweeps.h"
#undef PM_SWEEP_FWD
#undef PM_SWEEP_BWD
#undef PM_SWEEP_LR
#define PM_SWEEP_FWD pm_rollout_fwd_gmmr
#define PM_SWEEP_BWD pm_rollout_bwd_gmmr
#define PM_SWEEP_LR 1
#include "pmbrl_rollout_sweeps.h"
#undef PM_SWEEP_FWD
#undef PM_SWEEP_BWD
#undef PM_SWEEP_LR
