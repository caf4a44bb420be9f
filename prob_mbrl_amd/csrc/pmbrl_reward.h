// The reward kernels of a rollout: not part of the sweep kernels.  Non-template launches of the forward and adjoint calls,
// compiled into pmbrl.hip only.
#pragma once
#include "pmbrl_fast.h"

// All rewards of a rollout in one fully parallel pass: thread = one (t, b) row-step.
// r~ -> rt (if rewards are moment matched afterwards) or rewards; d r~/d x~ -> Jx; d r~/d a -> Ja;
// non-finite states / rewards are reported through the status word like in the sweep.
// The 256 state rows of a block go through LDS (row stride D | 1): a thread walks ITS row, so straight from HBM
// every load and every Jacobian store of a wave touched 64 cache lines (1.7 ms at D = 32, 1.6 M row-steps).  The
// Jacobian row overwrites the state row in place and leaves the same way.
// NU: compile-time bound on the action width (4: the common shapes, their path unchanged; 8 / 16: the quadratic forms of the
// action cost unrolled to that width -- an instance of their own: compiled into the one kernel their 30 KB of code sat
// between the halves of the narrow path and cost ITS launches 3 us of instruction fetch)
// KT: compile-time bound on the tip residuals k (2: the cart-pole class -- a tip position in the plane; KT: any):
// the loops over them are unrolled to KT with the entries beyond k dropped by selects, so at k = 2 an instance unrolled to
// eight carried sixteen times the loads and selects of its quadratic forms (4.6 of the launch's 10.5 us at C2 were this
// arithmetic).
template <int NU, int KT>
__global__ __launch_bounds__(256) void pm_reward_all_kernel(const RolloutArgs A) {
  extern __shared__ float rw_rows[];
  // The cache lines of the reward's constants a row-step will read -- the heads of its arrays: the scalar cache met each of
  // them as a miss of its own, one behind the other, in the middle of the arithmetic; requested here they arrive while
  // the states do.  The values are not used: the registers are held until the barrier below.
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned pf[16];
  {
    typedef __attribute__((address_space(4))) const unsigned* kup;
    const kup rp = (kup)A.rew;
    constexpr int PFO[16] = {0,
                             (int)offsetof(RewardDev, C), (int)offsetof(RewardDev, C) + 64, (int)offsetof(RewardDev, tt),
                             (int)offsetof(RewardDev, Q), (int)offsetof(RewardDev, Q) + 64, (int)offsetof(RewardDev, QQ),
                             (int)offsetof(RewardDev, QQ) + 64, (int)offsetof(RewardDev, R), (int)offsetof(RewardDev, RR),
                             (int)offsetof(RewardDev, phi_src), (int)offsetof(RewardDev, phi_mode),
                             (int)offsetof(RewardDev, d_copy), (int)offsetof(RewardDev, d_sin),
                             (int)offsetof(RewardDev, d_cos), (int)offsetof(RewardDev, w)};
#pragma unroll
    for (int u = 0; u < 16; ++u) asm volatile("s_load_dword %0, %1, %2" : "=s"(pf[u]) : "s"(rp), "n"(PFO[u]));
  }
#endif
  const long long n = (long long)A.H * A.B;
  const long long i0 = (long long)blockIdx.x * blockDim.x;
  const long long i = i0 + threadIdx.x;
  const int D = A.D, U = A.U;
  const int ld = D | 1;
  // (the adjoint call's failure flag, the status word's second entry: cleared here, by a launch every forward call makes)
  if (blockIdx.x == 0 && threadIdx.x == 0 && A.status) A.status[1] = 0;
  const int nrow = (int)min((long long)blockDim.x, n - i0);
  {
    const float* src = (A.flags & PMBRL_FLAG_MM_STATES) ? A.xt + (size_t)i0 * D : A.states + ((size_t)i0 + A.B) * D;
    // (eight loads in flight per thread: one at a time -- load, wait, write -- the D = 4 block was four memory round trips
    //  in a row, a third of this launch at C2)
    const int ne = nrow * D;
    for (int e0 = threadIdx.x; e0 < ne; e0 += 8 * 256) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[min(e0 + 256 * u, ne - 1)];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 256 * u;
        if (e < ne) {
          const int r = e / D, d = e - r * D;
          rw_rows[r * ld + d] = v[u];
        }
      }
    }
  }
  // (the row's first four actions: requested here, beside the states)
  float a4[4];
  {
    const float* ac = A.actions + (size_t)min(i, n - 1) * U;
#pragma unroll
    for (int u = 0; u < 4; ++u) a4[u] = ac[min(u, U - 1)];
  }
  // (wider action vectors: the NU = 8 / 16 instances)
  float av[NU];
  if constexpr (NU > 4) {
    const float* ac = A.actions + (size_t)min(i, n - 1) * U;
#pragma unroll
    for (int u = 0; u < NU; ++u) av[u] = ac[min(u, U - 1)];
  }
  __syncthreads();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int u = 0; u < 16; ++u) asm volatile("" ::"s"(pf[u]));
#endif
  if (i < n) {
  const int t = (int)(i / A.B);
  // (the reward's constants through a constant-address-space pointer: wave-uniform indices make scalar loads of them; as a
  //  generic pointer every coefficient was a vector load from global memory per thread -- a hundred of them a row-step)
  typedef __attribute__((address_space(4))) const RewardDev* rew_kptr;
#if defined(__HIP_DEVICE_COMPILE__)
  const rew_kptr rw = (rew_kptr)A.rew;
#else
  const RewardDev* rw = A.rew;
#endif
  float* xs = rw_rows + threadIdx.x * ld;
  // No per-thread array is indexed at run time (that would live in scratch): the feature map is
  // walked in gather form, x / a come from their (L1-resident) rows, only the k <= 8 tip
  // residuals sit in registers with static indices.
  const int k = rw->k, De = rw->De;
  bool ok = true;
  for (int d = 0; d < D; ++d) ok = ok && isfinite(xs[d]);
  float delta[KT];
#pragma unroll
  for (int q = 0; q < KT; ++q) delta[q] = 0.f;
  for (int j = 0; j < De; ++j) {
    const float xv = xs[rw->phi_src[j]];
    const int md = rw->phi_mode[j];
    const float ph = md == 0 ? xv : (md == 1 ? sinf(xv) : cosf(xv));
    // (the coefficients of all KT rows are loaded, the rows beyond k dropped by a select: every index is inside
    //  the array, and a load UNDER the condition is a scalar load, a wait and a branch of its own -- this kernel was a chain
    //  of ~190 of those, most of its 13 us at C2)
    float cj[KT];
#pragma unroll
    for (int q = 0; q < KT; ++q) cj[q] = rw->C[q * De + j];
#pragma unroll
    for (int q = 0; q < KT; ++q) delta[q] = q < k ? fmaf(ph, cj[q], delta[q]) : delta[q];
  }
#pragma unroll
  for (int q = 0; q < KT; ++q) {
    const float ttq = rw->tt[q];
    delta[q] -= (q < k) ? ttq : 0.f;
  }
  float cost = 0.f;
#pragma unroll
  for (int q = 0; q < KT; ++q) {
    float s = 0.f;
    float qv[KT];
#pragma unroll
    for (int p = 0; p < KT; ++p) qv[p] = rw->Q[p * k + q];      // (p k + q < KT^2 <= 64 for any k <= KT)
#pragma unroll
    for (int p = 0; p < KT; ++p) s = (p < k && q < k) ? fmaf(delta[p], qv[p], s) : s;
    cost = q < k ? fmaf(s, delta[q], cost) : cost;
  }
  // U > 4: s[q] = sum_p a_p M[p][q], p ascending, for a compile-time bound NU >= U on both indices: the rows of M loaded
  // whole (every index inside the 16 x 16 array), entries beyond U dropped by selects -- as run-time loops over U this was
  // a vector load of a_p, a scalar load of M[p][q] and a wait per term: 2 x 64 of them in a row at U = 8, half of the
  // launch's 0.5 ms at C5
  auto quad = [&](auto nu, auto Mx, float* sq) {
    constexpr int NW = decltype(nu)::value;
#pragma unroll
    for (int q = 0; q < NW; ++q) sq[q] = 0.f;
#pragma unroll
    for (int p = 0; p < NW; ++p) {
      float row[NW];
#pragma unroll
      for (int q = 0; q < NW; ++q) row[q] = Mx[p * U + q];
#pragma unroll
      for (int q = 0; q < NW; ++q) sq[q] = (p < U && q < U) ? fmaf(av[p], row[q], sq[q]) : sq[q];
    }
  };
  auto cost_part = [&](auto nu) {
    constexpr int NW = decltype(nu)::value;
    float sq[NW];
    quad(nu, &rw->R[0], sq);
#pragma unroll
    for (int q = 0; q < NW; ++q) cost = q < U ? fmaf(sq[q], av[q], cost) : cost;
  };
  auto ja_part = [&](auto nu, float gcv) {
    constexpr int NW = decltype(nu)::value;
    float sq[NW];
    quad(nu, &rw->RR[0], sq);
#pragma unroll
    for (int q = 0; q < NW; ++q)
      if (q < U) A.Ja[(size_t)i * U + q] = gcv * sq[q];
  };
  if constexpr (NU == 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float s = 0.f;
      float rv4[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) rv4[p] = rw->R[p * U + q];
#pragma unroll
      for (int p = 0; p < 4; ++p) s = (p < U && q < U) ? fmaf(a4[p], rv4[p], s) : s;
      cost = q < U ? fmaf(s, a4[q], cost) : cost;
    }
  } else {
    cost_part(std::integral_constant<int, NU>{});
  }
  cost *= rw->w;
  const float rv = rw->kind == PMBRL_REWARD_EXP ? expf(-cost) : -cost;
  ok = ok && isfinite(rv);
  if (!ok) atomicMin(A.status, t);
  // adjoint with unit upstream gradient
  const float gc = (rw->kind == PMBRL_REWARD_EXP ? -rv : -1.f) * rw->w;
  float gdelta[KT];
#pragma unroll
  for (int q = 0; q < KT; ++q) {
    float s = 0.f;
    float qv[KT];
#pragma unroll
    for (int p = 0; p < KT; ++p) qv[p] = rw->QQ[p * k + q];
#pragma unroll
    for (int p = 0; p < KT; ++p) s = (p < k && q < k) ? fmaf(delta[p], qv[p], s) : s;
    gdelta[q] = gc * s;
  }
  auto gphi = [&](int j) {
    float s = 0.f;
    float cj[KT];
#pragma unroll
    for (int q = 0; q < KT; ++q) cj[q] = rw->C[q * De + j];
#pragma unroll
    for (int q = 0; q < KT; ++q) s = q < k ? fmaf(gdelta[q], cj[q], s) : s;
    return s;
  };
  for (int d = 0; d < D; ++d) {
    float g = 0.f;
    const int jc = rw->d_copy[d], js = rw->d_sin[d];
    if (jc >= 0) g += gphi(jc);
    if (js >= 0) {
      const float th = xs[d];
      g += gphi(js) * cosf(th) - gphi(rw->d_cos[d]) * sinf(th);
    }
    xs[d] = g;      // (x_d has been read: only dimension d's own sine / cosine terms use it)
  }
  if constexpr (NU == 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float s = 0.f;
      float rv4[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) rv4[p] = rw->RR[p * U + q];
#pragma unroll
      for (int p = 0; p < 4; ++p) s = (p < U && q < U) ? fmaf(a4[p], rv4[p], s) : s;
      if (q < U) A.Ja[(size_t)i * U + q] = gc * s;
    }
  } else {
    ja_part(std::integral_constant<int, NU>{}, gc);
  }
  if (A.flags & PMBRL_FLAG_MM_REWARDS) A.rt[i] = rv;
  else A.rewards[i] = rv;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nrow * D; e += blockDim.x) {
    const int r = e / D, d = e - r * D;
    A.Jx[(size_t)i0 * D + e] = rw_rows[r * ld + d];
  }
}

// The reward launch of a learned reward head (PMBRL_REWARD_LEARNED): the forward sweep has sampled r~ from the dynamics
// head, written it where the analytic launch writes its value and checked it; no Jacobians exist (the adjoint seeds the
// head with dL/dr~).  What is left is the adjoint call's failure flag, which every forward call clears here.
__global__ __launch_bounds__(64) void pm_reward_learned_kernel(const RolloutArgs A) {
  if (threadIdx.x == 0 && A.status) A.status[1] = 0;
}

// moment matching of the rewards for all (t, group) at once (one wave each), and its adjoint
// A LARGE group (mm_groups=None: one group of 2 500 rows) first brings its rows -- rewards, noise, in the adjoint the
// upstream gradient -- into LDS, sixteen loads in flight per lane, and runs the same routine on them there: its sums walk
// the rows one dependent load at a time, three to five passes of 39 memory round trips on one wave (26 / 34 us per launch
// at 2 500 rows).  Same arithmetic in the same order: the results are the unstaged form's bit for bit.
#define PM_MMR_STAGE_MIN 128           // rows from which a group is staged
#define PM_MMR_STAGE_MAX 4096          // ... and up to which its three arrays fit (48 KB beside the scratch)
__host__ __device__ inline size_t pm_mmr_lds_bytes(int M, int arrays) {
  const size_t scr = pm_mm_scratch_doubles(1) * sizeof(double);
  return (M >= PM_MMR_STAGE_MIN && M <= PM_MMR_STAGE_MAX) ? scr + (size_t)arrays * M * sizeof(float) : scr;
}
// rows src[idx(i)] for i < M into dst[i]
template <class IDX>
__device__ __forceinline__ void pm_mmr_stage(float* dst, const float* src, int M, int lane, IDX idx) {
  for (int i0 = lane; i0 < M; i0 += 16 * 64) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = src[idx(min(i0 + 64 * u, M - 1))];
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (i0 + 64 * u < M) dst[i0 + 64 * u] = v[u];
  }
}
// A SMALL group (<= 64 rows: lane l holds row l) in registers: what pm_mm_fwd / pm_mm_bwd do at d = 1 -- the same sums
// in the same order (a lane's one row, the butterfly over the wave), the same formulas -- without their passes over
// memory: at 25 rows every pass of the general routine was a global load and a wait, three to five in a row per group
// (6 + 8 us per iteration at C3 for 4 000 groups).  Returns false on a non-positive pivot (pm_mm_chol's rule).
struct Mm1Fac { double mean, zmean, zistd, L, invd; };
__device__ __forceinline__ bool pm_mm1_reg_factor(float sv, float zv, bool in, int M, Mm1Fac& f) {
  const double inv_m = 1.0 / (double)M, inv_m1 = 1.0 / (double)(M - 1);
  double m = 0.0, zm = 0.0, zz = 0.0;
  if (in) {
    m += (double)sv;
    const double zd = (double)zv;
    zm += zd;
    zz += zd * zd;
  }
  m = pm_seg_sum(m, 64);
  zm = pm_seg_sum(zm, 64);
  zz = pm_seg_sum(zz, 64);
  m *= inv_m;
  zm *= inv_m;
  f.mean = m;
  f.zmean = zm;
  f.zistd = pm_rsqrt((zz - (double)M * zm * zm) * inv_m1);
  double acc = 0.0;
  if (in) acc += ((double)sv - m) * ((double)sv - m);
  acc = pm_seg_sum(acc, 64);
  const double c0 = acc * inv_m1 + 1e-12;
  double piv = c0;
  bool ok = true;
  if (!(piv > 6e-8 * c0)) {
    ok = false;
    piv = 1.0;
  }
  const double rs = pm_rsqrt(piv);
  f.L = piv * rs;
  f.invd = rs;
  return ok;
}
__global__ void pm_mm_rewards_fwd_kernel(const RolloutArgs A) {
  extern __shared__ __attribute__((aligned(16))) double mmscr_r[];
  const int t = blockIdx.x / A.G, gi = blockIdx.x - t * A.G, lane = threadIdx.x;
  const int r0 = gi * A.M;
  const float* s = A.rt + (size_t)t * A.B + r0;
  const float* z = pm_zbase(A.zrr, 1, t, A.Bg, A.flags);
  int zrow0 = pm_zrow0(t, A.row_off + r0, A.flags), Bg = A.Bg;
  if (A.M <= 64 && !(A.flags & PMBRL_FLAG_INFER_NS)) {
    const bool in = lane < A.M;
    const int li = min(lane, A.M - 1);
    const float sv = s[li], zv = z[(size_t)pm_zidx(zrow0, li, Bg)];
    Mm1Fac f;
    const bool ok = pm_mm1_reg_factor(sv, zv, in, A.M, f);
    if (in) {
      double acc = f.mean;
      acc += ((double)zv - f.zmean) * f.zistd * f.L;
      A.rewards[(size_t)t * A.B + r0 + lane] = (float)acc;
    }
    if (!ok && lane == 0) atomicMin(A.status, t);
    return;
  }
  if (A.M >= PM_MMR_STAGE_MIN && A.M <= PM_MMR_STAGE_MAX) {
    float* ls = reinterpret_cast<float*>(mmscr_r + pm_mm_scratch_doubles(1));
    float* lz = ls + A.M;
    pm_mmr_stage(ls, s, A.M, lane, [](int i) { return i; });
    pm_mmr_stage(lz, z, A.M, lane, [=](int i) { return (size_t)pm_zidx(zrow0, i, Bg); });
    pm_wave_sync();
    s = ls; z = lz; zrow0 = 0; Bg = 0;
  }
  const bool ok = pm_mm_fwd(s, 1, A.M, 1, z, 1, zrow0, Bg, (A.flags & PMBRL_FLAG_INFER_NS) != 0,
                            A.rewards + (size_t)t * A.B + r0, 1, mmscr_r, lane);
  if (!ok && lane == 0) atomicMin(A.status, t);
}
__global__ void pm_mm_rewards_bwd_kernel(const RolloutArgs A, float* gr_tilde) {
  extern __shared__ __attribute__((aligned(16))) double mmscr_r[];
  const int t = blockIdx.x / A.G, gi = blockIdx.x - t * A.G, lane = threadIdx.x;
  const int r0 = gi * A.M;
  if (A.nvalid && t >= *A.nvalid) return;   // a step the forward sweep did not complete
  const float* s = A.rt + (size_t)t * A.B + r0;
  const float* z = pm_zbase(A.zrr, 1, t, A.Bg, A.flags);
  const float* g = A.grad_rewards + (size_t)t * A.B + r0;
  int zrow0 = pm_zrow0(t, A.row_off + r0, A.flags), Bg = A.Bg;
  if (A.M <= 64 && !(A.flags & PMBRL_FLAG_INFER_NS)) {
    const bool in = lane < A.M;
    const int li = min(lane, A.M - 1);
    const float sv = s[li], zv = z[(size_t)pm_zidx(zrow0, li, Bg)], gv = g[li];
    Mm1Fac f;
    (void)pm_mm1_reg_factor(sv, zv, in, A.M, f);
    const double inv_m = 1.0 / (double)A.M, inv_m1 = 1.0 / (double)(A.M - 1);
    // mbar = sum_r g ;  Lbar = g^T zhat
    double a = 0.0, lb = 0.0;
    if (in) {
      a += (double)gv;
      lb += (double)gv * (((double)zv - f.zmean) * f.zistd);
    }
    const double mbar = pm_seg_sum(a, 64);
    lb = pm_seg_sum(lb, 64);
    // pm_mm_bwd_solve at d = 1: Phi = L Lbar / 2, X = Phi / L, Sbar = X / L, P = 2 Sbar / (M - 1)
    double phi = 0.0;
    phi += f.L * lb;
    phi *= 0.5;
    const double xs = phi * f.invd;
    const double sb = xs * f.invd;
    const double P = (sb + sb) * inv_m1;
    if (in) {
      double acc = mbar * inv_m;
      acc += ((double)sv - f.mean) * P;
      gr_tilde[(size_t)t * A.B + r0 + lane] = (float)acc;
    }
    return;
  }
  if (A.M >= PM_MMR_STAGE_MIN && A.M <= PM_MMR_STAGE_MAX) {
    float* ls = reinterpret_cast<float*>(mmscr_r + pm_mm_scratch_doubles(1));
    float* lz = ls + A.M;
    float* lg = lz + A.M;
    pm_mmr_stage(ls, s, A.M, lane, [](int i) { return i; });
    pm_mmr_stage(lz, z, A.M, lane, [=](int i) { return (size_t)pm_zidx(zrow0, i, Bg); });
    pm_mmr_stage(lg, g, A.M, lane, [](int i) { return i; });
    pm_wave_sync();
    s = ls; z = lz; g = lg; zrow0 = 0; Bg = 0;
  }
  pm_mm_bwd(s, 1, A.M, 1, z, 1, zrow0, Bg, (A.flags & PMBRL_FLAG_INFER_NS) != 0, g, 1,
            gr_tilde + (size_t)t * A.B + r0, 1, mmscr_r, lane);
}
