// The small kernels around the sweeps and their stand-alone entry points: mask packing and drawing, the weighted sum,
// the dW GEMM's reduction, the gradient norm, clip + Adam, and the sharded iteration tail.  pm_dw_reduce lives here and not
// with the dW GEMMs: it leaves the norm's and the loss' partial sums and the go / no-go decision in the device globals
// (g_norm_part, g_loss_part, g_adam_go) that pm_clip_adam_kernel and the pm_tail_* kernels read, and a device global is
// one object's.  The rollout adjoint call (pmbrl.hip) and the BNN step (pmbrl_bnn.hip) reach them through the launchers
// declared in pmbrl_host.h.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "pmbrl_host.h"

__global__ void pm_pack_mask_kernel(const float* __restrict__ m, int B, int h, int ld,
                                    uint16_t* __restrict__ bits) {
  const int nt = (h + 15) / 16;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * nt) return;
  const int r = i / nt, t = i - r * nt;
  unsigned w = 0;
  for (int j = 0; j < 16; ++j) {
    const int f = t * 16 + j;
    if (f < h && m[(size_t)r * ld + f] != 0.f) w |= 1u << j;
  }
  bits[i] = (uint16_t)w;
}
__global__ void pm_set_int(int* p, int v) { *p = v; }

// ---------------------------------------------------------------------------
// Dropout masks drawn on the device (pmbrl_draw_masks): bit rows straight from a counter-based generator.
// Philox4x32-10 (Salmon et al., SC'11) keyed by the caller's seed; counter = (row, 16-unit tile, quad + 4 * stream,
// offset): a draw depends on (seed, offset, row, unit) alone, not on the launch shape.  Stream 0: the uniform noise u;
// stream 1: the uniform the hard Bernoulli sample is thresholded with.
// ---------------------------------------------------------------------------
struct DrawArgs {
  int kind;              // 0: Bernoulli(keep) -- BDropout.update_noise, models/modules.py:40-44;  1: concrete -- :95-118
  unsigned long long seed, offset;
  const float* param;    // kind 0: keep probability; kind 1: logit_p  (param_len 1 or h)
  int param_len;
  float temp;
  int rows, h;
  const float *u_in, *v_in;     // [rows][h] uniforms to use instead of the generator's (nullptr: generate)
  uint16_t* bits;        // [rows][ceil(h/16)]
  int aux_row0, aux_rows;       // rows whose float values are also written (a module keeps its LAST draw as state)
  float *u_out, *hard_out, *probs_out;   // [aux_rows][h] each, or nullptr
};
__global__ __launch_bounds__(256) void pm_draw_masks_kernel(const DrawArgs A) {
  const int nt = (A.h + 15) / 16;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)A.rows * nt) return;
  const int r = (int)(i / nt), t = (int)(i - (long long)r * nt);
  const unsigned k0 = (unsigned)A.seed, k1 = (unsigned)(A.seed >> 32);
  const unsigned o0 = (unsigned)A.offset, o1 = (unsigned)(A.offset >> 32);
  unsigned w = 0;
  const bool aux = r >= A.aux_row0 && r < A.aux_row0 + A.aux_rows;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned ru[4], rv[4];
    if (!A.u_in) pm_philox((unsigned)r, (unsigned)t, (unsigned)q ^ (o1 << 3), o0, k0, k1, ru);
    if (A.kind == 1 && !A.v_in) pm_philox((unsigned)r, (unsigned)t, (unsigned)(4 + q) ^ (o1 << 3), o0, k0, k1, rv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int f = t * 16 + q * 4 + e;
      if (f >= A.h) continue;
      const size_t idx = (size_t)r * A.h + f;
      // 24-bit uniforms in [0, 1) (what torch.rand gives a float tensor)
      const float u = A.u_in ? A.u_in[idx] : (float)(ru[e] >> 8) * (1.0f / 16777216.0f);
      const float pr = A.param[A.param_len > 1 ? f : 0];
      float probs;
      bool bit;
      if (A.kind == 0) {
        probs = pr;
        bit = u < pr;                                    // torch.bernoulli(p): 1 with probability p
      } else {
        // models/modules.py:102-114: probs = sigmoid((logit_p + log((u + 1e-7) / (1 - (u - 1e-7)))) / temp)
        const float cp = pr + logf((u + 1e-7f) / (1.f - (u - 1e-7f)));
        probs = 1.f / (1.f + expf(-cp / A.temp));
        const float v = A.v_in ? A.v_in[idx] : (float)(rv[e] >> 8) * (1.0f / 16777216.0f);
        bit = v < probs;
      }
      if (bit) w |= 1u << (q * 4 + e);
      if (aux) {
        const size_t o = (size_t)(r - A.aux_row0) * A.h + f;
        if (A.u_out) A.u_out[o] = u;
        if (A.hard_out) A.hard_out[o] = bit ? 1.f : 0.f;
        if (A.probs_out) A.probs_out[o] = probs;
      }
    }
  }
  A.bits[i] = (uint16_t)w;
}

// Small reductions: per-block partial sums in a per-device scratch, finished in FIXED order
// (bit-reproducible).  The scratch is shared by all calls on a device: calls are expected to
// be stream-ordered (one optimisation loop per device), like the rest of a plan's work.
#define PM_RED_MAXB 128
__device__ double g_red_part[2][PM_RED_MAXB];
__device__ unsigned g_red_count;

__global__ __launch_bounds__(256) void pm_weighted_sum_kernel(const float* __restrict__ a,
                                                              const float* __restrict__ w,
                                                              long long n, float* __restrict__ out,
                                                              const int* __restrict__ nvalid, long long n_per_step) {
  __shared__ double sm[256];
  __shared__ unsigned ticket;
  if (nvalid) n = min(n, (long long)max(0, *nvalid) * n_per_step);   // truncated horizon
  double s = 0.0;
  // (eight elements' loads in flight at a time, added in the order a one-by-one loop adds them: as that loop -- load, wait,
  //  convert, add -- a thread's eight elements at C2 were eight memory round trips in a row, most of this launch)
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += 8 * stride) {
    float av[8], wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      // (beyond n: the last element's address, its value dropped below -- a load under a condition is waited for where
      //  the branches join, one at a time again)
      const long long j = min(i + u * stride, n - 1);
      av[u] = a[j];
      wv[u] = w[j];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s += i + u * stride < n ? (double)av[u] * (double)wv[u] : 0.0;
  }
  const double tot = pm_block_sum(s, sm);
  if (threadIdx.x == 0) {
    // (a device-scope store, then the ticket: a release FENCE here is a write-back of this XCD's whole L2 -- the reward
    //  launch's stash is still in it)
    __hip_atomic_store(&g_red_part[0][blockIdx.x], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ticket = __hip_atomic_fetch_add(&g_red_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (ticket == gridDim.x - 1) {          // last block: every partial is published
    // fixed-shape tree over the published partials (deterministic), not a serial chain of
    // L2 round trips
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double t = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += blockDim.x)
      t += __hip_atomic_load(&g_red_part[0][b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const double tt = pm_block_sum(t, sm);
    if (threadIdx.x == 0) {
      out[0] = (float)tt;
      __hip_atomic_store(&g_red_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Squared norm of the gradient for clip_grad_norm_ (algorithms/mc_pilco.py:199-200): partial sums over blocks of 256
// consecutive elements, ONE definition for the two kernels that form them -- pm_gradnorm_kernel (its own launch) and
// pm_dw_reduce (round 6: the fused iteration's reduction forms them on the way, one launch less) -- so that the two
// forms of an iteration walk the same trajectory bit for bit.  Lane c of a wave holds elements 4 c .. 4 c + 3 of the
// block: squares added in element order, then a fixed butterfly over the 64 lanes.
__device__ double g_norm_part[PM_NORM_MAXB];
__device__ double g_loss_part[PM_NORM_MAXB];   // the loss' partial sums, one per workgroup of pm_dw_reduce (loss_r != nullptr)
__device__ int g_adam_go;
__device__ __forceinline__ double pm_sq4_wave(const f32x4& t, long long i0, long long n) {
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double x = i0 + r < n ? (double)t[r] : 0.0;
    s += x * x;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return s;
}
// the optimiser step of a guarded iteration is taken if the rollout completed: status[0] = steps the forward sweep
// completed, status[1] = set by the adjoint sweep when one of its exchanges timed out (the gradient is garbage then)
__device__ __forceinline__ void pm_adam_decide(const int* status, int expect, long long* step) {
  const int go = (!status || (status[0] >= expect && status[1] == 0)) ? 1 : 0;
  g_adam_go = go;
  if (go && step) step[0] += 1;
}

// grad[i] = sum_s part[s][i] in fixed order.  A workgroup = 64 float4 columns x 8 slices of the
// split range: every wave reads whole 1 KiB rows, a thread keeps 16 independent loads in flight.
// norm_on: also the partial sums of squares of ITS 256 elements and (block 0) the decision whether the guarded optimiser
// step is taken -- what pm_gradnorm_kernel does in a launch of its own.
__global__ __launch_bounds__(512) void pm_dw_reduce(const float* __restrict__ part, int nsplit, int n,
                                                    int stride, float* __restrict__ grad,
                                                    const int* __restrict__ nvalid = nullptr, int chunks_per_step = 0,
                                                    int chunks_per_split = 1, int norm_on = 0,
                                                    const int* __restrict__ status = nullptr, int expect = 0,
                                                    long long* __restrict__ step = nullptr,
                                                    const float* __restrict__ loss_r = nullptr,
                                                    const float* __restrict__ loss_w = nullptr, long long loss_n = 0,
                                                    long long loss_per_step = 0, int col_lo = 0, int col_hi = 0,
                                                    int rows_in_range = 0) {
  __shared__ f32x4 sm[8][64];
  __shared__ double sl_[8];
  // loss_r: the fused iteration's loss on the way -- this workgroup's slice of sum_i r_i w_i over the valid steps (requested
  // here, added below: pm_clip_adam_kernel adds the workgroups' sums in workgroup order).  One launch less per iteration.
  float lr4[4] = {0.f, 0.f, 0.f, 0.f}, lw4[4] = {0.f, 0.f, 0.f, 0.f};
  long long l_n = 0;
  const long long l_i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, l_st = (long long)gridDim.x * blockDim.x;
  if (loss_r) {
    l_n = nvalid ? min(loss_n, (long long)max(0, *nvalid) * loss_per_step) : loss_n;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long j = min(l_i0 + u * l_st, loss_n - 1);
      lr4[u] = loss_r[j];
      lw4[u] = loss_w[j];
    }
  }
  if (nvalid) {   // truncated horizon: only the splits that own a chunk of a valid step wrote a partial
    const long long nc = (long long)max(0, *nvalid) * chunks_per_step;
    nsplit = (int)min((long long)nsplit, (nc + chunks_per_split - 1) / chunks_per_split);
  }
  const int col = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int c4 = blockIdx.x * 64 + col;            // float4 column
  const int per = (nsplit + 7) / 8;
  int k_hi = min(nsplit, sl * per + per);
  const int k_lo = sl * per;
  // [col_lo, col_hi): columns whose rows beyond the first rows_in_range hold no chunk (the streamed dW form's, DwArgs::own_lo).
  // A float4 column wholly inside adds those rows only -- the slices are the full range's, so every partial sum is the one
  // it was without additions of +0 to a sum that began as +0: the same bits, and the rows beyond are never read
  if (c4 * 4 >= col_lo && c4 * 4 + 4 <= col_hi) k_hi = min(k_hi, rows_in_range);
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (c4 * 4 < n) {
    const float* p = part + (size_t)c4 * 4;
    // (sixteen rows in flight per thread, the tail as one predicated batch of eight: at C2 a slice is 33 rows -- as
    //  8 + 8 + 8 + 8 + 1 it was five memory round trips in a row, now three; the order of the additions is the rows')
    int k = k_lo;
    for (; k + 16 <= k_hi; k += 16) {
      f32x4 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = ldg4(p + (size_t)(k + u) * stride);
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; k < k_hi; k += 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = ldg4(p + (size_t)min(k + u, k_hi - 1) * stride);   // (beyond: dropped below)
#pragma unroll
      for (int u = 0; u < 8; ++u) s += k + u < k_hi ? v[u] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  sm[sl][col] = s;
  if (loss_r) {
    double ls = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) ls += l_i0 + u * l_st < l_n ? (double)lr4[u] * (double)lw4[u] : 0.0;
    for (long long j = l_i0 + 4 * l_st; j < l_n; j += l_st) ls += (double)loss_r[j] * (double)loss_w[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ls += __shfl_xor(ls, o);
    if (col == 0) sl_[sl] = ls;
  }
  __syncthreads();
  if (loss_r && threadIdx.x == 0) {
    double t = sl_[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += sl_[k];
    g_loss_part[blockIdx.x] = t;
  }
  if (sl == 0) {
    f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c4 * 4 < n) {
      t = sm[0][col];
#pragma unroll
      for (int k = 1; k < 8; ++k) t += sm[k][col];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (c4 * 4 + r < n) grad[c4 * 4 + r] = t[r];
    }
    if (norm_on) {
      const double s2 = pm_sq4_wave(t, (long long)c4 * 4, n);
      if (col == 0) {
        g_norm_part[blockIdx.x] = s2;
        if (blockIdx.x == 0) pm_adam_decide(status, expect, step);
      }
    }
  }
}

static inline int pm_norm_blocks(long long n) { return (int)std::max<long long>(1, std::min<long long>(PM_NORM_MAXB, (n + 255) / 256)); }
// this workgroup's (one wave's) entry of g_norm_part: one block of 256 elements of src per workgroup up to PM_NORM_MAXB of
// them; a longer vector is walked in strides, the blocks' sums added in block order.  dst: the elements are also copied there
// (COPY: pm_tail_finish_kernel's form)
template <bool COPY>
__device__ __forceinline__ void pm_norm_walk(const float* __restrict__ src, float* __restrict__ dst, long long n) {
  double tot = 0.0;
  for (long long eb = blockIdx.x; eb * 256 < n; eb += gridDim.x) {
    const long long i0 = eb * 256 + 4 * (long long)threadIdx.x;
    f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i0 + 3 < n) {
      t = *reinterpret_cast<const f32x4*>(src + i0);
      if constexpr (COPY)
        for (int r = 0; r < 4; ++r) dst[i0 + r] = t[r];
    } else {
      for (int r = 0; r < 4; ++r) {
        t[r] = i0 + r < n ? src[i0 + r] : 0.f;
        if constexpr (COPY)
          if (i0 + r < n) dst[i0 + r] = t[r];
      }
    }
    tot += pm_sq4_wave(t, i0, n);
  }
  if (threadIdx.x == 0) g_norm_part[blockIdx.x] = tot;
}
// clip_grad_norm_ + Adam in two launches: (1) partial sums of g^2 over blocks of 256 elements (pm_sq4_wave above:
// the same partial sums the fused iteration's gradient reduction forms on the way), (2) every block adds the partials in
// the same order (identical norm everywhere) and updates its slice.
// Guarded form (pmbrl_clip_adam_guarded): block 0 also decides whether the step is taken (the rollout's status word says
// every horizon step completed) and, if so, advances the device-side step counter; pm_clip_adam_kernel (next launch)
// reads both.
__global__ __launch_bounds__(64) void pm_gradnorm_kernel(const float* __restrict__ g, long long n,
                                                         const int* __restrict__ status, int expect,
                                                         long long* __restrict__ step, int guarded) {
  if (guarded && blockIdx.x == 0 && threadIdx.x == 0) pm_adam_decide(status, expect, step);
  pm_norm_walk<false>(g, nullptr, n);
}

// The norm's partial sums as the optimiser launch takes them: the first four of this lane are REQUESTED before anything is
// decided (pm_norm_request) and added later (pm_norm_sum) -- block b on lane b mod 64 in block order, then a fixed
// butterfly: the same bits in every wave of every block
__device__ __forceinline__ void pm_norm_request(double (&part)[4], int lane, int n_part) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const double x = g_norm_part[min(lane + 64 * u, PM_NORM_MAXB - 1)];
    part[u] = lane + 64 * u < n_part ? x : 0.0;
  }
}
__device__ __forceinline__ double pm_norm_sum(const double (&part)[4], int lane, int n_part) {
  double t = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) t += part[u];                         // (absent: + 0)
  for (int b = lane + 256; b < n_part; b += 64) t += g_norm_part[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  return t;
}
// the fused iteration's loss: the sums pm_dw_reduce's workgroups left, added in workgroup order by one wave
__device__ __forceinline__ double pm_loss_sum(int lane, int n_loss_part) {
  double ls = 0.0;
  for (int b = lane; b < n_loss_part; b += 64) ls += g_loss_part[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ls += __shfl_xor(ls, o);
  return ls;
}

// ---------------------------------------------------------------------------
// clip + Adam: ONE kernel body (pm_clip_adam_kernel below), instantiated for a policy that says where an element's
// hyper-parameters come from.  AdamPlain: torch.optim.Adam with one set of them, scalars of the argument.  AdamTable: an
// optimiser rule (pmbrl_opt_rule: parameter groups, L2 / decoupled weight decay, amsgrad, maximize), without and with
// amsgrad's running maximum (VMAX: an instance of its own, no load under a condition).  A policy gives
//   prepare(lane, step)  this lane's record, the step-dependent entries included (step: the device-side counter of the
//                        guarded form, nullptr: the host's step count, already in the policy)
//   at(L, j, n)          the record of element j; every lane of the wave calls it together
//   done(i, lane, n)     whether a thread whose next element is i leaves the update loop
// ---------------------------------------------------------------------------
struct AdamLane {
  float b1, b2, omb1, omb2, eps;
  float wd, decay, sgn;          // OptGroupConsts (pmbrl_host.h)
  float step_size, bc2_sqrt;
  int ams;
};
struct AdamPlain {
  static constexpr bool kVmax = false;
  float b1, b2, omb1, omb2, eps;
  float bc1, bc2_sqrt;           // from the host's step count (not guarded)
  double ln_b1, ln_b2, lr_d;
  // (wd, decay, sgn and ams are constants here: the instance carries nothing of a rule -- x * 1.f and the dead branches fold)
  __device__ __forceinline__ AdamLane prepare(int, const long long* step) const {
    double step_size_d = lr_d / (double)bc1;
    float bc2 = bc2_sqrt;
    if (step) {
      // guarded form: bias corrections 1 - beta^t of the device-side step counter as -expm1(t ln beta), the exponent formed
      // and evaluated in double (torch forms them in Python floats; in fp32 the sixth digit of the step size differs and a
      // five-iteration comparison of the moments notices), ln beta from the host -- two double-precision pow calls were a
      // thousand instructions at the head of every thread, expm1 is a third of that
      const double st = (double)step[0];
      bc2 = (float)sqrt(-expm1(st * ln_b2));
      step_size_d = lr_d / -expm1(st * ln_b1);      // (torch: lr / bias_correction1 in Python floats, rounded once)
    }
    return AdamLane{b1, b2, omb1, omb2, eps, 0.f, 1.f, 1.f, (float)step_size_d, bc2, 0};
  }
  __device__ __forceinline__ AdamLane at(const AdamLane& L, long long, long long) const { return L; }
  __device__ __forceinline__ bool done(long long i, int, long long n) const { return i >= n; }
};

// The rule travels by value.  Segment boundaries and groups are read at CONSTANT offsets of the argument (scalar loads, no
// copy of the table in scratch): an element compares its index against the boundaries in turn.  The groups'
// hyper-parameters, the step-dependent ones included (lr / bc1, sqrt(bc2): one pair of expm1 per group, not per element),
// live in the lanes: lane l of every wave holds group l & 7, an element fetches its group's with a lane shuffle --
// neighbouring lanes may belong to different groups.
struct OptRuleDev {
  int n_segments, n_groups;
  int seg_group[PMBRL_OPT_MAX_SEGMENTS];
  long long seg_end[PMBRL_OPT_MAX_SEGMENTS];
  // per group (unused slots repeat group 0)
  float b1[PMBRL_OPT_MAX_GROUPS], b2[PMBRL_OPT_MAX_GROUPS], omb1[PMBRL_OPT_MAX_GROUPS], omb2[PMBRL_OPT_MAX_GROUPS];
  float eps[PMBRL_OPT_MAX_GROUPS];
  float wd[PMBRL_OPT_MAX_GROUPS], decay[PMBRL_OPT_MAX_GROUPS], sgn[PMBRL_OPT_MAX_GROUPS];   // OptGroupConsts (pmbrl_host.h)
  float step_size[PMBRL_OPT_MAX_GROUPS], bc2_sqrt[PMBRL_OPT_MAX_GROUPS];   // from the host's step count (not guarded)
  int amsgrad[PMBRL_OPT_MAX_GROUPS];
  double ln_b1[PMBRL_OPT_MAX_GROUPS], ln_b2[PMBRL_OPT_MAX_GROUPS], lr_d[PMBRL_OPT_MAX_GROUPS];
  float* vmax;
};
// a[gl] as a chain of selects between SCALAR operands.  The values are pinned to scalar registers first: left alone, the
// compiler folds the chain back into one load at a[gl] -- a per-lane load from the argument segment and a wait for it, one
// more memory round trip at the head of every thread (seen in the ISA: global_load_dword ... s_waitcnt vmcnt(0))
__device__ __forceinline__ int pm_scalar(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ float pm_scalar(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ double pm_scalar(double x) {
  const long long b = __double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll));
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <class T>
__device__ __forceinline__ T pm_pick_group(const T (&a)[PMBRL_OPT_MAX_GROUPS], int gl) {
  T r = pm_scalar(a[0]);
#pragma unroll
  for (int k = 1; k < PMBRL_OPT_MAX_GROUPS; ++k) r = gl == k ? pm_scalar(a[k]) : r;
  return r;
}
template <bool VMAX>
struct AdamTable : OptRuleDev {
  static constexpr bool kVmax = VMAX;
  __device__ __forceinline__ AdamLane prepare(int lane, const long long* step) const {
    const int gl = lane & (PMBRL_OPT_MAX_GROUPS - 1);
    AdamLane L{pm_pick_group(b1, gl),   pm_pick_group(b2, gl),        pm_pick_group(omb1, gl),
               pm_pick_group(omb2, gl), pm_pick_group(eps, gl),       pm_pick_group(wd, gl),
               pm_pick_group(decay, gl), pm_pick_group(sgn, gl),      pm_pick_group(step_size, gl),
               pm_pick_group(bc2_sqrt, gl), pm_pick_group(amsgrad, gl)};
    if (step) {
      // guarded form: the bias corrections of the device-side step counter, as AdamPlain forms them
      const double st = (double)step[0];
      const double bc1_d = -expm1(st * pm_pick_group(ln_b1, gl));
      L.bc2_sqrt = (float)sqrt(-expm1(st * pm_pick_group(ln_b2, gl)));
      L.step_size = (float)(pm_pick_group(lr_d, gl) / bc1_d);
    }
    return L;
  }
  __device__ __forceinline__ AdamLane at(const AdamLane& L, long long j, long long n) const {
    // the element's segment (every lane takes part in the shuffles: beyond n the last element's)
    const long long jc = min(j, n - 1);
    // (three walks by the number of segments, chosen by a scalar branch: none for one segment, 7 boundaries for up to 8
    //  -- weights / biases groups of a three-layer network are 6 segments -- and all 31 beyond.  Measured at n = 550 416,
    //  where the launch is no longer launch-bound: all 31 comparisons for every rule were 13 us of a 21.6 us launch with
    //  one group; a walk that leaves at the rule's last boundary, one branch per boundary, took 50 us for 32 segments)
    int grp = seg_group[0];
    if (n_segments > 8) {
#pragma unroll
      for (int q = 1; q < PMBRL_OPT_MAX_SEGMENTS; ++q)
        if (q < n_segments && jc >= seg_end[q - 1]) grp = seg_group[q];
    } else if (n_segments > 1) {
#pragma unroll
      for (int q = 1; q < 8; ++q)
        if (q < n_segments && jc >= seg_end[q - 1]) grp = seg_group[q];
    }
    // (one group: every lane holds its record -- the unused slots repeat group 0)
    if (n_groups <= 1) return L;
    return AdamLane{__shfl(L.b1, grp),   __shfl(L.b2, grp),        __shfl(L.omb1, grp),
                    __shfl(L.omb2, grp), __shfl(L.eps, grp),       __shfl(L.wd, grp),
                    __shfl(L.decay, grp), __shfl(L.sgn, grp),      __shfl(L.step_size, grp),
                    __shfl(L.bc2_sqrt, grp), __shfl(L.ams, grp)};
  }
  // (a wave leaves the loop as a whole -- its first lane's index decides: the shuffles above read the group records from
  //  lanes 0 .. 7, which must still be there when only some lanes have elements left)
  __device__ __forceinline__ bool done(long long i, int lane, long long n) const { return i - lane >= n; }
};

template <class RULE>
__global__ __launch_bounds__(256) void pm_clip_adam_kernel(float* __restrict__ p, float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           long long n, int n_part, float max_norm,
                                                           float* __restrict__ norm_out,
                                                           const long long* __restrict__ step, int guarded,
                                                           float* __restrict__ loss_out, int n_loss_part,
                                                           const RULE R) {
  // The first four elements of this thread (amsgrad's running maximum where the rule has one) and the norm's partial sums
  // are requested before anything is decided: as "go? -> step counter -> partial sums (a loop of dependent loads) ->
  // elements (a loop of four)" this launch was ten memory round trips in a row around a few hundred instructions.
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float gq[4], mq[4], vq[4], pq[4], xq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    // (beyond n: the last element's address, never used -- loads under a condition are waited for one by one)
    const long long j = min(i0 + u * stride, n - 1);
    gq[u] = g[j];
    mq[u] = m[j];
    vq[u] = v[j];
    pq[u] = p[j];
    if constexpr (RULE::kVmax) xq[u] = R.vmax[j];
  }
  const int lane = threadIdx.x & 63;
  double part[4];
  pm_norm_request(part, lane, n_part);
  // (the go flag with them: read where it is tested, its round trip sat between the rule's scalar loads and the exit)
  const int go = g_adam_go;
  // (taken or not, the step's loss is reported)
  if (loss_out && blockIdx.x == 0 && threadIdx.x >= 64 && threadIdx.x < 128) {
    const double ls = pm_loss_sum(lane, n_loss_part);
    if (lane == 0) loss_out[0] = (float)ls;
  }
  if (guarded && !go) return;   // the rollout failed: leave parameters and moments alone
  const AdamLane L = R.prepare(lane, step);
  const float norm = (float)sqrt(pm_norm_sum(part, lane, n_part));
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) norm_out[0] = norm;
  float coef = 1.f;
  if (max_norm > 0.f) coef = fminf(max_norm / (norm + 1e-6f), 1.f);
  for (long long i = i0;;) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long j = i + u * stride;
      const AdamLane E = R.at(L, j, n);
      if (j < n) {
        const float gi = gq[u] * coef;
        const float pd = pq[u] * E.decay;
        float gs = gi * E.sgn;
        if (E.wd != 0.f) gs = fmaf(E.wd, pd, gs);
        const float mi = mq[u] * E.b1 + E.omb1 * gs;
        const float vi = vq[u] * E.b2 + E.omb2 * gs * gs;
        float dv = vi;
        if constexpr (RULE::kVmax) {
          if (E.ams) {
            dv = fmaxf(xq[u], vi);
            R.vmax[j] = dv;
          }
        }
        const float denom = sqrtf(dv) / E.bc2_sqrt + E.eps;
        g[j] = gi;
        m[j] = mi;
        v[j] = vi;
        p[j] = pd - E.step_size * (mi / denom);
      }
    }
    i += 4 * stride;
    if (R.done(i, lane, n)) break;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long j = min(i + u * stride, n - 1);
      gq[u] = g[j];
      mq[u] = m[j];
      vq[u] = v[j];
      pq[u] = p[j];
      if constexpr (RULE::kVmax) xq[u] = R.vmax[j];
    }
  }
}

const char* pm_opt_rule_refusal(const pmbrl_opt_rule* r, int64_t n) {
  if (!r) return "pmbrl_opt_rule: null rule";
  if (n < 1) return "pmbrl_opt_rule: n < 1";
  if (r->n_groups < 1 || r->n_groups > PMBRL_OPT_MAX_GROUPS) return "pmbrl_opt_rule: n_groups outside 1 .. PMBRL_OPT_MAX_GROUPS";
  if (r->n_segments < 1 || r->n_segments > PMBRL_OPT_MAX_SEGMENTS)
    return "pmbrl_opt_rule: n_segments outside 1 .. PMBRL_OPT_MAX_SEGMENTS";
  bool ams = false;
  for (int k = 0; k < r->n_groups; ++k) {
    const pmbrl_opt_group& G = r->group[k];
    if (!(G.lr >= 0.0) || !std::isfinite(G.lr)) return "pmbrl_opt_rule: lr < 0";
    if (!(G.beta1 >= 0.0 && G.beta1 < 1.0) || !(G.beta2 >= 0.0 && G.beta2 < 1.0)) return "pmbrl_opt_rule: a beta outside [0, 1)";
    if (!(G.eps >= 0.0) || !std::isfinite(G.eps)) return "pmbrl_opt_rule: eps < 0";
    if (!(G.weight_decay >= 0.0) || !std::isfinite(G.weight_decay)) return "pmbrl_opt_rule: weight_decay < 0";
    if (G.flags & ~(PMBRL_OPT_DECOUPLED | PMBRL_OPT_AMSGRAD | PMBRL_OPT_MAXIMIZE)) return "pmbrl_opt_rule: unknown flag bits";
    ams = ams || (G.flags & PMBRL_OPT_AMSGRAD);
  }
  int64_t prev = 0;
  for (int q = 0; q < r->n_segments; ++q) {
    if (r->seg_end[q] <= prev) return "pmbrl_opt_rule: seg_end does not ascend";
    prev = r->seg_end[q];
    if (r->seg_group[q] < 0 || r->seg_group[q] >= r->n_groups) return "pmbrl_opt_rule: seg_group outside the groups";
  }
  if (prev != n) return "pmbrl_opt_rule: the last seg_end is not n";
  if (ams && !r->max_exp_avg_sq_d) return "pmbrl_opt_rule: AMSGRAD without max_exp_avg_sq_d";
  return nullptr;
}
extern "C" int pmbrl_opt_rule_check(const pmbrl_opt_rule* rule, int64_t n) {
  const char* why = pm_opt_rule_refusal(rule, n);
  return why ? fail(-2, why) : 0;
}

// the rule as the kernel takes it; step > 0: the host's step count (bias corrections as pmbrl_clip_adam forms them), 0: the
// device-side counter's (formed in the kernel)
static OptRuleDev opt_rule_dev(const pmbrl_opt_rule& r, long long step) {
  OptRuleDev D;
  D.n_segments = r.n_segments;
  D.n_groups = r.n_groups;
  for (int q = 0; q < PMBRL_OPT_MAX_SEGMENTS; ++q) {
    const int qq = std::min(q, r.n_segments - 1);
    D.seg_end[q] = r.seg_end[qq];
    D.seg_group[q] = r.seg_group[qq];
  }
  for (int k = 0; k < PMBRL_OPT_MAX_GROUPS; ++k) {
    const pmbrl_opt_group& G = r.group[k < r.n_groups ? k : 0];
    const OptGroupConsts c = pm_opt_group_consts(G);
    D.b1[k] = (float)G.beta1; D.b2[k] = (float)G.beta2;
    D.omb1[k] = (float)(1.0 - G.beta1); D.omb2[k] = (float)(1.0 - G.beta2);
    D.eps[k] = (float)G.eps;
    D.wd[k] = c.wd; D.decay[k] = c.decay; D.sgn[k] = c.sgn; D.amsgrad[k] = c.ams;
    D.ln_b1[k] = c.ln_b1; D.ln_b2[k] = c.ln_b2; D.lr_d[k] = G.lr;
    D.step_size[k] = D.bc2_sqrt[k] = 1.f;
    if (step > 0) {
      const float bc1 = (float)(1.0 - pow(G.beta1, (double)step));
      D.step_size[k] = (float)(G.lr / (double)bc1);
      D.bc2_sqrt[k] = (float)sqrt(1.0 - pow(G.beta2, (double)step));
    }
  }
  bool ams = false;
  for (int k = 0; k < r.n_groups; ++k) ams = ams || (r.group[k].flags & PMBRL_OPT_AMSGRAD);
  D.vmax = ams ? r.max_exp_avg_sq_d : nullptr;    // (no group asks for it: the instance without the stream)
  return D;
}

void launch_weighted_sum(hipStream_t s, const float* a, const float* w, long long n, float* out, const int* nvalid,
                                long long n_per_step) {
  const int nb = (int)std::max<long long>(1, std::min<long long>(PM_RED_MAXB, (n + 2047) / 2048));
  hipLaunchKernelGGL(pm_weighted_sum_kernel, dim3(nb), dim3(256), 0, s, a, w, n, out, nvalid, n_per_step);
}

// The optimiser step of an AdamStep (pmbrl_host.h): the only place that launches pm_gradnorm_kernel for it and
// pm_clip_adam_kernel.  The norm's launch: a guarded step always needs it (it takes the decision) unless the caller says
// both are done; an unguarded one has nothing for it to do without clipping and without a norm to report.
int pm_adam_launch(hipStream_t s, const AdamStep& A) {
  const int guarded = A.step_d ? 1 : 0;
  const int nb = (int)std::max<long long>(1, std::min<long long>(PM_RED_MAXB, (A.n + 1023) / 1024));
  const int np = pm_norm_blocks(A.n);
  const bool need_norm = guarded ? !A.norm_done : (A.max_norm > 0.0 || A.norm_out != nullptr);
  long long* const step_d = reinterpret_cast<long long*>(A.step_d);
  if (need_norm)
    hipLaunchKernelGGL(pm_gradnorm_kernel, dim3(np), dim3(64), 0, s, A.grads, (long long)A.n, (const int*)A.status,
                       (int)A.expect, step_d, guarded);
  const int n_part = guarded || need_norm ? np : 0;
  auto launch = [&](const auto& R) {
    hipLaunchKernelGGL(pm_clip_adam_kernel<std::decay_t<decltype(R)>>, dim3(nb), dim3(256), 0, s, A.params, A.grads, A.exp_avg,
                       A.exp_avg_sq, (long long)A.n, n_part, (float)A.max_norm, A.norm_out, (const long long*)step_d, guarded,
                       A.loss_out, A.n_loss_part, R);
  };
  if (A.rule) {
    const OptRuleDev D = opt_rule_dev(*A.rule, guarded ? 0 : (long long)A.step);
    if (D.vmax) launch(AdamTable<true>{D});
    else launch(AdamTable<false>{D});
  } else {
    AdamPlain P;
    P.b1 = (float)A.beta1; P.b2 = (float)A.beta2;
    P.omb1 = (float)(1.0 - A.beta1); P.omb2 = (float)(1.0 - A.beta2);
    P.eps = (float)A.eps;
    P.bc1 = P.bc2_sqrt = 1.f;
    if (!guarded) {
      P.bc1 = (float)(1.0 - pow(A.beta1, (double)A.step));
      P.bc2_sqrt = (float)sqrt(1.0 - pow(A.beta2, (double)A.step));
    }
    P.ln_b1 = log(A.beta1); P.ln_b2 = log(A.beta2); P.lr_d = A.lr;
    launch(P);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// the fused iteration tail on a sharded run (pmbrl_plan_set_grad_comm): what pmbrl_rollout_bwd_adam queues around the
// in-place sum of [flat gradient | loss partial | failure flag] over the ranks
// ---------------------------------------------------------------------------
// horizon agreement, 1: this rank's valid steps as entry `rank` of a vector the transport sums (both transports only sum)
__global__ __launch_bounds__(64) void pm_tail_hvec_kernel(float* __restrict__ hvec, int world, int rank,
                                                          const int* __restrict__ status, int H) {
  for (int q = threadIdx.x; q < world; q += blockDim.x) hvec[q] = q == rank ? (float)min(max(status[0], 0), H) : 0.f;
}
// 2: the ranks' minimum, written where it is smaller than what this rank's forward sweep left (a rank whose exchange
// timed out holds zeros for its peers: no step is valid, nothing is stepped)
__global__ __launch_bounds__(64) void pm_tail_hmin_kernel(const float* __restrict__ hvec, int world,
                                                          int* __restrict__ status, int H) {
  if (threadIdx.x != 0) return;
  int m = H;
  for (int q = 0; q < world; ++q) m = min(m, (int)hvec[q]);
  if (m < min(status[0], H)) status[0] = m;
}
// behind the gradient reduction: this rank's loss (the reduction's partial sums in workgroup order, as
// pm_clip_adam_kernel adds them; n_loss_part = 0: already in xb[n], or not asked for) and failure flag next to the gradient
__global__ __launch_bounds__(64) void pm_tail_pack_kernel(float* __restrict__ xb, int n, int n_loss_part, int loss_here,
                                                          const int* __restrict__ status, const int* __restrict__ err) {
  const int lane = threadIdx.x;
  if (n_loss_part > 0) {
    const double ls = pm_loss_sum(lane, n_loss_part);
    if (lane == 0) xb[n] = (float)ls;
  } else if (!loss_here && lane == 0) {
    xb[n] = 0.f;
  }
  if (lane == 0) xb[n + 1] = (status[1] != 0 || (err && *err != 0)) ? 1.f : 0.f;
}
// behind the exchange: the summed gradient into the caller's vector, the partial sums of ITS squares (pm_gradnorm_kernel's
// blocks: the separate calls' norm bit for bit), the summed loss where pm_clip_adam_kernel looks for it, and the decision
__global__ __launch_bounds__(64) void pm_tail_finish_kernel(const float* __restrict__ xb, float* __restrict__ g, long long n,
                                                            int* __restrict__ status, int expect,
                                                            long long* __restrict__ step, const int* __restrict__ err) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // a failure anywhere is a failure everywhere: the host reads it one iteration late.  (A wait of THIS rank that timed
    // out in the exchange just now is not in the sum -- the flag was packed before it: this rank says so in its own
    // status word, the others learn it from the sticky error word in the next exchange.)
    const int bad = (xb[n + 1] != 0.f || (err && *err != 0)) ? 1 : 0;
    if (bad) status[1] = 1;
    pm_adam_decide(status, expect, step);
    g_loss_part[0] = (double)xb[n];
  }
  pm_norm_walk<true>(xb, g, n);
}

// the launches of the kernels above that the rollout adjoint call and the BNN step queue (pmbrl_host.h)
void pm_dw_reduce_launch(hipStream_t s, const float* part, int nsplit, int n, int stride, float* grad, const int* nvalid,
                         int chunks_per_step, int chunks_per_split, int norm_on, const int* status, int expect, long long* step,
                         const float* loss_r, const float* loss_w, long long loss_n, long long loss_per_step, int col_lo,
                         int col_hi, int rows_in_range) {
  hipLaunchKernelGGL(pm_dw_reduce, dim3((n + 255) / 256), dim3(512), 0, s, part, nsplit, n, stride, grad, nvalid,
                     chunks_per_step, chunks_per_split, norm_on, status, expect, step, loss_r, loss_w, loss_n, loss_per_step,
                     col_lo, col_hi, rows_in_range);
}
void pm_tail_hvec_launch(hipStream_t s, float* hvec, int world, int rank, const int* status, int H) {
  hipLaunchKernelGGL(pm_tail_hvec_kernel, dim3(1), dim3(64), 0, s, hvec, world, rank, status, H);
}
void pm_tail_hmin_launch(hipStream_t s, const float* hvec, int world, int* status, int H) {
  hipLaunchKernelGGL(pm_tail_hmin_kernel, dim3(1), dim3(64), 0, s, hvec, world, status, H);
}
void pm_tail_pack_launch(hipStream_t s, float* xb, int n, int n_loss_part, int loss_here, const int* status, const int* err) {
  hipLaunchKernelGGL(pm_tail_pack_kernel, dim3(1), dim3(64), 0, s, xb, n, n_loss_part, loss_here, status, err);
}
void pm_tail_finish_launch(hipStream_t s, const float* xb, float* g, long long n, int* status, int expect, long long* step,
                           const int* err) {
  hipLaunchKernelGGL(pm_tail_finish_kernel, dim3(pm_norm_blocks(n)), dim3(64), 0, s, xb, g, n, status, expect, step, err);
}

extern "C" int pmbrl_pack_mask(void* stream, const float* mask_d, int32_t B, int32_t h,
                               int32_t src_ld, uint16_t* bits_d) {
  if (!mask_d || !bits_d || B < 1 || h < 1 || src_ld < h) return fail(-1, "bad argument");
  const int nt = (h + 15) / 16;
  const int n = B * nt;
  hipLaunchKernelGGL(pm_pack_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     mask_d, B, h, src_ld, bits_d);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int pmbrl_draw_masks(void* stream, int32_t kind, uint64_t seed, uint64_t offset, const float* param_d,
                                int32_t param_len, float temp, int32_t rows, int32_t h, const float* u_d, const float* v_d,
                                uint16_t* bits_d, int32_t aux_row0, int32_t aux_rows, float* u_out_d, float* hard_out_d,
                                float* probs_out_d) {
  if (!param_d || !bits_d || rows < 1 || h < 1 || (kind != 0 && kind != 1) || (param_len != 1 && param_len != h) ||
      aux_row0 < 0 || aux_rows < 0 || aux_row0 + aux_rows > rows)
    return fail(-1, "bad argument");
  if (kind == 1 && !(temp > 0.f)) return fail(-1, "concrete dropout needs a positive temperature");
  DrawArgs A;
  A.kind = kind; A.seed = seed; A.offset = offset; A.param = param_d; A.param_len = param_len; A.temp = temp;
  A.rows = rows; A.h = h; A.u_in = u_d; A.v_in = v_d; A.bits = bits_d;
  A.aux_row0 = aux_row0; A.aux_rows = aux_rows; A.u_out = u_out_d; A.hard_out = hard_out_d; A.probs_out = probs_out_d;
  const long long n = (long long)rows * ((h + 15) / 16);
  hipLaunchKernelGGL(pm_draw_masks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int pmbrl_weighted_sum(void* stream, const float* a_d, const float* w_d, int64_t n,
                                  float* out_d) {
  if (!a_d || !w_d || !out_d || n < 0) return fail(-1, "bad argument");
  launch_weighted_sum((hipStream_t)stream, a_d, w_d, n, out_d, nullptr, 0);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int pmbrl_weighted_sum_steps(void* stream, const float* a_d, const float* w_d, int64_t n_per_step,
                                        int32_t n_steps, const int32_t* status_d, float* out_d) {
  if (!a_d || !w_d || !out_d || n_per_step < 0 || n_steps < 0) return fail(-1, "bad argument");
  launch_weighted_sum((hipStream_t)stream, a_d, w_d, (long long)n_per_step * n_steps, out_d, status_d, n_per_step);
  HIPCHK(hipGetLastError());
  return 0;
}

// the four stand-alone optimiser calls: argument checks and an AdamStep
static AdamStep adam_step_on(float* params_d, float* grads_d, float* exp_avg_d, float* exp_avg_sq_d, int64_t n, double max_norm,
                             float* norm_out_d) {
  AdamStep A;
  A.params = params_d; A.grads = grads_d; A.exp_avg = exp_avg_d; A.exp_avg_sq = exp_avg_sq_d; A.n = n;
  A.max_norm = max_norm; A.norm_out = norm_out_d;
  return A;
}
extern "C" int pmbrl_clip_adam(void* stream, float* params_d, float* grads_d, float* exp_avg_d,
                               float* exp_avg_sq_d, int64_t n, int64_t step, double lr, double beta1,
                               double beta2, double eps, double max_norm, float* norm_out_d) {
  if (!params_d || !grads_d || !exp_avg_d || !exp_avg_sq_d || n < 1 || step < 1)
    return fail(-1, "bad argument");
  AdamStep A = adam_step_on(params_d, grads_d, exp_avg_d, exp_avg_sq_d, n, max_norm, norm_out_d);
  A.step = step;
  A.lr = lr; A.beta1 = beta1; A.beta2 = beta2; A.eps = eps;
  return pm_adam_launch((hipStream_t)stream, A);
}

extern "C" int pmbrl_clip_adam_guarded(void* stream, float* params_d, float* grads_d, float* exp_avg_d,
                                       float* exp_avg_sq_d, int64_t n, int64_t* step_d, double lr,
                                       double beta1, double beta2, double eps, double max_norm,
                                       float* norm_out_d, const int32_t* status_d, int32_t expect) {
  if (!params_d || !grads_d || !exp_avg_d || !exp_avg_sq_d || !step_d || !status_d || n < 1)
    return fail(-1, "bad argument");
  AdamStep A = adam_step_on(params_d, grads_d, exp_avg_d, exp_avg_sq_d, n, max_norm, norm_out_d);
  A.step_d = step_d; A.status = status_d; A.expect = expect;
  A.lr = lr; A.beta1 = beta1; A.beta2 = beta2; A.eps = eps;
  return pm_adam_launch((hipStream_t)stream, A);
}

extern "C" int pmbrl_clip_adam_rule(void* stream, float* params_d, float* grads_d, float* exp_avg_d, float* exp_avg_sq_d,
                                    int64_t n, int64_t step, double max_norm, float* norm_out_d, const pmbrl_opt_rule* rule) {
  if (!params_d || !grads_d || !exp_avg_d || !exp_avg_sq_d || n < 1 || step < 1) return fail(-1, "bad argument");
  if (int rc = pmbrl_opt_rule_check(rule, n)) return rc;
  AdamStep A = adam_step_on(params_d, grads_d, exp_avg_d, exp_avg_sq_d, n, max_norm, norm_out_d);
  A.step = step;
  A.rule = rule;
  return pm_adam_launch((hipStream_t)stream, A);
}

extern "C" int pmbrl_clip_adam_rule_guarded(void* stream, float* params_d, float* grads_d, float* exp_avg_d,
                                            float* exp_avg_sq_d, int64_t n, int64_t* step_d, double max_norm,
                                            float* norm_out_d, const int32_t* status_d, int32_t expect,
                                            const pmbrl_opt_rule* rule) {
  if (!params_d || !grads_d || !exp_avg_d || !exp_avg_sq_d || !step_d || !status_d || n < 1)
    return fail(-1, "bad argument");
  if (int rc = pmbrl_opt_rule_check(rule, n)) return rc;
  AdamStep A = adam_step_on(params_d, grads_d, exp_avg_d, exp_avg_sq_d, n, max_norm, norm_out_d);
  A.step_d = step_d; A.status = status_d; A.expect = expect;
  A.rule = rule;
  return pm_adam_launch((hipStream_t)stream, A);
}
