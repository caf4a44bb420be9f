// The ingest launch of a reward evaluated by the caller (PMBRL_REWARD_EXTERNAL, pmbrl_rollout_rewards): what the analytic
// reward launch (pmbrl_reward.h) leaves behind, from the caller's values instead of its own arithmetic.
//   r  [H][B]     -> rt (rewards are moment-matched afterwards) or rewards
//   jx [H][B][D]  -> Jx, ja [H][B][U] -> Ja, where every family's adjoint sweep reads them (both, or neither: forward only)
//   the first step with a non-finite sampled state, reward or Jacobian entry -> atomicMin(status[0], t)
//   status[1] (the adjoint call's failure flag) cleared
// Nothing here walks a row: every array is a flat copy, so a thread takes ELEMENTS -- consecutive lanes consecutive
// addresses, 16 bytes per lane where the arrays allow it, four loads in flight per array -- and the step of an element is
// its index divided by the elements per step.  A non-finite entry is rare: the wave votes, and only a wave that saw one
// reduces its smallest step over the lanes and sends ONE atomic.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "pmbrl_host.h"

#define PM_RX_NT 256
#define PM_RX_FLIGHT 4
#define PM_RX_MAX_BLOCKS 1024

struct RewardExtLaunch {
  RewardExtArgs a;
  int vec_r, vec_x, vec_a;   // the pass moves float4s (every pointer of it 16-byte aligned, a multiple of 4 elements)
};

template <int V> struct RxVec;
template <> struct RxVec<1> {
  typedef float T;
  static __device__ __forceinline__ float get(const float& v, int) { return v; }
  static __device__ __forceinline__ float zero() { return 0.f; }
};
template <> struct RxVec<4> {
  typedef float4 T;
  static __device__ __forceinline__ float get(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
  static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};

// One pass over n elements, per_step of them per time step: dst = src where both are given, src and chk (either may be
// null) checked for non-finite entries.  Every wave runs whole -- a lane beyond the end takes clamped loads and stores
// nothing -- so the vote and the reduction below see 64 lanes.
template <int V>
__device__ __forceinline__ void pm_rx_pass(const float* __restrict__ src, float* __restrict__ dst,
                                           const float* __restrict__ chk, long long n, long long per_step, int* status) {
  typedef typename RxVec<V>::T vec_t;
  const long long nv = n / V;
  const long long stride = (long long)gridDim.x * PM_RX_NT;
  const int lane = threadIdx.x & 63;
  const vec_t* sv = reinterpret_cast<const vec_t*>(src);
  const vec_t* cv = reinterpret_cast<const vec_t*>(chk);
  vec_t* dv = reinterpret_cast<vec_t*>(dst);
  for (long long i0 = (long long)blockIdx.x * PM_RX_NT + threadIdx.x; i0 - lane < nv; i0 += PM_RX_FLIGHT * stride) {
    vec_t a[PM_RX_FLIGHT], c[PM_RX_FLIGHT];
#pragma unroll
    for (int u = 0; u < PM_RX_FLIGHT; ++u) {
      const long long i = min(i0 + u * stride, nv - 1);
      a[u] = src ? sv[i] : RxVec<V>::zero();
      c[u] = chk ? cv[i] : RxVec<V>::zero();
    }
    int tbad = INT_MAX;      // (descending: what is left is the step of the lane's FIRST bad element)
#pragma unroll
    for (int u = PM_RX_FLIGHT - 1; u >= 0; --u) {
      const long long i = i0 + u * stride;
      if (i < nv) {
        if (dst && src) dv[i] = a[u];
#pragma unroll
        for (int j = V - 1; j >= 0; --j)
          if (!isfinite(RxVec<V>::get(a[u], j)) || !isfinite(RxVec<V>::get(c[u], j))) tbad = (int)((i * V + j) / per_step);
      }
    }
    if (__ballot(tbad != INT_MAX)) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) tbad = min(tbad, __shfl_xor(tbad, m));
      if (lane == 0) atomicMin(status, tbad);
    }
  }
}

__global__ __launch_bounds__(PM_RX_NT) void pm_reward_ext_kernel(const RewardExtLaunch L) {
  const RewardExtArgs& R = L.a;
  if (blockIdx.x == 0 && threadIdx.x == 0) R.status[1] = 0;
  const long long n = (long long)R.H * R.B;
  if (L.vec_r) pm_rx_pass<4>(R.r, R.dst_r, nullptr, n, R.B, R.status);
  else pm_rx_pass<1>(R.r, R.dst_r, nullptr, n, R.B, R.status);
  if (L.vec_x) pm_rx_pass<4>(R.jx, R.Jx, R.x, n * R.D, (long long)R.B * R.D, R.status);
  else pm_rx_pass<1>(R.jx, R.Jx, R.x, n * R.D, (long long)R.B * R.D, R.status);
  if (!R.ja) return;
  if (L.vec_a) pm_rx_pass<4>(R.ja, R.Ja, nullptr, n * R.U, (long long)R.B * R.U, R.status);
  else pm_rx_pass<1>(R.ja, R.Ja, nullptr, n * R.U, (long long)R.B * R.U, R.status);
}

void pm_reward_ext_launch(const RewardExtArgs& R, hipStream_t s) {
  auto vec_ok = [](long long n, std::initializer_list<const void*> ptrs) {
    bool ok = n % 4 == 0;
    for (const void* q : ptrs) ok = ok && (reinterpret_cast<uintptr_t>(q) & 15) == 0;      // (a null pointer passes)
    return ok ? 1 : 0;
  };
  const long long n = (long long)R.H * R.B;
  RewardExtLaunch L;
  L.a = R;
  L.vec_r = vec_ok(n, {R.r, R.dst_r});
  L.vec_x = vec_ok(n * R.D, {R.jx, R.Jx, R.x});
  L.vec_a = vec_ok(n * R.U, {R.ja, R.Ja});
  // the longest pass, in the units it moves, four per thread
  long long work = n / (L.vec_r ? 4 : 1);
  work = std::max(work, n * R.D / (L.vec_x ? 4 : 1));
  if (R.ja) work = std::max(work, n * R.U / (L.vec_a ? 4 : 1));
  const long long per_block = (long long)PM_RX_NT * PM_RX_FLIGHT;
  const unsigned blocks = (unsigned)std::min<long long>(std::max<long long>((work + per_block - 1) / per_block, 1), PM_RX_MAX_BLOCKS);
  hipLaunchKernelGGL(pm_reward_ext_kernel, dim3(blocks), dim3(PM_RX_NT), 0, s, L);
}
