// libpmbrl_hip.so -- C ABI (include/pmbrl.h) over the gfx950 kernels: the rollout plan and its two calls.
// Host side: shape validation, tiling choice, workspace carve-up, launches.  (pmbrl_host.h lists the other objects.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "pmbrl_host.h"
#include "pmbrl_mm.h"
#include "pmbrl_rollout.h"
#include "pmbrl_mmx.h"
#include "pmbrl_mm_wide.h"
#include "pmbrl_fast.h"
#include "pmbrl_reward.h"

static thread_local std::string g_err;
int pm_fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" const char* pmbrl_last_error(void) { return g_err.c_str(); }
extern "C" int pmbrl_version(void) { return 8; }

// ---------------------------------------------------------------------------
// hipGraph entry points: record the library calls queued on a stream between begin and end, replay them with one
// launch.  What it is for: the forms of the sweeps that are MANY launches per call (one per step: moment-matching
// groups beyond a workgroup, wide states; pipelined adjoint) -- a plain iteration is a dozen launches the queue
// already hides.  Everything the library queues is capturable (kernel launches, memsets, the event hand-offs of the
// second stream); a host-side collective attached with pmbrl_plan_set_collective is not.  The status word, the step
// counter of the guarded Adam and every pointer are device-side, so a replay is a whole new iteration as long as the
// caller's buffers stay where they were.  (The fp16 weight-range flag of a replayed call carries the generation number
// of the capture: exact unless an eager call on the same plan reported an overflow in between.)
// ---------------------------------------------------------------------------
struct pmbrl_graph {
  hipGraph_t graph;
  hipGraphExec_t exec;
};
extern "C" int pmbrl_graph_capture_begin(void* stream) {
  if (!stream) return fail(-1, "graph capture needs a non-default stream");
  HIPCHK(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed));
  return 0;
}
extern "C" int pmbrl_graph_capture_end(void* stream, pmbrl_graph** out) {
  if (!stream || !out) return fail(-1, "null argument");
  hipGraph_t g = nullptr;
  HIPCHK(hipStreamEndCapture((hipStream_t)stream, &g));
  if (!g) return fail(-3, "stream capture ended without a graph (a call inside it invalidated the capture)");
  pmbrl_graph* r = new pmbrl_graph();
  r->graph = g;
  r->exec = nullptr;
  hipError_t e = hipGraphInstantiate(&r->exec, g, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(g);
    delete r;
    return fail(-100 - (int)e, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
  }
  *out = r;
  return 0;
}
extern "C" int pmbrl_graph_launch(pmbrl_graph* g, void* stream) {
  if (!g || !g->exec) return fail(-1, "null argument");
  HIPCHK(hipGraphLaunch(g->exec, (hipStream_t)stream));
  return 0;
}
extern "C" int pmbrl_graph_num_nodes(pmbrl_graph* g, int64_t* n_out) {
  if (!g || !n_out) return fail(-1, "null argument");
  size_t n = 0;
  HIPCHK(hipGraphGetNodes(g->graph, nullptr, &n));
  *n_out = (int64_t)n;
  return 0;
}
extern "C" void pmbrl_graph_destroy(pmbrl_graph* g) {
  if (!g) return;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  delete g;
}

// hash of the kernel sources this library was built from (Makefile: pmbrl_build_id.inc)
extern "C" const char* pmbrl_build_id(void) {
  return
#include "pmbrl_build_id.inc"
      ;
}

// ---------------------------------------------------------------------------
// small kernels: the fragment packers of the test hook (pmbrl_debug_linear, below), then those of the rollout calls
// ---------------------------------------------------------------------------
// fragment packing: dst[((ot*n_kb + kb)*64 + lane)*4 + j] = W[ot*16 + (lane&15)][kb*16 + 4*(lane>>4) + j]
// (transpose=1: the roles of the two indices of W[O][K] are swapped)
__global__ void pm_pack_frag(const float* __restrict__ W, int O, int K, int transpose, int kb_mult,
                             float* __restrict__ dst) {
  const int n_out = transpose ? K : O, n_in = transpose ? O : K;
  const int n_ot = (n_out + 15) / 16;
  const int n_kb = ((n_in + 15) / 16 + kb_mult - 1) / kb_mult * kb_mult;   // zero-padded k-blocks
  const size_t total = (size_t)n_ot * n_kb * 256;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int j = i & 3, lane = (i >> 2) & 63;
    const size_t tb = i >> 8;
    const int kb = tb % n_kb, ot = tb / n_kb;
    const int o = ot * 16 + (lane & 15);
    const int k = kb * 16 + 4 * (lane >> 4) + j;
    float v = 0.f;
    if (o < n_out && k < n_in) v = transpose ? W[(size_t)k * K + o] : W[(size_t)o * K + k];
    dst[i] = v;
  }
}
__global__ void pm_pack_bias(const float* __restrict__ b, int O, int O16, float* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < O16) dst[i] = i < O ? b[i] : 0.f;
}

// the reward launch's instance for an action width (pmbrl_reward.h)
typedef void (*pm_reward_kernel_t)(const RolloutArgs);
static inline pm_reward_kernel_t pm_reward_kernel_for(int U, int k) {
  if (k <= 2) return U <= 4 ? pm_reward_all_kernel<4, 2> : (U <= 8 ? pm_reward_all_kernel<8, 2> : pm_reward_all_kernel<16, 2>);
  return U <= 4 ? pm_reward_all_kernel<4, PMBRL_MAX_TIP>
                : (U <= 8 ? pm_reward_all_kernel<8, PMBRL_MAX_TIP> : pm_reward_all_kernel<16, PMBRL_MAX_TIP>);
}

// all weight / bias repacking of one forward call in ONE launch (blockIdx.y = job)
__global__ void pm_pack_all(const PackArgs P) {
  if (P.status && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *P.status = 0x7fffffff;
  const PackJob j = P.job[blockIdx.y];
  if (j.is_bias) {
    const int O16 = (j.O + 15) / 16 * 16;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < O16; i += gridDim.x * blockDim.x)
      j.dst[i] = i < j.O ? j.src[i] : 0.f;
    return;
  }
  const int n_out = j.transpose ? j.K : j.O, n_in = j.transpose ? j.O : j.K;
  const int n_ot = (n_out + 15) / 16;
  if (j.planes) {
    // dst[((ot*n_kb + kb)*planes + p)*64 + lane][8 bf16] = piece p of W[ot*16 + (lane&15)][kb*32 + 8*(lane>>4) + e]
    const int n_kb = ((n_in + 31) / 32 + j.mult - 1) / j.mult * j.mult;
    const size_t total = (size_t)n_ot * n_kb * 64;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
      const int lane = i & 63;
      const size_t tb = i >> 6;
      const int kb = tb % n_kb, ot = tb / n_kb;
      const int o = ot * 16 + (lane & 15);
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = kb * 32 + 8 * (lane >> 4) + e;
        v[e] = (o < n_out && k < n_in) ? (j.transpose ? j.src[(size_t)k * j.K + o] : j.src[(size_t)o * j.K + k]) : 0.f;
      }
      for (int p = 0; p < j.planes; ++p) {
        unsigned w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (j.f16) {
            if (p == 0 && P.wflag && (!(fabsf(v[2 * e]) <= 65504.f) || !(fabsf(v[2 * e + 1]) <= 65504.f)))
              atomicMax(P.wflag, P.gen);
            // (the low piece is stored scaled by 2^11: pmbrl_split.h, PM_F16_LO_SCALE)
            const float sc = p ? PM_F16_LO_SCALE : 1.f;
            w[e] = pm_pk_f16(v[2 * e] * sc, v[2 * e + 1] * sc);
            const pm_f32x2 f = pm_unpk_f16(w[e]);
            v[2 * e] -= f[0];
            v[2 * e + 1] -= f[1];
          } else {
            w[e] = pm_pk_bf16(v[2 * e], v[2 * e + 1]);
            v[2 * e] -= pm_bf_lo(w[e]);
            v[2 * e + 1] -= pm_bf_hi(w[e]);
          }
        }
        *reinterpret_cast<uint4*>(j.dst + ((tb * j.planes + p) * 64 + lane) * 4) = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    return;
  }
  const int n_kb = ((n_in + 15) / 16 + j.mult - 1) / j.mult * j.mult;
  const size_t total = (size_t)n_ot * n_kb * 256;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int jj = i & 3, lane = (i >> 2) & 63;
    const size_t tb = i >> 8;
    const int kb = tb % n_kb, ot = tb / n_kb;
    const int o = ot * 16 + (lane & 15);
    const int k = kb * 16 + 4 * (lane >> 4) + jj;
    float v = 0.f;
    if (o < n_out && k < n_in)
      v = j.transpose ? j.src[(size_t)k * j.K + o] : j.src[(size_t)o * j.K + k];
    j.dst[i] = v;
  }
}
void pm_pack_all_launch(const PackArgs& PK, hipStream_t s) { hipLaunchKernelGGL(pm_pack_all, dim3(32, PK.n), dim3(256), 0, s, PK); }


// external moment matching (groups larger than a workgroup's rows): one workgroup of PM_MM_NW
// waves per group, rows in HBM; every wave takes a slice of the rows (pmbrl_mm.h, multi-wave
// forms).  Widths without a compile-time instantiation run the general code on wave 0.
#define PM_MM_NW 16
// (widths beyond the compile-time instances -- D > 6 -- run the one-wave routine: one wave's scratch; sixteen
//  of them would be 446 KB at D = 32)
__host__ __device__ inline int pm_mm_kernel_scratch_waves(int D) { return D <= 6 ? PM_MM_NW : 1; }
__host__ __device__ inline size_t pm_mm_kernel_doubles(int D) {
  return (size_t)pm_mm_kernel_scratch_waves(D) * pm_mm_scratch_doubles(D) + (size_t)PM_MM_NW * 256;
}
#define PM_MM_MW_SWITCH(D, CALL, ELSE) \
  switch (D) {                         \
    case 1: { CALL(1); break; }        \
    case 2: { CALL(2); break; }        \
    case 3: { CALL(3); break; }        \
    case 4: { CALL(4); break; }        \
    case 5: { CALL(5); break; }        \
    case 6: { CALL(6); break; }        \
    default: { ELSE; }                 \
  }
// the noise table of split groups in a launch of its own (pmbrl_mm.h: pm_ztab_block; the register-resident family's pack
// launch forms it with extra workgroups instead)
__global__ __launch_bounds__(256) void pm_mm_ztable_kernel(const ZtabArgs Z) { pm_ztab_block(Z, (int)blockIdx.x, (int)threadIdx.x); }
static ZtabArgs pm_ztab_args(const pmbrl_plan* p, const RolloutArgs& A) {
  ZtabArgs Z;
  Z.zmm = A.zmm; Z.tab = const_cast<double*>(A.mm_ztab);
  Z.pack = (p->M <= 64 && p->cfg.D <= 8) ? 1 : 0;
  Z.H = p->cfg.H; Z.G = p->G; Z.M = p->M; Z.D = p->cfg.D; Z.Bg = A.Bg;
  Z.per_step = (A.flags & PMBRL_FLAG_ZMM_PER_STEP) ? 1 : 0;
  Z.row_off = A.row_off;
  Z.n_blocks = pm_ztab_blocks(Z.H, Z.G, Z.pack);
  return Z;
}

__global__ __launch_bounds__(PM_MM_NW * 64) void pm_mm_fwd_kernel(RolloutArgs A, int t) {
  extern __shared__ __attribute__((aligned(16))) double mmscr[];
  const int gi = blockIdx.x, lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* part = mmscr + (size_t)pm_mm_kernel_scratch_waves(A.D) * pm_mm_scratch_doubles(A.D);
  const int r0 = gi * A.M;
  const bool ins = (A.flags & PMBRL_FLAG_INFER_NS) != 0;
  const int zrow0 = pm_zrow0(t, A.row_off + r0, A.flags);
  const float* zmm = pm_zbase(A.zmm, A.D, t, A.Bg, A.flags);
  const float* zrr = pm_zbase(A.zrr, 1, t, A.Bg, A.flags);
  if (A.flags & PMBRL_FLAG_MM_STATES) {
    const float* s = A.xt + ((size_t)t * A.B + r0) * A.D;
    float* out = A.states + ((size_t)(t + 1) * A.B + r0) * A.D;
    bool ok = true;
#define PM_CALL(DD) ok = pm_mm_fwd_mw<DD>(s, A.D, A.M, zmm, A.D, zrow0, A.Bg, out, A.D, mmscr, part, PM_MM_NW, wid, lane)
    if (ins) {   // infer_noise_variables: the general single-wave routine
      if (wid == 0) ok = pm_mm_fwd(s, A.D, A.M, A.D, zmm, A.D, zrow0, A.Bg, true, out, A.D, mmscr, lane);
    } else {
      PM_MM_MW_SWITCH(A.D, PM_CALL,
                      if (wid == 0) ok = pm_mm_fwd(s, A.D, A.M, A.D, zmm, A.D, zrow0, A.Bg, false, out, A.D, mmscr, lane))
    }
#undef PM_CALL
    if (!ok && threadIdx.x == 0) atomicMin(A.status, t);
  }
  if (A.flags & PMBRL_FLAG_MM_REWARDS) {
    __syncthreads();
    bool ok = true;
    if (ins) {
      if (wid == 0) ok = pm_mm_fwd(A.rt + (size_t)t * A.B + r0, 1, A.M, 1, zrr, 1, zrow0, A.Bg, true,
                                   A.rewards + (size_t)t * A.B + r0, 1, mmscr, lane);
    } else {
      ok = pm_mm_fwd_mw<1>(A.rt + (size_t)t * A.B + r0, 1, A.M, zrr, 1, zrow0, A.Bg,
                           A.rewards + (size_t)t * A.B + r0, 1, mmscr, part, PM_MM_NW, wid, lane);
    }
    if (!ok && threadIdx.x == 0) atomicMin(A.status, t);
  }
}
// adjoint: (gx_carry = dL/dx_{t+1}, grad_rewards[t]) -> (gx_carry = dL/dx~, gr_tilde[t] = dL/dr~)
__global__ __launch_bounds__(PM_MM_NW * 64) void pm_mm_bwd_kernel(RolloutArgs A, int t, float* gr_tilde) {
  extern __shared__ __attribute__((aligned(16))) double mmscr[];
  const int gi = blockIdx.x, lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* part = mmscr + (size_t)pm_mm_kernel_scratch_waves(A.D) * pm_mm_scratch_doubles(A.D);
  const int r0 = gi * A.M;
  if (A.nvalid && t >= *A.nvalid) return;   // a step the forward sweep did not complete
  const bool ins = (A.flags & PMBRL_FLAG_INFER_NS) != 0;
  const int zrow0 = pm_zrow0(t, A.row_off + r0, A.flags);
  const float* zmm = pm_zbase(A.zmm, A.D, t, A.Bg, A.flags);
  const float* zrr = pm_zbase(A.zrr, 1, t, A.Bg, A.flags);
  if (A.flags & PMBRL_FLAG_MM_STATES) {
    float* g = A.gx_carry + (size_t)r0 * A.D;
    const float* s = A.xt + ((size_t)t * A.B + r0) * A.D;
    // in place (g -> g): every read of g happens before the first write (pmbrl_mm.h)
#define PM_CALL(DD) pm_mm_bwd_mw<DD>(s, A.D, A.M, zmm, A.D, zrow0, A.Bg, g, A.D, g, A.D, mmscr, part, PM_MM_NW, wid, lane)
    if (ins) {
      if (wid == 0) pm_mm_bwd(s, A.D, A.M, A.D, zmm, A.D, zrow0, A.Bg, true, g, A.D, g, A.D, mmscr, lane);
    } else {
      PM_MM_MW_SWITCH(A.D, PM_CALL,
                      if (wid == 0) pm_mm_bwd(s, A.D, A.M, A.D, zmm, A.D, zrow0, A.Bg, false, g, A.D, g, A.D, mmscr, lane))
    }
#undef PM_CALL
  }
  const float* gsrc = A.grad_rewards + (size_t)t * A.B + r0;
  float* gdst = gr_tilde + (size_t)t * A.B + r0;
  if (A.flags & PMBRL_FLAG_MM_REWARDS) {
    __syncthreads();
    if (ins) {
      if (wid == 0) pm_mm_bwd(A.rt + (size_t)t * A.B + r0, 1, A.M, 1, zrr, 1, zrow0, A.Bg, true, gsrc, 1, gdst, 1, mmscr, lane);
    } else {
      pm_mm_bwd_mw<1>(A.rt + (size_t)t * A.B + r0, 1, A.M, zrr, 1, zrow0, A.Bg, gsrc, 1, gdst, 1, mmscr, part,
                      PM_MM_NW, wid, lane);
    }
  } else {
    for (int i = threadIdx.x; i < A.M; i += PM_MM_NW * 64) gdst[i] = gsrc[i];
  }
}

// wide states (6 < D <= 32), rows of a group staged in LDS (pmbrl_mm_wide.h); the forward leaves the factor block of
// (step, group) in fac_all for the adjoint
__global__ __launch_bounds__(PM_MMW_NT) void pm_mmw_fwd_kernel(RolloutArgs A, int t, double* fac_all) {
  extern __shared__ __attribute__((aligned(16))) double mmscr[];
  const int gi = blockIdx.x, r0 = gi * A.M;
  const int zrow0 = pm_zrow0(t, A.row_off + r0, A.flags);
  const float* zmm = pm_zbase(A.zmm, A.D, t, A.Bg, A.flags);
  const float* s = A.xt + ((size_t)t * A.B + r0) * A.D;
  float* out = A.states + ((size_t)(t + 1) * A.B + r0) * A.D;
  double* fac = fac_all + ((size_t)t * gridDim.x + gi) * pm_mmw_fac_doubles(A.D);
  const bool ok = pm_mmw_fwd(s, A.M, A.D, zmm, zrow0, A.Bg, out, fac, mmscr,
                             (A.prof && gi == 0) ? A.prof + (size_t)t * 32 : nullptr);
  if (!ok && threadIdx.x == 0) atomicMin(A.status, t);
}
__global__ __launch_bounds__(PM_MMW_NT) void pm_mmw_bwd_kernel(RolloutArgs A, int t, const double* fac_all) {
  extern __shared__ __attribute__((aligned(16))) double mmscr[];
  const int gi = blockIdx.x, r0 = gi * A.M;
  if (A.nvalid && t >= *A.nvalid) return;   // a step the forward sweep did not complete
  const int zrow0 = pm_zrow0(t, A.row_off + r0, A.flags);
  const float* zmm = pm_zbase(A.zmm, A.D, t, A.Bg, A.flags);
  const float* s = A.xt + ((size_t)t * A.B + r0) * A.D;
  float* g = A.gx_carry + (size_t)r0 * A.D;
  const double* fac = fac_all + ((size_t)t * gridDim.x + gi) * pm_mmw_fac_doubles(A.D);
  pm_mmw_bwd(s, A.M, A.D, zmm, zrow0, A.Bg, g, g, fac, mmscr);
}

// ---------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------
static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

const char* pm_act_refusal(int32_t act, int n_hidden) {
  if (n_hidden < 0 || n_hidden > PM_MAXL - 1) return "activation: n_hidden outside 0 .. PMBRL_MAX_LAYERS - 1";
  if (act < 0) return "unknown activation (a negative value)";
  if (!(act & PMBRL_ACT_PER_LAYER)) {
    // (the plain form stays what it was, three values; whatever it refused before it still refuses)
    if (act > PMBRL_ACT_SILU)
      return "unknown activation (PMBRL_ACT_RELU, PMBRL_ACT_TANH, PMBRL_ACT_SILU for every hidden layer, or "
             "PMBRL_ACT_PER_LAYER with one code PMBRL_ACT_RELU .. PMBRL_ACT_NONE per hidden layer, are offered)";
    return nullptr;
  }
  const int32_t codes = act & ~PMBRL_ACT_PER_LAYER;
  if (codes >> (3 * (PM_MAXL - 1))) return "activation: stray bits above the per-layer codes";
  if (codes >> (3 * n_hidden)) return "activation: a code for a hidden layer the network does not have";
  return nullptr;
}
extern "C" int pmbrl_act_check(int32_t act, int32_t n_hidden) {
  const char* why = pm_act_refusal(act, n_hidden);
  return why ? fail(-2, why) : 0;
}

static int net_plan(const pmbrl_mlp& m, int act, NetPlan& n, int in_expect, int out_expect,
                    const char* name) {
  if (m.n_layers < 1 || m.n_layers > PM_MAXL)
    return fail(-2, std::string(name) + ": n_layers out of range");
  n.nl = m.n_layers;
  size_t off = 0;
  for (int i = 0; i <= n.nl; ++i) {
    if (m.dims[i] < 1 || m.dims[i] > 4096) return fail(-2, std::string(name) + ": bad layer width");
    n.dim[i] = m.dims[i];
    n.nt[i] = (m.dims[i] + 15) / 16;
  }
  if (n.dim[0] != in_expect || n.dim[n.nl] != out_expect)
    return fail(-2, std::string(name) + ": input/output width does not match D/U");
  if (const char* why = pm_act_refusal(act, n.nl - 1)) return fail(-2, std::string(name) + ": " + why);
  n.act = pm_act_layers(act, n.nl - 1);
  for (int l = 0; l < n.nl; ++l) {
    n.keep[l] = (l < n.nl - 1) ? m.keep[l] : 1.f;
    if (l < n.nl - 1 && !(n.keep[l] > 0.f)) return fail(-2, std::string(name) + ": keep must be > 0");
    n.w_off[l] = off;
    off += (size_t)n.dim[l + 1] * n.dim[l];
    n.b_off[l] = off;
    off += n.dim[l + 1];
  }
  n.n_params = off;
  return 0;
}

// the general family in exact fp32: the instantiations of PM_GENERAL_F32_INSTANCES
#define PM_INST(RT, CA, CB, VAR, D, U, LD, NL, NT, TREE) \
  {reinterpret_cast<const void*>(&pm_rollout_fwd<RT>), reinterpret_cast<const void*>(&pm_rollout_bwd<RT>)},
static const PmInst general_f32_fns[] = {PM_GENERAL_F32_INSTANCES};
#undef PM_INST
static_assert(sizeof(general_f32_fns) / sizeof(general_f32_fns[0]) == pm_general_f32_n, "one kernel pair per key");

// ---------------------------------------------------------------------------
// plan creation: pmbrl_plan_create runs the stages below in order; each one fills its part of the plan from the
// configuration, the switches and what the stages before it chose
// ---------------------------------------------------------------------------
static constexpr size_t PM_LDS_CAP = 160 * 1024;

static bool env_set(const char* name) { return getenv(name) != nullptr; }
static bool env_on(const char* name) {      // unset, or a number other than 0
  const char* e = getenv(name);
  return !(e && atoi(e) == 0);
}
static PlanSwitches read_switches() {
  PlanSwitches s{};
  s.mm_perstep = env_set("PMBRL_MM_PERSTEP");
  s.mm_mode2 = env_set("PMBRL_MM_MODE2");
  s.mm_no_batch = env_set("PMBRL_MM_NO_BATCH");
  s.dw_no_wide = env_set("PMBRL_DW_NO_WIDE");
  s.reg_debug = env_set("PMBRL_REG_DEBUG");
  s.lds_tiles = env_on("PMBRL_LDS_TILES");
  s.mm_xch = env_on("PMBRL_MM_XCH");
  s.mm_tree = env_on("PMBRL_MM_TREE");
  s.reg = env_on("PMBRL_REG");
  s.reg_mm = env_on("PMBRL_REG_MM");
  s.reg_tree = env_on("PMBRL_REG_TREE");
  s.reg_bwd = env_on("PMBRL_REG_BWD");
  s.fuse_loss = env_on("PMBRL_FUSE_LOSS");
  s.ztab_merge = env_on("PMBRL_ZTAB_MERGE");
  s.wide = env_on("PMBRL_WIDE");
  if (const char* e = getenv("PMBRL_MM_PARTS")) { s.mm_parts_set = true; s.mm_parts = atoi(e); }
  s.replay = 1;
  if (const char* e = getenv("PMBRL_REPLAY")) s.replay = std::max(0, std::min(2, atoi(e)));
  if (const char* e = getenv("PMBRL_DW_PIPE")) {
    s.dw_pipe_off = !strcmp(e, "off");
    s.dw_pipe_ranges = e[0] >= '0' && e[0] <= '9';
    for (const char* q = e; s.dw_pipe_ranges && *q;) {
      const int v = atoi(q);
      if (v > 0) s.dw_pipe.push_back(v);
      while (*q && *q != ',') ++q;
      if (*q == ',') ++q;
    }
  }
  s.dw_head = -1;
  if (const char* e = getenv("PMBRL_DW_HEAD")) s.dw_head = !strcmp(e, "on") ? 1 : (!strcmp(e, "off") ? 0 : -1);
  if (const char* e = getenv("PMBRL_DW_STREAM")) {
    s.dw_stream_off = !strcmp(e, "off");
    s.dw_stream_set = e[0] >= '0' && e[0] <= '9';
    if (s.dw_stream_set) {
      s.dw_stream_steps = atoi(e);
      if (const char* q = strchr(e, ',')) s.dw_stream_wgs = std::max(0, atoi(q + 1));
    }
  }
  return s;
}

// stage 1: the configuration and the two networks
static int plan_nets(pmbrl_plan* p) {
  const pmbrl_config& c = p->cfg;
  if (c.n_pol_angle < 0 || c.n_pol_angle > PMBRL_MAX_ANGLE || c.n_dyn_angle < 0 || c.n_dyn_angle > PMBRL_MAX_ANGLE)
    return fail(-2, "n_pol_angle / n_dyn_angle out of range");
  if (c.dyn_components < 0 || c.dyn_components > PMBRL_MAX_COMP)
    return fail(-2, "dyn_components out of range (<= PMBRL_MAX_COMP)");
  const bool gmm = c.dyn_components > 1;
  if (c.reward.kind != PMBRL_REWARD_EXP && c.reward.kind != PMBRL_REWARD_NEG && c.reward.kind != PMBRL_REWARD_LEARNED &&
      c.reward.kind != PMBRL_REWARD_EXTERNAL)
    return fail(-2, "unknown reward kind");
  p->learned = c.reward.kind == PMBRL_REWARD_LEARNED;
  p->ext = c.reward.kind == PMBRL_REWARD_EXTERNAL;      // (nothing of the layout depends on it: the plan of an analytic reward)
  if (p->learned && c.mm_span_rows > 0)
    return fail(-2, "learned reward head: not offered with moment-matching groups spread over ranks (mm_span_rows > 0)");
  if (p->learned && c.D + 1 > PMBRL_MAX_DIM) return fail(-2, "learned reward head: D + 1 exceeds PMBRL_MAX_DIM");
  // (said here, not by net_plan: a head (2 D + 1) n + 1 wide -- the mixture of the states alone -- is the likely mistake)
  if (p->learned && gmm && c.dyn.n_layers >= 1 && c.dyn.n_layers <= PM_MAXL &&
      c.dyn.dims[c.dyn.n_layers] != (2 * (c.D + 1) + 1) * c.dyn_components + 1)
    return fail(-2, "learned reward head with the mixture head: the density has D + 1 dimensions, a dynamics head "
                    "(2 (D + 1) + 1) dyn_components + 1 wide");
  int rc = net_plan(c.pol, c.pol_act, p->pol, c.D + c.n_pol_angle, 2 * c.U, "policy");
  // (mixture head: n D means, n D log-stds, n logits, one log-temperature -- examples/deep_pilco_mm.py:117-121;
  //  learned reward: one more mean and log-std for the reward, examples/deep_pilco_mm.py:94-99; both: a mixture
  //  density of D + 1 dimensions)
  if (rc == 0)
    rc = net_plan(c.dyn, c.dyn_act, p->dyn, c.D + c.U + c.n_dyn_angle,
                  gmm ? (2 * (c.D + p->learned) + 1) * c.dyn_components + 1 : 2 * (c.D + p->learned), "dynamics");
  p->act = rc == 0 && (p->pol.act != 0 || p->dyn.act != 0);   // (some hidden layer of some network is not ReLU)
  return rc;
}

// stage 2: the layout of the sweeps.  What a choice of row tiles RT (16 rows each) asks for, as functions of the
// networks, the precision asked for and what is given
struct LayoutCalc {
  const pmbrl_plan* p;
  int maxnt;             // widest activation (any layer of either net), in 16-wide tiles
  // general family on split operands (pmbrl_gsplit.h): two fp16 pieces forward / two bf16 pieces in the adjoint;
  // an activation buffer row is then LD 16-bit elements per piece plane, LD = 16 (mod 32)
  bool gsplit;
  bool want_split;       // split-bf16 precision: offered by the fast family for workgroups of up to 32 rows
  // 64-row workgroups on split operands: two fp16 piece planes fit the LDS (three bf16 planes do not), and
  // only the shape-specialised instance keeps its inline-asm loads clear of register-allocator copies
  // (tools/check_inflight.py; the generic 64-row split instances fail that lint and are not compiled):
  // the double cart-pole shape with in-kernel moment matching (the 64-row row of PM_SPLIT2_INSTANCES), fp32 otherwise
  bool rt4_split;
  // LDS leading dimension of the general family: widest activation, +8 so that LD % 16 == 8 (conflict-free
  // ds_read_b128 for the MFMA B operand)
  int ld_generic() const { return gsplit ? (maxnt * 16 + 31) / 32 * 32 + 16 : maxnt * 16 + 8; }
  int prec(int RT) const {
    if (!p->fast) return gsplit ? (int)PMBRL_PREC_SPLIT_F16 : 0;
    return (want_split && (RT <= 2 || rt4_split)) ? (int)p->cfg.precision : 0;
  }
  // (kdiv: 16-wide k-blocks per stage unit -- 1 on the fp32 path, 2 = one K32 block on the split path)
  long stream_work(int m, int kdiv) const {
    long w = 0;
    for (const NetPlan* n : {&p->pol, &p->dyn})
      for (int l = 1; l <= n->nl - 2; ++l) {
        const int ki = (n->nt[l] + kdiv - 1) / kdiv, ko = (n->nt[l + 1] + kdiv - 1) / kdiv;
        w += (long)n->nt[l + 1] * ((ki + m - 1) / m * m) + (long)n->nt[l] * ((ko + m - 1) / m * m);
      }
    return w;
  }
  // stage sizes (k-blocks) of the weight stream: every streamed layer is padded to a whole number
  // of stage PAIRS (CA + CB k-blocks); pick, among the pairs the family has instances of for RT, the one that pads
  // least (pmbrl_instances.h).  (The general family streams no stage pairs: on split operands its plans report the pair
  // of the 32-row instances, as they always have.)
  StagePair stages(int RT) const {
    const int pr = prec(RT);
    return pm_inst_best_stages(pm_fast_keys(pr), pr && !p->fast ? std::min(RT, 2) : RT,
                               [&](int m) { return stream_work(m, pr ? 2 : 1); });
  }
  // split path: elements per row of a bf16 piece plane = padded K + 16 (conflict-free ds_read_b128)
  int ldb(int RT) const {
    if (!prec(RT)) return 0;
    if (!p->fast) return ld_generic();
    const StagePair sp = stages(RT);
    const int m = sp.ca + sp.cb;
    return ((maxnt + 1) / 2 + m - 1) / m * m * 32 + 16;
  }
  int ld(int RT) const {
    if (!p->fast) return ld_generic();
    if (prec(RT))   // floats per row of a buffer holding the piece planes (3 bf16 / 2 fp16 forward, 2 bf16 adjoint)
      return ((prec(RT) == PMBRL_PREC_SPLIT_F16 ? 2 : 3) * ldb(RT) / 2 + 3) / 4 * 4;
    const StagePair sp = stages(RT);
    const int m = sp.ca + sp.cb;
    return (maxnt + m - 1) / m * m * 16 + 8;   // room for the zero K padding
  }
  // LDS of a workgroup: moment matching of mmd-wide states inside the sweep (0: none), groups split over `parts`
  // workgroups, in-place layers (general family)
  // (latency-optimised family: its map, pmbrl_lds_map.h)
  PmFastMap fast_map(int RT, int mmd, int parts = 1) const {
    const pmbrl_config& c = p->cfg;
    // in-kernel moment matching: one wave per whole group of the workgroup (a group split over `parts`
    // workgroups: wave 0, and the whole group's rows in LDS)
    const int mw = parts > 1 ? 1 : (mmd && p->M <= 16 * RT) ? std::min(PF_NW, std::max(1, 16 * RT / p->M)) : PF_NW;
    return pm_fast_map(16 * RT, ld(RT), c.D, c.U, RT, p->pol.nt, p->pol.nl, p->dyn.nt, p->dyn.nl, mmd, prec(RT), mw,
                       parts > 1 ? (parts > 8 ? 16 : p->M) : 0, parts > 1 ? c.H : 0);
  }
  size_t lds(int RT, int mmd, int parts = 1, bool inplace = false) const {
    const pmbrl_config& c = p->cfg;
    if (p->fast) return fast_map(RT, mmd, parts).total * sizeof(float);
    return pm_lds_map(0, 16 * RT, ld(RT), c.D, c.U, RT, mmd, inplace).total * sizeof(float);
  }
};

// stage 2a: moment-matching groups -- rows per group, where the moment matching runs (mm_mode) and, in the sweep,
// the row tiles and how groups are split over workgroups
static int plan_groups(pmbrl_plan* p, LayoutCalc& L, int cus) {
  const pmbrl_config& c = p->cfg;
  const PlanSwitches& sw = p->sw;
  p->G = c.mm_groups > 0 ? c.mm_groups : 1;
  if (c.B % p->G) return fail(-2, "B must be divisible by mm_groups");
  p->M = c.B / p->G;
  if (p->M < 2) return fail(-2, "moment matching needs >= 2 rows per group");
  if (L.rt4_split && p->fast && L.lds(4, c.D) > PM_LDS_CAP) L.rt4_split = false;   // 64-row workgroups: fp32 then
  // groups spread over ranks: the statistics cross devices between the two halves of the moment matching, so it
  // stays outside the sweep kernels (mm_mode 2: one sweep launch per step)
  p->span = c.mm_span_rows > 0;
  if (p->span) {
    if (c.mm_span_ranks < 1 || c.mm_span_rank < 0 || c.mm_span_rank >= c.mm_span_ranks)
      return fail(-2, "mm_span_ranks / mm_span_rank out of range");
    if (c.mm_span_offset < 0 || c.mm_span_offset + p->M > c.mm_span_rows)
      return fail(-2, "mm_span_offset + rows per group on this rank exceeds mm_span_rows");
    if ((long long)p->G * c.mm_span_rows > c.B_global) return fail(-2, "mm_groups x mm_span_rows exceeds B_global");
  }
  // in-kernel if a whole number of groups fits a workgroup's row tiles and LDS
  p->mm_mode = 2;
  for (int RT : {1, 2, 4}) {
    if (p->span) break;
    const int R = 16 * RT;
    if (p->M <= R && L.lds(RT, c.D) <= PM_LDS_CAP) {
      p->mm_mode = 1;
      p->RT = RT;
      p->rows_per_wg = (R / p->M) * p->M;
      break;
    }
  }
  // A group of 33..64 rows in ONE 64-row workgroup is throughput-bound on its CU (52 tile epilogues and
  // 52 x 21 MFMAs per layer: 67 k cycles per step at the double cart-pole shape) while most of the chip idles.
  // Split over two workgroups of <= 32 rows a step is 26 k cycles of GEMMs; the halves exchange their
  // rows through HBM and meet at a group-local flag barrier (pm_group_sync), and each factors the whole
  // group redundantly (the d x d fp64 chain is serial anyway).  Needs every workgroup resident (checked
  // here like the device-wide barrier form).  PMBRL_MM_PARTS=1 keeps one workgroup per group.
  const int max_wg = std::min(cus, 1024);
  // By default where a group needs more than 16 rows: 64-row workgroups (M = 33..64) are throughput-bound on
  // their CU, and a 32-row workgroup (M = 17..32) still takes 30 k cycles per step against 24 k for two
  // 16-row ones with the exchange (measured on the cart-pole shapes, also with unshaped networks) -- and
  // where a group fits no workgroup at all (more than 64 rows, or LDS): the device-wide-barrier form would
  // take over otherwise (D = 6, 2 x 256 hidden units, 50-row groups: 8.9 ms against 4.0 ms per iteration).
  // Groups of up to 128 rows (beyond 64 the one-wave routines walk the rows in strides).  The fewest parts
  // that bring a part down to 16 rows while every workgroup stays resident, else to 32 rows.
  // PMBRL_MM_PARTS=n: n parts wherever that can be done (tests); 1: whole groups.
  const bool big = !p->span && ((p->mm_mode == 1 && p->RT >= 2) || p->mm_mode == 2 || (sw.mm_parts_set && p->mm_mode == 1));
  auto fits = [&](int parts, int max_rows, bool resident = true) {
    const int rpw = (p->M + parts - 1) / parts;      // the last part takes what is left of the group
    return rpw <= max_rows && (parts - 1) * rpw < p->M && (!resident || p->G * parts <= max_wg);
  };
  int want = 0;
  // Round 5: 16-row parts even where they are more workgroups than CUs (the double cart-pole shape: 100 groups of 50
  // rows = 400 parts of <= 13 rows) IF the register-resident family takes the shape (pmbrl_reg_mm.h) -- its 16-row step
  // is a third of the latency-optimised family's 32-row step, so two launches of 200 workgroups (batches of whole groups:
  // what the statistics exchange needs resident together is one GROUP's workgroups) beat one launch of 200 32-row ones
  bool batched = false;
  if (sw.mm_parts_set) want = sw.mm_parts;
  else {
    for (int parts = 2; parts <= 8 && !want; ++parts) if (fits(parts, 16)) want = parts;
    if (!want && max_wg >= 64 && pm_reg_mm_shape_ok(p, L.prec(1)) && !sw.mm_no_batch)
      for (int parts = 2; parts <= 8 && !want; ++parts)
        if (fits(parts, 16, false) && p->G * parts <= 1024) { want = parts; batched = true; }
    for (int parts = 2; parts <= 8 && !want; ++parts) if (fits(parts, 32)) want = parts;
  }
  if (p->fast && want >= 2 && want <= 8 && big && p->M <= 128 && (batched ? fits(want, 16, false) : fits(want, 32)) &&
      (c.flags & PMBRL_FLAG_MM_STATES)) {
    const int rpw = (p->M + want - 1) / want;
    const int rt = rpw <= 16 ? 1 : 2;
    if (L.lds(rt, c.D, want) <= PM_LDS_CAP) {
      p->mm_mode = 1;
      p->mm_parts = want;
      p->RT = rt;
      p->rows_per_wg = rpw;
      if (batched) {      // balanced batches of whole groups, each batch's workgroups resident together
        const int nb = (p->G * want + max_wg - 1) / max_wg;
        p->mm_gpb = (p->G + nb - 1) / nb;
        // (the register-resident family deals hardware workgroups in blocks of 8 groups -- a group's parts on one XCD --
        //  and launches whole blocks: a batch rounded UP to blocks must still be resident together, or the parts of
        //  the block that straddles the chip spin until other workgroups finish a whole sweep.  G = 97 in 5 parts on
        //  256 CUs: 49 groups -> 280 workgroups; 48 -> 240)
        const int cap = max_wg / want / 8 * 8;
        if (cap >= 8) p->mm_gpb = std::min((p->mm_gpb + 7) / 8 * 8, cap);
      }
    }
  }
  // A group beyond 8 parts of 32 rows -- ONE group over the whole batch, the reference's default (mm_groups=None,
  // examples/deep_pilco_mm.py:31): 16-row parts whose sums travel over two levels (pm_xch_get_tree), every workgroup
  // resident.  Only where the instance that exchanges sums runs (compile-time state width, the cart-pole shape: the
  // PfShapeTree row of PM_SPLIT2_INSTANCES) -- the rows + flags form of the generic instances keeps the whole group's rows in LDS.
  // 2 500 rows: 157 parts, 13 collectors; against the device-wide-barrier form (every workgroup re-reads and
  // re-reduces the whole group's rows every step) 3.0 -> see profiles/r04*_single_group.txt.  PMBRL_MM_TREE=0: off.
  const bool shaped_mm1 = p->fast && L.prec(1) == PMBRL_PREC_SPLIT_F16 &&
                          pm_inst_any(pm_fast_keys(L.prec(1)), 1, PF_VAR_MM, c.D, c.U, 3, hidden_tiles_3l(p), 1) &&
                          !(c.flags & PMBRL_FLAG_NO_SHAPED) && sw.lds_tiles && sw.mm_xch;
  if (p->mm_mode == 2 && !p->span && !sw.mm_parts_set && shaped_mm1 && (c.flags & PMBRL_FLAG_MM_STATES) && sw.mm_tree) {
    const int parts = (p->M + 15) / 16;
    if (parts > 8 && (long long)p->G * parts <= max_wg && L.ld(1) == 240) {
      if (L.lds(1, c.D, parts) + pm_lds_tiles_bytes(13) + 16 <= PM_LDS_CAP) {      // (the tiles of 13 hidden tiles)
        p->mm_mode = 1;
        p->mm_parts = parts;
        p->RT = 1;
        p->rows_per_wg = 16;
        int fan = 2;
        while (fan * fan < parts) ++fan;
        // ONE group (mm_groups=None): two collectors per XCD -- 2 fan parts of the group on every XCD, so that the
        // members' hop to their collector stays inside that XCD's L2 (the register-resident family deals its workgroups
        // that way: pmbrl_reg.h, pr_wg; the latency-optimised family walks the same slots in dispatch order)
        if (p->G == 1 && parts <= 256) fan = (parts + 15) / 16;
        p->mm_fan = fan;
      }
    }
  }
  return 0;
}

// stage 2b: row tiles of a plan whose moment matching (if any) does not run inside the sweep
static int plain_row_tiles(pmbrl_plan* p, const LayoutCalc& L, int cus) {
  const pmbrl_config& c = p->cfg;
  int RT = 1;
  if (c.rows_per_wg_hint >= 64) RT = 4;
  else if (c.rows_per_wg_hint >= 32) RT = 2;
  else if (c.rows_per_wg_hint == 0) {
    // fill the chip first: >= 2 waves of workgroups over 256 CUs before growing tiles
    if ((c.B + 15) / 16 > 1024) RT = 2;
    if ((c.B + 31) / 32 > 1024) RT = 4;
    // general family (wide networks, throughput-bound): 32-row workgroups halve the weight traffic
    // per row as soon as they still give every CU two workgroups' worth of rows
    if (!p->fast && RT == 1 && (c.B + 31) / 32 >= 512) RT = 2;
  }
  while (RT > 1 && L.lds(RT, 0) > PM_LDS_CAP) RT /= 2;
  // General family on split operands: 64-row workgroups with IN-PLACE layers (one activation buffer, pmbrl_gsplit.h:
  // gemm_layer_inplace_s) where two buffers of 64 rows do not fit the LDS.  Built to stream a 512 x 512 layer's weights
  // once per 64 rows instead of once per 32; measured at the C5 shape (profiles/r03b_inplace_*): a hidden layer's K loop
  // does become MFMA-bound (25 k cycles per 64 rows), but with every wave's epilogues behind one barrier they no
  // longer overlap another wave's MFMAs (+36 k), and the stash stores of a policy layer, issued back to back, cost
  // 26 k cycles more -- 46.7 ms per iteration against 45.3 ms for the two-buffer 32-row form.  So it is taken only
  // on request (rows_per_wg_hint >= 64): widths <= 512, every narrow width (2U, 2D, D + U) <= 64, no mixture head,
  // no angle features.
  const bool angles = c.n_pol_angle > 0 || c.n_dyn_angle > 0;
  // (!p->learned, dyn_components <= 1: the sweeps rely on it -- pm_rollout_fwd / _bwd take the (D + 1)-wide strides of a
  //  learned reward on the mixture head in kernels of their own, which exist for the two-buffer layers only; plan_workspace
  //  refuses a plan that would break it)
  if (L.gsplit && !angles && c.dyn_components <= 1 && !p->learned && !p->act && L.maxnt <= 32 && 2 * c.D <= PM_IP_NOFF && 2 * c.U <= PM_IP_NOFF &&
      c.D + c.U <= PM_IP_NOFF && RT < 4) {
    // every hidden layer 512 wide: the in-place layers of pmbrl_wide.h (compile-time shape, lean epilogue) -- taken by
    // default as soon as 64-row workgroups still give every CU one (PMBRL_WIDE=0: the generic in-place form on
    // request only, as before)
    bool wide = p->sw.wide;
    for (int i = 1; i < p->pol.nl; ++i) wide = wide && p->pol.nt[i] == 32;
    for (int i = 1; i < p->dyn.nl; ++i) wide = wide && p->dyn.nt[i] == 32;
    const bool want = c.rows_per_wg_hint >= 64 || (wide && c.rows_per_wg_hint == 0 && cus > 0 && (c.B + 63) / 64 >= cus);
    if (want) {
      p->inplace = wide ? 2 : 1;
      if (L.lds(4, 0, 1, true) <= PM_LDS_CAP) RT = 4;
      else p->inplace = 0;
    }
  }
  return RT;
}

static int plan_layout(pmbrl_plan* p, int cus) {
  const pmbrl_config& c = p->cfg;
  const PlanSwitches& sw = p->sw;
  const bool mm = (c.flags & (PMBRL_FLAG_MM_STATES | PMBRL_FLAG_MM_REWARDS)) != 0;
  // infer_noise_variables (utils/rollout.py:6-17, not a default anywhere) lives in the general
  // single-wave moment-matching routines only: general kernel family, mm_mode 1 or 2.  So does the learned reward
  // head (its sampling epilogue and head seed are written for that family's sweeps only)
  p->fast = !(c.flags & (PMBRL_FLAG_FORCE_GENERIC | PMBRL_FLAG_INFER_NS | PMBRL_FLAG_POL_MASKS_PER_STEP |
                         PMBRL_FLAG_DYN_MASKS_PER_STEP)) && c.n_pol_angle == 0 && c.n_dyn_angle == 0 && c.dyn_components <= 1 &&
            !p->learned && !p->act &&      // (an activation other than ReLU: the general family's ACT instances)
            pm_fast_net_ok(p->pol.dim, p->pol.nt, p->pol.nl) &&
            pm_fast_net_ok(p->dyn.dim, p->dyn.nt, p->dyn.nl);
  LayoutCalc L;
  L.p = p;
  L.maxnt = 1;
  for (int i = 0; i <= p->pol.nl; ++i) L.maxnt = std::max(L.maxnt, p->pol.nt[i]);
  for (int i = 0; i <= p->dyn.nl; ++i) L.maxnt = std::max(L.maxnt, p->dyn.nt[i]);
  L.gsplit = !p->fast && c.precision == PMBRL_PREC_SPLIT_F16;
  L.want_split = (c.precision == PMBRL_PREC_SPLIT || c.precision == PMBRL_PREC_SPLIT_F16) && p->fast;
  L.rt4_split = c.precision == PMBRL_PREC_SPLIT_F16 && mm &&
                pm_inst_any(pm_fast_keys(c.precision), 4, PF_VAR_MM, c.D, c.U, 3, hidden_tiles_3l(p)) &&
                !(c.flags & PMBRL_FLAG_NO_SHAPED);
  for (int RT : {1, 2, 4})
    if (!L.stages(RT).ca) return fail(-3, "no stage pair instantiated for " + std::to_string(16 * RT) + "-row workgroups");
  p->G = 1;
  p->M = c.B;
  p->mm_mode = 0;
  p->mm_parts = 1;
  if (mm)
    if (int rc = plan_groups(p, L, cus)) return rc;
  if (p->mm_mode != 1) {
    L.rt4_split = false;
    p->RT = plain_row_tiles(p, L, cus);
    p->rows_per_wg = 16 * p->RT;
  } else if (c.rows_per_wg_hint > 0 && p->mm_parts <= 1) {
    // allow the caller to force fewer groups per workgroup
    const int want = std::max(p->M, (c.rows_per_wg_hint / p->M) * p->M);
    if (want <= 16 * p->RT) p->rows_per_wg = want;
  }
  // groups that span workgroups: the fast family does the state moment matching in the prologue of
  // its per-step launches (mm_mode 3) when it has a compile-time-width instance and the partial
  // Gram tiles fit the activation buffers; otherwise separate kernels per step (mm_mode 2)
  if (p->mm_mode == 2 && !p->span && p->fast && (c.flags & PMBRL_FLAG_MM_STATES) && c.D >= 4 && c.D <= 6 &&
      !sw.mm_mode2 && L.lds(p->RT, c.D) <= PM_LDS_CAP &&
      (size_t)2 * 16 * p->RT * L.ld(p->RT) * sizeof(float) >= (size_t)8 * 256 * sizeof(double))
    p->mm_mode = 3;
  p->LD = L.ld(p->RT);
  int mmd = (p->mm_mode == 1 || p->mm_mode == 3) ? c.D : 0;      // moment matching inside the sweep: of states this wide
  p->lds_bytes = L.lds(p->RT, mmd, p->mm_parts, p->inplace != 0);
  const StagePair sp = L.stages(p->RT);
  p->CA = sp.ca;
  p->CB = sp.cb;
  p->prec = L.prec(p->RT);
  p->LDB = L.ldb(p->RT);
  if (p->lds_bytes > PM_LDS_CAP) return fail(-3, "network too wide for the fused kernel's LDS budget");
  p->nwg = p->mm_parts > 1 ? p->G * p->mm_parts : (c.B + p->rows_per_wg - 1) / p->rows_per_wg;
  // groups spanning workgroups, every workgroup resident at once (one per CU always fits): the
  // per-step launches become one launch whose workgroups meet at a device-wide barrier per step
  p->mm_grid = p->mm_mode == 3 && p->RT == 1 && !sw.mm_perstep && p->nwg <= cus && p->nwg <= 1024;
  // More workgroups than CUs under ONE launch cannot meet at a barrier: the sweeps would run one launch per step with
  // the whole group's moment matching redone in the prologue of EVERY workgroup (one group of 5000 rows: 9.7 ms per
  // forward + adjoint, 10 000 rows: 23.4 ms).  The form built for groups spread over ranks does better there --
  // statistics over 16 workgroups, one factorisation, rows by all threads (pmbrl_mmx.h): 4.3 / 6.4 ms -- so such a
  // plan is the span form with ONE rank, whose exchange is the identity (profiles/r02n_span_cost.txt).
  // PMBRL_MM_PERSTEP keeps the per-step prologue form (tests).
  if (p->mm_mode == 3 && !p->mm_grid && !p->span && p->M >= 2048 && cus > 0 && p->nwg > cus &&
      !(c.flags & PMBRL_FLAG_INFER_NS) && !sw.mm_perstep) {
    p->span = 1;
    p->cfg.mm_span_rows = p->M;
    p->cfg.mm_span_offset = p->cfg.row_offset;   // (the groups are local: only the noise row needs the shard's offset)
    p->cfg.mm_span_ranks = 1;
    p->cfg.mm_span_rank = 0;
    p->mm_mode = 2;
    mmd = 0;
    p->lds_bytes = L.lds(p->RT, mmd);
  }

  // LDS-resident tiles of the sweeps' second streamed layer (pmbrl_fast.h, lds_tile_s): the shape-specialised 16-row
  // split-precision instances (two streamed layers of 13 or 14 tiles, stage pair = one tile) keep 8 tiles of it in the
  // LDS the workgroup has to itself anyway; which variants use them is settled with the plan's kernels (resolve_sweeps).
  // PMBRL_LDS_TILES=0: off.
  const int ht = hidden_tiles_3l(p);
  if (p->fast && p->RT == 1 && p->prec == PMBRL_PREC_SPLIT_F16 && p->CA + p->CB == 7 && (ht == 13 || ht == 14) &&
      !(c.flags & PMBRL_FLAG_NO_SHAPED) && sw.lds_tiles) {
    // behind everything else; split groups: the instances that hold the tiles exchange sums and never touch the row
    // blocks of the rows + flags form, the generic instances that use those never copy tiles: the two share the end
    // of the LDS (a 100-row group in seven parts would not fit both) -- the map's tile_base either way
    const size_t base = L.fast_map(p->RT, mmd, p->mm_parts).m.tile_base * sizeof(float), tiles = pm_lds_tiles_bytes(ht);
    if (base + tiles <= PM_LDS_CAP) {
      p->wlds_off = (int)(base / sizeof(float));
      p->lds_last_lanes = pm_lds_tile_last_lanes(ht);
      p->lds_bytes = std::max(p->lds_bytes, base + tiles);
    }
  }

  // wide states between per-step launches: the LDS-staged multi-wave kernels
  p->mm_wide = p->mm_mode == 2 && !p->span && (c.flags & PMBRL_FLAG_MM_STATES) && pm_mmw_ok(p->M, c.D, c.flags);
  return 0;
}

// stage 3: reward constants
static int plan_reward(pmbrl_plan* p) {
  const pmbrl_config& c = p->cfg;
  HIPCHK(hipSetDevice(p->device));
  RewardDev r;
  memset(&r, 0, sizeof(r));
  const pmbrl_reward& s = c.reward;
  r.kind = s.kind;
  if (p->learned) {      // (no constants -- the reward comes out of the dynamics head -- and rew_d stays null)
    p->rew_k = 0;
    HIPCHK(hipMalloc(&p->wflag_d, sizeof(int)));
    HIPCHK(hipMemset(p->wflag_d, 0, sizeof(int)));
    return 0;
  }
  if (p->ext) {      // (no constants either, but rew_d stays NON-null -- an all-zero record nothing reads: a null one is how the
                     //  sweeps tell a learned head, fill_args and RolloutArgs::Jx)
    p->rew_k = 0;
    HIPCHK(hipMalloc(&p->rew_d, sizeof(RewardDev)));
    HIPCHK(hipMemcpy(p->rew_d, &r, sizeof(RewardDev), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&p->wflag_d, sizeof(int)));
    HIPCHK(hipMemset(p->wflag_d, 0, sizeof(int)));
    return 0;
  }
  r.expand = s.expand;
  r.k = s.k;
  r.n_angle = s.expand ? s.n_angle : 0;
  if (r.n_angle > PMBRL_MAX_ANGLE) return fail(-2, "too many angle dims");
  int no = 0;
  for (int i = 0; i < c.D; ++i) {
    bool isang = false;
    for (int j = 0; j < r.n_angle; ++j) isang |= (s.angle_dims[j] == i);
    if (!isang) r.other_dims[no++] = i;
  }
  for (int j = 0; j < r.n_angle; ++j) {
    if (s.angle_dims[j] < 0 || s.angle_dims[j] >= c.D) return fail(-2, "angle dim out of range");
    r.angle_dims[j] = s.angle_dims[j];
  }
  r.n_other = s.expand ? no : c.D;
  r.De = s.expand ? no + 2 * r.n_angle : c.D;
  if (r.De > PMBRL_MAX_DIM) return fail(-2, "expanded state too wide");
  for (int i = 0; i < s.k; ++i) {
    for (int j = 0; j < r.De; ++j) r.C[i * r.De + j] = s.C[i * r.De + j] / s.norm;
    r.tt[i] = s.tip_target[i] / s.norm;
  }
  r.w = s.w;
  for (int i = 0; i < s.k; ++i)
    for (int j = 0; j < s.k; ++j) {
      r.Q[i * s.k + j] = s.Q[i * s.k + j];
      r.QQ[i * s.k + j] = s.Q[i * s.k + j] + s.Q[j * s.k + i];
    }
  for (int i = 0; i < c.U; ++i)
    for (int j = 0; j < c.U; ++j) {
      r.R[i * c.U + j] = s.R[i * c.U + j];
      r.RR[i * c.U + j] = s.R[i * c.U + j] + s.R[j * c.U + i];
    }
  for (int d = 0; d < PMBRL_MAX_DIM; ++d) r.d_copy[d] = r.d_sin[d] = r.d_cos[d] = -1;
  if (s.expand) {
    for (int i = 0; i < no; ++i) { r.phi_src[i] = r.other_dims[i]; r.phi_mode[i] = 0; r.d_copy[r.other_dims[i]] = i; }
    for (int j = 0; j < r.n_angle; ++j) {
      r.phi_src[no + j] = r.angle_dims[j]; r.phi_mode[no + j] = 1; r.d_sin[r.angle_dims[j]] = no + j;
      r.phi_src[no + r.n_angle + j] = r.angle_dims[j]; r.phi_mode[no + r.n_angle + j] = 2;
      r.d_cos[r.angle_dims[j]] = no + r.n_angle + j;
    }
  } else {
    for (int i = 0; i < c.D; ++i) { r.phi_src[i] = i; r.phi_mode[i] = 0; r.d_copy[i] = i; }
  }
  if ((size_t)256 * (c.D | 1) * sizeof(float) > 64 * 1024)      // (rows of a block staged in LDS)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(pm_reward_kernel_for(c.U, r.k)),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 256 * (c.D | 1) * (int)sizeof(float)));
  p->rew_k = r.k;
  HIPCHK(hipMalloc(&p->rew_d, sizeof(RewardDev)));
  HIPCHK(hipMemcpy(p->rew_d, &r, sizeof(RewardDev), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&p->wflag_d, sizeof(int)));
  HIPCHK(hipMemset(p->wflag_d, 0, sizeof(int)));
  return 0;
}

// stage 4: angle_dims feature maps (utils/angles.py:29-42: others in order, then sin, then cos)
static int plan_angles(pmbrl_plan* p) {
  const pmbrl_config& c = p->cfg;
  if (c.n_pol_angle == 0 && c.n_dyn_angle == 0) return 0;
  AngleDev a;
  memset(&a, 0, sizeof(a));
  auto build = [&](FeatMap& m, int width, int n_ang, const int32_t* dims, int max_dim) -> bool {
    for (int d = 0; d < PMBRL_MAX_DIM; ++d) m.f_copy[d] = m.f_sin[d] = m.f_cos[d] = -1;
    for (int j = 0; j < n_ang; ++j) {
      if (dims[j] < 0 || dims[j] >= max_dim) return false;
      for (int i = 0; i < j; ++i)
        if (dims[i] == dims[j]) return false;
    }
    int no = 0;
    for (int i = 0; i < width; ++i) {
      bool isang = false;
      for (int j = 0; j < n_ang; ++j) isang |= (dims[j] == i);
      if (!isang) { m.src[no] = i; m.mode[no] = 0; m.f_copy[i] = no; ++no; }
    }
    for (int j = 0; j < n_ang; ++j) {
      m.src[no + j] = dims[j]; m.mode[no + j] = 1; m.f_sin[dims[j]] = no + j;
      m.src[no + n_ang + j] = dims[j]; m.mode[no + n_ang + j] = 2; m.f_cos[dims[j]] = no + n_ang + j;
    }
    m.n_feat = no + 2 * n_ang;
    return m.n_feat <= PMBRL_MAX_DIM;
  };
  if (!build(a.pol, c.D, c.n_pol_angle, c.pol_angle_dims, c.D) ||
      !build(a.dyn, c.D + c.U, c.n_dyn_angle, c.dyn_angle_dims, c.D))
    return fail(-2, "angle dims must be distinct state dims (0 <= d < D)");
  HIPCHK(hipMalloc(&p->ang_d, sizeof(AngleDev)));
  HIPCHK(hipMemcpy(p->ang_d, &a, sizeof(AngleDev), hipMemcpyHostToDevice));
  return 0;
}

// stage 6: the workspace carve-up
static int plan_workspace(pmbrl_plan* p) {
  const pmbrl_config& c = p->cfg;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = align_up(off + bytes, 256);
    return o;
  };
  for (NetPlan* n : {&p->pol, &p->dyn}) {
    for (int l = 0; l < n->nl; ++l) {
      const size_t fr = (size_t)(n->nt[l + 1] + 15) * (n->nt[l] + 15) * 256 * sizeof(float);
      n->wf[l] = take(fr);
      n->wb[l] = take(fr);
      n->bias[l] = take((size_t)n->nt[l + 1] * 16 * sizeof(float));
      if (l < n->nl - 1)
        // u16 (generic) or 4 nibble-bytes (fast); 256 bytes of slack behind it: where the register-resident family's
        // rows past the batch put their (zero) bytes -- lane (< 64) + 4 x tile (< 64) past the end (pmbrl_reg.h)
        // (a plan with an activation other than ReLU: act' x mask / keep per unit instead, [H][B][nt * 16] floats)
        n->abits[l] = take((size_t)c.H * c.B * n->nt[l + 1] * (p->act ? 16 * sizeof(float) : 4) + 256);
    }
  }
  const bool gmm = c.dyn_components > 1;
  if (p->learned && gmm && p->inplace)   // (cannot happen while plain_row_tiles keeps both off the in-place layers)
    return fail(-3, "learned reward head with the mixture head: the in-place sweeps do not serve it");
  const size_t Rw = 16 * p->RT;
  for (int l = 0; l < p->pol.nl; ++l) {
    p->off_actT[l] = take((size_t)c.H * p->nwg * p->pol.nt[l] * 16 * Rw * sizeof(float));
    p->off_gT[l] = take((size_t)c.H * p->nwg * p->pol.nt[l + 1] * 16 * Rw * sizeof(float));
  }
  p->off_Tp = take((size_t)c.H * c.B * c.U * sizeof(float));
  p->off_Td = take((size_t)c.H * c.B * c.D * sizeof(float));
  // (a learned reward head gives the coefficient table a column for r~)
  p->off_gmm_c = take(gmm ? (size_t)c.H * c.B * (c.dyn_components + 1) * (c.D + p->learned) * sizeof(float) : 0);
  p->off_gmm_k = take(gmm ? (size_t)c.H * c.B * sizeof(int) : 0);
  p->off_xt = take((size_t)c.H * c.B * c.D * sizeof(float));
  p->off_rt = take((size_t)c.H * c.B * sizeof(float));
  p->off_mmfac = take(p->mm_mode == 1 ? (size_t)c.H * (c.B / p->M) * pm_mm_fac_doubles(c.D) * sizeof(double)
                      : p->mm_wide    ? (size_t)c.H * p->G * pm_mmw_fac_doubles(c.D) * sizeof(double)
                                      : 0);
  p->off_Jx = take((size_t)c.H * c.B * c.D * sizeof(float));
  p->off_Ja = take((size_t)c.H * c.B * c.U * sizeof(float));
  p->off_gxc = take((size_t)c.B * c.D * sizeof(float));
  p->off_gxc2 = take((size_t)c.B * c.D * sizeof(float));
  p->off_gsync = take(2 * 1024 * sizeof(unsigned));   // one flag per workgroup for the device-wide barriers (forward, backward)
  // groups split over workgroups: the granules of their statistics exchange (pm_xch_sum; PMBRL_MM_XCH=0: rows + flags)
  if (p->mm_parts > 1 && p->sw.mm_xch) {
    // (more than 8 parts: a second set of slots, the collectors')
    p->xch_bytes = (size_t)(p->mm_parts > 8 ? 2 : 1) * p->nwg * PM_XCH_WG_WORDS(2) * sizeof(unsigned long long);
    p->off_xch = take(p->xch_bytes);
  }
  p->off_ztab = take((p->mm_fan || p->reg_mm) ? (size_t)c.H * p->G * 2 * c.D * sizeof(double) : 0);
  p->off_reg_linv = take(p->reg_mm ? (size_t)c.H * p->G * c.D * c.D * sizeof(double) : 0);
  p->off_grt = take((size_t)c.H * c.B * sizeof(float));
  // statistics exchange of groups spread over ranks: forward slots of every rank (states of one step, or the
  // rewards of all steps), the factors the adjoint reuses
  const size_t n_s = (size_t)p->G * pm_mmx_slot_doubles(c.D), n_r = (size_t)c.H * p->G * pm_mmx_slot_doubles(1);
  p->off_mmx_buf = take(p->span ? (size_t)c.mm_span_ranks * std::max(n_s * PM_MMX_NB, n_r) * sizeof(double) : 0);
  p->off_mmx_fac = take(p->span ? (size_t)c.H * p->G * pm_mm_fac_doubles(c.D) * sizeof(double) : 0);
  p->off_mmx_rfac = take(p->span ? (size_t)c.H * p->G * pm_mm_fac_doubles(1) * sizeof(double) : 0);
  p->off_reg_pack = take(p->reg ? pm_reg_pack_bytes() : 0);
  for (int n = 0; n < 2; ++n)
    for (int l = 0; l < 2; ++l) p->off_reg_ab[n][l] = take(p->reg ? (size_t)c.H * p->nwg * 1024 : 0);
  // the dW GEMM's partial rows, and the policy head's gradient as the adjoint sweep publishes it for the streamed form
  p->dw.off_part = take((size_t)p->dw.part_rows * p->dw.args.part_stride * sizeof(float));
  p->dw.off_pub = take(p->dw.pub_bytes);
  p->ws_bytes = off;
  if (p->ws_bytes >= ((size_t)1 << 32)) p->reg = p->reg_mm = p->dw.st_on = 0;      // (the family addresses its stashes with 32-bit workspace offsets)
  return 0;
}

// stage 7: the plan's sweep kernels, kernel attributes, and the residency the barrier form relies on
static PmInstTable sweep_table(const pmbrl_plan* p) {
  if (p->fast)
    return p->prec == PMBRL_PREC_SPLIT_F16 ? pm_fast_split2_instances() : p->prec ? pm_fast_split1_instances() : pm_fast_f32_instances();
  // (a learned reward head on the mixture head has sweeps of its own: pm_rollout_fwd_gmmr / _bwd_gmmr)
  if (p->learned && p->cfg.dyn_components > 1) return p->act ? pm_general_gmmr_act_instances() : pm_general_gmmr_instances();
  if (p->act) return pm_general_act_instances();
  return p->prec ? pm_general_split_instances() : PmInstTable{pm_general_f32_keys, general_f32_fns, pm_general_f32_n};
}
// do the shape-specialised 16-row instances of this plan's stage pair hold tiles of the second streamed layer in LDS
// (pmbrl_fast.h, lds_tile_s; plan_layout reserved them: wlds_off)?  Two fp16 pieces, a tile exactly one stage pair wide,
// two hidden layers of more than 8 tiles -- whose second stream entry (fill_args: add_stream) is then 7 K32 blocks x 2
// pieces and more than 8 tiles, which the kernels count on.  Worked out for 13 tiles, the only such rows (sd.n = 2,
// n_kb[1] = 14, n_ot[1] = 12 or 13); a shaped row of another width or depth has to establish it again.
static bool lds_tiles_row(const pmbrl_plan* p, const PmInstKey& k) {
  return p->prec == PMBRL_PREC_SPLIT_F16 && p->RT == 1 && p->CA + p->CB == 7 && k.var != PF_VAR_MMG && k.nl == 3 && k.nt > 8;
}
// p->sweep / p->sweep_key: per variant the shape-specialised row of the plan's shape if there is one and it may run, else
// the generic row.  A plan whose calls will ask for a variant that has neither is refused.
static int resolve_sweeps(pmbrl_plan* p) {
  const pmbrl_config& c = p->cfg;
  const PmInstTable T = sweep_table(p);
  auto take = [&](int slot, const PmInstKey& k) {
    const int i = pm_inst_find(T, k);
    if (i >= 0) { p->sweep[slot] = T.fn[i]; p->sweep_key[slot] = k; }
    return i >= 0;
  };
  if (!p->fast) {
    // the table of the networks that are not ReLU is keyed by piece planes, the split one by the in-place form (3: the
    // wide layers with pre-split stashes), the exact-fp32 one by row tiles alone
    const int wide_form = (p->inplace == 2 && p->dw.pre_mask) ? 3 : p->inplace;
    const bool planes = p->act || (p->learned && c.dyn_components > 1);      // (tables keyed by piece planes)
    const PmInstKey k = pm_general_key(p->RT, planes ? (p->prec ? 2 : 0) : p->prec ? wide_form : 0);
    return take(0, k) ? 0 : fail(-3, "no general-family instance for " + pm_inst_name(k));
  }
  // not on request (tests), and not for split groups without the statistics exchange (PMBRL_MM_XCH=0): only the generic
  // instances carry the rows + flags form
  const bool shaped_ok = !(c.flags & PMBRL_FLAG_NO_SHAPED) && !(p->mm_parts > 1 && !p->xch_bytes);
  for (int var = 0; var < PF_VAR_COUNT; ++var) {
    const bool mm_in = p->mm_mode == 1 || p->mm_mode == 3;
    const bool needed = var == PF_VAR_MMG ? p->mm_grid != 0 : (var == PF_VAR_MM) == mm_in;
    PmInstKey k = {p->RT, p->CA, p->CB, var, c.D, c.U, p->LD, 3, hidden_tiles_3l(p), 0};
    // groups split over more than 8 workgroups: the two-level exchange, which only that instance has
    k.tree = var == PF_VAR_MM && p->mm_mode == 1 && p->mm_parts > 8;
    if (shaped_ok && (!lds_tiles_row(p, k) || p->wlds_off > 0) && take(var, k)) continue;
    if (k.tree) return fail(-3, "no instance for a moment-matching group split over more than 8 workgroups: " + pm_inst_name(k));
    k = PmInstKey{p->RT, p->CA, p->CB, var, 0, 0, 0, 0, 0, 0};
    if (!take(var, k) && needed) return fail(-3, "no latency-optimised instance for " + pm_inst_name(k));
  }
  return 0;
}
static int plan_attrs(pmbrl_plan* p, int cus) {
  const pmbrl_config& c = p->cfg;
  if (int rc = resolve_sweeps(p)) return rc;
  // the LDS the plan asks for: on the general family's pair, on every latency-optimised instance of the plan's (row
  // tiles, stage pair)
  const PmInstTable T = sweep_table(p);
  for (int i = 0; i < T.n; ++i) {
    const PmInstKey& k = T.key[i];
    if (p->fast ? k.rt != p->RT || k.ca != p->CA || k.cb != p->CB : T.fn[i].fwd != p->sweep[0].fwd) continue;
    HIPCHK(hipFuncSetAttribute(T.fn[i].fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds_bytes));
    HIPCHK(hipFuncSetAttribute(T.fn[i].bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds_bytes));
  }
  if (p->mm_wide) {
    const int smem = (int)pm_mmw_lds_bytes(p->M, c.D, true);
    if (smem > 64 * 1024 &&
        (hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mmw_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             smem) != hipSuccess ||
         hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mmw_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             smem) != hipSuccess)) {
      (void)hipGetLastError();
      return fail(-3, "hipFuncSetAttribute(wide moment-matching kernels) failed");
    }
  }
  if (p->mm_mode == 2 || p->mm_mode == 3) {
    const int smem = (int)(pm_mm_kernel_doubles(c.D) * sizeof(double));
    if (smem > (int)PM_LDS_CAP) return fail(-3, "moment-matching scratch exceeds the LDS");
    if (smem > 64 * 1024 &&
        (hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mm_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             smem) != hipSuccess ||
         hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_mm_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             smem) != hipSuccess)) {
      (void)hipGetLastError();
      return fail(-3, "hipFuncSetAttribute(moment-matching kernels) failed");
    }
  }
  if (p->reg)
    if (int rc = pm_reg_resolve(p)) return rc;
  if (p->mm_grid) {
    // the barrier-form sweep needs every workgroup resident at once: ask the runtime how many of the generic barrier-form
    // kernel of this stage pair (registers, LDS) fit a CU instead of assuming one (min over forward / adjoint)
    const int i = pm_inst_find(T, {1, p->CA, p->CB, PF_VAR_MMG, 0, 0, 0, 0, 0, 0});
    int a = 0, b = 0;
    if (i < 0 || hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, T.fn[i].fwd, PF_NT, p->lds_bytes) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, T.fn[i].bwd, PF_NT, p->lds_bytes) != hipSuccess)
      a = b = 0;
    if (std::min(a, b) < 1 || p->nwg > cus) p->mm_grid = 0;     // (one per CU is all that is relied upon)
  }
  return 0;
}

extern "C" int pmbrl_plan_create(const pmbrl_config* cfg, int device, pmbrl_plan** out) {
  if (!cfg || !out) return fail(-1, "null argument");
  const pmbrl_config& c = *cfg;
  if (c.B < 1 || c.D < 1 || c.U < 1 || c.H < 1) return fail(-2, "B, D, U, H must be >= 1");
  if (c.D > 32 || c.U > 16) return fail(-2, "supported widths: D <= 32, U <= 16");
  if (c.reward.kind != PMBRL_REWARD_LEARNED && c.reward.kind != PMBRL_REWARD_EXTERNAL &&
      (c.reward.k < 1 || c.reward.k > PMBRL_MAX_TIP))
    return fail(-2, "reward.k out of range");
  // (every failure below frees the plan and whatever it already owns)
  std::unique_ptr<pmbrl_plan, void (*)(pmbrl_plan*)> p(new pmbrl_plan(), pmbrl_plan_destroy);
  p->cfg = c;
  if (p->cfg.B_global <= 0) p->cfg.B_global = c.B;
  p->device = device;
  p->sw = read_switches();
  p->replay = p->sw.replay;
  if (int rc = plan_nets(p.get())) return rc;
  int cus = 0;      // (of the device the plan is for, not of the current one)
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  if (int rc = plan_layout(p.get(), cus)) return rc;
  if (int rc = plan_reward(p.get())) return rc;
  if (int rc = plan_angles(p.get())) return rc;
  // stage 5: whether the register-resident family serves the plan (its predicates read the layout alone -- nothing of the
  // dW plan, which asks for them), then the policy's dW GEMM (pm_dw_plan_create, pmbrl_dw.hip; the rules: pmbrl_dw_plan.h)
  p->reg = pm_reg_plan_ok(p.get()) ? 1 : 0;
  p->reg_mm = pm_reg_mm_width(p.get());
  if (int rc = pm_dw_plan_create(p.get(), cus)) return rc;
  if (int rc = plan_workspace(p.get())) return rc;
  if (int rc = plan_attrs(p.get(), cus)) return rc;
  *out = p.release();
  return 0;
}

// ---------------------------------------------------------------------------
// replay of repeated calls (include/pmbrl.h: pmbrl_plan_set_replay)
// ---------------------------------------------------------------------------
static bool per_step_launches(const pmbrl_plan* p) {
  const SweepForm f = sweep_form(p);
  return (f == SweepForm::StepExternal || f == SweepForm::StepInSweep) && p->cfg.H >= 4;
}
static bool replay_wanted(const pmbrl_plan* p) {
  if (p->replay == 0 || p->span || p->coll) return false;
  return p->replay >= 2 || per_step_launches(p);
}
// what makes two calls "the same": every argument byte, kept (a hash alone would replay a stale recording on a collision)
struct ReplayKey {
  unsigned long long h = 1469598103934665603ull;
  std::vector<unsigned char> bytes;
  void add(const void* q, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(q);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    bytes.insert(bytes.end(), b, b + n);
  }
  template <class T> void val(const T& v) { add(&v, sizeof(T)); }
};
// is this stream recording a graph?  (the legacy default stream cannot be asked, and cannot be recording)
static bool pm_stream_recording(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (!s) return false;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
  return cs != hipStreamCaptureStatusNone;
}
// body(): queues the call on s.  Returns its code; *replayed = the call went out as a graph launch.
template <class Body>
static int replay_call(pmbrl_plan* p, int slot, const ReplayKey& K, hipStream_t s, Body body) {
  const unsigned long long key = K.h;
  pmbrl_plan::ReplaySlot& R = p->rp[slot];
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  // (the legacy default stream cannot be asked, and cannot be recording)
  const bool usable = replay_wanted(p) && !p->timing && !p->prof_fwd && !p->prof_bwd && !R.dead &&
                      (!s || (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone));
  if (!usable) {
    if (R.exec || R.seen) replay_drop(p, slot);
    return body(s);
  }
  const bool same = R.key == key && R.bytes == K.bytes;
  if (R.exec && same) {
    HIPCHK(hipGraphLaunch(R.exec, s));
    ++R.launches;
    // (the host-side notes the recorded forward call left: which families' weights it packed, the form of its activity bits)
    if (slot == 0) { p->old_pack_stale = R.aux & 1; p->abits_packed = (R.aux >> 1) & 1; }
    return 0;
  }
  if (!same || R.seen == 0) {      // first sight of these arguments: as usual, remember them
    replay_drop(p, slot);
    R.key = key;
    R.bytes = K.bytes;
    R.seen = 1;
    return body(s);
  }
  // second identical call: record it on a stream of the plan's own (the caller's may be the legacy default stream, which
  // cannot record; nothing runs while recording), then launch what was recorded on the caller's
  hipGraph_t g = nullptr;
  if (!p->cap_stream && hipStreamCreateWithFlags(&p->cap_stream, hipStreamNonBlocking) != hipSuccess) p->cap_stream = nullptr;
  if (!p->cap_stream || hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    R.dead = 1;
    return body(s);
  }
  const int rc = body(p->cap_stream);
  const hipError_t e = hipStreamEndCapture(p->cap_stream, &g);
  if (rc != 0 || e != hipSuccess || !g) {
    // (a call inside invalidated the capture, or the body failed: nothing was queued -- run it eagerly, never try again)
    (void)hipGetLastError();
    if (g) (void)hipGraphDestroy(g);
    R.dead = 1;
    replay_drop(p, slot);
    return rc != 0 ? rc : body(s);
  }
  hipGraphExec_t ex = nullptr;
  const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ei != hipSuccess || !ex) {
    (void)hipGetLastError();
    R.dead = 1;
    replay_drop(p, slot);
    return body(s);
  }
  R.exec = ex;
  R.aux = (p->old_pack_stale & 1) | ((p->abits_packed & 1) << 1);
  HIPCHK(hipGraphLaunch(R.exec, s));
  ++R.launches;
  return 0;
}

extern "C" int pmbrl_plan_set_replay(pmbrl_plan* p, int on) {
  if (!p || on < 0 || on > 2) return fail(-1, "bad argument");
  p->replay = on;
  for (int k = 0; k < 2; ++k) { replay_drop(p, k); p->rp[k].dead = 0; }
  return 0;
}

extern "C" int pmbrl_plan_replay_count(const pmbrl_plan* p, int64_t* n_out) {
  if (!p || !n_out) return fail(-1, "null argument");
  for (int k = 0; k < 2; ++k) n_out[k] = p->rp[k].launches;
  return 0;
}

extern "C" int pmbrl_plan_set_prof(pmbrl_plan* p, long long* fwd_d, long long* bwd_d) {
  if (!p) return fail(-1, "null argument");
  p->prof_fwd = fwd_d;
  p->prof_bwd = bwd_d;
  return 0;
}

extern "C" int pmbrl_plan_set_timing(pmbrl_plan* p, int on) {
  if (!p) return fail(-1, "null argument");
  if (on && !p->ev[0][0]) {
    for (int i = 0; i < PMBRL_TIMER_COUNT; ++i)
      for (int j = 0; j < 2; ++j) HIPCHK(hipEventCreate(&p->ev[i][j]));
  }
  p->timing = on ? 1 : 0;
  for (int i = 0; i < PMBRL_TIMER_COUNT; ++i) p->ev_set[i] = false;
  return 0;
}

extern "C" int pmbrl_plan_read_timing(pmbrl_plan* p, float* ms) {
  if (!p || !ms) return fail(-1, "null argument");
  for (int i = 0; i < PMBRL_TIMER_COUNT; ++i) {
    ms[i] = -1.f;
    if (p->timing && p->ev_set[i]) {
      HIPCHK(hipEventSynchronize(p->ev[i][1]));
      HIPCHK(hipEventElapsedTime(&ms[i], p->ev[i][0], p->ev[i][1]));
    }
  }
  return 0;
}

extern "C" void pmbrl_plan_destroy(pmbrl_plan* p) {
  if (!p) return;
  if (p->ev[0][0])
    for (int i = 0; i < PMBRL_TIMER_COUNT; ++i)
      for (int j = 0; j < 2; ++j) (void)hipEventDestroy(p->ev[i][j]);
  for (int k = 0; k < 2; ++k) replay_drop(p, k);
  if (p->cap_stream) (void)hipStreamDestroy(p->cap_stream);
  if (p->rew_d) (void)hipFree(p->rew_d);
  if (p->wflag_d) (void)hipFree(p->wflag_d);
  if (p->ang_d) (void)hipFree(p->ang_d);
  pm_dw_plan_destroy(p);
  if (p->tail_buf_d) (void)hipFree(p->tail_buf_d);
  delete p;
}

extern "C" int pmbrl_plan_sweep_kernel(const pmbrl_plan* p, int variant, int adjoint, const char** name) {
  if (!p || !name) return fail(-1, "null argument");
  PmInst k{};
  if (variant == PMBRL_SWEEP_REG) k = p->reg ? p->reg_k[0] : k;
  else if (!p->fast) k = p->sweep[0];
  else if (variant >= 0 && variant < PF_VAR_COUNT) k = p->sweep[variant];
  else return fail(-1, "variant out of range");
  const void* f = adjoint ? k.bwd : k.fwd;
  *name = f ? hipKernelNameRefByPtr(f, nullptr) : "";
  if (!*name) *name = "";
  return 0;
}

extern "C" size_t pmbrl_plan_workspace_bytes(const pmbrl_plan* p) { return p ? p->ws_bytes : 0; }

extern "C" int pmbrl_plan_dw_stream(const pmbrl_plan* p, int32_t* out) {
  if (!p || !out) return fail(-1, "null argument");
  out[0] = p->dw.st_on ? p->cfg.H - p->dw.st_cut : -1;
  out[1] = p->dw.st_on ? p->dw.st_wgs : 0;
  return 0;
}

extern "C" int pmbrl_plan_dw_head(const pmbrl_plan* p) { return p && p->dw.st_on && p->dw.st_head ? 1 : 0; }

extern "C" int pmbrl_plan_info(const pmbrl_plan* p, int32_t* info) {
  if (!p || !info) return fail(-1, "null argument");
  memset(info, 0, sizeof(int32_t) * PMBRL_INFO_COUNT);
  info[PMBRL_INFO_ROWS_PER_WG] = p->rows_per_wg;
  info[PMBRL_INFO_N_WG] = p->nwg;
  info[PMBRL_INFO_ROW_TILES] = p->RT;
  info[PMBRL_INFO_LDS_BYTES] = (int32_t)p->lds_bytes;
  info[PMBRL_INFO_N_POL_PARAMS] = (int32_t)p->pol.n_params;
  info[PMBRL_INFO_N_DYN_PARAMS] = (int32_t)p->dyn.n_params;
  info[PMBRL_INFO_DW_SPLITS] = p->dw.args.nsplit;
  info[PMBRL_INFO_MM_MODE] = p->mm_mode;
  info[PMBRL_INFO_LD] = p->LD;
  info[PMBRL_INFO_DW_BLOCKS] = p->dw.n_blocks();
  info[PMBRL_INFO_FAST] = p->fast;
  info[PMBRL_INFO_STAGES] = p->CA * 16 + p->CB;
  info[PMBRL_INFO_MM_GRID] = p->mm_grid;
  info[PMBRL_INFO_PRECISION] = p->prec;
  info[PMBRL_INFO_DW_PIPE] = p->dw.pipe_K;
  info[PMBRL_INFO_MM_PARTS] = p->mm_parts;
  info[PMBRL_INFO_REG] = p->reg;
  info[PMBRL_INFO_REPLAY] = replay_wanted(p) ? 1 : 0;
  info[PMBRL_INFO_INPLACE] = p->inplace;
  info[PMBRL_INFO_REG_FWD_CALLS] = p->reg_calls[0];
  info[PMBRL_INFO_REG_BWD_CALLS] = p->reg_calls[1];
  info[PMBRL_INFO_TAIL_CALLS] = p->tail_calls;
  return 0;
}


// ---------------------------------------------------------------------------
// argument assembly
// ---------------------------------------------------------------------------
static void fill_net(const NetPlan& n, char* ws, const uint16_t* const* masks, NetDev& d) {
  d.nl = n.nl;
  for (int i = 0; i <= n.nl; ++i) {
    d.dim[i] = n.dim[i];
    d.nt[i] = n.nt[i];
  }
  for (int l = 0; l < n.nl; ++l) {
    d.keep[l] = n.keep[l];
    d.inv_keep[l] = 1.f / n.keep[l];
    d.wf[l] = reinterpret_cast<const float*>(ws + n.wf[l]);
    d.wb[l] = reinterpret_cast<const float*>(ws + n.wb[l]);
    d.bias[l] = reinterpret_cast<const float*>(ws + n.bias[l]);
    d.mask[l] = (l < n.nl - 1) ? masks[l] : nullptr;
    d.abits[l] = (l < n.nl - 1) ? reinterpret_cast<uint16_t*>(ws + n.abits[l]) : nullptr;
  }
}

static int fill_args(const pmbrl_plan* p, void* workspace, const pmbrl_inputs* in, RolloutArgs& A) {
  const pmbrl_config& c = p->cfg;
  char* ws = static_cast<char*>(workspace);
  memset(&A, 0, sizeof(A));
  A.B = c.B; A.D = c.D; A.U = c.U; A.H = c.H;
  A.Bg = c.B_global; A.row_off = c.row_offset; A.flags = c.flags;
  A.pol_acts = p->pol.act; A.dyn_acts = p->dyn.act;   // (read by the ACT instances only)
  A.G = p->G; A.M = p->M; A.mm_mode = p->mm_mode;
  A.t0 = 0; A.t1 = c.H;
  A.rows_per_wg = p->rows_per_wg; A.nwg = p->nwg; A.Rw = 16 * p->RT; A.LD = p->LD; A.LDB = p->LDB;
  A.mls_pol = c.max_log_std_pol; A.mls_dyn = c.max_log_std_dyn;
  for (int l = 0; l < p->pol.nl - 1; ++l)
    if (!in->pol_mask_bits_d[l]) return fail(-1, "missing policy mask bits");
  for (int l = 0; l < p->dyn.nl - 1; ++l)
    if (!in->dyn_mask_bits_d[l]) return fail(-1, "missing dynamics mask bits");
  fill_net(p->pol, ws, in->pol_mask_bits_d, A.pol);
  fill_net(p->dyn, ws, in->dyn_mask_bits_d, A.dyn);
  A.rew = p->rew_d;     // (nullptr: the learned reward head, see RolloutArgs::Jx)
  A.ang = p->ang_d;
  A.x0 = in->x0_d; A.mx = in->mx_d; A.iSx = in->iSx_d; A.my = in->my_d; A.Sy = in->Sy_d;
  A.pscale = in->pol_scale_d; A.pbias = in->pol_bias_d;
  A.zpol = in->z_pol_d; A.zdyn = in->z_dyn_d; A.zmm = in->z_mm_d; A.zrr = in->z_rr_d;
  A.zpol_ss = in->z_pol_step_stride; A.zdyn_ss = in->z_dyn_step_stride;
  if (!A.x0 || !A.mx || !A.iSx || !A.my || !A.Sy || !A.pscale || !A.pbias || !A.zpol || !A.zdyn)
    return fail(-1, "null input pointer");
  if ((c.flags & PMBRL_FLAG_MM_STATES) && !A.zmm) return fail(-1, "mm_states needs z_mm");
  if ((c.flags & PMBRL_FLAG_MM_REWARDS) && !A.zrr) return fail(-1, "mm_rewards needs z_rr");
  for (int l = 0; l < p->pol.nl; ++l) {
    A.actT[l] = reinterpret_cast<float*>(ws + p->off_actT[l]);
    A.gT[l] = reinterpret_cast<float*>(ws + p->off_gT[l]);
  }
  A.Tp = reinterpret_cast<float*>(ws + p->off_Tp);
  A.Td = reinterpret_cast<float*>(ws + p->off_Td);
  A.gmm_n = p->cfg.dyn_components > 1 ? p->cfg.dyn_components : 0;
  A.zpi = A.ucat = A.zdyn_grad = nullptr;
  A.gmm_k = nullptr;
  A.gmm_c = nullptr;
  if (A.gmm_n) {
    if (!in->z_pi_d || !in->u_cat_d) return fail(-1, "mixture head: z_pi_d and u_cat_d are required");
    if (in->z_dyn_step_stride == 0) return fail(-1, "mixture head: z_dyn_d must be a per-step draw [H, B, D]");
    A.zpi = in->z_pi_d;
    A.ucat = in->u_cat_d;
    // the reference's autograd differentiates the noise term with the LAST step's noise at every step
    if (!(p->cfg.flags & PMBRL_FLAG_GMM_EXACT_NOISE_GRAD))
      A.zdyn_grad = in->z_dyn_d + (size_t)(p->cfg.H - 1) * in->z_dyn_step_stride;
    A.gmm_c = reinterpret_cast<float*>(ws + p->off_gmm_c);
    A.gmm_k = reinterpret_cast<int*>(ws + p->off_gmm_k);
  }
  A.xt = reinterpret_cast<float*>(ws + p->off_xt);
  A.rt = reinterpret_cast<float*>(ws + p->off_rt);
  A.mmfac = reinterpret_cast<double*>(ws + p->off_mmfac);
  A.mmfac_groups = p->mm_mode == 1 ? c.B / p->M : 0;
  A.Jx = reinterpret_cast<float*>(ws + p->off_Jx);
  A.Ja = reinterpret_cast<float*>(ws + p->off_Ja);
  A.gx_carry = reinterpret_cast<float*>(ws + p->off_gxc);
  A.mm_grid = p->mm_grid;
  A.mm_parts = p->mm_parts;
  A.mm_fan = p->mm_fan;
  A.mm_ztab = (p->mm_fan || p->reg_mm) ? reinterpret_cast<const double*>(ws + p->off_ztab) : nullptr;
  A.gsync = reinterpret_cast<unsigned*>(ws + p->off_gsync);
  A.xch = p->xch_bytes ? reinterpret_cast<unsigned long long*>(ws + p->off_xch) : nullptr;
  A.gx_carry_out = nullptr;
  if (p->fast) {
    // weight streams (hidden->hidden layers) and the per-layer LDS offsets
    const NetDev& P = A.pol;
    const NetDev& F = A.dyn;
    const int pm = p->CA + p->CB;
    auto padk = [pm](int nkb) { return (nkb + pm - 1) / pm * pm; };
    // streamed layer: weights, output tiles, padded / real k-blocks; a layer with 4m+1 output
    // tiles hands its last tile to the K-split path (pm_fast_ksplit)
    auto add_stream = [&](StreamDesc& sd, const float* wf, int n_ot, int n_kb_real, int& tw_off) {
      const int i = sd.n++;
      sd.wf[i] = wf;
      // split precision: the stream counts 1 KiB weight loads = pieces of K32 blocks (3 per block in the
      // forward sweep's table, 2 in the adjoint's)
      const int np = (&sd == &A.sd_fwd && p->prec != PMBRL_PREC_SPLIT_F16) ? 3 : 2;
      sd.n_kb[i] = p->prec ? padk((n_kb_real + 1) / 2) * np : padk(n_kb_real);
      sd.n_kb_real[i] = n_kb_real;
      sd.ks[i] = pm_fast_ksplit(n_ot, p->RT, p->prec) ? 1 : 0;
      sd.n_ot[i] = n_ot - sd.ks[i];
      sd.tw_off[i] = tw_off;
      if (sd.ks[i]) tw_off += n_kb_real * 256;
    };
    StreamDesc& f = A.sd_fwd;
    f.n = 0;
    int twf = 0, twb = 0;
    for (int l = 1; l < P.nl - 1; ++l) add_stream(f, P.wf[l], P.nt[l + 1], P.nt[l], twf);
    for (int l = 1; l < F.nl - 1; ++l) add_stream(f, F.wf[l], F.nt[l + 1], F.nt[l], twf);
    StreamDesc& b = A.sd_bwd;
    b.n = 0;
    for (int l = F.nl - 2; l >= 1; --l) add_stream(b, F.wb[l], F.nt[l], F.nt[l + 1], twb);
    for (int l = P.nl - 2; l >= 1; --l) add_stream(b, P.wb[l], P.nt[l], P.nt[l + 1], twb);
    const PmFastMap m = pm_fast_map(16 * p->RT, p->LD, c.D, c.U, p->RT, P.nt, P.nl, F.nt, F.nl, 0, p->prec);
    for (int l = 0; l < P.nl; ++l) A.fo.pbias[l] = (int)m.pbias[l];
    for (int l = 0; l < F.nl; ++l) A.fo.dbias[l] = (int)m.dbias[l];
    for (int l = 0; l < P.nl - 1; ++l) A.fo.pmask[l] = (int)m.pmask[l];
    for (int l = 0; l < F.nl - 1; ++l) A.fo.dmask[l] = (int)m.dmask[l];
  }
  if (in->pol_params_d && in->dyn_params_d) {
    A.pol_head_w = in->pol_params_d + p->pol.w_off[p->pol.nl - 1];
    A.dyn_head_w = in->dyn_params_d + p->dyn.w_off[p->dyn.nl - 1];
    A.pol_first_w = in->pol_params_d + p->pol.w_off[0];
    A.dyn_first_w = in->dyn_params_d + p->dyn.w_off[0];
  }
  // (plan_attrs resolved every variant the plan's calls can ask for -- LEAN and EXT, or MM / MMG; never a null launch)
  const int var = p->fast ? fast_variant(p->RT, A) : 0;
  if (!p->sweep[var].fwd || (var == PF_VAR_LEAN && p->fast && !p->sweep[PF_VAR_EXT].fwd))
    return fail(-3, "the plan resolved no sweep kernel for this call's variant");
  return 0;
}

static void pack_jobs(const NetPlan& n, char* ws, const float* params, int pair_kb, PackArgs& P, int prec = 0,
                      bool general = false) {
  for (int l = 0; l < n.nl; ++l) {
    const int O = n.dim[l + 1], K = n.dim[l];
    if (general && prec) {
      // general family on split operands: every layer as two piece planes of whole K32 blocks
      P.job[P.n++] = PackJob{params + n.w_off[l], reinterpret_cast<float*>(ws + n.wf[l]), O, K, 0, 1, 0, 2, 1};
      P.job[P.n++] = PackJob{params + n.w_off[l], reinterpret_cast<float*>(ws + n.wb[l]), O, K, 1, 1, 0, 2, 0};
      P.job[P.n++] = PackJob{params + n.b_off[l], reinterpret_cast<float*>(ws + n.bias[l]), O, K, 0, 1, 1, 0, 0};
      continue;
    }
    // hidden->hidden layers feed the streamed GEMMs of the fast kernels: k-blocks padded to CA+CB
    const int mult = (pair_kb >= 1 && l >= 1 && l <= n.nl - 2) ? pair_kb : 1;
    // split precision: bf16 pieces for every product with K = a hidden width -- forward: hidden->hidden layers
    // (streamed, padded to stage pairs) and the head (3 pieces); adjoint: their transposes and the tail (2 pieces)
    const bool hid_in = l >= 1, hid_out = l <= n.nl - 2;   // K is a hidden width forward / in the transposed product
    const int pf = (prec && hid_in) ? (prec == PMBRL_PREC_SPLIT_F16 ? 2 : 3) : 0, pb = (prec && hid_out) ? 2 : 0;
    const int mf = pf ? ((l <= n.nl - 2) ? pair_kb : 1) : mult, mb = pb ? ((l >= 1) ? pair_kb : 1) : mult;
    P.job[P.n++] = PackJob{params + n.w_off[l], reinterpret_cast<float*>(ws + n.wf[l]), O, K, 0, mf, 0, pf,
                           prec == PMBRL_PREC_SPLIT_F16 ? 1 : 0};
    P.job[P.n++] = PackJob{params + n.w_off[l], reinterpret_cast<float*>(ws + n.wb[l]), O, K, 1, mb, 0, pb, 0};
    P.job[P.n++] = PackJob{params + n.b_off[l], reinterpret_cast<float*>(ws + n.bias[l]), O, K, 0, 1, 1, 0, 0};
  }
}

// Tiles of the streamed layers that a 16-row split-precision sweep holds outside the weight stream, whose table then
// starts behind them.  k: the instance that will run.
static void resident_tiles(const pmbrl_plan* p, const PmInstKey& k, RolloutArgs& A, bool fwd) {
  StreamDesc& sd = fwd ? A.sd_fwd : A.sd_bwd;
  const int np = (fwd && p->prec != PMBRL_PREC_SPLIT_F16) ? 3 : 2;
  if (!p->prec || p->RT != 1 || p->CA + p->CB != 7 || np != 2) return;
  // Register-resident first tiles (pmbrl_fast.h, resident_tile_s): the plain variants keep output tile `wave` of the
  // sweep's first streamed layer in registers when a tile is exactly one stage pair and two pieces wide; the stream
  // table then starts at tile 8 of that layer.
  if ((k.var == PF_VAR_LEAN || k.var == PF_VAR_EXT) && sd.n >= 1 && sd.n_kb[0] == 7 * np && sd.n_ot[0] > 8) {
    A.res_tiles = 8;
    A.res_w = sd.wf[0];
    sd.wf[0] += (size_t)8 * sd.n_kb[0] * 256;
    sd.n_ot[0] -= 8;
  }
  // LDS-resident tiles (lds_tile_s): tiles 0..7 of the SECOND streamed layer, in the LDS the plan reserved
  if (lds_tiles_row(p, k)) {
    A.lds_w = sd.wf[1];
    A.wlds_off = p->wlds_off;
    A.lds_last_lanes = p->lds_last_lanes;
    sd.wf[1] += (size_t)8 * sd.n_kb[1] * 256;
    sd.n_ot[1] -= 8;
  }
}
// one sweep on the kernels the plan resolved (plan_attrs); the latency-optimised family picks the variant per call
static void launch_sweep(const pmbrl_plan* p, const RolloutArgs& A0, hipStream_t s, bool fwd) {
  const int var = p->fast ? fast_variant(p->RT, A0) : 0;
  const void* k = fwd ? p->sweep[var].fwd : p->sweep[var].bwd;
  RolloutArgs A = A0;
  void* args[] = {&A};
  if (!p->fast) {
    (void)hipLaunchKernel(k, dim3(p->nwg), dim3(PM_NT), args, p->lds_bytes, s);
    return;
  }
  resident_tiles(p, p->sweep_key[var], A, fwd);
  // (more groups than fit the chip at once: batches of whole groups, one launch each -- pmbrl_host.h, mm_gpb)
  const int per = (p->mm_gpb > 0 && A0.mm_mode == 1) ? p->mm_gpb * p->mm_parts : p->nwg;
  for (int w0 = 0; w0 < p->nwg; w0 += per) {
    A.wg0 = w0;
    A.launch_wg = std::min(per, p->nwg - w0);
    (void)hipLaunchKernel(k, dim3(A.launch_wg), dim3(PF_NT), args, p->lds_bytes, s);
  }
}
static void launch_fwd_rt(const pmbrl_plan* p, const RolloutArgs& A, hipStream_t s) { launch_sweep(p, A, s, true); }
static void launch_bwd_rt(const pmbrl_plan* p, const RolloutArgs& A, hipStream_t s) { launch_sweep(p, A, s, false); }

// groups spread over ranks (pmbrl_mmx.h): the in-place fp64 sum of the statistics buffer over the ranks
static int mmx_exchange(pmbrl_plan* p, hipStream_t s, double* buf, size_t n) {
  if (!p->coll) return 0;   // one rank (check_collective): the sum over the ranks is the identity
  if (int rc = p->coll(p->coll_ctx, (void*)s, buf, (int64_t)n)) return fail(-4, "statistics all-reduce failed (" + std::to_string(rc) + ")");
  return 0;
}
// ... which more than one rank cannot do without a collective: refused by both calls before they queue anything
static int check_collective(const pmbrl_plan* p) {
  if (p->span && p->cfg.mm_span_ranks != 1 && !p->coll)
    return fail(-3, "moment-matching groups spread over ranks: attach a collective first (pmbrl_plan_set_comm / pmbrl_plan_set_collective)");
  return 0;
}
// dynamic LDS of pm_mmx_apply_kernel: room for the slots of every (rank, workgroup) if that fits (pmbrl_mmx.h)
static size_t mmx_apply_lds(int d, const MmxArgs& X, size_t other) {
  const size_t want = pm_mmx_apply_lds_doubles(d, X.nranks * X.nb) * sizeof(double);
  return want <= PM_MMX_LDS_MAX ? std::max(want, other) : other;
}
// one exchange's launch shape: the states of step t (width D, G groups, the sums of a group over X.nb workgroups) or the
// rewards of all steps at once (width 1, H x G items of one workgroup with fewer waves each)
struct MmxShape {
  MmxArgs X;
  int d, items, nw, nws;   // waves of the apply / of the statistics workgroups
  size_t scr;
};
static MmxShape mmx_shape(const pmbrl_plan* p, char* ws, bool rewards, int t) {
  MmxShape S;
  MmxArgs& X = S.X;
  X.nranks = p->cfg.mm_span_ranks;
  X.rank = p->cfg.mm_span_rank;
  X.span_rows = p->cfg.mm_span_rows;
  X.span_off = p->cfg.mm_span_offset;
  X.buf = reinterpret_cast<double*>(ws + p->off_mmx_buf);
  X.fac = reinterpret_cast<double*>(ws + (rewards ? p->off_mmx_rfac : p->off_mmx_fac));
  X.nb = rewards ? 1 : pm_mmx_blocks(p->M);
  if (!rewards) X.fac += (size_t)t * p->G * pm_mm_fac_doubles(p->cfg.D);
  S.d = rewards ? 1 : p->cfg.D;
  S.items = rewards ? p->cfg.H * p->G : p->G;
  S.nw = rewards ? std::min(4, pm_mmx_waves(p->M, 1)) : pm_mmx_waves(p->M, p->cfg.D);
  S.nws = rewards ? S.nw : pm_mmx_waves((p->M + X.nb - 1) / X.nb, p->cfg.D);
  S.scr = pm_mmx_lds_doubles(S.d, S.nw) * sizeof(double);
  return S;
}
// forward: own statistics -> sum over the ranks -> factor + own rows.  (Here and in mmx_bwd the branches name the kernel
// instances in the order the device code object has always laid them out: states first forward, rewards first adjoint)
static int mmx_fwd(pmbrl_plan* p, char* ws, const RolloutArgs& A, bool rewards, int t, hipStream_t s) {
  const MmxShape S = mmx_shape(p, ws, rewards, t);
  const dim3 gs(S.items * S.X.nb, S.X.nranks), bs(64 * S.nws), ga(S.items), ba(64 * S.nw);
  const size_t n = (size_t)S.X.nranks * S.X.nb * S.items * pm_mmx_slot_doubles(S.d), lds = mmx_apply_lds(S.d, S.X, S.scr);
  if (!rewards) {
    hipLaunchKernelGGL(pm_mmx_stats_kernel<0>, gs, bs, S.scr, s, A, S.X, t);
    if (int rc = mmx_exchange(p, s, S.X.buf, n)) return rc;
    hipLaunchKernelGGL(pm_mmx_apply_kernel<0>, ga, ba, lds, s, A, S.X, t);
  } else {
    hipLaunchKernelGGL(pm_mmx_stats_kernel<1>, gs, bs, S.scr, s, A, S.X, t);
    if (int rc = mmx_exchange(p, s, S.X.buf, n)) return rc;
    hipLaunchKernelGGL(pm_mmx_apply_kernel<1>, ga, ba, lds, s, A, S.X, t);
  }
  return 0;
}
// adjoint: own sums -> sum over the ranks -> own rows (grt: where the rewards' adjoint leaves dL/dr~)
static int mmx_bwd(pmbrl_plan* p, char* ws, const RolloutArgs& A, bool rewards, int t, float* grt, hipStream_t s) {
  const MmxShape S = mmx_shape(p, ws, rewards, t);
  const dim3 gs(S.items * S.X.nb), bs(64 * S.nws), ga(S.items), ba(64 * S.nw);
  const size_t n = (size_t)S.X.nb * S.items * pm_mmx_bwd_doubles(S.d);
  if (rewards) {
    hipLaunchKernelGGL(pm_mmx_bwd_sums_kernel<1>, gs, bs, S.scr, s, A, S.X, t);
    if (int rc = mmx_exchange(p, s, S.X.buf, n)) return rc;
    hipLaunchKernelGGL(pm_mmx_bwd_apply_kernel<1>, ga, ba, S.scr, s, A, S.X, t, grt);
  } else {
    hipLaunchKernelGGL(pm_mmx_bwd_sums_kernel<0>, gs, bs, S.scr, s, A, S.X, t);
    if (int rc = mmx_exchange(p, s, S.X.buf, n)) return rc;
    hipLaunchKernelGGL(pm_mmx_bwd_apply_kernel<0>, ga, ba, S.scr, s, A, S.X, t, grt);
  }
  return 0;
}

// groups split over workgroups (mm_parts > 1), before a whole-horizon sweep: the group-local barrier flags and the tags of
// the exchange granules.  The latency-optimised family counts both from zero in every launch.  The register-resident
// family (reg_now) touches no flags and tags its granules with a launch generation instead -- once zeroed, never again:
// four 5 us fill kernels less per iteration.
// (A RECORDED launch is replayed with the generation it was recorded with: two replays of a forward call with no
//  adjoint call between them would meet their own tags of the replay before -- stale sums accepted.  A recording
//  therefore carries the fill; what it leaves behind is its generation's tags, which no later launch takes for its own)
static int xch_prepare(pmbrl_plan* p, const RolloutArgs& A, bool reg_now, hipStream_t s) {
  if (p->mm_parts <= 1) return 0;
  if (!reg_now) HIPCHK(hipMemsetAsync(A.gsync, 0, 1024 * sizeof(unsigned), s));
  const bool rec = pm_stream_recording(s);
  if (A.xch && (!reg_now || !p->xch_zeroed || rec)) {
    HIPCHK(hipMemsetAsync(A.xch, 0, p->xch_bytes, s));
    p->xch_zeroed = (reg_now && !rec) ? 1 : 0;
  }
  return 0;
}

// the sweep families' fragment-packed weights of this call's parameters (pm_pack_all); status_d: the forward
// sweep's status word, reset by the launch (nullptr: leave it)
static void launch_pack_all(pmbrl_plan* p, char* ws, const pmbrl_inputs* in, hipStream_t s, int32_t* status_d) {
  PackArgs PK;
  PK.n = 0;
  pack_jobs(p->pol, ws, in->pol_params_d, p->fast ? p->CA + p->CB : 0, PK, p->prec, !p->fast);
  pack_jobs(p->dyn, ws, in->dyn_params_d, p->fast ? p->CA + p->CB : 0, PK, p->prec, !p->fast);
  PK.status = status_d;
  PK.wflag = p->prec == PMBRL_PREC_SPLIT_F16 ? p->wflag_d : nullptr;
  PK.gen = p->wgen;
  pm_pack_all_launch(PK, s);
}

// the arguments of one pmbrl_rollout_fwd call: filled once by the entry point (which also derives the replay key from them)
struct FwdCall {
  hipStream_t stream;
  void* workspace;
  const pmbrl_inputs* in;
  float *states, *actions, *rewards;
  int32_t* status;
};

// every refusal that depends on the plan and the arguments alone: nothing has been queued when one is returned
static int check_fwd(const pmbrl_plan* p, const FwdCall& C) {
  if (!p || !C.workspace || !C.in || !C.states || !C.actions || !C.rewards || !C.status) return fail(-1, "null argument");
  if (!C.in->pol_params_d || !C.in->dyn_params_d) return fail(-1, "null parameter pointer");
  return check_collective(p);
}

// stage 1: the weights of this call's parameters in the form the sweep's family reads.  *ztab_done: the noise table of split
// moment-matching groups rode along
static int fwd_pack(pmbrl_plan* p, const FwdCall& C, const RolloutArgs& A, bool reg_fwd, bool* ztab_done) {
  hipStream_t s = C.stream;
  char* ws = static_cast<char*>(C.workspace);
  ScopedTimer tm(p, PMBRL_TIMER_PACK, s);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(s, &cap);
  // (the flag only ever grows: start over before the counter wraps -- and in every recorded call, whose replays all
  //  carry the generation number of the recording)
  if (p->wgen >= 0x7ffffff0 || cap == hipStreamCaptureStatusActive) {
    HIPCHK(hipMemsetAsync(p->wflag_d, 0, sizeof(int), s));
    if (p->wgen >= 0x7ffffff0) p->wgen = 0;
  }
  ++p->wgen;
  // the register-resident family serves this call (pmbrl_reg.h): only ITS weights are packed now -- the
  // latency-optimised family's are packed by the adjoint call if it turns out to need them (optional outputs)
  if (!reg_fwd) launch_pack_all(p, ws, C.in, s, C.status);
  p->old_pack_stale = reg_fwd ? 1 : 0;
  p->abits_packed = reg_fwd ? 1 : 0;
  // (the noise table of split moment-matching groups rides in the same launch: extra workgroups, PMBRL_ZTAB_MERGE=0 for
  //  the launch of its own)
  ZtabArgs Zt;
  Zt.n_blocks = 0;
  if (p->reg && reg_fwd && (p->mm_fan || p->reg_mm) && p->mm_mode == 1 && p->sw.ztab_merge) {
    Zt = pm_ztab_args(p, A);
    *ztab_done = true;
  }
  if (p->reg)
    pm_reg_pack_launch(p, ws, C.in->pol_params_d, C.in->dyn_params_d, p->wflag_d, p->wgen, s, reg_fwd ? C.status : nullptr, &Zt);
  return 0;
}

// stage 2, SweepForm::Barrier: one launch; the workgroups meet after every step and moment-match the sampled states (x_H included)
static int fwd_sweep_barrier(pmbrl_plan* p, const FwdCall& C, RolloutArgs A) {
  HIPCHK(hipMemsetAsync(A.gsync, 0, 1024 * sizeof(unsigned), C.stream));
  A.t0 = 0; A.t1 = p->cfg.H;
  launch_fwd_rt(p, A, C.stream);
  return 0;
}

// SweepForm::StepInSweep: one launch per step; step t's launch first moment-matches the states sampled by step t-1
static int fwd_sweep_steps(pmbrl_plan* p, const FwdCall& C, RolloutArgs A) {
  for (int t = 0; t < p->cfg.H; ++t) {
    A.t0 = t; A.t1 = t + 1;
    launch_fwd_rt(p, A, C.stream);
  }
  A.flags &= ~PMBRL_FLAG_MM_REWARDS;
  hipLaunchKernelGGL(pm_mm_fwd_kernel, dim3(p->G), dim3(PM_MM_NW * 64),
                     pm_mm_kernel_doubles(p->cfg.D) * sizeof(double), C.stream, A, p->cfg.H - 1);   // x_H
  return 0;
}

// the sweep's own arguments where the rewards are formed behind it
static RolloutArgs fwd_sweep_args(const pmbrl_plan* p, const RolloutArgs& A) {
  RolloutArgs As = A;
  if (!p->fast) { As.ext_reward = 1; As.flags &= ~PMBRL_FLAG_MM_REWARDS; }   // general family: rewards after the sweep
  if (p->learned && (p->cfg.flags & PMBRL_FLAG_MM_REWARDS)) As.rewards = As.rt;     // (learned reward head: r~ before its moment matching)
  return As;
}

// SweepForm::Whole: the whole horizon in one launch of the register-resident or the latency-optimised / general family
static int fwd_sweep_whole(pmbrl_plan* p, const FwdCall& C, const RolloutArgs& A, bool ztab_done) {
  hipStream_t s = C.stream;
  const RolloutArgs As = fwd_sweep_args(p, A);
  if ((p->mm_fan || p->reg_mm) && !ztab_done) {
    const ZtabArgs Z = pm_ztab_args(p, As);
    hipLaunchKernelGGL(pm_mm_ztable_kernel, dim3(Z.n_blocks), dim3(256), 0, s, Z);
  }
  const bool reg_now = pm_reg_can_run(p, As, true);
  if (int rc = xch_prepare(p, As, reg_now, s)) return rc;
  if (reg_now) pm_reg_launch(p, static_cast<char*>(C.workspace), As, C.in->pol_params_d, C.in->dyn_params_d, s, true);
  else launch_fwd_rt(p, As, s);
  return 0;
}

// SweepForm::StepExternal: one launch per step, the moment matching of its states in kernels of their own behind it
static int fwd_sweep_external(pmbrl_plan* p, const FwdCall& C, const RolloutArgs& A) {
  hipStream_t s = C.stream;
  char* ws = static_cast<char*>(C.workspace);
  const size_t smem = pm_mm_kernel_doubles(p->cfg.D) * sizeof(double);
  RolloutArgs Am = A, As = fwd_sweep_args(p, A);
  Am.flags &= ~PMBRL_FLAG_MM_REWARDS;   // both families: rewards are handled after the sweep
  for (int t = 0; t < p->cfg.H; ++t) {
    As.t0 = t; As.t1 = t + 1;
    launch_fwd_rt(p, As, s);
    if (p->mm_wide) {
      hipLaunchKernelGGL(pm_mmw_fwd_kernel, dim3(p->G), dim3(PM_MMW_NT), pm_mmw_lds_bytes(p->M, p->cfg.D, false), s, Am, t,
                         reinterpret_cast<double*>(ws + p->off_mmfac));
    } else if (!p->span) {
      hipLaunchKernelGGL(pm_mm_fwd_kernel, dim3(p->G), dim3(PM_MM_NW * 64), smem, s, Am, t);
    } else if (p->cfg.flags & PMBRL_FLAG_MM_STATES) {
      if (int rc = mmx_fwd(p, ws, Am, false, t, s)) return rc;
    }
  }
  return 0;
}

// stage 3: rewards (+ Jacobians) of all row-steps in one parallel pass, then their moment matching
static int fwd_rewards(pmbrl_plan* p, const FwdCall& C, const RolloutArgs& A) {
  hipStream_t s = C.stream;
  const long long n = (long long)p->cfg.H * p->cfg.B;
  if (p->learned)     // (the sweep sampled r~ and checked it: what is left of this launch's duties)
    hipLaunchKernelGGL(pm_reward_learned_kernel, dim3(1), dim3(64), 0, s, A);
  else
    hipLaunchKernelGGL(pm_reward_kernel_for(p->cfg.U, p->rew_k), dim3((unsigned)((n + 255) / 256)), dim3(256),
                       (size_t)256 * (p->cfg.D | 1) * sizeof(float), s, A);
  if (!(p->cfg.flags & PMBRL_FLAG_MM_REWARDS)) return 0;
  if (p->span) return mmx_fwd(p, static_cast<char*>(C.workspace), A, true, 0, s);   // one exchange for the whole horizon
  hipLaunchKernelGGL(pm_mm_rewards_fwd_kernel, dim3(p->cfg.H * p->G), dim3(64), pm_mmr_lds_bytes(p->M, 2), s, A);
  return 0;
}

static int rollout_fwd_impl(pmbrl_plan* p, const FwdCall& C) {
  hipStream_t s = C.stream;
  RolloutArgs A;
  if (int rc = fill_args(p, C.workspace, C.in, A)) return rc;
  A.states = C.states; A.actions = C.actions; A.rewards = C.rewards; A.status = C.status;
  A.prof = p->prof_fwd;
  const bool reg_fwd = pm_reg_can_run(p, A, true);
  bool ztab_done = false;
  if (int rc = fwd_pack(p, C, A, reg_fwd, &ztab_done)) return rc;
  A.wflag = p->prec == PMBRL_PREC_SPLIT_F16 ? p->wflag_d : nullptr;
  A.wgen = p->wgen;
  {
    ScopedTimer tm(p, PMBRL_TIMER_FWD, s);
    int rc = 0;
    switch (sweep_form(p)) {
      case SweepForm::Barrier: rc = fwd_sweep_barrier(p, C, A); break;
      case SweepForm::StepInSweep: rc = fwd_sweep_steps(p, C, A); break;
      case SweepForm::Whole: rc = fwd_sweep_whole(p, C, A, ztab_done); break;
      case SweepForm::StepExternal: rc = fwd_sweep_external(p, C, A); break;
    }
    if (rc) return rc;
  }
  // (a reward evaluated by the caller: stage 3 and the loss are pmbrl_rollout_rewards' -- rewards_d is left alone)
  if (!p->ext) {
    ScopedTimer tm(p, PMBRL_TIMER_REWARD, s);
    if (int rc = fwd_rewards(p, C, A)) return rc;
    // the loss (pmbrl_plan_set_loss).  (Folding this sum into the reward launch -- per-block partials, last block finishes --
    // was measured: the reward launch grew by what the separate reduction costs, 391 arrivals on one counter; not kept)
    if (p->loss_w)
      launch_weighted_sum(s, C.rewards, p->loss_w, (long long)p->cfg.H * p->cfg.B, p->loss_out, C.status, p->cfg.B);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int pmbrl_rollout_fwd(pmbrl_plan* p, void* stream, void* workspace, const pmbrl_inputs* in,
                                 float* states_d, float* actions_d, float* rewards_d,
                                 int32_t* status_d) {
  const FwdCall C{(hipStream_t)stream, workspace, in, states_d, actions_d, rewards_d, status_d};
  if (int rc = check_fwd(p, C)) return rc;
  HIPCHK(hipSetDevice(p->device));
  ReplayKey K;
  K.val(C.stream); K.val(C.workspace); K.add(C.in, sizeof(*C.in));
  K.val(C.states); K.val(C.actions); K.val(C.rewards); K.val(C.status); K.val(p->loss_w); K.val(p->loss_out);
  const int rc = replay_call(p, 0, K, C.stream, [&](hipStream_t on) {
    FwdCall Con = C;
    Con.stream = on;
    return rollout_fwd_impl(p, Con);
  });
  if (p->ext) {      // (host-side notes, taken here and not in the body: a replayed call leaves them too)
    p->ext_state = rc == 0 ? 1 : 0;
    p->ext_in = *C.in;
    p->ext_states = C.states;
    p->ext_actions = C.actions;
  }
  return rc;
}

// ---------------------------------------------------------------------------
// a reward evaluated by the caller (PMBRL_REWARD_EXTERNAL): where its argument lives, and the rest of the forward call
// ---------------------------------------------------------------------------
extern "C" int pmbrl_plan_reward_input(const pmbrl_plan* p, int64_t* ws_offset_out) {
  if (!p || !ws_offset_out) return fail(-1, "null argument");
  *ws_offset_out = (p->cfg.flags & PMBRL_FLAG_MM_STATES) ? (int64_t)p->off_xt : -1;
  return 0;
}

extern "C" int pmbrl_rollout_rewards(pmbrl_plan* p, void* stream, void* workspace, const float* r_d, const float* jx_d,
                                     const float* ja_d, float* rewards_d, int32_t* status_d) {
  if (!p) return fail(-1, "null plan");
  if (!p->ext) return fail(-2, "pmbrl_rollout_rewards: the plan's reward kind is not PMBRL_REWARD_EXTERNAL");
  if (!workspace || !r_d || !rewards_d || !status_d) return fail(-1, "null argument");
  if ((jx_d == nullptr) != (ja_d == nullptr))
    return fail(-1, "pmbrl_rollout_rewards: jx_d and ja_d go together (both NULL: a forward-only rollout)");
  if (p->ext_state == 0) return fail(-3, "pmbrl_rollout_rewards: no pmbrl_rollout_fwd call on this plan before it");
  if (int rc = check_collective(p)) return rc;
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  RolloutArgs A;
  if (int rc = fill_args(p, workspace, &p->ext_in, A)) return rc;
  A.states = p->ext_states; A.actions = p->ext_actions; A.rewards = rewards_d; A.status = status_d;
  const pmbrl_config& c = p->cfg;
  const bool mmr = (c.flags & PMBRL_FLAG_MM_REWARDS) != 0;
  ScopedTimer tm(p, PMBRL_TIMER_REWARD, s);
  RewardExtArgs R;
  R.r = r_d; R.jx = jx_d; R.ja = ja_d;
  R.x = (c.flags & PMBRL_FLAG_MM_STATES) ? A.xt : A.states + (size_t)c.B * c.D;
  R.dst_r = mmr ? A.rt : A.rewards;
  R.Jx = A.Jx; R.Ja = A.Ja;
  R.status = status_d;
  R.H = c.H; R.B = c.B; R.D = c.D; R.U = c.U;
  pm_reward_ext_launch(R, s);
  p->ext_state = jx_d ? 3 : 2;
  // behind it, what fwd_rewards queues behind the analytic launch: the rewards' moment matching, then the loss
  if (mmr) {
    if (p->span) {
      if (int rc = mmx_fwd(p, static_cast<char*>(workspace), A, true, 0, s)) return rc;
    } else {
      hipLaunchKernelGGL(pm_mm_rewards_fwd_kernel, dim3(c.H * p->G), dim3(64), pm_mmr_lds_bytes(p->M, 2), s, A);
    }
  }
  if (p->loss_w) launch_weighted_sum(s, rewards_d, p->loss_w, (long long)c.H * c.B, p->loss_out, status_d, c.B);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int pmbrl_plan_set_loss(pmbrl_plan* p, const float* loss_weights_d, float* loss_out_d) {
  if (!p || (loss_weights_d && !loss_out_d)) return fail(-1, "bad argument");
  p->loss_w = loss_weights_d;
  p->loss_out = loss_weights_d ? loss_out_d : nullptr;
  return 0;
}

extern "C" int pmbrl_plan_set_optimizer(pmbrl_plan* p, const pmbrl_opt_rule* rule) {
  if (!p) return fail(-1, "null plan");
  if (!rule) { p->has_opt_rule = 0; return 0; }
  if (int rc = pmbrl_opt_rule_check(rule, (int64_t)p->pol.n_params)) return rc;
  p->opt_rule = *rule;
  p->has_opt_rule = 1;
  return 0;
}

// the in-place fp32 sum over the ranks through the plan's gradient transport (pmbrl_plan_set_grad_comm)
static int tail_allreduce(pmbrl_plan* p, hipStream_t s, float* buf_d, int64_t n) {
  if (p->grad_p2p) return pmbrl_p2p_allreduce_f32(p->grad_p2p, s, buf_d, n);
  return pmbrl_allreduce_sum(p->grad_comm, s, buf_d, n);
}

// the arguments of one pmbrl_rollout_bwd(_adam) call: filled once by the entry point (opt: nullptr without the optimiser)
struct BwdCall {
  hipStream_t stream;
  void* workspace;
  const pmbrl_inputs* in;
  const float *states, *actions, *rewards;
  const float *grad_rewards, *grad_states, *grad_actions;
  float *grad_pol_flat, *grad_x0, *action_grad_norms;
  int32_t* status;
  const pmbrl_adam* opt;
};
// rows sharded over ranks, optimiser attached (pmbrl_plan_set_grad_comm): the exchange runs inside the call
static bool bwd_tail(const pmbrl_plan* p, const BwdCall& C) { return C.opt && (p->grad_comm || p->grad_p2p); }
static int expect_steps(const pmbrl_plan* p, const pmbrl_adam* opt) {
  return opt ? (opt->expect_steps > 0 ? opt->expect_steps : p->cfg.H) : 0;
}

// every refusal that depends on the plan and the arguments alone (reg_bwd: the register-resident family serves the sweep):
// nothing has been queued when one is returned
static int check_bwd(const pmbrl_plan* p, const BwdCall& C, bool reg_bwd) {
  if (bwd_tail(p, C) && p->span && p->cfg.mm_span_ranks > 1)
    return fail(-3, "pmbrl_rollout_bwd_adam with a gradient transport: moment-matching groups spread over ranks are not offered");
  if (p->reg && p->old_pack_stale && !reg_bwd && (!C.in->pol_params_d || !C.in->dyn_params_d)) return fail(-1, "null parameter pointer");
  if (int rc = check_collective(p)) return rc;
  const SweepForm form = sweep_form(p);
  if (C.grad_states && (form == SweepForm::Barrier || form == SweepForm::StepInSweep))
    return fail(-3, "grad_states with moment-matching groups spanning workgroups: not offered");
  if (C.grad_states && form == SweepForm::StepExternal) return fail(-3, "grad_states with external moment matching: not offered");
  return 0;
}

// the sweep arguments of this call
static int bwd_args(const pmbrl_plan* p, const BwdCall& C, RolloutArgs& A) {
  if (int rc = fill_args(p, C.workspace, C.in, A)) return rc;
  A.states = const_cast<float*>(C.states);
  A.actions = const_cast<float*>(C.actions);
  A.rewards = const_cast<float*>(C.rewards);
  A.grad_rewards = C.grad_rewards;
  A.grad_states = C.grad_states;
  A.grad_actions = C.grad_actions;
  A.grad_x0 = C.grad_x0;
  A.agn = C.action_grad_norms;
  A.prof = p->prof_bwd;
  // status[0]: valid steps of the forward sweep (the adjoint covers only those); status[1]: set by
  // the sweep if its device-wide barrier timed out
  // (cleared by the FORWARD call's reward launch -- pm_reward_all_kernel -- since round 5: as a memset of its own here it
  //  was a 5 us fill kernel in every iteration, 1 % of the cart-pole shape's)
  A.nvalid = C.status;
  A.status = C.status ? C.status + 1 : nullptr;
  if (!p->fast) A.ext_reward = 1;
  return 0;
}

// stage 1 (sharded tail): the ranks agree on the horizon first -- the sweep, the dW GEMM and the loss read the agreed status[0]
static int bwd_agree_horizon(pmbrl_plan* p, const BwdCall& C) {
  hipStream_t s = C.stream;
  float* hvec = p->tail_buf_d + ((size_t)p->pol.n_params + 2 + 3) / 4 * 4;
  pm_tail_hvec_launch(s, hvec, p->tail_world, p->tail_rank, C.status, p->cfg.H);
  if (int rc = tail_allreduce(p, s, hvec, p->tail_world)) return rc;
  pm_tail_hmin_launch(s, hvec, p->tail_world, C.status, p->cfg.H);
  return 0;
}

// stage 2: this call goes to the latency-optimised family after a forward call that served the register-resident one -- pack
// the other family's weights now (same parameters: the caller hands the same inputs to both calls) and unpack the activity
// bits from that family's form.  (Neither note is cleared here: a recorded adjoint call -- pmbrl_plan_set_replay -- must
// contain both conversions whenever the forward call before it was of that kind.)
static void bwd_convert_family(pmbrl_plan* p, const BwdCall& C) {
  char* ws = static_cast<char*>(C.workspace);
  if (p->old_pack_stale) launch_pack_all(p, ws, C.in, C.stream, nullptr);
  if (p->abits_packed) pm_reg_unpack_abits(p, ws, C.stream);
}

// stage 3: adjoint of the reward moment matching for all (t, group) up front; the sweep then reads dL/dr~ from the workspace
static int bwd_reward_adjoint(pmbrl_plan* p, const BwdCall& C, RolloutArgs& A, float* grt) {
  if (p->cfg.flags & PMBRL_FLAG_MM_REWARDS) {
    if (p->span) {
      if (int rc = mmx_bwd(p, static_cast<char*>(C.workspace), A, true, 0, grt, C.stream)) return rc;
    } else {
      hipLaunchKernelGGL(pm_mm_rewards_bwd_kernel, dim3(p->cfg.H * p->G), dim3(64), pm_mmr_lds_bytes(p->M, 3), C.stream, A, grt);
    }
    A.grad_rewards = grt;
  }
  if (!p->fast) A.flags &= ~PMBRL_FLAG_MM_REWARDS;   // (general sweeps: the reward side is done, see ext_reward)
  return 0;
}

// stage 4, the groups spanning workgroups (mm_mode 3): dL/dx travels between the steps through two carry buffers.
// SweepForm::Barrier: one launch, the workgroups meet at a device-wide barrier per step
static int bwd_sweep_barrier(pmbrl_plan* p, const BwdCall& C, RolloutArgs A) {
  hipStream_t s = C.stream;
  HIPCHK(hipMemsetAsync(A.gx_carry, 0, (size_t)p->cfg.B * p->cfg.D * sizeof(float), s));
  A.gx_from_carry = 1;
  A.gsync += 1024;
  HIPCHK(hipMemsetAsync(A.gsync, 0, 1024 * sizeof(unsigned), s));
  A.gx_carry_out = reinterpret_cast<float*>(static_cast<char*>(C.workspace) + p->off_gxc2);
  A.t0 = 0; A.t1 = p->cfg.H;
  launch_bwd_rt(p, A, s);
  return 0;
}
// SweepForm::StepInSweep: one launch per step
static int bwd_sweep_steps(pmbrl_plan* p, const BwdCall& C, RolloutArgs A) {
  hipStream_t s = C.stream;
  float* cbuf[2] = {A.gx_carry, reinterpret_cast<float*>(static_cast<char*>(C.workspace) + p->off_gxc2)};
  HIPCHK(hipMemsetAsync(cbuf[0], 0, (size_t)p->cfg.B * p->cfg.D * sizeof(float), s));
  A.gx_from_carry = 1;
  for (int t = p->cfg.H - 1, k = 0; t >= 0; --t, k ^= 1) {
    A.gx_carry = cbuf[k];           // dL/dx_{t+1}, all rows (read by every workgroup of the group)
    A.gx_carry_out = cbuf[k ^ 1];   // dL/dx_t of this workgroup's rows
    A.t0 = t; A.t1 = t + 1;
    launch_bwd_rt(p, A, s);
  }
  return 0;
}
// SweepForm::Whole as K launches over the descending step ranges [lo[k], lo[k-1]) (lo[-1] = H; one range: [0, H)).  More
// than one (the plan's pipe_lo): the dW GEMM of range k goes out on the second stream behind the sweep of that range, next
// to the sweep of range k+1; the last range's GEMM is bwd_dw's
// (W.st_on, the streamed form -- one range: the sweep publishes the policy head's gradient and the layer's consumers go
//  out on the second stream next to it, behind everything the call's stream held in front of the sweep; bwd_dw joins them)
static int bwd_sweep_whole(pmbrl_plan* p, const BwdCall& C, RolloutArgs A, const DwArgs& W, bool reg_bwd, int K, const int* lo) {
  hipStream_t s = C.stream;
  char* ws = static_cast<char*>(C.workspace);
  if (W.st_on) {
    // the granules' tags: zeroed once per workspace; a RECORDED launch carries the fill -- its replays repeat its generation
    // and would meet their own tags of the replay before
    const bool rec = pm_stream_recording(s);
    if (p->dw.pub_ws != C.workspace || rec) {
      HIPCHK(hipMemsetAsync(ws + p->dw.off_pub, 0, p->dw.pub_bytes, s));
      p->dw.pub_ws = rec ? nullptr : C.workspace;
    }
    HIPCHK(hipEventRecord(p->dw.pipe_ev[0], s));
  }
  if (p->mm_parts > 1) {
    // groups split over workgroups: their own flags, and two buffers for the rows of dL/dx they exchange
    A.gsync += 1024;
    A.gx_carry_out = reinterpret_cast<float*>(ws + p->off_gxc2);
    if (int rc = xch_prepare(p, A, reg_bwd, s)) return rc;
  }
  for (int k = 0; k < K; ++k) {
    A.t0 = lo[k];
    A.t1 = k ? lo[k - 1] : p->cfg.H;
    A.gx_from_carry = k > 0;
    if (reg_bwd) pm_reg_launch(p, ws, A, C.in->pol_params_d, C.in->dyn_params_d, s, false, W.st_on ? (unsigned)p->dw.off_pub : 0u, W.st_tag);
    else launch_bwd_rt(p, A, s);
    if (W.st_on) {
      HIPCHK(hipStreamWaitEvent(p->dw.pipe_stream, p->dw.pipe_ev[0], 0));
      pm_dw_stream_launch(p, W, p->dw.pipe_stream);
      HIPCHK(hipEventRecord(p->dw.pipe_ev[1], p->dw.pipe_stream));
    }
    if (k + 1 < K) {
      HIPCHK(hipEventRecord(p->dw.pipe_ev[k], s));
      HIPCHK(hipStreamWaitEvent(p->dw.pipe_stream, p->dw.pipe_ev[k], 0));
      pm_dw_launch_range(p, W, k, p->dw.pipe_stream);
    }
  }
  return 0;
}
// SweepForm::StepExternal: one launch per step behind the adjoint of that step's moment matching
static int bwd_sweep_external(pmbrl_plan* p, const BwdCall& C, RolloutArgs A, float* grt) {
  hipStream_t s = C.stream;
  char* ws = static_cast<char*>(C.workspace);
  const size_t smem = pm_mm_kernel_doubles(p->cfg.D) * sizeof(double);
  HIPCHK(hipMemsetAsync(A.gx_carry, 0, (size_t)p->cfg.B * p->cfg.D * sizeof(float), s));
  RolloutArgs Am = A;
  Am.flags &= ~PMBRL_FLAG_MM_REWARDS;   // rewards already handled (bwd_reward_adjoint)
  A.gx_from_carry = 1;
  for (int t = p->cfg.H - 1; t >= 0; --t) {
    if (p->mm_wide) {
      hipLaunchKernelGGL(pm_mmw_bwd_kernel, dim3(p->G), dim3(PM_MMW_NT), pm_mmw_lds_bytes(p->M, p->cfg.D, true), s, Am, t,
                         reinterpret_cast<const double*>(ws + p->off_mmfac));
    } else if (!p->span) {
      hipLaunchKernelGGL(pm_mm_bwd_kernel, dim3(p->G), dim3(PM_MM_NW * 64), smem, s, Am, t, grt);
    } else if (p->cfg.flags & PMBRL_FLAG_MM_STATES) {
      if (int rc = mmx_bwd(p, ws, Am, false, t, nullptr, s)) return rc;
    }
    A.t0 = t; A.t1 = t + 1;
    launch_bwd_rt(p, A, s);
  }
  return 0;
}

// stage 5: the dW GEMM over the stashes (piped: what is left of it, the last range)
static int bwd_dw(pmbrl_plan* p, const BwdCall& C, const DwArgs& W, bool piped) {
  ScopedTimer tm(p, PMBRL_TIMER_DW, C.stream);
  if (!piped) {
    // (streamed: the layer's kernel takes the steps below the cut and adds to the consumers' rows -- behind them)
    pm_dw_launch(p, W, C.stream, W.st_on ? p->dw.pipe_ev[1] : nullptr);
    return 0;
  }
  // the rows of the last range are added to what the second stream left: join it first
  HIPCHK(hipEventRecord(p->dw.pipe_ev[p->dw.pipe_K - 1], p->dw.pipe_stream));
  HIPCHK(hipStreamWaitEvent(C.stream, p->dw.pipe_ev[p->dw.pipe_K - 1], 0));
  pm_dw_launch_range(p, W, p->dw.pipe_K - 1, C.stream);
  return 0;
}

// does this call's dW GEMM of the second hidden layer run beside its sweep (pm_dw_plan_stream)?  The plan's form, on the family
// that publishes; not with the cycle stamps, nor with the exchange inside (one form of the sharded tail)
static bool bwd_streamed(const pmbrl_plan* p, const BwdCall& C, bool reg_bwd) {
  return p->dw.st_on && reg_bwd && sweep_form(p) == SweepForm::Whole && p->dw.pipe_K <= 1 && !p->prof_bwd && !bwd_tail(p, C);
}
// A0, reg_bwd: the call's sweep arguments (bwd_args) and the family they go to, assembled once by rollout_bwd_replay --
// its replay key holds the family too
static int rollout_bwd(pmbrl_plan* p, const BwdCall& C, const RolloutArgs& A0, bool reg_bwd) {
  hipStream_t s = C.stream;
  RolloutArgs A = A0;
  if (int rc = check_bwd(p, C, reg_bwd)) return rc;
  // the register-resident adjoint (always over its own family's forward stashes: the forward call takes the family
  // whenever the adjoint call can) stashes no delta of the policy's second hidden layer -- every dW launch of THIS call,
  // pipelined ranges and the sharded tail's included, rebuilds it; the other family's adjoint on the same forward
  // (optional outputs, PMBRL_REG_BWD=0) writes gT[1] and keeps the classic kernel: pm_dw_call_args' `rebuilt`
  const pmbrl_adam* opt = C.opt;
  const bool tail = bwd_tail(p, C);
  float* const xb = p->tail_buf_d;
  if (tail)
    if (int rc = bwd_agree_horizon(p, C)) return rc;
  if (p->reg && !reg_bwd) bwd_convert_family(p, C);
  float* grt = reinterpret_cast<float*>(static_cast<char*>(C.workspace) + p->off_grt);
  if (int rc = bwd_reward_adjoint(p, C, A, grt)) return rc;
  const SweepForm form = sweep_form(p);
  const bool piped = form == SweepForm::Whole && p->dw.pipe_K > 1 && !p->prof_bwd;
  const bool streamed = bwd_streamed(p, C, reg_bwd);
  const DwArgs W = pm_dw_call_args(p, C.workspace, C.status, A, reg_bwd, streamed);
  {
    ScopedTimer tm(p, PMBRL_TIMER_BWD, s);
    static const int whole[1] = {0};
    int rc = 0;
    switch (form) {
      case SweepForm::Barrier: rc = bwd_sweep_barrier(p, C, A); break;
      case SweepForm::StepInSweep: rc = bwd_sweep_steps(p, C, A); break;
      case SweepForm::Whole: rc = bwd_sweep_whole(p, C, A, W, reg_bwd, piped ? p->dw.pipe_K : 1, piped ? p->dw.pipe_lo : whole); break;
      case SweepForm::StepExternal: rc = bwd_sweep_external(p, C, A, grt); break;
    }
    if (rc) return rc;
  }
  if (int rc = bwd_dw(p, C, W, piped)) return rc;
  const int n = (int)p->pol.n_params;
  const int expect = expect_steps(p, opt);
  // the fused iteration (one process, optimiser attached): the reduction forms the gradient norm's partial sums and the
  // go / no-go decision on the way -- pm_gradnorm_kernel's launch is not needed.  (Rows sharded over ranks: the norm is
  // that of the SUMMED gradient -- pm_tail_finish_kernel, behind the exchange.)
  const bool part_ok = opt && !piped && (n + 255) / 256 <= PM_NORM_MAXB;
  const bool norm_fused = part_ok && !tail;
  // ... and, asked for (pmbrl_adam::loss_out_d), the loss' partial sums: the optimiser launch adds them -- no loss launch
  // behind the forward call (PMBRL_FUSE_LOSS=0: pm_weighted_sum_kernel, here)
  const bool loss_fused = part_ok && opt->loss_out_d && p->sw.fuse_loss;
  const int n_loss_part = loss_fused ? (n + 255) / 256 : 0;
  float* const red_out = tail ? xb : C.grad_pol_flat;
  {
    ScopedTimer tm(p, PMBRL_TIMER_DW_REDUCE, s);
    if (piped)   // every partial row was written (pm_dw_range)
      pm_dw_reduce_launch(s, W.part, p->dw.pipe_rows, n, W.part_stride, red_out, (const int*)nullptr, 0, 1);
    else
      pm_dw_reduce_launch(s, W.part, p->dw.args.nsplit, n, W.part_stride, red_out, (const int*)C.status, W.chunks_per_step,
                          W.chunks_per_split, norm_fused ? 1 : 0, (const int*)C.status, expect,
                          opt ? reinterpret_cast<long long*>(opt->step_d) : (long long*)nullptr,
                          loss_fused ? C.rewards : (const float*)nullptr, C.grad_rewards, (long long)p->cfg.H * p->cfg.B,
                          (long long)p->cfg.B, W.own_lo, W.own_hi, W.st_wgs);
  }
  // the loss asked for with the optimiser step, where the reduction does not form it on the way: a launch of its own
  if (opt && opt->loss_out_d && !loss_fused)
    launch_weighted_sum(s, C.rewards, C.grad_rewards, (long long)p->cfg.H * p->cfg.B, tail ? xb + n : opt->loss_out_d, C.status,
                        p->cfg.B);
  HIPCHK(hipGetLastError());
  if (!opt) return 0;
  if (tail) {
    // [gradient | loss partial | failure flag] summed over the ranks in place, then the summed gradient's norm and the
    // decision every rank takes alike; the optimiser launch is the one-process one
    pm_tail_pack_launch(s, xb, n, n_loss_part, opt->loss_out_d && !loss_fused ? 1 : 0, C.status, p->tail_err_d);
    if (int rc = tail_allreduce(p, s, xb, (int64_t)n + 2)) return rc;
    pm_tail_finish_launch(s, xb, C.grad_pol_flat, n, C.status, expect, reinterpret_cast<long long*>(opt->step_d), p->tail_err_d);
    HIPCHK(hipGetLastError());
  }
  // the optimiser step behind it, decided on the device (a form with the reduction, the norm and the update in ONE launch
  // around a device-wide barrier was measured at the C2 shape: 25.6 us against 13.7 + 4.7 + 7.1 us for the three launches
  // -- the barrier's L2 round trips cost what two launches do; not kept).  Behind the exchange the norm is done and the
  // loss is one summed partial; otherwise both are as the reduction left them
  // (a rule attached to the plan -- pmbrl_plan_set_optimizer: its instance of the launch, the hyper-parameters from the rule)
  AdamStep S;
  S.params = opt->params_d; S.grads = C.grad_pol_flat; S.exp_avg = opt->exp_avg_d; S.exp_avg_sq = opt->exp_avg_sq_d; S.n = n;
  S.step_d = opt->step_d; S.status = C.status; S.expect = expect;
  S.max_norm = opt->max_norm; S.norm_out = opt->norm_out_d;
  S.norm_done = tail || norm_fused;
  S.loss_out = tail || loss_fused ? opt->loss_out_d : nullptr;
  S.n_loss_part = tail ? (opt->loss_out_d ? 1 : 0) : n_loss_part;
  S.lr = opt->lr; S.beta1 = opt->beta1; S.beta2 = opt->beta2; S.eps = opt->eps;
  S.rule = p->has_opt_rule ? &p->opt_rule : nullptr;   // (checked for this vector when it was attached)
  return pm_adam_launch(s, S);
}

// what makes two adjoint calls "the same" (pmbrl_plan_set_replay)
static ReplayKey bwd_key(const pmbrl_plan* p, const BwdCall& C, bool reg_bwd) {
  const pmbrl_adam* opt = C.opt;
  ReplayKey K;
  K.val(C.stream); K.val(C.workspace); K.add(C.in, sizeof(*C.in));
  K.val(C.states); K.val(C.actions); K.val(C.rewards); K.val(C.grad_rewards); K.val(C.grad_states); K.val(C.grad_actions);
  K.val(C.grad_pol_flat); K.val(C.grad_x0); K.val(C.action_grad_norms); K.val(C.status);
  const int has_opt = opt ? 1 : 0;
  K.val(has_opt);
  if (opt) {      // field by field: the struct's padding bytes are not arguments (a caller's stack copy need not repeat them)
    K.val(opt->params_d); K.val(opt->exp_avg_d); K.val(opt->exp_avg_sq_d); K.val(opt->step_d);
    K.val(opt->lr); K.val(opt->beta1); K.val(opt->beta2); K.val(opt->eps); K.val(opt->max_norm);
    K.val(opt->norm_out_d); K.val(opt->expect_steps);
    // the attached rule, field by field like the struct above: a recording must never replay a stale learning rate
    K.val(p->has_opt_rule);
    if (p->has_opt_rule) {
      const pmbrl_opt_rule& R = p->opt_rule;
      K.val(R.n_groups); K.val(R.n_segments); K.val(R.max_exp_avg_sq_d);
      for (int g = 0; g < R.n_groups; ++g) {
        const pmbrl_opt_group& G = R.group[g];
        K.val(G.lr); K.val(G.beta1); K.val(G.beta2); K.val(G.eps); K.val(G.weight_decay); K.val(G.flags);
      }
      for (int q = 0; q < R.n_segments; ++q) { K.val(R.seg_end[q]); K.val(R.seg_group[q]); }
    }
  }
  if (bwd_tail(p, C)) {     // the transport, its buffer and the loss output: every pointer of a call with the exchange inside
    K.val(p->grad_comm); K.val(p->tail_buf_d); K.val(opt->loss_out_d);
  }
  // what the forward call left behind decides which conversions the adjoint call queues (weights repacked for the other
  // family, activity words unpacked): a recording is only good for the state it was recorded in
  K.val(p->old_pack_stale); K.val(p->abits_packed);
  // ... and the family this call's sweep takes decides which form of the layer's dW kernel follows it (pm_dw_call_args' `rebuilt`)
  const int g1_rebuilt = reg_bwd ? 1 : 0;
  K.val(g1_rebuilt);
  // ... and whether the layer's GEMM runs beside the sweep (bwd_streamed)
  const int streamed = bwd_streamed(p, C, reg_bwd) ? 1 : 0;
  K.val(streamed);
  const int head = streamed && p->dw.st_head ? 1 : 0;      // ... with the policy head's dW in the consumers (pm_dw_plan_head)
  K.val(head);
  return K;
}

static int rollout_bwd_replay(pmbrl_plan* p, const BwdCall& C) {
  if (!p || !C.workspace || !C.in || !C.states || !C.actions || !C.rewards || !C.grad_rewards || !C.grad_pol_flat)
    return fail(-1, "null argument");
  // a reward evaluated by the caller: the sweeps read its Jacobians from the workspace, where only a pmbrl_rollout_rewards
  // call that was given them, behind the latest forward call, has left them
  if (p->ext && p->ext_state == 2)
    return fail(-3, "external reward: the latest pmbrl_rollout_rewards call was given no Jacobians (a forward-only rollout); "
                    "the adjoint needs a rewards call with jx_d and ja_d behind the forward call");
  if (p->ext && p->ext_state != 3)
    return fail(-3, "external reward: no pmbrl_rollout_rewards call since the latest pmbrl_rollout_fwd on this plan");
  HIPCHK(hipSetDevice(p->device));
  RolloutArgs A;      // (no stream in it: the same for the eager call, the recording and the key)
  if (int rc = bwd_args(p, C, A)) return rc;
  const bool reg_bwd = pm_reg_can_run(p, A, false);
  const bool tail = bwd_tail(p, C);
  if (tail) ++p->tail_calls;
  if (tail && p->grad_p2p) {
    // the peer-to-peer exchange cannot be recorded (its generation is a kernel argument): eagerly, whatever
    // pmbrl_plan_set_replay says
    if (p->rp[1].exec || p->rp[1].seen) replay_drop(p, 1);
    return rollout_bwd(p, C, A, reg_bwd);
  }
  return replay_call(p, 1, bwd_key(p, C, reg_bwd), C.stream, [&](hipStream_t on) {
    BwdCall Con = C;
    Con.stream = on;
    return rollout_bwd(p, Con, A, reg_bwd);
  });
}

extern "C" int pmbrl_rollout_bwd(pmbrl_plan* p, void* stream, void* workspace, const pmbrl_inputs* in,
                                 const float* states_d, const float* actions_d,
                                 const float* rewards_d, const float* grad_rewards_d,
                                 const float* grad_states_d, const float* grad_actions_d,
                                 float* grad_pol_flat_d, float* grad_x0_d,
                                 float* action_grad_norms_d, int32_t* status_d) {
  return rollout_bwd_replay(p, BwdCall{(hipStream_t)stream, workspace, in, states_d, actions_d, rewards_d, grad_rewards_d,
                                       grad_states_d, grad_actions_d, grad_pol_flat_d, grad_x0_d, action_grad_norms_d,
                                       status_d, nullptr});
}

extern "C" int pmbrl_rollout_bwd_adam(pmbrl_plan* p, void* stream, void* workspace, const pmbrl_inputs* in,
                                      const float* states_d, const float* actions_d,
                                      const float* rewards_d, const float* grad_rewards_d,
                                      const float* grad_states_d, const float* grad_actions_d,
                                      float* grad_pol_flat_d, float* grad_x0_d,
                                      float* action_grad_norms_d, int32_t* status_d, const pmbrl_adam* opt) {
  if (!opt || !status_d || !opt->params_d || !opt->exp_avg_d || !opt->exp_avg_sq_d || !opt->step_d)
    return fail(-1, "null argument");
  return rollout_bwd_replay(p, BwdCall{(hipStream_t)stream, workspace, in, states_d, actions_d, rewards_d, grad_rewards_d,
                                       grad_states_d, grad_actions_d, grad_pol_flat_d, grad_x0_d, action_grad_norms_d,
                                       status_d, opt});
}

// ---------------------------------------------------------------------------
// test hook: y = x W^T + b through gemm_tiles / gemm_narrow, with the fragment packers only it launches.  gemm_tiles<RT> and
// gemm_narrow<RT> are not __forceinline__, so how the compiler inlines them depends on their other users in the module:
// the hook is compiled in this object, with the general family's exact-fp32 instances, to keep the code it is there to test.
// ---------------------------------------------------------------------------
template <int RT>
__global__ __launch_bounds__(PM_NT, 1) void pm_debug_linear_kernel(const float* x, const float* wf,
                                                                  const float* bias, int R, int K,
                                                                  int O, int LD, int narrow,
                                                                  float* y) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  constexpr int RR = 16 * RT;
  float* X = smem;
  float* Y = X + RR * LD;
  float* part = pm_part_alias_ok(RR, LD, RT) ? nullptr : Y + RR * LD;   // (same rule as the rollout kernels)
  const int n_kb = (K + 15) / 16, n_ot = (O + 15) / 16;
  for (int i = tid; i < RR * LD; i += PM_NT) {
    const int r = i / LD, k = i - r * LD;
    X[i] = (r < R && k < K) ? x[(size_t)r * K + k] : 0.f;
  }
  __syncthreads();
  if (narrow) {
    gemm_narrow<RT>(wf, n_ot, n_kb, bias, X, Y, LD, part, wid, lane, tid);
  } else {
    EpiPlain e{bias, Y, LD, lane};
    gemm_tiles<RT>(wf, n_ot, n_kb, X, LD, wid, lane, e);
    __syncthreads();
  }
  for (int i = tid; i < R * O; i += PM_NT) {
    const int r = i / O, o = i - r * O;
    y[i] = Y[r * LD + o];
  }
}

extern "C" int pmbrl_debug_linear(void* stream, const float* x_d, const float* W_d, const float* b_d,
                                  int32_t R, int32_t K, int32_t O, int32_t transpose_w, float* y_d,
                                  float* scratch_d) {
  // transpose_w: treat W as [K_out... ] i.e. compute y = x W (W is [K][O] row-major = stored [in][out])
  if (R < 1 || R > 64 || K < 1 || O < 1) return fail(-1, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int n_kb = (K + 15) / 16, n_ot = (O + 15) / 16;
  const int LD = std::max(n_kb, n_ot) * 16 + 8;
  float* wf = scratch_d;
  float* bias = scratch_d + (size_t)n_ot * n_kb * 256;
  const size_t tot = (size_t)n_ot * n_kb * 256;
  const int grid = (int)std::min<size_t>((tot + 255) / 256, 1024);
  if (!transpose_w)
    hipLaunchKernelGGL(pm_pack_frag, dim3(grid), dim3(256), 0, s, W_d, O, K, 0, 1, wf);
  else  // W_d is [K][O]: out feature index is the second one
    hipLaunchKernelGGL(pm_pack_frag, dim3(grid), dim3(256), 0, s, W_d, K, O, 1, 1, wf);
  hipLaunchKernelGGL(pm_pack_bias, dim3((n_ot * 16 + 255) / 256), dim3(256), 0, s, b_d, O, n_ot * 16,
                     bias);
  auto lds_for = [&](int RT) {
    return ((size_t)2 * 16 * RT * LD +
            (pm_part_alias_ok(16 * RT, LD, RT) ? 0 : (size_t)PM_NW * PM_KS_NT * RT * 256)) * sizeof(float);
  };
  const int narrow = n_ot <= PM_KS_NT ? 1 : 0;
  // rows in slabs of the largest tile height whose LDS fits
  int RT = R <= 16 ? 1 : (R <= 32 ? 2 : 4);
  while (RT > 1 && lds_for(RT) > (size_t)160 * 1024) RT /= 2;
  const size_t lds = lds_for(RT);
#define DBG_LAUNCH(RTV, X0, Y0, RR)                                                             \
  do {                                                                                          \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_debug_linear_kernel<RTV>),     \
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));          \
    hipLaunchKernelGGL(pm_debug_linear_kernel<RTV>, dim3(1), dim3(PM_NT), lds, s, X0, wf, bias, RR, \
                       K, O, LD, narrow, Y0);                                                   \
  } while (0)
  for (int r0 = 0; r0 < R; r0 += 16 * RT) {
    const int rr = std::min(R - r0, 16 * RT);
    const float* x0 = x_d + (size_t)r0 * K;
    float* y0 = y_d + (size_t)r0 * O;
    if (RT == 1) DBG_LAUNCH(1, x0, y0, rr);
    else if (RT == 2) DBG_LAUNCH(2, x0, y0, rr);
    else DBG_LAUNCH(4, x0, y0, rr);
  }
#undef DBG_LAUNCH
  HIPCHK(hipGetLastError());
  return 0;
}
