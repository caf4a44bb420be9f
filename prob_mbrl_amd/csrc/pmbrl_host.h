// Host-side declarations shared by the translation units of libpmbrl_hip.so: the plan, the records the launchers take
// and the launchers themselves.  A kernel is compiled in exactly one object; another object that needs it calls the
// launcher declared here, or, for the sweep kernels, takes it from the instance table that object exports
// (pmbrl_instances.h).  The objects:
//   pmbrl.hip                error string, version, build id, graph capture, the rollout plan, argument assembly and the two
//                            rollout calls, with the kernels only they launch (the general family in exact fp32, external
//                            moment matching, the reward kernels, pm_pack_all), the host side of pmbrl_rollout_rewards,
//                            and the GEMM test hook
//                            (it also resolves a plan's sweep kernels from the tables and launches them)
//   pmbrl_general_split.hip  the general family on split operands: instances and table, nothing else
//   pmbrl_general_act.hip    the general family for networks that are not ReLU: the same
//   pmbrl_general_gmmr.hip   the general family's sweeps for a learned reward head on the mixture head: the same; compiled
//                            once for ReLU networks and once for the others (two objects)
//   pmbrl_fast_f32.hip       latency-optimised sweeps, exact fp32 MFMA: the same
//   pmbrl_fast_split.hip     the same on split bf16 / fp16 operands; compiled once per precision (two objects)
//   pmbrl_reg.hip            register-resident family: instances, resolution, packer and launch
//   pmbrl_dw.hip             the policy-gradient dW GEMMs: kernels, the plan's dW record made and released
//                            (pmbrl_dw_plan.h: the host-only planner), a call's argument record, the launches
//   pmbrl_reward_ext.hip     the ingest launch of a reward evaluated by the caller (pmbrl_rollout_rewards)
//   pmbrl_tail.hip           mask packing / drawing, weighted sum, dW reduction, gradient norm, clip + Adam, sharded tail
//   pmbrl_bnn.hip            BNN training step
//   pmbrl_bnn_spill.hip      its spill form (networks wider than the LDS-resident kernel takes): instances and launcher
//   pmbrl_mlp.hip            stand-alone network evaluation
//   pmbrl_comm.hip           RCCL through dlopen, the plan's transports (host code only)
//   pmbrl_p2p.hip            peer-to-peer transport
// Host-only headers, each checked by a program of the host compiler alone: pmbrl_dw_plan.h (the dW GEMM's planner) and
// pmbrl_lds_map.h (the LDS maps of the general and the latency-optimised sweeps: one walk per family gives the launch's
// size, the kernels' pointers and the per-layer offsets in their arguments)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "pmbrl.h"
#include "pmbrl_dev.h"
#include "pmbrl_dw.h"
#include "pmbrl_dw_plan.h"
#include "pmbrl_instances.h"

int pm_fail(int code, const std::string& msg);
static inline int fail(int code, const std::string& msg) { return pm_fail(code, msg); }
#define HIPCHK(expr)                                                               \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess)                                                          \
      return pm_fail(-100 - (int)_e, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

struct NetPlan {
  int nl;
  int dim[PM_MAXL + 1], nt[PM_MAXL + 1];
  float keep[PM_MAXL];
  int act;                                 // PMBRL_ACT_* per hidden layer (pm_act_layers); 0: every layer is ReLU
  size_t w_off[PM_MAXL], b_off[PM_MAXL];   // offsets (floats) in the flat parameter vector
  size_t n_params;
  // workspace offsets (bytes)
  size_t wf[PM_MAXL], wb[PM_MAXL], bias[PM_MAXL], abits[PM_MAXL];
};

// The environment switches of a rollout plan (include/pmbrl.h lists them), read once when it is created
// (the dW GEMM's: DwSwitches, pmbrl_dw_plan.h)
struct PlanSwitches : DwSwitches {
  bool mm_perstep, mm_mode2, mm_no_batch, reg_debug;   // set at all: on
  bool lds_tiles, mm_xch, mm_tree, reg, reg_mm, reg_tree, reg_bwd, fuse_loss, ztab_merge, wide;   // =0: off
  bool mm_parts_set;    // PMBRL_MM_PARTS=mm_parts
  int mm_parts;
  int replay;           // PMBRL_REPLAY (default 1)
};

struct pmbrl_plan {
  pmbrl_config cfg;
  PlanSwitches sw;
  int device;
  int RT, rows_per_wg, nwg, LD, mm_mode, G, M, fast, CA, CB;   // CA/CB: k-blocks per weight-stream stage
  int prec, LDB;   // PMBRL_PREC_* in use; split precision: leading dimension of the bf16 piece planes
  size_t lds_bytes;
  NetPlan pol, dyn;
  RewardDev* rew_d;
  int act;             // some hidden layer of some network is not ReLU: the general family's ACT instances, per-unit act' stashes in place of the activity bits
  int learned;         // PMBRL_REWARD_LEARNED: the dynamics head predicts the reward (general family only)
  int rew_k = PMBRL_MAX_TIP;   // tip residuals of the reward (which instance of the reward launch: pm_reward_kernel_for)
  // PMBRL_REWARD_EXTERNAL: the caller evaluates the reward between pmbrl_rollout_fwd and pmbrl_rollout_rewards (rew_d is
  // then an all-zero record, never read: the sweeps take a null one for a learned head).  ext_state: 0 no forward call yet,
  // 1 a forward call with no rewards call behind it, 2 rewards taken in without Jacobians, 3 with them (what an adjoint
  // call needs); ext_in / ext_states / ext_actions: the latest forward call's arguments, which the rewards call goes on from
  int ext = 0, ext_state = 0;
  pmbrl_inputs ext_in;
  float *ext_states = nullptr, *ext_actions = nullptr;
  int* wflag_d;        // weight-range flag of the fp16 packer (see RolloutArgs::wflag)
  int wgen;            // generation of the last forward call
  AngleDev* ang_d;
  DwPlan dw;           // everything the plan decides about the policy's dW GEMM, and what it owns for it (pmbrl_dw_plan.h)
  // workspace offsets (bytes)
  size_t off_actT[PM_MAXL], off_gT[PM_MAXL], off_Tp, off_Td, off_xt, off_rt, off_mmfac,
      off_gxc, off_gxc2, off_gsync, off_xch, xch_bytes, off_grt, off_Jx, off_Ja, off_gmm_c, off_gmm_k, ws_bytes;
  int wlds_off, lds_last_lanes;   // LDS-resident tiles (lds_tile_s): where they go (floats), lanes stored of the last K32 block
  const float* loss_w;   // pmbrl_plan_set_loss: dL/dr [H][B]; the forward call also leaves the loss in *loss_out
  float* loss_out;

  int mm_grid;   // mm_mode 3 as one launch per sweep with a device-wide barrier per step
  // moment-matching groups spread over ranks (pmbrl_config.mm_span_rows; mm_mode 2 with the statistics exchanged
  // through `coll` between the two halves of the external moment matching, pmbrl_mmx.h)
  int span;
  size_t off_mmx_buf, off_mmx_fac, off_mmx_rfac;
  int (*coll)(void* ctx, void* stream, double* buf_d, int64_t n);
  void* coll_ctx;
  int inplace;   // general family on split operands: 64-row workgroups with in-place layers (pm_rollout_fwd<4, 2, true>)
  int mm_wide;   // mm_mode 2 through the LDS-staged kernels for 6 < D <= 32 (pmbrl_mm_wide.h)
  int mm_parts;  // mm_mode 1 with every group split over this many workgroups (RolloutArgs::mm_parts); 1: whole groups
  int xch_zeroed;          // the exchange's granules hold no tag a launch of the register-resident family could mistake for its own
  mutable unsigned xch_gen;   // ... whose tags carry this launch generation (pmbrl_reg_mm.h)
  int mm_gpb;    // ... launched in batches of this many groups (0: all at once) -- more workgroups than CUs, and the
                 // statistics exchange needs a group's workgroups resident together
  int mm_fan;    // ... more than 8: parts per collector of the two-level sum exchange (0: one level)
  size_t off_ztab;   // ... and the noise standardisation of the whole group per step (pm_mm_ztable_kernel)
  // the sweep kernels, resolved from the instance tables when the plan is created (plan_attrs): one pair per PF_VAR_* for
  // the latency-optimised family ({nullptr, nullptr}: this plan has none for that variant), sweep[0] for the general one;
  // sweep_key: the table rows they came from
  PmInst sweep[PF_VAR_COUNT];
  PmInstKey sweep_key[PF_VAR_COUNT];
  PmInst reg_k[2];   // ... and the register-resident family's: [0] plain, [1] with cycle stamps (pm_reg_resolve)
  int reg;       // the register-resident family (pmbrl_reg.h) serves this plan's plain whole-horizon launches
  mutable int reg_calls[2];   // sweeps it has served: [0] forward, [1] adjoint (pmbrl_plan_info)
  int reg_mm;    // ... including the sweeps that moment-match the states of split groups (pmbrl_reg_mm.h): state width, 0 = no
  size_t off_reg_linv;   // [H][groups][D D] doubles: L^-1, forward sweep -> adjoint sweep
  size_t off_reg_pack;   // its packed weights in the workspace
  size_t off_reg_ab[2][2];   // its activity words [net][hidden layer]: [step][workgroup][wave][lane] x 32 bits (pmbrl_reg.h)
  int abits_packed;      // the last forward call left the activity bits in that form only (pm_reg_unpack_abits: -> NetPlan::abits)
  int old_pack_stale;    // the last forward call packed the register-resident family's weights only
  // Replay (pmbrl_plan_set_replay): a call whose arguments equal the previous call's is recorded as a hipGraph the second
  // time it is seen and launched as one graph from then on.  Slot 0: pmbrl_rollout_fwd, slot 1: pmbrl_rollout_bwd(_adam).
  int replay;            // 0 off, 1 the one-launch-per-step forms, 2 every form
  hipStream_t cap_stream;   // what the calls are recorded on
  struct ReplaySlot { unsigned long long key; std::vector<unsigned char> bytes; int seen, dead, aux; hipGraphExec_t exec; long long launches; } rp[2];
  // gradient transport of the fused iteration tail on a sharded run (pmbrl_plan_set_grad_comm): at most one of the two
  pmbrl_comm* grad_comm;
  pmbrl_p2p* grad_p2p;
  int tail_rank, tail_world;
  float* tail_buf_d;       // [n + 2 rounded up to 4 | tail_world]: gradient, loss partial, failure flag | horizon vector
  int* tail_err_d;         // the peer-to-peer object's error word (nullptr: RCCL)
  mutable int tail_calls;  // pmbrl_rollout_bwd_adam calls that ran with the exchange inside (pmbrl_plan_info)
  // optimiser rule (pmbrl_plan_set_optimizer): while attached, the optimiser launch of pmbrl_rollout_bwd_adam is the rule's
  int has_opt_rule;
  pmbrl_opt_rule opt_rule;
  // optional per-kernel timing (hipEvents on the caller's stream)
  long long* prof_fwd;
  long long* prof_bwd;
  int timing;
  hipEvent_t ev[PMBRL_TIMER_COUNT][2];
  bool ev_set[PMBRL_TIMER_COUNT];
};

// How a plan's sweeps go out: what the two rollout calls, the replay default and the dW pipeline branch on
enum class SweepForm {
  Barrier,        // one launch; groups spanning workgroups meet at a device-wide barrier per step (mm_mode 3, mm_grid)
  StepInSweep,    // one launch per step, each moment-matching the states of the step before in its prologue (mm_mode 3)
  Whole,          // the whole horizon in one launch, moment matching (if any) inside it (mm_mode 0 / 1)
  StepExternal    // one launch per step with the moment-matching kernels between them (mm_mode 2)
};
static inline SweepForm sweep_form(const pmbrl_plan* p) {
  if (p->mm_mode == 3) return p->mm_grid ? SweepForm::Barrier : SweepForm::StepInSweep;
  return p->mm_mode == 2 ? SweepForm::StepExternal : SweepForm::Whole;
}

// forget what a replay slot has recorded (pmbrl_plan_set_replay)
static inline void replay_drop(pmbrl_plan* p, int slot) {
  if (p->rp[slot].exec) (void)hipGraphExecDestroy(p->rp[slot].exec);
  p->rp[slot].exec = nullptr;
  p->rp[slot].seen = 0;
}

struct ScopedTimer {
  pmbrl_plan* p; int slot; hipStream_t s;
  ScopedTimer(pmbrl_plan* p_, int slot_, hipStream_t s_) : p(p_), slot(slot_), s(s_) {
    if (p->timing) (void)hipEventRecord(p->ev[slot][0], s);
  }
  ~ScopedTimer() {
    if (p->timing) { (void)hipEventRecord(p->ev[slot][1], s); p->ev_set[slot] = true; }
  }
};

// a key as text, for the message of a plan that asks for an instance no table has
static inline std::string pm_inst_name(const PmInstKey& k) {
  std::string s;
  for (int v : {k.rt, k.ca, k.cb, k.var, k.d, k.u, k.ld, k.nl, k.nt, k.tree}) s += (s.empty() ? "(" : ", ") + std::to_string(v);
  return s + ") [row tiles, stage pair, variant, D, U, LD, layers, hidden tiles, tree]";
}

// 16-wide tiles of the hidden layers of the shape-specialised instances' networks (two hidden layers each, all of one
// width); -1 for any other pair of networks
static inline int hidden_tiles_3l(const pmbrl_plan* p) {
  if (p->pol.nl != 3 || p->dyn.nl != 3) return -1;
  const int nt = p->pol.nt[1];
  return p->pol.nt[2] == nt && p->dyn.nt[1] == nt && p->dyn.nt[2] == nt ? nt : -1;
}
static inline int fast_variant(int RT, const RolloutArgs& A) {
  // variant: see pmbrl_fast.h (PF_VAR_*)
  const bool mm = A.mm_mode == 1 || A.mm_mode == 3;   // moment matching inside the sweep launches
  const bool ext = A.prof || A.grad_states || A.grad_actions || A.agn || A.zpol_ss != 0 || A.zdyn_ss != 0 ||
                   (A.flags & PMBRL_FLAG_MM_STATES) || A.t0 != 0 || A.t1 != A.H || A.gx_from_carry;
  const bool mmg = RT == 1 && A.mm_mode == 3 && A.mm_grid;
  return mmg ? PF_VAR_MMG : mm ? PF_VAR_MM : (ext ? PF_VAR_EXT : PF_VAR_LEAN);
}

// all weight / bias repacking of one forward call in ONE launch (blockIdx.y = job)
struct PackJob {
  const float* src;
  float* dst;
  int O, K, transpose, mult, is_bias;
  int planes;   // 0: fp32 fragments of 16-wide k-blocks; 2 / 3: bf16 pieces of K32 blocks (pmbrl_split.h), mult in K32 blocks
  int f16;      // pieces are fp16 instead of bf16
};
struct PackArgs {
  int n;
  int* wflag;       // fp16 pieces: set to `gen` when a weight is beyond +-65504 or not finite (nullptr: no check)
  int gen;
  int* status;      // reset to "no failure" by the same launch (nullptr: leave alone)
  PackJob job[6 * PM_MAXL];
};
void pm_pack_all_launch(const PackArgs& PK, hipStream_t s);   // (pmbrl.hip)

// the dW GEMMs (pmbrl_dw.hip; the planner and build_dw_blocks: pmbrl_dw_plan.h)
int pm_dw_plan_create(pmbrl_plan* p, int cus);   // plans (pm_dw_plan), uploads the tables, creates the second stream and the events
void pm_dw_plan_destroy(pmbrl_plan* p);
// a block table on the device (*out stays nullptr if it cannot be had) and in the argument record; also the BNN step's
hipError_t pm_dw_upload_blocks(const std::vector<DwBlock>& blocks, DwBlock** out);
void pm_dw_bind_blocks(DwArgs& W, const DwBlock* blocks_d, const int* wave_first);
// a call's argument record: the plan's part + its stashes (A.actT / A.gT), partial rows and status word; rebuilt: the
// call's sweep left no delta of the second hidden layer; streamed: the layer's GEMM runs beside the sweep
DwArgs pm_dw_call_args(const pmbrl_plan* p, void* workspace, int32_t* status, const RolloutArgs& A, bool rebuilt, bool streamed);
void pm_dw_launch(const pmbrl_plan* p, const DwArgs& W, hipStream_t s, hipEvent_t after = nullptr);
void pm_dw_stream_launch(const pmbrl_plan* p, const DwArgs& W, hipStream_t s);   // the streamed form's consumers
void pm_dw_launch_range(const pmbrl_plan* p, const DwArgs& W, int k, hipStream_t s);   // launch k of the pipelined form
void pm_dw_blocks_launch(const DwArgs& W, hipStream_t s);
// the kernels around the sweeps (pmbrl_tail.hip); pm_dw_reduce's arguments are the kernel's
#define PM_NORM_MAXB 8192      // blocks of 256 elements: gradients of up to 2 M parameters (beyond: pm_gradnorm_kernel strides)
void pm_dw_reduce_launch(hipStream_t s, const float* part, int nsplit, int n, int stride, float* grad,
                         const int* nvalid = nullptr, int chunks_per_step = 0, int chunks_per_split = 1, int norm_on = 0,
                         const int* status = nullptr, int expect = 0, long long* step = nullptr, const float* loss_r = nullptr,
                         const float* loss_w = nullptr, long long loss_n = 0, long long loss_per_step = 0, int col_lo = 0,
                         int col_hi = 0, int rows_in_range = 0);
void launch_weighted_sum(hipStream_t s, const float* a, const float* w, long long n, float* out, const int* nvalid,
                         long long n_per_step);
// One clip_grad_norm_ + Adam step on flat vectors, as every caller states it (the four pmbrl_clip_adam* entry points, the
// fused iteration of pmbrl_rollout_bwd_adam).  pm_adam_launch decides the launch shapes and whether the norm's launch is
// needed, and queues it and the optimiser launch.
struct AdamStep {
  float *params, *grads, *exp_avg, *exp_avg_sq;
  int64_t n;
  int64_t step = 0;                // the host's step count (>= 1), or
  int64_t* step_d = nullptr;       // the GUARDED form: the device-side counter, advanced if status says `expect` steps completed
  const int32_t* status = nullptr;
  int32_t expect = 0;
  double max_norm = 0.0;           // <= 0: no clipping
  float* norm_out = nullptr;
  float* loss_out = nullptr;       // the fused iteration's loss: the sum of the first n_loss_part entries of g_loss_part
  int n_loss_part = 0;
  // the partial sums of squares and the go / no-go decision are already on the device (the fused iteration's gradient
  // reduction formed them: pm_dw_reduce with norm_on, or pm_tail_finish_kernel behind the exchange)
  bool norm_done = false;
  double lr = 0.0, beta1 = 0.0, beta2 = 0.0, eps = 0.0;   // torch.optim.Adam's, or
  const pmbrl_opt_rule* rule = nullptr;                   // a rule that pmbrl_opt_rule_check passed for n: the hyper-parameters are its
};
int pm_adam_launch(hipStream_t s, const AdamStep& A);
// what the kernels take of a rule's group beside lr, the betas and eps
struct OptGroupConsts {
  float wd;             // L2: g += wd p (0: none, and for a decoupled group)
  float decay;          // decoupled: p *= 1 - lr wd, formed in double, rounded once (1: none)
  float sgn;            // maximize: -1
  int ams;
  double ln_b1, ln_b2;  // for the bias corrections of a device-side step counter
};
inline OptGroupConsts pm_opt_group_consts(const pmbrl_opt_group& G) {
  const bool dec = G.flags & PMBRL_OPT_DECOUPLED;
  return {dec ? 0.f : (float)G.weight_decay, dec ? (float)(1.0 - G.lr * G.weight_decay) : 1.f,
          (G.flags & PMBRL_OPT_MAXIMIZE) ? -1.f : 1.f, (G.flags & PMBRL_OPT_AMSGRAD) ? 1 : 0, log(G.beta1), log(G.beta2)};
}
// what pmbrl_act_check refuses, as text (nullptr: nothing); host code only (pmbrl.hip)
const char* pm_act_refusal(int32_t act, int n_hidden);
// An activation field that passed pmbrl_act_check, in the one form the kernels read (pm_act_code, pmbrl_dev.h): the code
// of hidden layer l in bits 3 l .. 3 l + 2, the plain form (0 .. 2) spread over the n_hidden layers; 0 = every layer is ReLU
inline int pm_act_layers(int32_t act, int n_hidden) {
  if (act & PMBRL_ACT_PER_LAYER) return act & ~PMBRL_ACT_PER_LAYER;
  int v = 0;
  for (int l = 0; l < n_hidden; ++l) v |= PMBRL_ACT_LAYER(act, l);
  return v;
}
// what pmbrl_opt_rule_check refuses, as text (nullptr: nothing); host code only
const char* pm_opt_rule_refusal(const pmbrl_opt_rule* r, int64_t n);
void pm_tail_hvec_launch(hipStream_t s, float* hvec, int world, int rank, const int* status, int H);
void pm_tail_hmin_launch(hipStream_t s, const float* hvec, int world, int* status, int H);
void pm_tail_pack_launch(hipStream_t s, float* xb, int n, int n_loss_part, int loss_here, const int* status, const int* err);
void pm_tail_finish_launch(hipStream_t s, const float* xb, float* g, long long n, int* status, int expect, long long* step,
                           const int* err);
// a reward evaluated by the caller (pmbrl_reward_ext.hip): r -> dst_r, jx -> Jx, ja -> Ja (both or neither), the first
// step with a non-finite entry of x, r, jx or ja -> atomicMin(status[0]), status[1] cleared; one launch
struct RewardExtArgs {
  const float *r, *jx, *ja, *x;     // [H][B], [H][B][D], [H][B][U] (or both nullptr), [H][B][D]
  float *dst_r, *Jx, *Ja;
  int* status;
  int H, B, D, U;
};
void pm_reward_ext_launch(const RewardExtArgs& R, hipStream_t s);
// peer-to-peer transport (pmbrl_p2p.hip): what the fused iteration tail needs to know of one
void pm_p2p_describe(const pmbrl_p2p* p, int* rank, int* nranks, size_t* cap_bytes, int** err_d);
// register-resident family (pmbrl_reg.hip)
bool pm_reg_plan_ok(const pmbrl_plan* p);
bool pm_reg_shape_ok(const pmbrl_plan* p, int prec1);
bool pm_reg_mm_shape_ok(const pmbrl_plan* p, int prec1);
int pm_reg_mm_width(const pmbrl_plan* p);
size_t pm_reg_pack_bytes();
int pm_reg_resolve(pmbrl_plan* p);
bool pm_reg_can_run(const pmbrl_plan* p, const RolloutArgs& A, bool fwd);
struct ZtabArgs;   // (pmbrl_mm.h: the noise table of split moment-matching groups, formed by extra workgroups of the pack launch)
void pm_reg_pack_launch(const pmbrl_plan* p, char* ws, const float* pol_params, const float* dyn_params, int* wflag, int gen,
                        hipStream_t s, int* status_reset, const ZtabArgs* ztab);
void pm_reg_unpack_abits(const pmbrl_plan* p, char* ws, hipStream_t s);
void pm_reg_dw_rebuild_args(const pmbrl_plan* p, char* ws, DwArgs& W);   // what pm_dw_layer_rc_kernel reads of the family's workspace
// (pub / pub_tag: the adjoint sweep publishes the policy head's gradient at this workspace offset -- RegArgs::pub; 0: no)
void pm_reg_launch(const pmbrl_plan* p, char* ws, const RolloutArgs& A, const float* pol_params, const float* dyn_params,
                   hipStream_t s, bool fwd, unsigned pub = 0, unsigned pub_tag = 0);
// the sweep kernels' instance tables, one per object (pmbrl_instances.h; pmbrl.hip holds the general family's in exact fp32)
PmInstTable pm_fast_f32_instances();
PmInstTable pm_fast_split1_instances();     // PMBRL_PREC_SPLIT
PmInstTable pm_fast_split2_instances();     // PMBRL_PREC_SPLIT_F16
PmInstTable pm_general_split_instances();
PmInstTable pm_general_act_instances();
PmInstTable pm_general_gmmr_instances();       // learned reward on the mixture head: ReLU networks ...
PmInstTable pm_general_gmmr_act_instances();   // ... and networks with a hidden layer that is not ReLU
