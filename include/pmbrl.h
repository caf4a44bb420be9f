/*
 * pmbrl.h -- C ABI of libpmbrl_hip.so: the MI355X (gfx950) implementation of the
 * MC-PILCO particle-rollout + back-prop-through-rollout hot path of
 * mcgillmrl/prob_mbrl.
 *
 * The reference has no FFI (it is pure Python on torch); the boundary it offers
 * is the Python call surface.  Each entry point below names the reference
 * function(s) whose arithmetic it replaces (paths relative to the reference
 * repository root).  The Python host layer (prob_mbrl_amd/) keeps the
 * reference's signatures and calls these through ctypes; see INTEGRATION.md.
 *
 * Conventions
 *  - plain C, no exceptions, no Python/torch types; every pointer named *_d is
 *    a DEVICE pointer owned by the caller (a torch tensor's data_ptr()) that
 *    must stay alive until `stream` has drained; all arrays are contiguous,
 *    row-major, fp32 unless stated.
 *  - return value: 0 = ok, < 0 = usage / HIP error (message via
 *    pmbrl_last_error()).  Numerical failures inside a rollout (non-finite
 *    state, non-positive Cholesky pivot) do not fail the call: they are
 *    reported through the int32 `status_d` word (see pmbrl_rollout_fwd), which
 *    the host turns into the RuntimeError the reference's control flow relies
 *    on (utils/rollout.py:154-157, algorithms/mc_pilco.py:122-131).
 *  - calls on one plan are stream-ordered and not thread-safe; different plans
 *    may be used from different host threads.
 */
#ifndef PMBRL_H
#define PMBRL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMBRL_MAX_LAYERS 8  /* Linear layers per network (hidden + output) */
#define PMBRL_MAX_ANGLE 8
#define PMBRL_MAX_TIP 8
#define PMBRL_MAX_DIM 64    /* max state / action / expanded-state width */

#define PMBRL_FLAG_MM_STATES 1   /* utils/rollout.py:121-132 */
#define PMBRL_FLAG_MM_REWARDS 2  /* utils/rollout.py:135-145 */
#define PMBRL_FLAG_INFER_NS 4    /* utils/rollout.py:6-17 (mm_resample_infer_ns_) */
#define PMBRL_FLAG_FORCE_GENERIC 16 /* do not use the latency-optimised kernel variants (tests) */
#define PMBRL_FLAG_NO_SHAPED 32 /* do not use the shape-specialised instantiations (tests) */
#define PMBRL_FLAG_POL_MASKS_PER_STEP 64  /* pol_mask_bits_d[l] is [H, B, ceil(h/16)]: a fresh dropout mask at every
                                            step (utils/rollout.py:95-98 resample_policy=True -> models/modules.py:55-58) */
#define PMBRL_FLAG_DYN_MASKS_PER_STEP 128 /* the same for the dynamics model (resample_model=True, utils/rollout.py:110-115
                                            -> models/modules.py:134-139,155-157).  Either flag selects the general
                                            kernel family (the latency-optimised one keeps the masks in LDS for the launch) */
#define PMBRL_FLAG_GMM_EXACT_NOISE_GRAD 256 /* mixture head: differentiate the noise term with the step's own noise
                                   * (default: with the LAST step's, as the reference's autograd does -- its
                                   * sampler swaps the storage of a saved tensor, models/densities.py:229-231) */
#define PMBRL_MAX_COMP 8          /* mixture components of the dynamics head */
#define PMBRL_FLAG_ZMM_PER_STEP 8 /* z_mm/z_rr are [H, B_global, .] fresh draws per step
                                     (utils/rollout.py:58-59, z=None) instead of the cyclic
                                     PEGASUS buffer of utils/rollout.py:53-57 */

/* Arithmetic of the hidden-width (K >= 32) products of the sweep kernels.  Everything else (first
 * layers, elementwise phases, moment matching, the dW GEMM, the optimiser) is fp32 / fp64 either way.
 *  F32    v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation (1/16 of the bf16 matrix rate)
 *  SPLIT  every fp32 operand as a sum of bf16 pieces on v_mfma_f32_16x16x32_bf16 with fp32
 *         accumulation: three pieces (6 MFMAs per K=32, fp32-equivalent) in the forward sweep, two
 *         (3 MFMAs) in the adjoint sweep -- prob_mbrl_amd/csrc/pmbrl_split.h.  Offered by the
 *         latency-optimised kernel family for workgroups of up to 32 rows; other plans run F32
 *         (pmbrl_plan_info reports the arithmetic in use). */
#define PMBRL_PREC_F32 0
#define PMBRL_PREC_SPLIT 1
/*  SPLIT_F16  as SPLIT, with the forward sweep on TWO fp16 pieces (22 significant bits, 3 MFMAs per K=32,
 *         4 instead of 6 bytes per weight on the weight stream -- which is what bounds the sweeps).  fp16's
 *         range applies to the forward sweep's hidden activations and weights: a value beyond +-65504
 *         becomes inf and the rollout is reported as failed at that step (status word). */
#define PMBRL_PREC_SPLIT_F16 2

#define PMBRL_REWARD_EXP 0 /* r = exp(-w (d'Qd + u'Ru)): envs/cartpole/env.py:41-86 */
#define PMBRL_REWARD_NEG 1 /* r = -w (d'Qd + u'Ru):      envs/rendezvous/env.py:32-45 */
/* Learned reward: the dynamics head predicts the transition's reward next to the state change
 * (examples/deep_pilco_mm.py:94-99,117: DiagGaussianDensity(D + 1)).  dyn.dims[n_layers] = 2 (D + 1), split as
 * [mean_0..mean_{D-1}, mean_r | log_std_0..log_std_{D-1}, log_std_r]; my_d / Sy_d and the z_dyn_d rows are D + 1 wide
 * (z_dyn_step_stride = B (D + 1) for a per-step draw), and r~ = my[D] + Sy[D] mean_r + z[D] exp(ls_r + log Sy[D]) with
 * ls_r clamped as the states' log-stds (models/core.py:265-303 with the D of the tuple path).  The other fields of
 * pmbrl_reward are ignored.  Runs on the general kernel family only (pmbrl_plan_info reports fast = 0), F32 or
 * SPLIT_F16; not offered with groups spread over ranks (mm_span_rows).
 * With the mixture head (dyn_components = n > 1: examples/deep_pilco_mm.py:117-121 with --learn_reward) the density has
 * Dh = D + 1 dimensions: dyn.dims[n_layers] = (2 Dh + 1) n + 1, the row [n Dh means | n Dh log-stds | n logits | 1
 * log-temperature] with means and log-stds viewed as [Dh, n], component fastest -- the mixture layout with D -> Dh.  One
 * component draw per row and step (z_pi_d, u_cat_d) serves all Dh dimensions; dimensions 0 .. D-1 of the sample are the
 * state change, dimension D is r~.  my_d / Sy_d are Dh wide and z_dyn_d is the per-step draw [H, B, Dh]
 * (z_dyn_step_stride = B Dh); the noise term's derivative is taken with the last step's rows, or each step's own under
 * PMBRL_FLAG_GMM_EXACT_NOISE_GRAD, in all Dh dimensions. */
#define PMBRL_REWARD_LEARNED 2
/* The reward is evaluated by the CALLER, between the library's calls (models/core.py:290-293: any reward_func(states,
 * actions) the host language can express).  The other fields of pmbrl_reward are ignored.  Kernel family, pmbrl_plan_info
 * and pmbrl_plan_sweep_kernel are those of the same configuration with an analytic reward; groups spread over ranks
 * (mm_span_rows) are served.  The sequence of one rollout on such a plan:
 *   pmbrl_rollout_fwd       packs and sweeps only: states and actions are final, rewards_d is left alone, no loss is formed
 *   (caller)                r [H][B] and, for a rollout that will be differentiated, Jx = d r / d x~ [H][B][D] and
 *                           Ja = d r / d a [H][B][U] for unit upstream gradient, on the same stream, from the array
 *                           pmbrl_plan_reward_input names and from actions_d
 *   pmbrl_rollout_rewards   takes them in, moment-matches the rewards where the plan does, forms the loss of
 *                           pmbrl_plan_set_loss
 *   pmbrl_rollout_bwd(_adam) as for any plan; -3 unless a pmbrl_rollout_rewards call WITH Jacobians followed the latest
 *                           forward call */
#define PMBRL_REWARD_EXTERNAL 3

/* Activation of a network's hidden layers (models/core.py:15-99, nonlin=; models/activations.py), chosen per network and,
 * within a network, per hidden layer -- pmbrl_config::pol_act / dyn_act, pmbrl_mlp_call::act, pmbrl_bnn_config::act, each
 * the LAST field of its struct (pmbrl_mlp keeps its layout).  With a the pre-activation, j the unit's index and n the
 * layer's width:
 *   RELU     max(a, 0)                      TANH  torch.nn.Tanh          SILU  torch.nn.SiLU = Swish, a sigmoid(a)
 *   SIN      sin a                          EXP   exp(-a^2 / 2)          SINLU a if a > 0, else sin a
 *   HHSINLU  with s_j = -1 for even j, +1 for odd j: sin(s_j a) for j < ceil(n / 2), else max(s_j a, 0)
 *   NONE     a (a hidden Linear with no activation behind it)
 * sin / cos are the accurate library forms at any argument.  Two forms of the field:
 *   - the plain form, a value 0 .. 2 (RELU, TANH, SILU): that code for every hidden layer, exactly the values the field
 *     has always taken (0 = ReLU, so a zero-initialised struct means what it did); a plain 3 .. 7 is refused as every
 *     plain value above 2 has always been -- callers that probed with such a value see what they saw;
 *   - the per-layer form, the only one that carries SIN .. NONE (the same code in every layer for a uniform network):
 *     PMBRL_ACT_PER_LAYER | code_0 | code_1 << 3 | ... | code_l << (3 l): hidden layer l has code_l (PMBRL_ACT_LAYER;
 *     at most PMBRL_MAX_LAYERS - 1 = 7 hidden layers, 21 bits).  Bits of layers the network does not have must be 0.
 * A rollout plan with a hidden layer that is not ReLU runs on the general kernel family (pmbrl_plan_info: fast = 0,
 * PMBRL_INFO_REG = 0, PMBRL_INFO_INPLACE = 0), F32 or SPLIT_F16; its forward sweep leaves act'(pre-activation) x mask /
 * keep per hidden unit and row-step for the adjoint (4 bytes each, in place of the 1-bit activity flags of ReLU); a
 * plan whose layers are all ReLU, in either form, runs what it always ran.
 * Any other value: plan creation (pmbrl_plan_create, pmbrl_bnn_plan_create) and the stand-alone calls return -2
 * (pmbrl_act_check). */
#define PMBRL_ACT_RELU 0
#define PMBRL_ACT_TANH 1
#define PMBRL_ACT_SILU 2
#define PMBRL_ACT_SIN 3
#define PMBRL_ACT_EXP 4
#define PMBRL_ACT_SINLU 5
#define PMBRL_ACT_HHSINLU 6
#define PMBRL_ACT_NONE 7
#define PMBRL_ACT_PER_LAYER (1 << 30)
#define PMBRL_ACT_LAYER(code, l) ((code) << (3 * (l)))

/* One MLP as built by models/core.py:15-99 (mlp): Linear -> activation -> dropout ...
 * -> Linear.  dims[0] = input width, dims[n_layers] = output width.
 * n_layers = 1 .. PMBRL_MAX_LAYERS.  A rollout plan takes a network of ONE Linear layer -- no hidden layer, no mask:
 * the linear policy, a linear dynamics model -- on the general kernel family (tests/test_gpu_general_envelope.py: l0-*).
 * keep[i] is the keep-probability the masked activation of hidden layer i is
 * DIVIDED by (BDropout, models/modules.py:61) or 1.0 (eval-mode CDropout,
 * models/modules.py:158-160, and layers without dropout). */
typedef struct pmbrl_mlp {
  int32_t n_layers;
  int32_t dims[PMBRL_MAX_LAYERS + 1];
  float keep[PMBRL_MAX_LAYERS];
} pmbrl_mlp;

/* Analytic reward, the common form of envs/<env>/env.py:*Reward.forward and
 * losses.py:67-75:  phi = expand ? [others, sin(angles), cos(angles)] : x
 * (utils/angles.py:7-42);  delta = (C phi - tip_target) / norm;
 * cost = w (delta' Q delta + u' R u);  r = exp(-cost) | -cost. */
typedef struct pmbrl_reward {
  int32_t kind;   /* PMBRL_REWARD_* */
  int32_t expand; /* 1: expand angle_dims inside the reward */
  int32_t n_angle;
  int32_t angle_dims[PMBRL_MAX_ANGLE];
  int32_t k; /* rows of C (tip coordinates) */
  float C[PMBRL_MAX_TIP * PMBRL_MAX_DIM]; /* [k, De] row-major, De = D + (expand ? n_angle : 0) */
  float tip_target[PMBRL_MAX_TIP];
  float norm;
  float w;
  float Q[PMBRL_MAX_TIP * PMBRL_MAX_TIP]; /* [k, k] */
  float R[PMBRL_MAX_DIM * PMBRL_MAX_DIM]; /* [U, U] */
} pmbrl_reward;

/* Problem shape.  B is the number of particle rows resident on THIS device;
 * rows are laid out as utils/core.py:188-190 (tile): row = particle*S + sample.
 * With moment matching, rows are grouped contiguously: mm_groups groups of
 * B/mm_groups rows (utils/rollout.py:125-129); mm_groups = 0 with an MM flag
 * set means one group of all B rows (the examples' default).
 * For multi-GPU sharding B_global / row_offset locate this shard in the global
 * batch: the cyclic noise index of utils/rollout.py:53-59 is
 * (t + row_offset + b) mod B_global. */
typedef struct pmbrl_config {
  int32_t B, D, U, H;
  int32_t B_global, row_offset;
  int32_t flags;
  int32_t mm_groups;
  float max_log_std_pol; /* models/densities.py:75: log(max_noise_std) */
  float max_log_std_dyn;
  pmbrl_mlp pol; /* dims[0] = D + n_pol_angle, dims[n] = 2U */
  pmbrl_mlp dyn; /* dims[0] = D + U + n_dyn_angle, dims[n] = 2D (2 (D + 1) with PMBRL_REWARD_LEARNED) */
  pmbrl_reward reward;
  int32_t rows_per_wg_hint; /* 0 = choose automatically */
  int32_t precision;        /* PMBRL_PREC_*: arithmetic of the hidden-width GEMMs of the sweeps */
  /* angle_dims of Policy (models/core.py:233-234) and of the dynamics Regressor (models/core.py:173-174):
   * the network sees utils/angles.py:39-42's [other dims in order | sin(angles) | cos(angles)] of the
   * state (policy) or of [state | action] (dynamics; angle dims must be state dims).  mx / iSx of the
   * rollout arguments then have dyn.dims[0] entries, in that feature order. */
  int32_t n_pol_angle;
  int32_t pol_angle_dims[PMBRL_MAX_ANGLE];
  int32_t n_dyn_angle;
  int32_t dyn_angle_dims[PMBRL_MAX_ANGLE];
  /* GaussianMixtureDensity dynamics head (models/densities.py:151-259; examples/deep_pilco_mm.py:117-121):
   * n components, dyn.dims[n_layers] = (2D + 1) n + 1 = [n D means | n D log-stds | n logits | log-temperature],
   * means / log-stds indexed [d * n + c].  0 or 1: the DiagGaussianDensity head (dyn.dims[n_layers] = 2D).
   * Needs z_pi_d and u_cat_d, and z_dyn_d as a per-step draw (z_dyn_step_stride = B * D: the reference redraws
   * the Gaussian noise of this head at every step).  With PMBRL_REWARD_LEARNED: D + 1 in place of D, see there. */
  int32_t dyn_components;
  /* Moment-matching groups whose rows are spread over several ranks (e.g. mm_groups=None of
   * examples/deep_pilco_mm.py:31 on a sharded run: ONE Gaussian over the particles of all GPUs, utils/rollout.py:20-29).
   * mm_span_rows: rows of one group over all ranks (0: groups are local to this device, the fields above say it
   * all); mm_span_offset: position of this rank's B / mm_groups rows inside each group -- the cyclic noise row of
   * local row i of group g is then (t + g * mm_span_rows + mm_span_offset + i) mod B_global, row_offset is not used
   * by the moment matching.  Per step the ranks exchange the groups' sufficient statistics (fp64; forward: one
   * in-place sum of ranks x groups x (D^2 + 3 D + 1) values, adjoint: groups x (D^2 + D)) through the
   * collective attached with pmbrl_plan_set_comm / pmbrl_plan_set_collective; the sweeps then run as one launch
   * per step.  Not offered together with grad_states. */
  int32_t mm_span_rows, mm_span_offset;
  int32_t mm_span_ranks, mm_span_rank; /* ranks a group is spread over and this rank's index among them */
  int32_t pol_act, dyn_act;            /* PMBRL_ACT_*: the hidden layers' activation of the policy / the dynamics model */
} pmbrl_config;

/* Environment switches of a rollout plan, read by pmbrl_plan_create (and by nothing else in the library: a plan keeps
 * what it read).  They select between code paths that compute the same results -- the tests use them to hold a
 * non-default path against the default one, the profiles to time alternatives -- and are not needed for normal use:
 * what they override is chosen from the configuration.
 * Set at all (any value, 0 included):
 *   PMBRL_MM_PERSTEP        mm_mode 3 as one launch per step instead of one launch with a device-wide barrier per step,
 *                           and a group beyond the CU count keeps that form instead of the one-rank span form
 *   PMBRL_MM_MODE2          groups that span workgroups: separate moment-matching kernels between per-step launches
 *                           instead of the in-sweep form (mm_mode 3)
 *   PMBRL_MM_NO_BATCH       no batches of whole groups beyond the CU count: split groups keep every workgroup resident
 *   PMBRL_DW_NO_WIDE        no LDS-staged tile kernels for the dW GEMM of layers >= 128 x 128 (the block kernel instead).
 *                           On a plan of the register-resident family the ADJOINT sweep then goes to the
 *                           latency-optimised family (the forward sweep stays): the register-resident adjoint stashes no
 *                           delta of the second hidden layer, and only the whole-layer kernel rebuilds it -- slower, and
 *                           the adjoint call needs the parameter pointers in its inputs
 *   PMBRL_REG_DEBUG         the register-resident family prints its workspace offsets at every launch
 * Off when set to 0 (on when unset or any other number):
 *   PMBRL_LDS_TILES         LDS-resident weight tiles (pmbrl_fast.h, lds_tile_s): the shape-specialised 16-row
 *                           split-precision instances count on them, so =0 launches the generic instances
 *   PMBRL_MM_XCH            split groups exchange fp64 sums as data-tagged granules; =0: they exchange their rows and
 *                           meet at a flag barrier (the generic kernel instances)
 *   PMBRL_MM_TREE           one group in more than 8 parts through the two-level sum exchange
 *   PMBRL_REG, PMBRL_REG_MM, PMBRL_REG_TREE, PMBRL_REG_BWD   the register-resident family (pmbrl_reg.h): at all / with
 *                           in-sweep moment matching / with the two-level exchange / for the adjoint sweep
 *   PMBRL_FUSE_LOSS         the loss asked for through pmbrl_adam::loss_out_d formed by the gradient reduction and
 *                           the optimiser launch; =0: a launch of its own inside the backward call
 *   PMBRL_ZTAB_MERGE        the noise table of split moment-matching groups formed by extra workgroups of the
 *                           weight-pack launch; =0: a launch of its own
 *   PMBRL_WIDE              the in-place layers of pmbrl_wide.h for 512-wide hidden layers; =0: the generic in-place
 *                           form, on request (rows_per_wg_hint >= 64) only
 * Values:
 *   PMBRL_MM_PARTS=n        moment-matching groups split over n workgroups where that can be done (1: whole groups)
 *   PMBRL_REPLAY=0|1|2      default of pmbrl_plan_set_replay (1)
 *   PMBRL_DW_PIPE=off | n0,n1,...   dW GEMM behind the adjoint sweep on a second stream: never / these step ranges
 *   PMBRL_DW_STREAM=off | steps[,workgroups]   dW GEMM of the policy's second hidden layer BESIDE the one-launch
 *                           register-resident adjoint sweep (pmbrl_plan_dw_stream): never / this many of the highest steps
 *                           on this many consumer workgroups, on any plan whose sweep can publish for it
 * Read by the Python layer: PMBRL_PRECISION (default arithmetic: f32 | split | split_f16), PMBRL_LIB_PATH (the shared
 * library to load), PMBRL_SHARDED_TAIL=0 (mc_pilco keeps the separate calls on a sharded run even where the gradient
 * exchange could run inside pmbrl_rollout_bwd_adam), PMBRL_TORCH_ALLREDUCE=1 (gradient all-reduce through torch.distributed instead of the C ABI). */

typedef struct pmbrl_plan pmbrl_plan;

/* plan->info indices for pmbrl_plan_info */
enum {
  PMBRL_INFO_ROWS_PER_WG = 0,
  PMBRL_INFO_N_WG = 1,
  PMBRL_INFO_ROW_TILES = 2,
  PMBRL_INFO_LDS_BYTES = 3,
  PMBRL_INFO_N_POL_PARAMS = 4,
  PMBRL_INFO_N_DYN_PARAMS = 5,
  PMBRL_INFO_DW_SPLITS = 6,
  PMBRL_INFO_MM_MODE = 7,
  PMBRL_INFO_LD = 8,
  PMBRL_INFO_DW_BLOCKS = 9,
  PMBRL_INFO_FAST = 10,      /* 1: the latency-optimised kernel family */
  PMBRL_INFO_STAGES = 11,    /* ... its stage pair: 16 CA + CB */
  PMBRL_INFO_MM_GRID = 12,
  PMBRL_INFO_PRECISION = 13, /* PMBRL_PREC_* actually in use */
  PMBRL_INFO_DW_PIPE = 14,   /* launches the adjoint sweep is cut into so that the dW GEMM runs behind it (1: no) */
  PMBRL_INFO_MM_PARTS = 15,  /* workgroups a moment-matching group is split over (in-kernel moment matching; 1: whole groups) */
  PMBRL_INFO_REG = 16,       /* 1: the plain whole-horizon sweeps of this plan run on the register-resident family (pmbrl_reg.h) */
  PMBRL_INFO_REPLAY = 17,    /* 1: repeated calls of this plan are replayed as hipGraphs (pmbrl_plan_set_replay) */
  PMBRL_INFO_INPLACE = 18,   /* general family: 0 two activation buffers, 1 in-place layers (64-row workgroups), 2 the same on the 512-wide layers of pmbrl_wide.h */
  PMBRL_INFO_REG_FWD_CALLS = 19, /* forward sweeps of this plan the register-resident family has served so far (a graph replay counts once, when recorded) */
  PMBRL_INFO_REG_BWD_CALLS = 20, /* ... adjoint sweeps */
  PMBRL_INFO_TAIL_CALLS = 21,    /* pmbrl_rollout_bwd_adam calls of this plan that ran with the gradient exchange inside (pmbrl_plan_set_grad_comm) */
  PMBRL_INFO_COUNT = 22
};

const char* pmbrl_last_error(void);
/* Pure host code: is `act` a valid activation field (PMBRL_ACT_*, above) for a network with n_hidden hidden layers
 * (0 .. PMBRL_MAX_LAYERS - 1)?  0, or -2 with a message: a plain value above 2; in the per-layer form a non-zero code
 * of a layer the network does not have, or any bit other than PMBRL_ACT_PER_LAYER above the 21 code bits; a negative
 * value; n_hidden out of range.  Every entry point that takes an activation goes through it. */
int pmbrl_act_check(int32_t act, int32_t n_hidden);
int pmbrl_version(void);
/* 16 hex digits: hash of the kernel sources the library was built from.  Hardware-counter measurements under
 * profiles/ record it; bench.py reports such a measurement only if it was taken on the build it is running. */
const char* pmbrl_build_id(void);

/* hipGraph replay of library calls (the H-step loop as one captured graph).  Queue any sequence of library
 * calls on `stream` (not the default stream) between begin and end -- a forward call, the loss, the adjoint call with its
 * optimiser step: a whole iteration -- and replay it with ONE launch.  Pays where a call is many launches (one per
 * step: moment-matching groups beyond a workgroup, states wider than 6, the pipelined adjoint: C5 with moment matching is
 * 400+ launches per iteration); the sweeps of the cart-pole shapes are one launch each already.  Every buffer the calls
 * were given must stay where it was; the status word and the optimiser's step counter are read and written on the
 * device, so every replay is a new iteration.  Not capturable: a host-side collective (pmbrl_plan_set_collective) and the
 * peer-to-peer all-reduce (pmbrl_p2p_allreduce_*: returns -4 on a recording stream). */
typedef struct pmbrl_graph pmbrl_graph;
int pmbrl_graph_capture_begin(void* stream);
int pmbrl_graph_capture_end(void* stream, pmbrl_graph** graph_out);
int pmbrl_graph_launch(pmbrl_graph* graph, void* stream);
int pmbrl_graph_num_nodes(pmbrl_graph* graph, int64_t* n_out);
void pmbrl_graph_destroy(pmbrl_graph* graph);

/* Validates the shape, chooses the tiling and sizes the workspace. */
int pmbrl_plan_create(const pmbrl_config* cfg, int device, pmbrl_plan** out);
void pmbrl_plan_destroy(pmbrl_plan* plan);
/* Bytes of scratch the caller must provide (one device allocation, 256-byte
 * aligned) to every fwd/bwd call on this plan: fragment-packed weights, the
 * activation / gradient stashes, bit masks, dW partial sums. */
size_t pmbrl_plan_workspace_bytes(const pmbrl_plan* plan);
int pmbrl_plan_info(const pmbrl_plan* plan, int32_t* info /* [PMBRL_INFO_COUNT] */);
/* Which sweep kernels the plan resolved when it was created: *name = the runtime's name (hipKernelNameRefByPtr) of the
 * forward (adjoint = 0) or adjoint sweep kernel.  Latency-optimised family (pmbrl_plan_info: fast = 1): variant = 0 plain
 * and lean, 1 plain with optional outputs or a step range, 2 moment matching inside the sweep, 3 the same as one launch
 * with a device-wide barrier per step -- the call picks among them by its arguments; "" where the plan has no instance
 * for that variant.  General family: variant is ignored.  PMBRL_SWEEP_REG: the register-resident family's pair
 * (PMBRL_INFO_REG; "" where it does not serve the plan).  The string belongs to the runtime. */
#define PMBRL_SWEEP_REG 4
int pmbrl_plan_sweep_kernel(const pmbrl_plan* plan, int variant, int adjoint, const char** name);
/* Does the plan run the dW GEMM of the policy's second hidden layer BESIDE its one-launch adjoint sweep, on the CUs the
 * sweep leaves idle (the streamed form)?  out[0]: steps of the horizon that are streamed (-1: the form is off), out[1]:
 * consumer workgroups.  Environment PMBRL_DW_STREAM=off | <steps>[,<workgroups>] (read when the plan is created). */
int pmbrl_plan_dw_stream(const pmbrl_plan* plan, int32_t* out /* [2] */);
/* 1: the streamed consumers also form the policy head's dW / db, else 0.  The plan's rule: every step is streamed and the
 * form was not forced through PMBRL_DW_STREAM=<steps>.  PMBRL_DW_HEAD=on overrides the second condition (a forced
 * PMBRL_DW_STREAM that streams every step then streams the head too; with a cut the head stays in the block kernel),
 * PMBRL_DW_HEAD=off never streams the head. */
int pmbrl_plan_dw_head(const pmbrl_plan* plan);

/* {0,1} float mask [B, h] -> bit rows [B, ceil(h/16)] uint16 (little-endian bit
 * order).  Replaces the per-step fp32 mask multiply of models/modules.py:61,160
 * by a one-off packing at resample() time (models/modules.py:40-44,95-118). */
int pmbrl_pack_mask(void* stream, const float* mask_d, int32_t B, int32_t h,
                    int32_t src_ld, uint16_t* bits_d);

/* Dropout masks drawn ON THE DEVICE, as the bit rows the sweeps read (same layout as pmbrl_pack_mask): one launch
 * for all `rows` = H x B rows of a rollout that resamples its masks at every step (utils/rollout.py:95-98,110-115:
 * resample_policy / resample_model) or of a resample() between iterations (algorithms/mc_pilco.py:99-105, pegasus=False).
 *   kind 0  BDropout.update_noise (models/modules.py:40-44):   bit = u < keep[j]
 *   kind 1  CDropout in eval mode (models/modules.py:95-118):  probs = sigmoid((logit_p[j] + log((u + 1e-7) /
 *           (1 - (u - 1e-7)))) / temp),  bit = v < probs      (the hard sample of torch.bernoulli(probs))
 * u, v: 24-bit uniforms of Philox4x32-10 keyed by `seed`, counter (row, unit, stream, offset) -- a draw is a
 * function of (seed, offset, row, unit) only; advance `offset` between draws under one seed.  param_d: `param_len`
 * (1 or h) keep probabilities / logits.  u_d / v_d non-NULL: uniforms [rows][h] to use instead (replaying recorded
 * draws).  aux_*: for rows [aux_row0, aux_row0 + aux_rows) the float uniforms / hard samples / probabilities are
 * written too ([aux_rows][h] each, any may be NULL) -- a module keeps its last draw as state. */
int pmbrl_draw_masks(void* stream, int32_t kind, uint64_t seed, uint64_t offset, const float* param_d,
                     int32_t param_len, float temp, int32_t rows, int32_t h, const float* u_d, const float* v_d,
                     uint16_t* bits_d, int32_t aux_row0, int32_t aux_rows, float* u_out_d, float* hard_out_d,
                     float* probs_out_d);

/* Network + noise inputs shared by forward and backward. */
typedef struct pmbrl_inputs {
  const float* x0_d;          /* [B, D] */
  const float* pol_params_d;  /* flat, torch parameter order: W0[out,in], b0, W1, b1, ... */
  const float* dyn_params_d;  /* same for the dynamics MLP */
  const float* mx_d;          /* [dyn.dims[0]] (= D+U without angle dims)  models/core.py:141-145 */
  const float* iSx_d;         /* [D+U] */
  const float* my_d;          /* [D] ([D + 1] with PMBRL_REWARD_LEARNED: the reward column last) */
  const float* Sy_d;          /* [D] (the same) */
  const float* pol_scale_d;   /* [U]  models/core.py:201-206 */
  const float* pol_bias_d;    /* [U] */
  const uint16_t* pol_mask_bits_d[PMBRL_MAX_LAYERS]; /* per hidden layer, from pmbrl_pack_mask */
  const uint16_t* dyn_mask_bits_d[PMBRL_MAX_LAYERS];
  const float* z_pol_d;       /* [B, U]  models/densities.py:78,111-119 */
  const float* z_dyn_d;       /* [B, D] ([B, D + 1] with PMBRL_REWARD_LEARNED); mixture head: [H, B, D] ([H, B, D + 1]) */
  int64_t z_pol_step_stride;  /* elements between steps; 0 = the same frozen z at every step
                                 (resample_noise=False), B*U = a fresh [H,B,U] draw per step */
  int64_t z_dyn_step_stride;
  const float* z_mm_d;        /* [>= B_global, D] or NULL  algorithms/mc_pilco.py:57-62 */
  const float* z_rr_d;        /* [>= B_global, 1] or NULL */
  /* mixture head only (NULL otherwise) */
  const float* z_pi_d;        /* [B, n] frozen Gumbel noise (models/densities.py:166-167,213-216) */
  const float* u_cat_d;       /* [H, B] uniforms in [0, 1): the component of (t, b) is drawn by inverse CDF over the
                                 tempered softmax (the reference draws it from torch's generator at every step,
                                 models/densities.py:221-222) */
} pmbrl_inputs;

/* utils/rollout.py:62-163 (rollout) fused over all H steps, including
 * models/core.py:221-248 (Policy.forward), models/core.py:265-303
 * (DynamicsModel.forward), models/densities.py:87-121, the reward module and
 * utils/rollout.py:20-29 (mm_resample_).
 * Outputs: states [H+1,B,D], actions [H,B,U], rewards [H,B,1].
 * status_d: device int32[2].  [0] is set to 0x7fffffff on entry; on a numerical
 * failure at step t (non-finite state/reward, non-positive pivot) atomically
 * min'ed with t (= number of valid steps before the failure).  [1] is the adjoint
 * sweep's failure flag (pmbrl_rollout_bwd) and is CLEARED by this call: a caller
 * that only ever evaluates forward must still hand over two words. */
int pmbrl_rollout_fwd(pmbrl_plan* plan, void* stream, void* workspace_d,
                      const pmbrl_inputs* in, float* states_d, float* actions_d,
                      float* rewards_d, int32_t* status_d);

/* The adjoint of the above = what loss.backward() computes in
 * algorithms/mc_pilco.py:190-197 for loss = sum_{t,b} grad_rewards[t,b] *
 * rewards[t,b] (+ sum grad_states[t,b,:] . states[t,b,:] when grad_states_d
 * [H+1,B,D] is given -- terminal value bootstrap, algorithms/mc_pilco.py:136-140;
 * + sum grad_actions[t,b,:] . actions[t,b,:] when grad_actions_d [H,B,U] is given).
 * Must follow a pmbrl_rollout_fwd on the same plan/workspace/inputs.
 * Outputs: grad_pol_flat_d [n_pol_params] (overwritten), optional grad_x0_d
 * [B,D], optional action_grad_norms_d [H,B] (||dL/da_t|| per row, the
 * prioritised-replay hook of algorithms/mc_pilco.py:156-188).
 * status_d (optional, device int32[2]): status_d[0] is the word pmbrl_rollout_fwd
 * wrote; the adjoint is taken over the first n = min(H, status_d[0]) steps only --
 * the truncated horizon the reference continues with after a late failure
 * (utils/rollout.py:154-157): grad_rewards / grad_actions of steps >= n are ignored,
 * the terminal state gradient is grad_states[n], action_grad_norms rows >= n are
 * left untouched.  Read on the device: no host round trip between the sweeps.
 * status_d[1] is set non-zero if the sweep itself failed (a barrier or a statistics
 * exchange of a moment-matching group spanning workgroups timed out); it is CLEARED BY
 * pmbrl_rollout_fwd (the forward call's status array must be this one: int32[2]) --
 * a second adjoint call behind a failed one still reports the failure.
 * NULL: the full horizon. */
int pmbrl_rollout_bwd(pmbrl_plan* plan, void* stream, void* workspace_d,
                      const pmbrl_inputs* in, const float* states_d,
                      const float* actions_d, const float* rewards_d,
                      const float* grad_rewards_d, const float* grad_states_d,
                      const float* grad_actions_d, float* grad_pol_flat_d,
                      float* grad_x0_d, float* action_grad_norms_d, int32_t* status_d);

/* ---- a reward evaluated by the caller (PMBRL_REWARD_EXTERNAL) -------------------------------------------------------
 * pmbrl_plan_reward_input: where the [H][B][D] array the reward is a function of lives -- the sampled next states BEFORE
 * their moment matching, row (t, b) being the state r[t][b] is the reward of (models/core.py:292: prev_states + dstates).
 * *ws_offset_out: its byte offset into workspace_d (a multiple of 256) when the plan moment-matches its states
 * (PMBRL_FLAG_MM_STATES), else -1: the array is then states_d + B D, the states of steps 1 .. H.  No launch; any plan kind.
 * pmbrl_rollout_rewards: the rest of a forward call on an external plan.  r_d [H][B]; jx_d [H][B][D] and ja_d [H][B][U]
 * together, or both NULL for a forward-only rollout; the arrays are read by the call's first launch and may be reused
 * once the stream has passed it.  One launch copies r to where the plan's reward moment matching (or rewards_d) expects
 * it and the Jacobians to where the adjoint sweeps read them, reports the first step with a non-finite sampled state,
 * reward or Jacobian entry by atomicMin(status_d[0], t) and clears status_d[1]; behind it the reward moment matching
 * (PMBRL_FLAG_MM_REWARDS; groups spread over ranks: one exchange through the attached collective) and the loss of
 * pmbrl_plan_set_loss.  Rows of steps at or beyond a failed one may hold anything; what they hold is ignored.
 * workspace_d, stream and status_d are the forward call's; the forward call's inputs (pmbrl_inputs and what it points
 * at) must still be alive.  Never recorded or replayed (pmbrl_plan_set_replay).
 * Returns -1 for a NULL plan, workspace_d, r_d, rewards_d or status_d and for exactly one of jx_d / ja_d being NULL, -2 on
 * a plan of another reward kind, -3 without a forward call on the plan before it; nothing is queued then. */
int pmbrl_plan_reward_input(const pmbrl_plan* plan, int64_t* ws_offset_out);
int pmbrl_rollout_rewards(pmbrl_plan* plan, void* stream, void* workspace_d, const float* r_d, const float* jx_d,
                          const float* ja_d, float* rewards_d, int32_t* status_d);

/* out[0] = sum_i a[i] * w[i]  (the discounted-return loss of
 * algorithms/mc_pilco.py:134-144,190 given w = dL/dr). Deterministic. */
int pmbrl_weighted_sum(void* stream, const float* a_d, const float* w_d,
                       int64_t n, float* out_d);
/* The same over the first min(n_steps, *status_d) blocks of n_per_step entries: the loss of
 * a truncated horizon (status_d = the word pmbrl_rollout_fwd wrote, read on the device). */
int pmbrl_weighted_sum_steps(void* stream, const float* a_d, const float* w_d,
                             int64_t n_per_step, int32_t n_steps, const int32_t* status_d,
                             float* out_d);

/* torch.nn.utils.clip_grad_norm_ (algorithms/mc_pilco.py:209-210) fused with
 * torch.optim.Adam.step (examples/deep_pilco_mm.py:166; no weight decay, no
 * amsgrad).  max_norm <= 0 disables clipping.  norm_out_d (optional) receives
 * the pre-clip global L2 norm.  grads are left scaled by the clip coefficient,
 * like the reference. */
int pmbrl_clip_adam(void* stream, float* params_d, float* grads_d,
                    float* exp_avg_d, float* exp_avg_sq_d, int64_t n,
                    int64_t step, double lr, double beta1, double beta2, double eps,
                    double max_norm, float* norm_out_d);

/* The same step, decided on the device: taken only if the rollout that produced
 * the gradient completed (*status_d >= expect, status_d = the word
 * pmbrl_rollout_fwd wrote; expect = H to require the whole horizon, or
 * min(H, 6) to continue on a truncated horizon of more than 5 steps like
 * utils/rollout.py:154-157), in which case the device-side step
 * counter *step_d is advanced first and its bias corrections are used;
 * otherwise parameters, moments and counter are left untouched.  This is the
 * reference's "RuntimeError -> skip the optimiser step" (algorithms/
 * mc_pilco.py:122-131) without a host round trip per iteration: the host may
 * read the status word one iteration late.  status_d is the two-word status of
 * pmbrl_rollout_fwd / _bwd: the step is also skipped when status_d[1] != 0 (the adjoint
 * sweep reported a failure of its own -- a barrier between workgroups timed out). */
int pmbrl_clip_adam_guarded(void* stream, float* params_d, float* grads_d,
                            float* exp_avg_d, float* exp_avg_sq_d, int64_t n,
                            int64_t* step_d, double lr, double beta1, double beta2,
                            double eps, double max_norm, float* norm_out_d,
                            const int32_t* status_d, int32_t expect);

/* ---- fused iteration tail (one process, or rows sharded over ranks: pmbrl_plan_set_grad_comm below) ----------------
 * pmbrl_plan_set_loss: dL/dr weights [H][B] (device, resident; algorithms/mc_pilco.py:134-144: +-gamma_t / B) -- every
 * pmbrl_rollout_fwd on the plan then also leaves sum_{t < valid, b} w r in *loss_out_d (the reduction of
 * pmbrl_weighted_sum_steps, queued by the forward call itself); NULL switches it off.
 * pmbrl_rollout_bwd_adam: pmbrl_rollout_bwd followed by clip_grad_norm_ + Adam.step as pmbrl_clip_adam_guarded defines
 * them (taken on the device only if the rollout completed `expect_steps` steps and the adjoint reported no failure), in
 * one call: the whole tail of an iteration is queued without returning to the host language.  status_d: int32[2],
 * required. */
typedef struct pmbrl_adam {
  float* params_d;        /* flat policy parameters (the vector pmbrl_inputs::pol_params_d points at) */
  float* exp_avg_d;
  float* exp_avg_sq_d;
  int64_t* step_d;        /* device-side step counter, advanced when the step is taken */
  double lr, beta1, beta2, eps, max_norm;   /* max_norm <= 0: no clipping */
  float* norm_out_d;      /* optional: the gradient norm before clipping */
  int32_t expect_steps;   /* the step is taken if the rollout completed at least this many steps (0: H) */
  float* loss_out_d;      /* optional (round 6): the loss sum_{t < valid steps, b} grad_rewards[t][b] * rewards[t][b] of THIS
                           * call's arguments, written by the optimiser launch whether or not the step is taken -- the
                           * launch pmbrl_plan_set_loss queues behind the forward call is then not needed (one launch
                           * less per iteration); NULL: not wanted */
} pmbrl_adam;
int pmbrl_plan_set_loss(pmbrl_plan* plan, const float* loss_weights_d, float* loss_out_d);
int pmbrl_rollout_bwd_adam(pmbrl_plan* plan, void* stream, void* workspace_d, const pmbrl_inputs* in,
                           const float* states_d, const float* actions_d, const float* rewards_d,
                           const float* grad_rewards_d, const float* grad_states_d, const float* grad_actions_d,
                           float* grad_pol_flat_d, float* grad_x0_d, float* action_grad_norms_d, int32_t* status_d,
                           const pmbrl_adam* opt);

/* ---- optimiser rules: any torch.optim.Adam / AdamW configuration -----------------------------------------------------
 * What the optimiser-step lines of the reference do when the caller hands them another Adam than the plain one
 * (algorithms/mc_pilco.py:209-214, utils/train_regressor.py:113-131, examples/deep_pilco_no_mm_with_value.py:60: they
 * accept any torch.optim optimiser): up to PMBRL_OPT_MAX_GROUPS parameter groups with their own lr / betas / eps /
 * weight_decay, L2 or decoupled (AdamW) decay, amsgrad and maximize.  A segment is a contiguous run of the flat parameter
 * vector that belongs to one group (the caller merges neighbouring tensors of the same group).  Per element, in torch's
 * order (coef: the clip coefficient of the global norm of the RAW gradient over all groups):
 *   g = coef g_raw (stored back, without the decay term);  MAXIMIZE: g = -g from here on (the stored one keeps its sign);
 *   DECOUPLED: p *= (1 - lr wd), the factor formed in double and rounded once;  else wd != 0: g += wd p;
 *   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  AMSGRAD: vmax = max(vmax, v), used in place of v below;
 *   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).
 * Bias corrections as pmbrl_clip_adam(_guarded) forms them; one step counter for all groups.  One launch covers all
 * groups.  A rule with one group, no flags and weight_decay 0 gives the bits of the calls without a rule. */
#define PMBRL_OPT_MAX_GROUPS   8
#define PMBRL_OPT_MAX_SEGMENTS 32
#define PMBRL_OPT_DECOUPLED 1
#define PMBRL_OPT_AMSGRAD   2
#define PMBRL_OPT_MAXIMIZE  4
typedef struct pmbrl_opt_group { double lr, beta1, beta2, eps, weight_decay; int32_t flags; } pmbrl_opt_group;
typedef struct pmbrl_opt_rule {
  int32_t n_groups;   pmbrl_opt_group group[PMBRL_OPT_MAX_GROUPS];
  int32_t n_segments; int64_t seg_end[PMBRL_OPT_MAX_SEGMENTS];   /* ascending, last == n */
  int32_t seg_group[PMBRL_OPT_MAX_SEGMENTS];
  float*  max_exp_avg_sq_d;   /* required iff any group has AMSGRAD; n floats */
} pmbrl_opt_rule;
/* Pure host code: 0, or -2 with a message for counts out of range, a seg_end that does not ascend or does not end at n, a
 * group index out of range, lr < 0, a beta outside [0, 1), eps < 0, weight_decay < 0, unknown flag bits, AMSGRAD without
 * max_exp_avg_sq_d.  Every call below goes through it. */
int pmbrl_opt_rule_check(const pmbrl_opt_rule* rule, int64_t n);
/* pmbrl_clip_adam / pmbrl_clip_adam_guarded with the hyper-parameters of `rule` */
int pmbrl_clip_adam_rule(void* stream, float* params_d, float* grads_d, float* exp_avg_d, float* exp_avg_sq_d, int64_t n,
                         int64_t step, double max_norm, float* norm_out_d, const pmbrl_opt_rule* rule);
int pmbrl_clip_adam_rule_guarded(void* stream, float* params_d, float* grads_d, float* exp_avg_d, float* exp_avg_sq_d,
                                 int64_t n, int64_t* step_d, double max_norm, float* norm_out_d, const int32_t* status_d,
                                 int32_t expect, const pmbrl_opt_rule* rule);
/* The rule is copied into the plan; NULL detaches it.  While one is attached, pmbrl_rollout_bwd_adam (the sharded tail
 * included) takes the hyper-parameters from it: lr / beta1 / beta2 / eps of pmbrl_adam are ignored, its pointers,
 * max_norm, expect_steps and loss_out_d are kept.  The rule's contents, max_exp_avg_sq_d included, are part of what makes
 * two backward calls "the same" for pmbrl_plan_set_replay. */
int pmbrl_plan_set_optimizer(pmbrl_plan* plan, const pmbrl_opt_rule* rule);

/* ---- gradient all-reduce over xGMI (RCCL) ---------------------------------- */
/* The one collective of the sharded path: the sum of the flat policy gradient over the
 * ranks, in place, issued on the caller's stream right behind pmbrl_rollout_bwd -- no host round
 * trip, no second stream.  Rows are sharded by whole moment-matching groups, so nothing else crosses
 * GPUs (algorithms/mc_pilco.py has no counterpart: the reference is single-process).
 *   pmbrl_comm_unique_id: rank 0 obtains the 128-byte RCCL id and hands it to the other ranks by
 *   whatever channel the launcher has (prob_mbrl_amd.distributed broadcasts it over
 *   torch.distributed's store); pmbrl_comm_init: every rank, once; collective.
 * librccl is loaded at run time (dlopen; the copy the process already has, else the system's), so
 * the library has no link-time dependency on it and single-GPU users never load it. */
#define PMBRL_COMM_ID_BYTES 128
typedef struct pmbrl_comm pmbrl_comm;
int pmbrl_comm_unique_id(void* id_out /* host, PMBRL_COMM_ID_BYTES */);
int pmbrl_comm_init(const void* id /* host, PMBRL_COMM_ID_BYTES */, int32_t rank, int32_t nranks,
                    int32_t device, pmbrl_comm** out);
int pmbrl_allreduce_sum(pmbrl_comm* comm, void* stream, float* buf_d, int64_t n);
/* the number of ranks the COMMUNICATOR reports (ncclCommCount) -- what bench.py prints as rccl_ranks, so that a
 * scaling record proves RCCL saw N ranks rather than echoing WORLD_SIZE */
int pmbrl_comm_count(pmbrl_comm* comm, int32_t* nranks_out);
void pmbrl_comm_destroy(pmbrl_comm* comm);

/* In-place fp64 sum over the ranks of buf_d[0..n) on `stream`: the per-step statistics exchange of
 * moment-matching groups that span ranks (pmbrl_config.mm_span_rows).  pmbrl_plan_set_comm: RCCL through the
 * communicator above (no host round trip; capturable).  pmbrl_plan_set_collective: any other transport --
 * fn(ctx, stream, buf_d, n) must return 0 once the sum is ORDERED on `stream` (it may block the host); e.g. a
 * host-staged torch.distributed / MPI all-reduce, which is how the two-process tests run on one device.
 * The plan keeps the pointer, not the communicator: destroy the plan first. */
typedef int (*pmbrl_collective_fn)(void* ctx, void* stream, double* buf_d, int64_t n);
int pmbrl_plan_set_comm(pmbrl_plan* plan, pmbrl_comm* comm);
int pmbrl_plan_set_collective(pmbrl_plan* plan, pmbrl_collective_fn fn, void* ctx);

/* ---- one-shot peer-to-peer all-reduce for latency-bound messages (pmbrl_p2p.hip) -------------------------------
 * The per-step statistics of moment-matching groups spread over ranks (a few KB, 2 H + 2 times per iteration) and the
 * flat policy gradient (163 KiB) are latency-, not bandwidth-bound: a ring pays 2 (N - 1) hops.  Here every rank writes
 * its contribution into a slot of every peer's buffer (stores through IPC-mapped pointers: xGMI between GPUs), raises
 * a flag per peer, waits for its own N flags and adds the N slots in rank order -- one hop, the same bits on every rank,
 * one kernel per rank on the caller's stream.  Setup: every rank creates its object (one uncached device allocation
 * sized for messages of up to max_bytes), exports a 64-byte handle (hipIpcGetMemHandle), the launcher carries the
 * handles to all ranks by any channel, every rank opens every peer's.  Ranks may be processes on different GPUs of
 * one node, or on ONE GPU (how the tests run it).  Waits are bounded: pmbrl_p2p_error reports a peer that never
 * arrived.  pmbrl_plan_set_p2p attaches it as the statistics exchange of a plan (like pmbrl_plan_set_comm).
 * NOT capturable: pmbrl_p2p_allreduce_* returns -4 on a stream that is recording (pmbrl_graph_capture_begin): the
 * generation its flags carry is a kernel argument, a replay would read stale slots. */
#define PMBRL_P2P_HANDLE_BYTES 64
#define PMBRL_P2P_MAX_RANKS 16
typedef struct pmbrl_p2p pmbrl_p2p;
int pmbrl_p2p_create(int32_t rank, int32_t nranks, int32_t device, int64_t max_bytes, pmbrl_p2p** out);
int pmbrl_p2p_handle(pmbrl_p2p* p, void* handle_out /* host, PMBRL_P2P_HANDLE_BYTES */);
int pmbrl_p2p_open(pmbrl_p2p* p, int32_t peer, const void* handle /* host, PMBRL_P2P_HANDLE_BYTES */);
int pmbrl_p2p_allreduce_f32(pmbrl_p2p* p, void* stream, float* buf_d, int64_t n);    /* in place */
int pmbrl_p2p_allreduce_f64(pmbrl_p2p* p, void* stream, double* buf_d, int64_t n);
int pmbrl_plan_set_p2p(pmbrl_plan* plan, pmbrl_p2p* p);
int pmbrl_p2p_error(pmbrl_p2p* p, int32_t* err_out);   /* host sync; 1: a wait timed out since the last call */
void pmbrl_p2p_destroy(pmbrl_p2p* p);

/* ---- the fused iteration tail on a sharded run: the collective inside pmbrl_rollout_bwd_adam ----------------------
 * pmbrl_plan_set_grad_comm attaches the transport of the flat policy gradient to a plan: an RCCL communicator or a
 * peer-to-peer object, at most one of the two non-NULL; both NULL detaches it.  The plan keeps the pointer and owns a
 * small exchange buffer of its own: destroy the plan (or detach) before the transport.  Not offered for plans whose
 * moment-matching groups are spread over ranks (mm_span_rows).
 * With a transport attached, pmbrl_rollout_bwd_adam queues on the caller's stream, without a host synchronisation:
 *   1. horizon agreement: every rank contributes min(status_d[0], H) as entry `rank` of a vector of `nranks` floats
 *      (zero elsewhere), the vector is summed over the ranks, and the minimum of its entries is written to status_d[0]
 *      where it is smaller: the adjoint sweep, the dW GEMM and the loss of every rank stop at the same step;
 *   2. the adjoint sweep, the dW GEMM and the gradient reduction as without a transport, the reduction leaving the flat
 *      gradient, this rank's partial loss and this rank's failure flag (status_d[1] != 0, or a peer-to-peer wait that
 *      timed out on this rank) in one buffer of n + 2 floats;
 *   3. ONE in-place sum of that buffer over the ranks (ncclAllReduce / the one-hop exchange: rank order, the same bits
 *      on every rank);
 *   4. the summed gradient into grad_pol_flat_d, the partial sums of ITS norm, and the decision: clip + Adam are taken
 *      as pmbrl_clip_adam_guarded defines them, and also skipped when the summed failure flag is non-zero (on every
 *      rank alike; status_d[1] is then set on every rank).  loss_out_d receives the loss summed over the ranks,
 *      norm_out_d the norm of the summed gradient.
 *      A peer-to-peer wait that times out INSIDE exchange 3 is not in that exchange's flag: the rank it happened on
 *      skips the step and sets its own status_d[1] in this call, the other ranks have taken the step and learn of it in
 *      the NEXT call's exchange (the error word of pmbrl_p2p is sticky until pmbrl_p2p_error reads it) -- one
 *      iteration late.  The replicas differ from then on: the caller must stop, not resample.
 * Every rank must make the call: it is a collective.  A plan with a peer-to-peer transport runs the call eagerly
 * whatever pmbrl_plan_set_replay says (the exchange cannot be recorded); with RCCL it may be recorded, the transport is
 * part of what two calls must have in common.  Without a transport the call is what it was, bit for bit; so is a
 * transport of one rank.  PMBRL_INFO_TAIL_CALLS counts the calls that ran this way.
 * Launches this adds to the one-process call: three for the horizon (vector, exchange, minimum) and three around the
 * gradient (pack, exchange, finish).  The reduction's last stage does not yet store into the peers' slots itself, and
 * the horizon vector is not yet written by the forward call.
 * Returns -2 if the flat gradient (+ 2 floats) does not fit the peer-to-peer slots, -3 for groups spread over ranks:
 * the plan is left without a transport, the separate calls still work. */
int pmbrl_plan_set_grad_comm(pmbrl_plan* plan, pmbrl_comm* comm, pmbrl_p2p* p2p);

/* Optional per-kernel timing for bench.py's roofline line: when enabled, the
 * library brackets its kernels with hipEvents on the caller's stream;
 * pmbrl_plan_read_timing waits for them and returns the last call's durations
 * in milliseconds (-1 = not run). */
enum {
  PMBRL_TIMER_PACK = 0,      /* weight fragment packing */
  PMBRL_TIMER_FWD = 1,       /* pm_rollout_fwd (+ external mm kernels) */
  PMBRL_TIMER_BWD = 2,       /* pm_rollout_bwd (+ external mm kernels) */
  PMBRL_TIMER_DW = 3,        /* pm_dw_kernel */
  PMBRL_TIMER_DW_REDUCE = 4, /* pm_dw_reduce */
  PMBRL_TIMER_REWARD = 5,    /* pm_reward_all_kernel (+ reward moment matching) */
  PMBRL_TIMER_COUNT = 8
};
int pmbrl_plan_set_timing(pmbrl_plan* plan, int on);

/* Replay of repeated calls.  Some forms of the sweeps are ONE LAUNCH PER STEP (moment-matching groups
 * beyond what a workgroup or a set of exchanging workgroups holds, wide states): 100-400 launches per iteration, whose
 * launch cost is then most of the iteration.  With replay on, pmbrl_rollout_fwd / pmbrl_rollout_bwd(_adam) compare their
 * arguments (stream, workspace, every pointer and scalar of the call, the queued loss) with the previous call's: the
 * second identical call is recorded as a hipGraph (nothing but launches, memsets and event
 * hand-offs is queued by these calls) and launched, every further one is ONE hipGraphLaunch.  Any difference drops the
 * graph and runs the call as usual: an optimisation loop that keeps its buffers gets the replay, a caller that
 * allocates new outputs every time never pays for a capture.  Results are those of the eager calls bit for bit (the
 * same kernels in the same order).  The recording is made on a stream of the plan's own, so the caller's may be the
 * legacy default stream.  Not used while per-kernel timing or the cycle-stamp profile is on, inside a capture of the
 * caller's own, or with a host-side collective attached.
 * Default: on for the one-launch-per-step forms, off elsewhere (a plain iteration is a dozen launches the queue
 * already hides).  on = 0: never; 1: the default; 2: every form.  Environment PMBRL_REPLAY=0|1|2 sets the default. */
int pmbrl_plan_set_replay(pmbrl_plan* plan, int on);
/* calls that went out as one graph launch so far: n_out[0] forward calls, n_out[1] adjoint calls */
int pmbrl_plan_replay_count(const pmbrl_plan* plan, int64_t* n_out /* [2] */);
int pmbrl_plan_read_timing(pmbrl_plan* plan, float* ms /* [PMBRL_TIMER_COUNT] */);

/* Debug: workgroup 0 writes shader-clock stamps [H][32] at its phase boundaries
 * (forward into fwd_d, backward sweep into bwd_d; NULL = off). */
int pmbrl_plan_set_prof(pmbrl_plan* plan, long long* fwd_d, long long* bwd_d);

/* ---- stand-alone network evaluation ------------------------------------- */
/* One Bayesian MLP with a diagonal-Gaussian head evaluated on B independent rows: what the
 * reference's Policy.forward (models/core.py:221-248) and Regressor / DynamicsModel.forward
 * (models/core.py:169-187, 265-303) compute outside a rollout (apply_controller, model
 * evaluation):
 *   xin = (x - in_shift) * in_iscale                      (both NULL: xin = x)
 *   h   = act(xin W0^T + b0) * mask0 / keep0 ; ...        (mask NULL: no dropout on that layer; act = pmbrl_mlp_call::act)
 *   (mu, l) = split(h W_L^T + b_L) ;  l <- -softplus(-l + max_log_std) + max_log_std
 *   out_scale/out_shift given:  mu <- mu*out_scale + out_shift ;  l <- l + log(out_scale)
 *   sample = mu + z * exp(l)                              (z NULL: sample = mu)
 *   sq_scale/sq_bias given:    sample <- sq_scale * tanh(sample) + sq_bias
 * Outputs may be NULL.  mask_bits are bit rows as produced by pmbrl_pack_mask.
 * Accepted: 2 .. 8 Linear layers, every width (input and head included) 1 .. 1024, an even head; else -2.  The forward
 * keeps two 16-row buffers of (widest layer rounded up to 16, + 8) floats + 24 KB in LDS: 156 672 B at 1024, so its own
 * LDS refusal (-3, "too wide for LDS") cannot be reached with widths the range check lets through. */
typedef struct {
  int32_t B;                  /* rows */
  pmbrl_mlp net;              /* dims[0] = input width, dims[n_layers] = 2 * output width */
  float max_log_std;
  int32_t act;                /* PMBRL_ACT_*: the hidden layers' activation */
} pmbrl_mlp_call;

size_t pmbrl_mlp_workspace_bytes(const pmbrl_mlp_call* call);
int pmbrl_mlp_forward(void* stream, const pmbrl_mlp_call* call, void* workspace_d,
                      const float* x_d, const float* params_flat_d,
                      const uint16_t* const* mask_bits_d /* [n_layers-1], entries may be NULL */,
                      const float* z_d /* [B][n_out] or NULL */,
                      const float* in_shift_d, const float* in_iscale_d,
                      const float* out_scale_d, const float* out_shift_d,
                      const float* sq_scale_d, const float* sq_bias_d,
                      float* sample_d /* [B][n_out] */, float* mean_d, float* log_std_d);

/* Gradient of pmbrl_mlp_forward's outputs with respect to its input rows (network constant):
 * grad_x = (d sample / d x)^T g_sample + (d mean / d x)^T g_mean + (d log_std / d x)^T g_log_std,
 * same arguments as the forward; any of the three upstream gradients may be NULL.  Used when a
 * stand-alone network sits inside a differentiable computation (the terminal value V(x_H) of
 * algorithms/mc_pilco.py:136-140).
 * LDS: the kernel keeps every Linear's input and two gradient buffers -- and, where a hidden layer is not ReLU, the
 * first hidden layer's derivatives (the others live in dead input buffers) -- resident:
 *   (n_layers + 2 [+ 1]) * 16 * (widest layer rounded up to 16, + 8) floats + 24 KB,
 * the widest taken over ALL widths, input and head included.  Beyond 160 KB the call is refused with -3 and "LDS" in
 * the message (there is no workspace query of its own: pmbrl_mlp_workspace_bytes serves the forward too and does not
 * refuse).  One hidden layer of 528 units (4 buffers) is the widest it takes, 416 with two (5), 208 with seven (10). */
int pmbrl_mlp_grad_input(void* stream, const pmbrl_mlp_call* call, void* workspace_d,
                         const float* x_d, const float* params_flat_d,
                         const uint16_t* const* mask_bits_d, const float* z_d,
                         const float* in_shift_d, const float* in_iscale_d,
                         const float* out_scale_d, const float* out_shift_d,
                         const float* sq_scale_d, const float* sq_bias_d,
                         const float* g_sample_d, const float* g_mean_d, const float* g_log_std_d,
                         float* grad_x_d /* [B][n_in] */);

/* Backward of pmbrl_mlp_forward with respect to its input rows AND its parameters, one launch (plus a small
 * reduction): grad_x as pmbrl_mlp_grad_input gives it, and
 *   grad_params = (d sample / d theta)^T g_sample + (d mean / d theta)^T g_mean + (d log_std / d theta)^T g_log_std
 * in the layout of params_flat (W0 [out][in], b0, W1, b1, ...).  What a loss on a stand-alone Policy / Regressor /
 * critic call needs (behaviour cloning, a custom dynamics or critic loss) and what a per-step rollout hook
 * (utils/rollout.py:93-163, on_pol_eval) differentiates through.  The masks are constants (eval-mode dropout).
 *  - Same ten inputs as the forward; any of the three upstream gradients may be NULL, all three NULL is -1.
 *  - Either output may be NULL and its work is skipped; outputs are OVERWRITTEN, not accumulated into.
 *  - No float atomics: two calls with the same inputs give the same bits.  At most PMBRL_MLP_BWD_MAX_BLOCKS workgroups
 *    run; each walks its 16-row tiles in order and sums its share of the gradient in a slab [n_params] of its own in
 *    the workspace, and a second launch adds the slabs in slab order.  The workspace therefore stops growing at
 *    B = 16 * PMBRL_MLP_BWD_MAX_BLOCKS rows.  A network so large that this many slabs would exceed
 *    PMBRL_MLP_BWD_SLAB_BYTES gets fewer workgroups (PMBRL_MLP_BWD_SLAB_BYTES / (4 n_params), at least one; "at least
 *    one" needs more than 16 M parameters, which no network within the LDS limit below has: the largest, one hidden
 *    layer of 528 between 528 inputs and a head of 528, has 0.56 M and gets 30).
 *  - The kernel keeps every Linear's input -- and with Tanh / SiLU every hidden layer's derivatives -- in LDS:
 *    (n_layers + 2 [+ n_layers - 1]) * 16 * (widest layer rounded up to 16, + 8) floats + 24 KB.  Beyond 160 KB the
 *    workspace query gives 0 and the call -3, both with a message (pmbrl_mlp_grad_input, which needs less, is a
 *    separate call and unchanged).
 * The workspace is pmbrl_mlp_backward_workspace_bytes (>= pmbrl_mlp_workspace_bytes; 0 + pmbrl_last_error on a bad
 * call); it may be shared with the forward of the same call. */
#define PMBRL_MLP_BWD_MAX_BLOCKS 256
#define PMBRL_MLP_BWD_SLAB_BYTES (64u << 20)
size_t pmbrl_mlp_backward_workspace_bytes(const pmbrl_mlp_call* call);
int pmbrl_mlp_backward(void* stream, const pmbrl_mlp_call* call, void* workspace_d,
                       const float* x_d, const float* params_flat_d,
                       const uint16_t* const* mask_bits_d, const float* z_d,
                       const float* in_shift_d, const float* in_iscale_d,
                       const float* out_scale_d, const float* out_shift_d,
                       const float* sq_scale_d, const float* sq_bias_d,
                       const float* g_sample_d, const float* g_mean_d, const float* g_log_std_d,
                       float* grad_x_d /* [B][n_in] or NULL */,
                       float* grad_params_d /* flat, the layout of params_flat, or NULL */);

/* pmbrl_mlp_backward for a network some of whose hidden layers are concrete dropout in TRAIN mode
 * (models/modules.py:102-118,151-153): the mask of such a layer is a hard Bernoulli sample of
 *   probs = sigmoid((logit_p[j] + log((u[r][j] + 1e-7) / (1 - (u[r][j] - 1e-7)))) / temp),   h = a * hard  (keep = 1),
 * and the backward goes through probs, which is how a dropout rate is learned:
 *   grad_logit[j] = sum_r gh[r][j] * a[r][j] * probs[r][j] * (1 - probs[r][j]) / temp
 * with a the activation before the mask and gh the gradient at the layer's output before the mask, both at dropped
 * units too.  mask_bits_d stay the caller's hard sample (it may be a replayed recording); u_d is the noise it was drawn
 * from.  Layers with u_d[l] == NULL (Bernoulli dropout, no dropout) are as in pmbrl_mlp_backward, and grad_x / grad_params
 * are the bits pmbrl_mlp_backward gives on the same inputs.  grad_logit_d: the concrete layers' [h_l], concatenated in
 * layer order, OVERWRITTEN; formed like the weight gradient (slabs summed in slab order, no atomics: the same bits
 * call after call).  probs (1 - probs) is formed as e / (1 + e)^2, e = exp(-|c / temp|): finite for any c / temp.
 * LDS: one more 16-row buffer per concrete layer than pmbrl_mlp_backward; beyond 160 KB the workspace query gives 0 and
 * the call -3, both with a message.  At least one layer must be concrete (else -2); keep of a concrete layer must be 1. */
typedef struct {
  const float* u_d[PMBRL_MAX_LAYERS];     /* [B][h_l] fp32 uniform noise, NULL: hidden layer l is not concrete */
  const float* logit_d[PMBRL_MAX_LAYERS]; /* [h_l] */
  float temp[PMBRL_MAX_LAYERS];           /* > 0 */
} pmbrl_mlp_concrete;
size_t pmbrl_mlp_backward_concrete_workspace_bytes(const pmbrl_mlp_call* call, const pmbrl_mlp_concrete* conc);
int pmbrl_mlp_backward_concrete(void* stream, const pmbrl_mlp_call* call, void* workspace_d,
                                const float* x_d, const float* params_flat_d,
                                const uint16_t* const* mask_bits_d, const float* z_d,
                                const float* in_shift_d, const float* in_iscale_d,
                                const float* out_scale_d, const float* out_shift_d,
                                const float* sq_scale_d, const float* sq_bias_d,
                                const float* g_sample_d, const float* g_mean_d, const float* g_log_std_d,
                                float* grad_x_d /* [B][n_in] or NULL */,
                                float* grad_params_d /* flat, the layout of params_flat, or NULL */,
                                const pmbrl_mlp_concrete* conc,
                                float* grad_logit_d /* the concrete layers' [h_l] in layer order */);

/* Layer-normalised hidden layers (models/core.py:56-58: torch.nn.LayerNorm(h_l) between fc_l and nonlin_l).  A hidden
 * layer l with gamma_d[l] != NULL computes, over its h_l true units (padding never enters the statistics),
 *   v = h_{l-1} W_l^T + b_l ;  mu_r = mean_j v[r][j] ;  var_r = mean_j (v[r][j] - mu_r)^2     (biased, two passes)
 *   zhat = (v - mu_r) / sqrt(var_r + eps_l) ;  y = gamma_l zhat + beta_l ;  h_l = act(y) * mask / keep
 * (a row of constant v gives 1 / sqrt(eps_l): finite), and the backward
 *   g_y = g_h act'(y) mask / keep ;  d beta = sum_r g_y ;  d gamma = sum_r g_y zhat ;  g_zhat = g_y gamma
 *   g_v = (g_zhat - mean_j g_zhat - zhat mean_j (g_zhat zhat)) / sqrt(var_r + eps_l)
 * A train-mode concrete layer's probabilities multiply a = act(y).  params_flat keeps its W, b layout; gamma and beta are
 * separate [h_l] vectors and their gradient comes back in grad_ln_d: per layer-norm layer [d gamma | d beta], in layer
 * order, OVERWRITTEN, formed like the bias gradient (per-workgroup slabs summed in slab order; no atomics: the same bits
 * call after call).  ln == NULL: no layer is normalised, and each call is the call it extends, bit for bit
 * (pmbrl_mlp_forward, pmbrl_mlp_grad_input, pmbrl_mlp_backward, or pmbrl_mlp_backward_concrete where conc != NULL).
 * Refused: a struct with no gamma_d at all (-2), gamma_d at an index that is no hidden layer (-2), beta_d missing (-1),
 * eps <= 0 (-2).
 * LDS: the forward needs no more than pmbrl_mlp_forward; the input gradient and the backward keep zhat, one more 16-row
 * buffer per layer-norm layer (1 / sqrt(var + eps) sits in its rows' spare columns).  Beyond 160 KB the workspace query
 * gives 0 and the call -3, both with "LDS" in the message.  With two hidden layers of 200 units (buffers of 16 x 216
 * floats, + 24 KB), the backward holds 5 buffers, + 2 with Tanh / SiLU / ..., + 1 per concrete layer, + 1 per layer-norm
 * layer:
 *   ReLU, 2 LN               7  121 344 B  fits        Tanh, 2 LN               9  148 992 B  fits
 *   ReLU, 2 LN + 1 concrete  8  135 168 B  fits        Tanh, 2 LN + 1 concrete 10  162 816 B  fits
 *   ReLU, 2 LN + 2 concrete  9  148 992 B  fits        Tanh, 2 LN + 2 concrete 11  176 640 B  refused
 *   Tanh, 1 LN + 2 concrete 10  162 816 B  fits        (160 KB = 163 840 B)
 * conc (pmbrl_mlp_backward_ln only) may be NULL; given, it is pmbrl_mlp_backward_concrete's and grad_logit_d is
 * required.  grad_ln_d may be NULL (not wanted). */
typedef struct {
  const float* gamma_d[PMBRL_MAX_LAYERS];  /* [h_l], NULL: hidden layer l has no layer norm */
  const float* beta_d[PMBRL_MAX_LAYERS];   /* [h_l] */
  float eps[PMBRL_MAX_LAYERS];             /* > 0 (torch's default: 1e-5) */
} pmbrl_mlp_layer_norm;
size_t pmbrl_mlp_ln_workspace_bytes(const pmbrl_mlp_call* call, const pmbrl_mlp_layer_norm* ln);
int pmbrl_mlp_forward_ln(void* stream, const pmbrl_mlp_call* call, void* workspace_d,
                         const float* x_d, const float* params_flat_d,
                         const uint16_t* const* mask_bits_d, const float* z_d,
                         const float* in_shift_d, const float* in_iscale_d,
                         const float* out_scale_d, const float* out_shift_d,
                         const float* sq_scale_d, const float* sq_bias_d,
                         float* sample_d, float* mean_d, float* log_std_d, const pmbrl_mlp_layer_norm* ln);
int pmbrl_mlp_grad_input_ln(void* stream, const pmbrl_mlp_call* call, void* workspace_d,
                            const float* x_d, const float* params_flat_d,
                            const uint16_t* const* mask_bits_d, const float* z_d,
                            const float* in_shift_d, const float* in_iscale_d,
                            const float* out_scale_d, const float* out_shift_d,
                            const float* sq_scale_d, const float* sq_bias_d,
                            const float* g_sample_d, const float* g_mean_d, const float* g_log_std_d,
                            float* grad_x_d, const pmbrl_mlp_layer_norm* ln);
size_t pmbrl_mlp_backward_ln_workspace_bytes(const pmbrl_mlp_call* call, const pmbrl_mlp_concrete* conc,
                                             const pmbrl_mlp_layer_norm* ln);
int pmbrl_mlp_backward_ln(void* stream, const pmbrl_mlp_call* call, void* workspace_d,
                          const float* x_d, const float* params_flat_d,
                          const uint16_t* const* mask_bits_d, const float* z_d,
                          const float* in_shift_d, const float* in_iscale_d,
                          const float* out_scale_d, const float* out_shift_d,
                          const float* sq_scale_d, const float* sq_bias_d,
                          const float* g_sample_d, const float* g_mean_d, const float* g_log_std_d,
                          float* grad_x_d /* [B][n_in] or NULL */,
                          float* grad_params_d /* flat, the layout of params_flat, or NULL */,
                          const pmbrl_mlp_concrete* conc /* or NULL */,
                          float* grad_logit_d /* the concrete layers' [h_l] in layer order (conc given) */,
                          const pmbrl_mlp_layer_norm* ln /* or NULL */,
                          float* grad_ln_d /* per layer-norm layer [d gamma | d beta] in layer order, or NULL */);

/* ---- BNN maximum-likelihood training of the dynamics model ---------------- */
/* Loss and gradient of one minibatch: the iteration body of the reference's
 * utils.train_regressor (utils/train_regressor.py:113-131) with the model in train() mode --
 * Regressor.forward(x, normalize=False, resample=True) (models/core.py:169-187), concrete
 * dropout with a straight-through Bernoulli sample (models/modules.py:102-118,120-160), Gaussian
 * log-likelihood (losses.py:16-37) and the dropout regulariser (models/modules.py:30-35,88-93,
 * 234-274):   loss = -mean_rows lml + reg_weight * reg / N.
 * Every hidden layer has a dropout kind: none, concrete (temperature[l] > 0) or fixed-rate
 * Bernoulli (drop_kind[l] = PMBRL_DROP_BERNOULLI; BDropout.forward, models/modules.py:46-61:
 * out = act(.) * m / p_j with m = (bvar < p_j); its regulariser on the Linear behind it is
 * reg_scale_l (sum_j p_j sum_o W[o, j]^2 + sum_o b[o]^2), models/modules.py:30-35).
 * params / grad are flat in the module's parameter order: W0, b0, [logit_p0], W1, b1, [logit_p1],
 * ..., W_L, b_L  (logit_p_l, one per unit of hidden layer l, present iff the layer is CONCRETE:
 * a Bernoulli layer has no parameter and no slot; pmbrl_bnn_plan_n_params counts accordingly).
 * u / bvar: the uniform noise of the concrete relaxation and the uniform variate of the Bernoulli
 * draw (hard = bvar < probs; Bernoulli layer: m = bvar < p_j), per dropout layer OF EITHER KIND a
 * block [M][h_l], blocks concatenated in layer order; a Bernoulli layer's u block is not read (u
 * may be NULL when no layer is concrete).  For plans whose dropout layers are all concrete both
 * layouts are what they were.  The optimiser step is pmbrl_clip_adam on the same flat vectors. */
#define PMBRL_DROP_BY_TEMPERATURE 0   /* none or concrete, as temperature[l] says */
#define PMBRL_DROP_BERNOULLI 1        /* fixed keep probability bern_keep[l] (or per unit, below) */
typedef struct {
  int32_t M;                  /* minibatch rows */
  int32_t N;                  /* dataset rows (the regulariser is divided by N) */
  pmbrl_mlp net;              /* dims[0] = input width, dims[n_layers] = 2 * output width; keep unused */
  float max_log_std;
  float temperature[PMBRL_MAX_LAYERS];   /* <= 0: hidden layer l has no dropout */
  float reg_scale[PMBRL_MAX_LAYERS];     /* CDropout.regularizer_scale buffer (= 0.5 * ctor argument) */
  float drop_reg[PMBRL_MAX_LAYERS];      /* CDropout.dropout_regularizer */
  float reg_weight;
  int32_t loss_kind;                     /* 0: Gaussian negative log-likelihood (losses.py:16-37);
                                          * 1: mean squared error of the mean head against the targets
                                          *    (the critic fit of examples/deep_pilco_no_mm_with_value.py:40-44;
                                          *    the log-std half of the head is ignored);
                                          * 2: negative log-likelihood of a mixture of diagonal Gaussians
                                          *    (losses.py:40-64 over models/densities.py:173-207,
                                          *    return_samples=False): net.dims[n_layers] =
                                          *    (2 n_out + 1) n_components + 1, see pmbrl_config.dyn_components */
  int32_t n_components;                  /* loss_kind 2 only */
  int32_t act;                           /* PMBRL_ACT_*: the hidden layers' activation */
  int32_t drop_kind[PMBRL_MAX_LAYERS];   /* PMBRL_DROP_*; zero: today's behaviour.  Any other value: -2 */
  float bern_keep[PMBRL_MAX_LAYERS];     /* Bernoulli layer l: keep probability p = 1 - rate in (0, 1], else -2;
                                          * its reg_scale[l] is BDropout.regularizer_scale, temperature / drop_reg unused */
} pmbrl_bnn_config;
typedef struct pmbrl_bnn_plan pmbrl_bnn_plan;

int pmbrl_bnn_plan_create(const pmbrl_bnn_config* cfg, int device, pmbrl_bnn_plan** out);
/* The kernel form of the step's forward + backward launch.  RESIDENT keeps every layer's values in LDS between the two
 * passes: pmbrl_bnn_plan_create, which returns -3 ("... LDS budget") beyond two hidden layers of 256 with ReLU.  SPILL keeps
 * one layer's working set in LDS and what the backward pass needs of the others in the workspace: any depth, activation
 * and mix of dropout kinds up to 688 units a layer (inputs and head included; -3 "... LDS ..." beyond), e.g. 3 x 512.
 * AUTO: RESIDENT where it fits, else SPILL.  Where both fit they return the same bits.  Any other value: -2.  Every call
 * that takes a pmbrl_bnn_plan serves both forms; a SPILL plan's workspace includes its stashes. */
#define PMBRL_BNN_FORM_RESIDENT 0
#define PMBRL_BNN_FORM_SPILL 1
#define PMBRL_BNN_FORM_AUTO 2
int pmbrl_bnn_plan_create_form(const pmbrl_bnn_config* cfg, int device, int32_t form, pmbrl_bnn_plan** out);
int32_t pmbrl_bnn_plan_form(const pmbrl_bnn_plan* plan);      /* the form the plan took (RESIDENT or SPILL) */
void pmbrl_bnn_plan_destroy(pmbrl_bnn_plan* plan);
/* Per-unit keep probabilities of Bernoulli layer `layer` (BDropout with a tensor rate): keep_h, n host values in
 * (0, 1], copied into memory the plan owns (the call waits for the device).  n must be the layer's width; a layer
 * that is not Bernoulli, a wrong n or a value out of range return -2.  Unlike the rollout plans, which fold 1 / p_j
 * into ReLU weights, the step divides per unit: every activation is served. */
int pmbrl_bnn_plan_set_unit_keep(pmbrl_bnn_plan* plan, int32_t layer, const float* keep_h, int32_t n);
size_t pmbrl_bnn_plan_workspace_bytes(const pmbrl_bnn_plan* plan);
int64_t pmbrl_bnn_plan_n_params(const pmbrl_bnn_plan* plan);
int pmbrl_bnn_loss_grad(pmbrl_bnn_plan* plan, void* stream, void* workspace_d,
                        const float* Xn_d /* [N][n_in] */, const float* Yn_d /* [N][n_out] */,
                        const int32_t* idx_d /* [M] */, const float* params_flat_d,
                        const float* u_d, const float* bvar_d,
                        float* grad_flat_d, float* loss_out_d /* [3]: loss, -E[lml], reg */);

/* The same step with the options of utils/train_regressor.py:113-147:
 *  - row_weight_d [M] (optional): importance-sampling weight of every minibatch
 *    row's log-likelihood (prioritized_sampling, :117-131);
 *  - row_logprob_d [M] (optional, out): the rows' unweighted log-likelihoods,
 *    from which the caller updates its priorities;
 *  - terms: 1 = likelihood only, 2 = regulariser only (its gradient alone, for
 *    the separate SGD step of decoupled_reg, :133-147), 3 = both. */
int pmbrl_bnn_loss_grad_ex(pmbrl_bnn_plan* plan, void* stream, void* workspace_d,
                           const float* Xn_d, const float* Yn_d, const int32_t* idx_d,
                           const float* params_flat_d, const float* u_d, const float* bvar_d,
                           float* grad_flat_d, float* loss_out_d,
                           const float* row_weight_d, float* row_logprob_d, int32_t terms);

/* Whole training iterations of utils/train_regressor.py:113-131 (loss_kind 0: Gaussian likelihood + regulariser, then
 * torch.optim.Adam's step -- the reference clips nothing here) queued by ONE call, two launches an iteration:
 * forward + backward over the minibatch, then dW / db / regulariser / Adam / re-packed weights / loss in one kernel.
 * Minibatch i = rows idx_all_d[i * M .. (i + 1) * M).  Dropout noise: recorded draws u_d / bvar_d
 * ([n_steps][M * sum_h], the layout of pmbrl_bnn_loss_grad, sum_h over the dropout layers of either kind) or, when
 * both are null, drawn inside the kernel (Philox keyed by `seed`, counter = (row, unit, layer, first_step + i); a
 * Bernoulli layer draws its variate from the same stream).  exp_avg / exp_avg_sq / step_d: Adam's state (the
 * device-side step counter is advanced by every iteration).  loss_out_d [3]: the last iteration's loss, -E[lml],
 * reg; loss_hist_d (optional) [n_steps][3]: every iteration's.  Replaces eight launches and two torch.rand calls per
 * iteration (train_regressor.py:58-165 runs 2 000 of them per policy-search round). */
int pmbrl_bnn_train_steps(pmbrl_bnn_plan* plan, void* stream, void* workspace_d, const float* Xn_d, const float* Yn_d,
                          const int32_t* idx_all_d, int32_t n_steps, float* params_flat_d, float* exp_avg_d,
                          float* exp_avg_sq_d, int64_t* step_d, double lr, double beta1, double beta2, double eps,
                          uint64_t seed, uint64_t first_step, const float* u_d, const float* bvar_d,
                          float* loss_out_d, float* loss_hist_d);
/* An optimiser rule (pmbrl_opt_rule above) for pmbrl_bnn_train_steps: copied into the plan, NULL detaches it.  While one
 * is attached the step of every iteration is the rule's (no clipping: coef = 1) and lr / beta1 / beta2 / eps of the call
 * are ignored; the fragments the tail re-packs are the decayed, updated weights.  The flat layout is W0, b0, [logit_p0],
 * W1, ...: every one of these tensors must lie in ONE segment (-2 otherwise). */
int pmbrl_bnn_plan_set_optimizer(pmbrl_bnn_plan* plan, const pmbrl_opt_rule* rule);

/* ---- test hooks (used by tests/ only) ---------------------------------- */
/* y[R,O] = x[R,K] W[O,K]^T + b through the same MFMA tile routine the rollout
 * kernels use (R <= 64). */
int pmbrl_debug_linear(void* stream, const float* x_d, const float* W_d,
                       const float* b_d, int32_t R, int32_t K, int32_t O,
                       int32_t transpose_w, float* y_d, float* scratch_d);

#ifdef __cplusplus
}
#endif
#endif /* PMBRL_H */
