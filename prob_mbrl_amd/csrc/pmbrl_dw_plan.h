// The plan of the policy-gradient dW GEMM: ONE record (DwPlan, pmbrl_plan::dw) for everything a rollout plan decides about
// it, and the planner that fills it.  Host code only, no HIP call, no allocation, no environment read: pm_dw_plan is pure
// arithmetic on the network shape, the layout, the CU count and the switches, so that tests/dw_plan_check.cpp checks its
// rules with the host compiler alone.  pmbrl_dw.hip turns the record into device tables, a stream and events
// (pm_dw_plan_create / pm_dw_plan_destroy) and launches from it (pm_dw_launch); DESIGN.md, "the dW plan", has the forms
// and their precedence.
#pragma once
#include <algorithm>
#include <cassert>
#include <utility>
#include <vector>

#include "pmbrl_dw.h"

// the handles the record owns, as the HIP runtime's header declares them (it is not included: host compiler alone)
typedef struct ihipStream_t* hipStream_t;
typedef struct ihipEvent_t* hipEvent_t;

#define PM_PIPE_MAX 8
#define PM_REG_DW_LAYER 1      // the policy layer whose delta the register-resident adjoint does not stash: the second hidden one (200 x 200)

// The dW switches of a rollout plan (include/pmbrl.h lists them; PlanSwitches, pmbrl_host.h, holds them with the others)
struct DwSwitches {
  bool dw_no_wide;                    // PMBRL_DW_NO_WIDE set at all
  bool dw_pipe_off, dw_pipe_ranges;   // PMBRL_DW_PIPE=off | n0,n1,... (the positive ones in dw_pipe)
  std::vector<int> dw_pipe;
  int dw_head;                        // PMBRL_DW_HEAD=on | off: the policy head's dW in the streamed consumers (-1: the plan's rule)
  bool dw_stream_off, dw_stream_set;  // PMBRL_DW_STREAM=off | <steps streamed>[,<consumer workgroups>]
  int dw_stream_steps, dw_stream_wgs; // (wgs 0: the plan's)
};

// What the planner reads of a rollout plan
struct DwShape {
  int nl, nt[PM_MAXL + 1], dim[PM_MAXL + 1];      // the policy
  int w_off[PM_MAXL], b_off[PM_MAXL], n_params;
  int dyn_n_params;
  int prec, RT, fast, inplace, nwg, H, U, cus;    // the layout, the horizon, the action width, the device's CUs
  bool whole;                                     // the sweeps go out as SweepForm::Whole
  int mm_parts, reg, reg_mm;
  bool reg_bwd;                                   // PlanSwitches::reg_bwd
  DwSwitches sw;
};

// the kernels of pmbrl_dw_kernels.h a launch can go to, resolved per table / layer when the plan is made
enum class DwKernel : int {
  None,
  Block, BlockSplit,        // pm_dw_kernel / pm_dw_kernel_s: the wave-block table in exact fp32 / on split bf16 operands
  BlockRing,                // pm_dw_kernel_nh: the table without the head, every block at most 2 x 1 tiles, a deeper ring
  NarrowPre1, NarrowPre2,   // pm_dw_narrow_pre_kernel<1> / <2>: a layer narrow on one side (one / two tiles), pre-split stashes
  Wide, WidePre,            // pm_dw_wide_kernel / pm_dw_wide_pre_kernel: 128 x 128 units / 256 x 256 units over pre-split stashes
  Layer                     // pm_dw_layer_kernel and its rebuilding forms: a whole layer of at most 13 x 13 tiles per workgroup
};

struct DwPlan {
  // The plan's part of the GEMM's argument record: shape, chunk deal, split_prec, the block table with the head (blocks,
  // wave_first).  A call copies it and adds its own (pm_dw_call_args).  Nothing in it is repeated below.
  DwArgs args;
  // Block tables, with the head (args) and without it (where the streamed consumers form it); skip: the layers NOT in them
  std::vector<DwBlock> blocks, blocks_nh;
  bool skip[PM_MAXL];
  DwBlock* blocks_nh_d;
  int wave_first_nh[PM_DW_NW + 1], nh_ring;      // nh_ring: every block of the table without the head is at most 2 x 1 tiles
  DwKernel table_k, table_nh_k;                  // which kernel walks each
  // Wide and pre-split units: output tiles of the wide layers, 128 x 128 (Wide) or 256 x 256 over pre-split stashes (WidePre)
  std::vector<DwUnit> units;
  DwUnit* units_d;
  DwKernel unit_k;
  int narrow[PM_MAXL];          // 1: first-layer type (delta stash 512 wide), 2: head type (input stash 512 wide): NarrowPre*
  unsigned pre_mask;            // layers whose dW GEMM reads pre-split stashes (WidePre; the wide sweeps write them)
  DwKernel layer_k[PM_MAXL];    // per layer, what serves it (a block-kernel layer: the table's kernel)
  int layer13;                  // >= 0: this layer (at most 13 x 13 tiles) runs whole in one workgroup per row-step range (Layer)
  // Pipelined form, the dW GEMM behind the adjoint sweep (pmbrl_rollout_bwd): the sweep as pipe_K launches over descending
  // step ranges [pipe_lo[k], pipe_lo[k-1]); the GEMM of range k runs on pipe_stream, on the CUs the sweep leaves idle,
  // while the sweep is in range k+1.  pipe_K <= 1: off.
  int pipe_K, pipe_lo[PM_PIPE_MAX], pipe_rows, pipe_grid;
  hipStream_t pipe_stream;      // (the streamed form's too)
  hipEvent_t pipe_ev[PM_PIPE_MAX];
  // Streamed form, the second hidden layer's dW GEMM BESIDE the one-launch adjoint sweep (DwArgs::st_on): st_wgs consumer
  // workgroups on pipe_stream follow the sweep over the steps [st_cut, H) through the head gradients it publishes
  // (off_pub: tagged granules, pub_gen their launch generation), the steps below the cut follow the sweep as before;
  // st_head: with the policy head's dW / db formed by the consumers too, the block kernel of such a call walks blocks_nh
  int st_on, st_cut, st_wgs, st_head;
  size_t off_pub, pub_bytes;
  const void* pub_ws;           // the workspace whose granules hold no tag a later launch could take for its own (xch_prepare's rule)
  mutable unsigned pub_gen;
  // Partial rows [part_rows][args.part_stride] in the workspace: the most any form writes
  int part_rows;
  size_t off_part;
  int n_blocks() const { return args.wave_first[PM_DW_NW]; }
};

// the CUs a one-launch sweep of nwg workgroups leaves idle: workgroups go round-robin to the 8 XCDs, so per XCD
// CUs / 8 - ceil(nwg / 8) are free
static inline int pm_dw_idle_cus(int cus, int nwg) { return cus >= 64 && cus % 8 == 0 ? 8 * (cus / 8 - (nwg + 7) / 8) : 0; }

// dW wave blocks: balanced splits of every layer's output tile grid into <= 4 x 7 tile
// blocks, dealt to the four SIMDs (waves w and w+4 share SIMD w) by decreasing size so that
// every SIMD issues the same number of MFMAs.  Returns the number of blocks; `blocks` comes back
// sorted by wave, wave w owning [wave_first[w], wave_first[w+1]).
// (ot_parts_min: a layer's output tiles in at least this many parts where it has as many -- the table without the policy
//  head, pm_dw_kernel_nh, has one layer left and wants a block on every wave)
inline int build_dw_blocks(int nl, const int* nt, std::vector<DwBlock>& blocks, int* wave_first, int tn_max = PM_DW_TN,
                           const bool* skip = nullptr, int ot_parts_min = 1) {
  blocks.clear();
  auto split = [](int n, int maxsz, std::vector<std::pair<int, int>>& out, int parts_min = 1) {
    const int parts = std::max((n + maxsz - 1) / maxsz, std::min(n, parts_min));
    int lo = 0;
    for (int i = 0; i < parts; ++i) {
      const int sz = n / parts + (i < n % parts ? 1 : 0);
      out.push_back({lo, sz});
      lo += sz;
    }
  };
  for (int l = 0; l < nl; ++l) {
    if (skip && skip[l]) continue;      // a wide layer: pm_dw_wide_kernel
    std::vector<std::pair<int, int>> os, is;
    split(nt[l + 1], PM_DW_TM, os, ot_parts_min);
    split(nt[l], tn_max, is);
    for (auto& o : os)
      for (auto& i : is)      // (layer, ot0, it0, n_ot, n_it, pad)
        blocks.push_back(DwBlock{(int16_t)l, (int16_t)o.first, (int16_t)i.first, (int16_t)o.second, (int16_t)i.second, 0});
  }
  const int n_blocks = (int)blocks.size();
  // cost of a block = MFMAs per chunk in the shape class it runs in (see pm_dw_kernel)
  auto cost = [tn_max](const DwBlock& b) {
    const int ni = b.n_ot <= 1 ? 1 : (b.n_ot <= 3 ? 3 : 4);
    const int nj = b.n_it <= 1 ? 1 : (b.n_it <= 4 ? 4 : (b.n_it <= 6 ? 6 : 7));
    return ni * (tn_max <= 4 && nj > 1 ? 4 : nj);
  };
  std::stable_sort(blocks.begin(), blocks.end(),
                   [&](const DwBlock& a, const DwBlock& b) { return cost(a) > cost(b); });
  std::vector<DwBlock> per_wave[PM_DW_NW];
  long wave_load[PM_DW_NW] = {0};
  // waves w and w+4 of a workgroup share SIMD w (measured: pairing (2k, 2k+1) instead is 5% slower)
  for (const DwBlock& b : blocks) {
    int best_simd = 0;
    for (int sm = 1; sm < 4; ++sm)
      if (wave_load[sm] + wave_load[sm + 4] < wave_load[best_simd] + wave_load[best_simd + 4]) best_simd = sm;
    const int w = wave_load[best_simd] <= wave_load[best_simd + 4] ? best_simd : best_simd + 4;
    per_wave[w].push_back(b);
    wave_load[w] += cost(b);
  }
  blocks.clear();
  // the small blocks are latency-bound (a handful of MFMAs per chunk): the second wave of a SIMD runs
  // its FIRST, while the SIMD's other wave keeps the MFMA pipe busy with its big block
  for (int w = 0; w < PM_DW_NW; ++w) {
    wave_first[w] = (int)blocks.size();
    if (w >= 4) std::reverse(per_wave[w].begin(), per_wave[w].end());
    for (const DwBlock& b : per_wave[w]) blocks.push_back(b);
  }
  wave_first[PM_DW_NW] = (int)blocks.size();
  return n_blocks;
}

// stage 1 of the planner: wave blocks of the block kernels, tile units of the wide layers, chunks
inline void pm_dw_plan_blocks(const DwShape& S, DwPlan& P) {
  DwArgs& W = P.args;
  // split-operand form of the dW GEMM (pmbrl_dw_kernels.h, pm_dw_kernel_s): where the fp32 form is bound by the matrix
  // core -- 32- / 64-row workgroups and the general family's wide networks; the 16-row sweeps' dW is HBM-bound
  W.split_prec = S.prec != 0 && (S.RT >= 2 || !S.fast);
  // wide layers of the split form go to the LDS-staged tile kernel (pmbrl_dw_kernels.h, pm_dw_wide_kernel)
  bool* wide = P.skip;
  std::vector<DwUnit>& units = P.units;
  // (layers of at least 128 x 128 on the split-precision plans: also the 200 x 200 layer of the cart-pole shapes,
  //  whose block-kernel GEMM re-read its stash 1.5 x -- C2 0.116 -> 0.102 ms, C4 0.50 -> 0.38 ms; the exact-fp32
  //  plans keep the fp32 block kernel for every layer)
  P.layer13 = -1;
  if (S.prec != 0 && !S.sw.dw_no_wide)
    for (int l = 0; l < S.nl; ++l)
      if (S.nt[l + 1] * 16 >= 128 && S.nt[l] * 16 >= 128) {
        wide[l] = true;
        if (P.layer13 < 0 && S.nt[l + 1] <= PM_DWL_NT && S.nt[l] <= PM_DWL_NT) {
          // a whole layer of up to 13 x 13 tiles per workgroup
          P.layer13 = l;
          continue;
        }
        for (int m0 = 0; m0 < S.nt[l + 1] * 16; m0 += PM_DWW_TM)
          for (int n0 = 0; n0 < S.nt[l] * 16; n0 += PM_DWW_TN) units.push_back(DwUnit{(int16_t)l, (int16_t)m0, (int16_t)n0, 0});
      }
  P.unit_k = units.empty() ? DwKernel::None : DwKernel::Wide;
  // Round 6: the wide sweeps (64-row workgroups, in-place 512-wide layers: pmbrl_wide.h) write the stashes of the 512 x 512
  // layers PRE-SPLIT, in the layout pm_dw_wide_pre_kernel streams into LDS without touching a register (pmbrl_dw_kernels.h).
  // Every wide layer 512 x 512 exactly (32 tiles: the stash block's tile count).  (Such a plan has split_prec: the
  // pre-split kernels walk chunk pairs.)
  if (!units.empty() && S.inplace == 2 && S.RT == 4) {
    bool all = true;
    for (const DwUnit& u : units) all = all && S.nt[u.layer] == 32 && S.nt[u.layer + 1] == 32 &&
                                        S.dim[u.layer] == 512 && S.dim[u.layer + 1] == 512;
    // ... and every OTHER layer narrow on one side, 512 wide on the other (first layer: <= 32 inputs; head: <= 32 outputs):
    // pm_dw_narrow_pre_kernel -- so that EVERY 512-wide stash is pre-split and the sweeps carry one form of stash store
    for (int l = 0; l < S.nl && all; ++l) {
      bool is = false;
      for (const DwUnit& u : units) is = is || u.layer == l;
      P.narrow[l] = 0;
      if (is) continue;
      if (S.nt[l + 1] == 32 && S.dim[l + 1] == 512 && S.nt[l] <= 2) P.narrow[l] = 1;
      else if (S.nt[l] == 32 && S.dim[l] == 512 && S.nt[l + 1] <= 2) P.narrow[l] = 2;
      else all = false;
    }
    if (all) {
      std::vector<DwUnit> pre;
      for (int l = 0; l < S.nl; ++l) {
        if (P.narrow[l]) { wide[l] = true; continue; }      // (not the block kernels': skipped by build_dw_blocks)
        P.pre_mask |= 1u << l;
        for (int m0 = 0; m0 < 512; m0 += PM_DWP_TM)
          for (int n0 = 0; n0 < 512; n0 += PM_DWP_TN) pre.push_back(DwUnit{(int16_t)l, (int16_t)m0, (int16_t)n0, 0});
      }
      units = pre;
      P.unit_k = DwKernel::WidePre;
      assert(W.split_prec);
    } else {
      for (int l = 0; l < PM_MAXL; ++l) P.narrow[l] = 0;
    }
  }
  build_dw_blocks(S.nl, S.nt, P.blocks, W.wave_first, W.split_prec ? PM_DW_TN_S : PM_DW_TN, wide);
  P.table_k = P.blocks.empty() ? DwKernel::None : (W.split_prec ? DwKernel::BlockSplit : DwKernel::Block);
  // which kernel serves each layer: the narrow side of a narrow layer is the input of the first-layer type, the output of
  // the head type -- one tile or two
  for (int l = 0; l < S.nl; ++l) {
    const int nt_n = P.narrow[l] == 1 ? S.nt[l] : S.nt[l + 1];
    P.layer_k[l] = P.narrow[l]      ? (nt_n <= 1 ? DwKernel::NarrowPre1 : DwKernel::NarrowPre2)
                   : l == P.layer13 ? DwKernel::Layer
                   : wide[l]        ? P.unit_k
                                    : P.table_k;
  }
  W.n_chunks = S.H * S.nwg * S.RT;
  int nsplit = std::min(256, W.n_chunks);   // one 8-wave workgroup per CU
  W.chunks_per_split = (W.n_chunks + nsplit - 1) / nsplit;
  if (W.split_prec) W.chunks_per_split = (W.chunks_per_split + 1) & ~1;   // whole chunk pairs
  W.nsplit = (W.n_chunks + W.chunks_per_split - 1) / W.chunks_per_split;
  // the rest of what the GEMM's argument record holds of the plan
  W.nl = S.nl;
  W.RT = S.RT;
  W.Rw = 16 * S.RT;
  W.n_params = S.n_params;
  W.part_stride = (W.n_params + 3) / 4 * 4;
  for (int i = 0; i <= S.nl; ++i) { W.dim[i] = S.dim[i]; W.nt[i] = S.nt[i]; }
  for (int l = 0; l < S.nl; ++l) { W.w_off[l] = S.w_off[l]; W.b_off[l] = S.b_off[l]; }
  W.chunks_per_step = S.nwg * S.RT;
}

// stage 2: dW GEMM behind the adjoint sweep.  The sweep is latency-bound and holds nwg CUs completely (its
// workgroups take a CU's whole register file); with fewer workgroups than CUs the rest of the chip idles
// for its duration, and the dW GEMM -- 12-17 % of an iteration -- used to start when the sweep had
// finished.  It needs only the deltas of the steps already swept: the sweep becomes pipe_K launches
// over descending step ranges (the state gradient is carried through HBM, as in the per-step launch
// modes) and the GEMM of range k runs next to the sweep of range k+1, on a second stream, in a grid that
// fits the idle CUs (pm_dw_idle_cus) with workgroups that cannot share a CU with the sweep's.  Only the last,
// short range is exposed.
// Correctness never depends on the overlap: every dependency is a stream event.
// (The pipelined ranges never meet a plan without block-kernel layers or with pre-split stashes: such a plan has
//  pre_mask -- the first layer's input is at most 40 wide, so only pm_dw_narrow_pre_kernel takes it from the block
//  kernel -- and the pipeline stays off for it.)
inline void pm_dw_plan_pipe(const DwShape& S, DwPlan& P, int n_free) {
  const DwSwitches& sw = S.sw;
  const int H = S.H, cus = S.cus;
  P.pipe_K = 1;
  const bool no_pipe_pre = P.pre_mask != 0;      // (the pre-split GEMMs run once, behind the whole sweep)
  const bool single = S.whole && S.mm_parts <= 1;   // (no second kernel next to flag barriers)
  // Worth it where a range of the sweep is long against a launch boundary (tail of the last step, launch
  // gap, the next launch's prologue: 15 us at 16 rows per workgroup, 40 us at 64) -- measured: the double
  // cart-pole shape (64-row workgroups, 30 us per step) gains 7 % of an iteration, the cart-pole shapes
  // (6 / 13 us per step) lose 1-5 %.  Proxy for the step time: rows per workgroup x weights of both nets.
  const bool long_steps = (long long)S.RT * (long long)(S.n_params + S.dyn_n_params) >= 256 * 1024 && H >= 16;
  if (!single || no_pipe_pre || n_free < cus / 8 || H < 2 || sw.dw_pipe_off || !(long_steps || sw.dw_pipe_ranges))
    return;
  std::vector<int> cnt;
  if (sw.dw_pipe_ranges) {     // PMBRL_DW_PIPE=n0,n1,...: steps per range, highest steps first (tests, tuning)
    cnt = sw.dw_pipe;
    int sum = 0;
    for (int v : cnt) sum += v;
    if (sum != H || (int)cnt.size() > PM_PIPE_MAX) cnt.clear();
  }
  if (cnt.empty() && long_steps) {
    // 40 / 30 / 20 / 10 % of the horizon: the exposed tail is the GEMM of the last tenth
    const int a3 = std::max(2, H / 10), a2 = a3 + std::max(2, H / 5), a1 = a2 + std::max(2, (3 * H) / 10);
    cnt = {H - a1, a1 - a2, a2 - a3, a3};
  }
  // lower step bound of every range (the last one ends at step 0; ranges emptied by the adjustment are dropped)
  int K = 0, lo = H;
  for (size_t k = 0; k < cnt.size() && lo > 0; ++k) {
    lo = k + 1 == cnt.size() ? 0 : std::max(0, lo - cnt[k]);
    // split-operand GEMM: a K = 32 chunk pair must not straddle two launches
    if (P.args.split_prec && ((S.nwg * S.RT) & 1) && (lo & 1)) lo -= 1;
    if (K > 0 && lo >= P.pipe_lo[K - 1]) continue;
    P.pipe_lo[K++] = lo;
  }
  if (K >= 2 && P.pipe_lo[K - 1] == 0) {
    P.pipe_K = K;
    P.pipe_grid = n_free;                     // workgroups (= partial rows) of a GEMM launch next to the sweep
    P.pipe_rows = std::max(n_free, cus);      // ... of the last launch, which has the chip to itself
  }
}

// stage 3: the second hidden layer's dW GEMM BESIDE the adjoint sweep (the streamed form).  Cutting the sweep into ranges
// (above) costs ~15 us a cut at the cart-pole shapes, more than it hides.  Behind a register-resident adjoint sweep the
// layer's kernel REBUILDS its delta operand from the forward sweep's stashes and the policy head's gradient -- 2 U floats a
// row, the only input the adjoint sweep produces.  So the sweep stays ONE launch and publishes that gradient step by step
// (tagged granules, RegArgs::pub); st_wgs consumer workgroups (pm_dw_layer_st_kernel), one per CU the sweep leaves idle,
// launched on the second stream next to it, follow it down the steps [st_cut, H); the steps below the cut go to the
// layer's kernel behind the sweep, over the whole chip, which adds to the consumers' partial rows.  The sweep waits for
// nothing; the consumers wait (bounded) for sweep workgroups only and are fewer than the CUs the sweep leaves: serialised
// in submission order the form is merely not faster.
//   PMBRL_DW_STREAM=off | <steps streamed>[,<consumer workgroups>] (the second: any plan that meets the first four
//   conditions -- tests, tuning)
inline void pm_dw_plan_stream(const DwShape& S, DwPlan& P, int n_free) {
  const DwSwitches& sw = S.sw;
  const int H = S.H, cus = S.cus;
  P.st_on = 0;
  // the plain register-resident instance serves the adjoint in one launch, and its dW GEMM rebuilds the delta
  const bool fam = S.reg && !S.reg_mm && S.reg_bwd && P.layer13 == PM_REG_DW_LAYER && S.RT == 1;
  const bool single = S.whole && S.mm_parts <= 1 && P.pipe_K <= 1;
  if (!fam || !single || n_free < 1 || n_free < cus / 8 || sw.dw_stream_off || H >= 4095) return;
  // Large enough to hide something: every consumer gets at least a chunk of every sweep step (fewer, and it runs single
  // chunks on half-empty K = 32 MFMAs or idles), and the layer's GEMM over the whole chip -- ~3.5 us per chunk pair and
  // workgroup -- is worth more than what the form adds behind the sweep (the consumers' write-out and a launch, ~12 us):
  // H nwg / (2 cus) pairs x 3.5 us >= 2 x 12 us
  const bool large = S.nwg >= n_free && (long long)H * S.nwg >= 14ll * cus;
  if (!large && !sw.dw_stream_set) return;
  // The cut.  A consumer's share of a sweep step is ceil(nwg / n_free) chunks, taken in pairs.  With at most one pair a
  // step -- nwg <= 2 n_free -- the consumers wait for the sweep at every step (2 us of work against a 4 us step at the
  // cart-pole shape) and finish a write-out behind it, hidden behind the block kernel: EVERY step is streamed and no
  // launch of the layer's kernel follows.  (Measured, DESIGN_LOG.md "dW beside the sweep": 40 of 40 steps 410 us an
  // iteration, 38: 426, 35: 428, 30: 432, 20: 442, off: 430 -- a launch behind the sweep costs ~25 us before its first
  // chunk; 64 consumers with two pairs a step fall behind: 494 us.)  More than a pair: the consumers do the share they can
  // keep up with, the highest steps, and the launch behind the sweep takes the rest
  int steps = S.nwg <= 2 * n_free ? H : (int)((long long)H * 2 * n_free / S.nwg);
  int wgs = n_free;
  if (sw.dw_stream_set) {
    steps = sw.dw_stream_steps;
    if (sw.dw_stream_wgs > 0) wgs = std::min(wgs, sw.dw_stream_wgs);
  }
  steps = std::max(0, std::min(H, steps));
  P.st_on = 1;
  P.st_cut = H - steps;
  P.st_wgs = wgs;
}

// stage 4: ... and the policy HEAD's dW / db with it.  The head's only adjoint-side input is the head gradient -- what the
// consumers receive anyway -- and its other operand, actT of the head, is the forward sweep's: the consumers form the head's
// gradient beside the sweep too (pm_dw_layer_body, PmDwHead) and half of the block kernel's bytes leave the critical path.
// Where every step is streamed (no launch behind the sweep shares the consumers' rows) and the form was not forced through
// PMBRL_DW_STREAM=<steps>, which keeps its meaning: the head in the block kernel.  PMBRL_DW_HEAD=on | off forces it where
// every step is streamed / never.  The block kernel of such a call walks a table without the head, built here.
inline void pm_dw_plan_head(const DwShape& S, DwPlan& P) {
  const DwSwitches& sw = S.sw;
  const DwArgs& W = P.args;
  const int l = P.layer13, h = l + 1;
  P.st_head = 0;
  if (!P.st_on || P.st_cut != 0 || sw.dw_head == 0 || (sw.dw_head < 0 && sw.dw_stream_set)) return;
  // the head is the last layer, one tile of outputs, a block-kernel layer of the fp32 form; the columns W_l, b_l, W_h, b_h are
  // one contiguous range of the flat vector (what the reduction reads of the consumers' rows only)
  if (h != S.nl - 1 || S.nt[h + 1] != 1 || S.dim[h + 1] > 16 || P.skip[h] || W.split_prec) return;
  if (W.b_off[l] != W.w_off[l] + W.dim[l + 1] * W.dim[l] || W.w_off[h] != W.b_off[l] + W.dim[l + 1] ||
      W.b_off[h] != W.w_off[h] + W.dim[h + 1] * W.dim[h])
    return;
  bool skip[PM_MAXL];
  for (int i = 0; i < PM_MAXL; ++i) skip[i] = P.skip[i] || i == h;
  build_dw_blocks(S.nl, S.nt, P.blocks_nh, P.wave_first_nh, PM_DW_TN, skip, PM_DW_NW);
  // (pm_dw_kernel_nh, the deeper ring: every block at most 2 x 1 tiles; else the block kernel as it is, on this table)
  P.nh_ring = 1;
  for (const DwBlock& b : P.blocks_nh) P.nh_ring = P.nh_ring && b.n_ot <= 2 && b.n_it <= 1;
  P.table_nh_k = P.blocks_nh.empty() ? DwKernel::None : (P.nh_ring ? DwKernel::BlockRing : DwKernel::Block);
  P.st_head = 1;
  assert(P.pipe_K <= 1);      // (pm_dw_kernel_nh has no branch for a row of zeros: only a piped range asks for one)
}

// Everything a rollout plan decides about its dW GEMM, in the order of precedence: blocks / wide units / whole layer /
// pre-split, then the pipelined form, then -- only where that stayed off -- the streamed form, then the head in its
// consumers.  The device tables, the stream and the events are pm_dw_plan_create's (pmbrl_dw.hip); off_part / off_pub
// the workspace carve-up's.
inline void pm_dw_plan(const DwShape& S, DwPlan& P) {
  P = DwPlan();
  const int n_free = pm_dw_idle_cus(S.cus, S.nwg);
  pm_dw_plan_blocks(S, P);
  pm_dw_plan_pipe(S, P, n_free);
  pm_dw_plan_stream(S, P, n_free);
  pm_dw_plan_head(S, P);
  P.part_rows = std::max(P.args.nsplit, P.pipe_K > 1 ? P.pipe_rows : 0);
  // the policy head's gradient as the adjoint sweep publishes it for the streamed dW GEMM: [H][nwg][2 U][16] granules
  P.pub_bytes = P.st_on ? (size_t)S.H * S.nwg * 2 * S.U * 16 * sizeof(unsigned long long) : 0;
}
