// Host-only check of the dW GEMM's planner (prob_mbrl_amd/csrc/pmbrl_dw_plan.h); compiled and run by tests/test_dw_plan.py.
// One smallest shape per form the planner can choose, at 256 CUs.  Every expected value is worked out by hand from the
// rule it follows (written next to it), none is taken from the planner.  Prints one line per failed check and returns how
// many failed.
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "pmbrl_dw_plan.h"

static int failed = 0;
static const char* now = "";
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { ++failed; printf("FAILED [%s] %s (line %d)\n", now, #cond, __LINE__); } \
  } while (0)

// a plan's inputs: the policy's widths (parameters laid out W0 b0 W1 b1 ..., as plan_nets does), everything else at the
// values of a plain one-launch plan without the register-resident family and without switches
static DwShape shape(std::initializer_list<int> dims, int prec, int RT, int fast, int nwg, int H) {
  DwShape S{};
  S.nl = (int)dims.size() - 1;
  int i = 0, off = 0;
  for (int d : dims) { S.dim[i] = d; S.nt[i] = (d + 15) / 16; ++i; }
  for (int l = 0; l < S.nl; ++l) {
    S.w_off[l] = off; off += S.dim[l + 1] * S.dim[l];
    S.b_off[l] = off; off += S.dim[l + 1];
  }
  S.n_params = off;
  S.dyn_n_params = 43008;
  S.prec = prec; S.RT = RT; S.fast = fast; S.inplace = 0; S.nwg = nwg; S.H = H; S.U = 1; S.cus = 256;
  S.whole = true; S.mm_parts = 1; S.reg = 0; S.reg_mm = 0; S.reg_bwd = true;
  S.sw.dw_head = -1;
  return S;
}
static void pipe_ranges(DwShape& S, std::initializer_list<int> r) { S.sw.dw_pipe_ranges = true; S.sw.dw_pipe = r; }
// the register-resident family serves the plan (the 4-200-200-2 policy at 16 rows per workgroup, fp16 pieces)
static DwShape reg_shape(int nwg, int H) {
  DwShape S = shape({4, 200, 200, 2}, PMBRL_PREC_SPLIT_F16, 1, 1, nwg, H);
  S.reg = 1;
  return S;
}

// what build_dw_blocks guarantees of a table: every (layer, output tile, input tile) of a layer that is not skipped in
// exactly one block, none of a skipped one; wave_first non-decreasing from 0 to the block count; no block beyond 4 x tn_max
static void table_ok(const DwShape& S, const std::vector<DwBlock>& blocks, const int* wave_first, const bool* skip, int tn_max) {
  for (int l = 0; l < S.nl; ++l) {
    std::vector<int> seen((size_t)S.nt[l + 1] * S.nt[l], 0);
    for (const DwBlock& b : blocks) {
      if (b.layer != l) continue;
      CHECK(b.n_ot >= 1 && b.n_ot <= PM_DW_TM && b.n_it >= 1 && b.n_it <= tn_max);
      CHECK(b.ot0 >= 0 && b.ot0 + b.n_ot <= S.nt[l + 1] && b.it0 >= 0 && b.it0 + b.n_it <= S.nt[l]);
      for (int o = b.ot0; o < b.ot0 + b.n_ot && o < S.nt[l + 1]; ++o)
        for (int i = b.it0; i < b.it0 + b.n_it && i < S.nt[l]; ++i) ++seen[(size_t)o * S.nt[l] + i];
    }
    for (int v : seen) CHECK(v == (skip[l] ? 0 : 1));
  }
  for (const DwBlock& b : blocks) CHECK(b.layer >= 0 && b.layer < S.nl);
  CHECK(wave_first[0] == 0 && wave_first[PM_DW_NW] == (int)blocks.size());
  for (int w = 0; w < PM_DW_NW; ++w) CHECK(wave_first[w] <= wave_first[w + 1]);
}
static DwPlan plan(const char* name, const DwShape& S) {
  now = name;
  DwPlan P;
  pm_dw_plan(S, P);
  table_ok(S, P.blocks, P.args.wave_first, P.skip, P.args.split_prec ? PM_DW_TN_S : PM_DW_TN);
  CHECK(P.n_blocks() == (int)P.blocks.size());
  if (P.st_head) {
    bool skip[PM_MAXL];
    for (int l = 0; l < PM_MAXL; ++l) skip[l] = P.skip[l] || l == S.nl - 1;
    table_ok(S, P.blocks_nh, P.wave_first_nh, skip, PM_DW_TN);
    CHECK(P.wave_first_nh[PM_DW_NW] == (int)P.blocks_nh.size());
  } else {
    CHECK(P.blocks_nh.empty() && P.table_nh_k == DwKernel::None);
  }
  // the chunk deal, for every plan: H nwg RT chunks over at most 256 rows, whole pairs on split operands
  const DwArgs& W = P.args;
  CHECK(W.n_chunks == S.H * S.nwg * S.RT && W.chunks_per_step == S.nwg * S.RT && W.Rw == 16 * S.RT);
  CHECK(W.nsplit <= 256 && W.nsplit * W.chunks_per_split >= W.n_chunks && (W.nsplit - 1) * W.chunks_per_split < W.n_chunks);
  CHECK(!W.split_prec || W.chunks_per_split % 2 == 0);
  CHECK(W.part_stride == (S.n_params + 3) / 4 * 4);
  // rows of the workspace: the one-launch deal's, or the pipelined form's last launch's if more
  CHECK(P.part_rows == (P.pipe_K > 1 && P.pipe_rows > W.nsplit ? P.pipe_rows : W.nsplit));
  CHECK(P.pub_bytes == (P.st_on ? (size_t)S.H * S.nwg * 2 * S.U * 16 * 8 : 0));
  return P;
}
static bool unit_is(const DwUnit& u, int l, int m0, int n0) { return u.layer == l && u.m0 == m0 && u.n0 == n0; }

int main() {
  using K = DwKernel;
  {
    // fp32 block kernel: an exact-fp32 plan never splits operands and has no wide layer; 5-16-16-1 is one tile a side
    // per layer, so one 1 x 1 block per layer.  16 chunks (4 steps x 4 workgroups x 1 row tile) are fewer than 256: one
    // chunk a row.  385 parameters -> rows of 388 floats
    const DwPlan P = plan("fp32 block", shape({5, 16, 16, 1}, PMBRL_PREC_F32, 1, 1, 4, 4));
    CHECK(P.args.split_prec == 0 && P.table_k == K::Block && P.n_blocks() == 3);
    CHECK(P.layer13 == -1 && P.units.empty() && P.unit_k == K::None && P.pre_mask == 0);
    for (int l = 0; l < 3; ++l) CHECK(P.layer_k[l] == K::Block && !P.skip[l] && P.narrow[l] == 0);
    CHECK(P.args.nsplit == 16 && P.args.chunks_per_split == 1 && P.args.n_params == 385 && P.args.part_stride == 388);
    CHECK(P.pipe_K == 1 && P.st_on == 0 && P.st_head == 0 && P.part_rows == 16);
  }
  {
    // split block kernel: split precision at two row tiles.  Tiles 1-2-2-1: 2 x 1, 2 x 2 and 1 x 2 tiles all fit one block
    // of at most 4 x 4.  24 chunks, one a row, rounded to whole pairs: 12 rows of 2
    const DwPlan P = plan("split block", shape({5, 32, 32, 1}, PMBRL_PREC_SPLIT, 2, 1, 3, 4));
    CHECK(P.args.split_prec == 1 && P.table_k == K::BlockSplit && P.n_blocks() == 3);
    CHECK(P.layer13 == -1 && P.units.empty());
    for (int l = 0; l < 3; ++l) CHECK(P.layer_k[l] == K::BlockSplit);
    CHECK(P.args.nsplit == 12 && P.args.chunks_per_split == 2);
    // the 16-row latency-optimised sweeps keep the fp32 form on any precision
    CHECK(plan("split prec, 16 rows", shape({5, 32, 32, 1}, PMBRL_PREC_SPLIT, 1, 1, 3, 4)).table_k == K::Block);
  }
  {
    // wide units: a 256 x 256 layer is 16 x 16 tiles -- at least 128 a side, more than 13 tiles -- so 2 x 2 units of
    // 128 x 128.  The block kernel keeps layer 0 (16 output tiles in 4 blocks of 4) and the head (16 input tiles in 4 blocks)
    const DwPlan P = plan("wide units", shape({5, 256, 256, 1}, PMBRL_PREC_SPLIT, 2, 1, 3, 4));
    CHECK(P.units.size() == 4 && P.unit_k == K::Wide && P.layer13 == -1 && P.pre_mask == 0);
    if (P.units.size() == 4)
      CHECK(unit_is(P.units[0], 1, 0, 0) && unit_is(P.units[1], 1, 0, 128) && unit_is(P.units[2], 1, 128, 0) && unit_is(P.units[3], 1, 128, 128));
    CHECK(!P.skip[0] && P.skip[1] && !P.skip[2] && P.n_blocks() == 8);
    CHECK(P.layer_k[0] == K::BlockSplit && P.layer_k[1] == K::Wide && P.layer_k[2] == K::BlockSplit);
    // PMBRL_DW_NO_WIDE: every layer back in the block kernel -- 4 + 4 x 4 + 4 blocks
    DwShape S = shape({5, 256, 256, 1}, PMBRL_PREC_SPLIT, 2, 1, 3, 4);
    S.sw.dw_no_wide = true;
    const DwPlan Q = plan("no wide", S);
    CHECK(Q.units.empty() && Q.unit_k == K::None && Q.n_blocks() == 24 && Q.layer_k[1] == K::BlockSplit);
  }
  {
    // whole-layer kernel: 200 x 200 is 13 x 13 tiles, at least 128 a side and at most 13 tiles: the first such layer runs
    // whole.  The block kernel (fp32 form: 16 rows) has layer 0's 13 output tiles in 4 blocks and the head's 13 input tiles
    // in 2 blocks of at most 7
    const DwPlan P = plan("whole layer", shape({4, 200, 200, 2}, PMBRL_PREC_SPLIT_F16, 1, 1, 157, 40));
    CHECK(P.layer13 == 1 && P.units.empty() && P.unit_k == K::None && P.args.split_prec == 0);
    CHECK(P.layer_k[0] == K::Block && P.layer_k[1] == K::Layer && P.layer_k[2] == K::Block && P.n_blocks() == 6);
    // 6280 chunks over 256 rows: 25 a row, 252 rows
    CHECK(P.args.nsplit == 252 && P.args.chunks_per_split == 25);
    CHECK(P.st_on == 0);      // (not without the register-resident family)
    // a second such layer goes to the units: 4-200-200-200-2 has layer 1 whole and layer 2 in 2 x 2 units (208 / 128)
    const DwPlan Q = plan("two 13-tile layers", shape({4, 200, 200, 200, 2}, PMBRL_PREC_SPLIT_F16, 1, 1, 8, 4));
    CHECK(Q.layer13 == 1 && Q.units.size() == 4 && Q.layer_k[2] == K::Wide);
  }
  DwShape pre = shape({20, 512, 512, 8}, PMBRL_PREC_SPLIT_F16, 4, 0, 4, 6);
  pre.inplace = 2;
  {
    // pre-split: in-place wide sweeps at 4 row tiles; the one wide layer is 512 x 512 exactly, the first layer has 2 input
    // tiles against 512 outputs (type 1), the head 1 output tile against 512 inputs (type 2).  Four 256 x 256 units of
    // layer 1; nothing is left for the block kernels.  Narrow side of two tiles: <2>, of one: <1>
    const DwPlan P = plan("pre-split", pre);
    CHECK(P.pre_mask == 2u && P.narrow[0] == 1 && P.narrow[1] == 0 && P.narrow[2] == 2);
    CHECK(P.units.size() == 4 && P.unit_k == K::WidePre && P.args.split_prec == 1);
    if (P.units.size() == 4)
      CHECK(unit_is(P.units[0], 1, 0, 0) && unit_is(P.units[1], 1, 0, 256) && unit_is(P.units[2], 1, 256, 0) && unit_is(P.units[3], 1, 256, 256));
    CHECK(P.skip[0] && P.skip[1] && P.skip[2] && P.n_blocks() == 0 && P.table_k == K::None);
    CHECK(P.layer_k[0] == K::NarrowPre2 && P.layer_k[1] == K::WidePre && P.layer_k[2] == K::NarrowPre1);
    // pipeline refused for pre-split stashes, whatever the switch asks
    DwShape S = pre;
    pipe_ranges(S, {3, 2, 1});
    CHECK(plan("pre-split, ranges asked", S).pipe_K == 1);
  }
  {
    // pre-split refused: the wide layer is 496 x 512 -- not 512 x 512 exactly -- so plain units (4 x 4 of 128 x 128; 496
    // outputs are 31 tiles, the fourth unit row is partial) and no narrow layer.  Blocks of at most 4 x 4: layer 0's 32
    // output tiles in 8, the head's 31 input tiles in 8
    DwShape S = shape({20, 512, 496, 8}, PMBRL_PREC_SPLIT_F16, 4, 0, 4, 6);
    S.inplace = 2;
    const DwPlan P = plan("pre-split refused", S);
    CHECK(P.pre_mask == 0 && P.units.size() == 16 && P.unit_k == K::Wide);
    for (int l = 0; l < PM_MAXL; ++l) CHECK(P.narrow[l] == 0);
    CHECK(!P.skip[0] && P.skip[1] && !P.skip[2] && P.n_blocks() == 16 && P.table_k == K::BlockSplit);
  }
  {
    // pipelined: PMBRL_DW_PIPE=3,2,1 at H = 6 -> ranges [3, 6), [1, 3), [0, 1).  4 workgroups leave 8 x (32 - 1) = 248 CUs:
    // the grid next to the sweep; the last launch has max(248, 256) rows, which is what the workspace holds
    DwShape S = shape({5, 16, 16, 1}, PMBRL_PREC_F32, 1, 1, 4, 6);
    pipe_ranges(S, {3, 2, 1});
    const DwPlan P = plan("pipelined", S);
    CHECK(P.pipe_K == 3 && P.pipe_lo[0] == 3 && P.pipe_lo[1] == 1 && P.pipe_lo[2] == 0);
    CHECK(P.pipe_grid == 248 && P.pipe_rows == 256 && P.part_rows == 256 && P.args.nsplit == 24);
    CHECK(P.st_on == 0);
    // ranges that do not add up to the horizon are not taken (and the shape's steps are not long: off)
    pipe_ranges(S, {3, 2});
    CHECK(plan("ranges off the horizon", S).pipe_K == 1);
    // PMBRL_DW_PIPE=off; a sweep that is not one launch; groups split over workgroups
    pipe_ranges(S, {3, 2, 1});
    DwShape T = S; T.sw.dw_pipe_off = true;
    CHECK(plan("pipe off", T).pipe_K == 1);
    T = S; T.whole = false;
    CHECK(plan("not one launch", T).pipe_K == 1);
    T = S; T.mm_parts = 2;
    CHECK(plan("split groups", T).pipe_K == 1);
    // no switch: long steps (row tiles x weights of both nets >= 256 K, H >= 16) cut 40 / 30 / 20 / 10 %: H = 40 -> 4, 8, 12
    // steps from the end for the last three -> lower bounds 24, 12, 4, 0
    T = shape({20, 512, 512, 8}, PMBRL_PREC_SPLIT_F16, 4, 0, 4, 40);
    const DwPlan Q = plan("long steps", T);
    CHECK(Q.pipe_K == 4 && Q.pipe_lo[0] == 24 && Q.pipe_lo[1] == 12 && Q.pipe_lo[2] == 4 && Q.pipe_lo[3] == 0);
  }
  {
    // parity adjustment: split operands (general family at 16 rows) and 3 x 1 chunks a step, odd: a range may not start at
    // an odd step.  3,4,3 at H = 10: 7 -> 6, then 6 - 4 = 2, then 0
    DwShape S = shape({5, 32, 32, 1}, PMBRL_PREC_SPLIT, 1, 0, 3, 10);
    pipe_ranges(S, {3, 4, 3});
    const DwPlan P = plan("parity", S);
    CHECK(P.args.split_prec == 1 && P.pipe_K == 3 && P.pipe_lo[0] == 6 && P.pipe_lo[1] == 2 && P.pipe_lo[2] == 0);
    // an even number of chunks a step needs none: 7, 3, 0
    S.nwg = 4;
    const DwPlan Q = plan("no parity", S);
    CHECK(Q.pipe_K == 3 && Q.pipe_lo[0] == 7 && Q.pipe_lo[1] == 3 && Q.pipe_lo[2] == 0);
  }
  {
    // pipeline refused for too few idle CUs: 232 workgroups leave 8 x (32 - 29) = 24, fewer than 256 / 8
    DwShape S = shape({5, 16, 16, 1}, PMBRL_PREC_F32, 1, 1, 232, 6);
    pipe_ranges(S, {3, 2, 1});
    CHECK(pm_dw_idle_cus(256, 232) == 24 && plan("few idle CUs", S).pipe_K == 1);
    CHECK(pm_dw_idle_cus(256, 4) == 248 && pm_dw_idle_cus(60, 4) == 0 && pm_dw_idle_cus(260, 4) == 0);
  }
  {
    // streamed, cut 0: 157 workgroups leave 8 x (32 - 20) = 96 CUs; 157 >= 96 and 40 x 157 >= 14 x 256: large; 157 <= 2 x 96:
    // at most a pair a step, every step streamed, one consumer per idle CU
    const DwShape S = reg_shape(157, 40);
    const DwPlan P = plan("streamed, cut 0", S);
    CHECK(P.pipe_K == 1 && P.st_on == 1 && P.st_cut == 0 && P.st_wgs == 96);
    CHECK(P.pub_bytes == (size_t)40 * 157 * 2 * 16 * 8);
    // head joins: cut 0, not forced, the head is the last layer with one output tile, W1 b1 W2 b2 contiguous.  The
    // table without it has layer 0 alone: 13 output tiles in at least 8 parts -> 2 2 2 2 2 1 1 1, one input tile: every
    // block at most 2 x 1, the ring kernel
    CHECK(P.st_head == 1 && P.wave_first_nh[PM_DW_NW] == 8 && P.nh_ring == 1 && P.table_nh_k == K::BlockRing);
    int twos = 0, ones = 0;
    for (const DwBlock& b : P.blocks_nh) { CHECK(b.layer == 0 && b.n_it == 1); twos += b.n_ot == 2; ones += b.n_ot == 1; }
    CHECK(twos == 5 && ones == 3);
    for (int w = 0; w <= PM_DW_NW; ++w) CHECK(P.wave_first_nh[w] == w);      // (equal costs: one block a wave)
    CHECK(P.table_k == K::Block && P.n_blocks() == 6);      // (the table with the head is as without the form)
    // head stays: PMBRL_DW_HEAD=off
    DwShape T = S; T.sw.dw_head = 0;
    CHECK(plan("head off", T).st_on == 1 && plan("head off", T).st_head == 0);
    // head stays: the columns are not contiguous (b1 moved behind everything)
    T = S; T.b_off[1] = T.n_params; T.n_params += 200;
    CHECK(plan("columns apart", T).st_on == 1 && plan("columns apart", T).st_head == 0);
    // a first layer of two input tiles: the head-less table's blocks are 2 x 2 and 1 x 2, the block kernel walks it
    T = shape({20, 200, 200, 2}, PMBRL_PREC_SPLIT_F16, 1, 1, 157, 40); T.reg = 1;
    const DwPlan Q = plan("head-less table, no ring", T);
    CHECK(Q.st_head == 1 && Q.nh_ring == 0 && Q.table_nh_k == K::Block && Q.wave_first_nh[PM_DW_NW] == 8);
    // not large (fewer workgroups than idle CUs) and not forced: off
    CHECK(plan("small", reg_shape(16, 40)).st_on == 0);
    // refused: H >= 4095; the pipelined form on (PMBRL_DW_PIPE=20,20); PMBRL_DW_STREAM=off; the adjoint not the family's;
    // its moment-matching instance; the whole-layer kernel not at the second hidden layer (PMBRL_DW_NO_WIDE)
    CHECK(plan("H 4095", reg_shape(157, 4095)).st_on == 0 && plan("H 4094", reg_shape(157, 4094)).st_on == 1);
    T = S; pipe_ranges(T, {20, 20});
    CHECK(plan("piped", T).pipe_K == 2 && plan("piped", T).st_on == 0 && plan("piped", T).st_head == 0);
    T = S; T.sw.dw_stream_off = true;
    CHECK(plan("stream off", T).st_on == 0);
    T = S; T.reg_bwd = false;
    CHECK(plan("no family adjoint", T).st_on == 0);
    T = S; T.reg_mm = 4;
    CHECK(plan("moment-matching instance", T).st_on == 0);
    T = S; T.reg = 0;
    CHECK(plan("no family", T).st_on == 0);
    T = S; T.sw.dw_no_wide = true;
    CHECK(plan("no whole layer", T).layer13 == -1 && plan("no whole layer", T).st_on == 0);
  }
  {
    // streamed with a cut: 200 workgroups leave 8 x (32 - 25) = 56 CUs, 200 > 2 x 56: the consumers keep up with
    // 40 x 2 x 56 / 200 = 22 steps (22.4 rounded down), the 18 below go to the launch behind the sweep; the head stays
    const DwPlan P = plan("streamed, cut", reg_shape(200, 40));
    CHECK(P.st_on == 1 && P.st_cut == 18 && P.st_wgs == 56 && P.st_head == 0 && P.table_nh_k == K::None);
  }
  {
    // streamed, forced: PMBRL_DW_STREAM=3,8 on a plan that is not large -- 3 of 6 steps, min(248, 8) consumers
    DwShape S = reg_shape(4, 6);
    S.sw.dw_stream_set = true; S.sw.dw_stream_steps = 3; S.sw.dw_stream_wgs = 8;
    const DwPlan P = plan("forced 3,8", S);
    CHECK(P.st_on == 1 && P.st_cut == 3 && P.st_wgs == 8 && P.st_head == 0);
    // ... every step forced (more than H asked: H), the plan's consumers: cut 0, but the head stays -- a forced form keeps
    // its meaning
    S.sw.dw_stream_steps = 9; S.sw.dw_stream_wgs = 0;
    const DwPlan Q = plan("forced all", S);
    CHECK(Q.st_on == 1 && Q.st_cut == 0 && Q.st_wgs == 248 && Q.st_head == 0);
    // ... unless PMBRL_DW_HEAD=on; which does nothing where a cut is left
    S.sw.dw_head = 1;
    CHECK(plan("forced all, head on", S).st_head == 1);
    S.sw.dw_stream_steps = 3;
    CHECK(plan("forced cut, head on", S).st_cut == 3 && plan("forced cut, head on", S).st_head == 0);
    // ... and 0 steps forced streams nothing but keeps the form (cut = H)
    S.sw.dw_stream_steps = 0;
    CHECK(plan("forced 0", S).st_on == 1 && plan("forced 0", S).st_cut == 6);
  }
  if (failed) printf("%d checks failed\n", failed);
  return failed;
}
