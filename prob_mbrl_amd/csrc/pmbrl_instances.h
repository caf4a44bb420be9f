// Which sweep-kernel instances exist: the lists every object instantiates its kernels from, the tables built from them
// and the lookups over those tables.  Host-only and free of HIP, so that a plain host compiler can check the lists
// (tests/instances_check.cpp).  An object compiles the kernels of one list and exports one table (PmInstTable: the
// keys below next to the kernels' host pointers, same order); pmbrl_plan_create resolves a plan's kernels from the
// tables once (pmbrl.hip: plan_attrs) and refuses a plan whose instance is missing.
#pragma once
#include <stddef.h>

#include "pmbrl.h"

// kernel variants of the latency-optimised family (pmbrl_fast.h)
#define PF_VAR_LEAN 0
#define PF_VAR_EXT 1
#define PF_VAR_MM 2
#define PF_VAR_MMG 3   // mm_mode 3 as ONE launch: the workgroups meet at a device-wide barrier every step
#define PF_VAR_COUNT 4

// One instance.  Latency-optimised family: row tiles, stage pair, PF_VAR_*, and the compile-time shape (PfShape: state
// and action width, LDS leading dimension, layers, 16-wide tiles per hidden layer; all 0 = PfShapeAny) or PfShapeTree.
// General family: rt, and var = the in-place form (PMBRL_INFO_INPLACE; 3 = 2 with every 512-wide stash pre-split) or, in
// the table of the networks that are not ReLU, the piece planes (0 exact fp32, 2 split).  Register-resident family:
// d = width of the states it moment-matches (0 none), tree, var = with cycle stamps.
struct PmInstKey { int rt, ca, cb, var, d, u, ld, nl, nt, tree; };
// ... the keys of the other two families, by what their fields mean there
static inline PmInstKey pm_general_key(int rt, int form_or_planes) { return {rt, 0, 0, form_or_planes, 0, 0, 0, 0, 0, 0}; }
static inline PmInstKey pm_reg_key(int mm_width, bool tree, bool stamps) { return {1, 0, 0, stamps, mm_width, 0, 0, 0, 0, tree}; }
struct PmInst { const void *fwd, *bwd; };
struct PmInstTable { const PmInstKey* key; const PmInst* fn; int n; };

// ---- the lists.  PM_INST(RT, CA, CB, VAR, D, U, LD, NL, NT, TREE) is defined by whoever expands one.
#define PM_PLAIN_ROWS(RT, CA, CB)                                                               \
  PM_INST(RT, CA, CB, PF_VAR_LEAN, 0, 0, 0, 0, 0, 0) PM_INST(RT, CA, CB, PF_VAR_EXT, 0, 0, 0, 0, 0, 0) \
  PM_INST(RT, CA, CB, PF_VAR_MM, 0, 0, 0, 0, 0, 0)
// the one-launch form of mm_mode 3 exists for 16-row workgroups
#define PM_MMG_ROWS_1(CA, CB) PM_INST(1, CA, CB, PF_VAR_MMG, 0, 0, 0, 0, 0, 0)
#define PM_MMG_ROWS_2(CA, CB)
#define PM_MMG_ROWS_4(CA, CB)
#define PM_FAST_SHAPED(RT, CA, CB, VAR, D, U, LD, NL, NT) PM_INST(RT, CA, CB, VAR, D, U, LD, NL, NT, 0)

// exact fp32: the instantiated (row tiles, stage pair) combinations, in the order LayoutCalc::stages (pmbrl.hip) tries
// them -- the first listed wins a tie
#define PM_FAST_CASE(RT, CA, CB) PM_PLAIN_ROWS(RT, CA, CB) PM_MMG_ROWS_##RT(CA, CB)
#define PM_FAST_CASES                                                                  \
  PM_FAST_CASE(1, 8, 8) PM_FAST_CASE(1, 7, 6) PM_FAST_CASE(1, 4, 4) PM_FAST_CASE(1, 2, 2) \
  PM_FAST_CASE(2, 4, 4) PM_FAST_CASE(2, 4, 3) PM_FAST_CASE(2, 2, 2) PM_FAST_CASE(4, 2, 2) PM_FAST_CASE(4, 1, 1)
// shape-specialised instantiations (pmbrl_fast.h: PfShape): RT, CA, CB, variant, D, U, LD, layers,
// 16-wide tiles per hidden layer.
// The shipped configurations: cart-pole (D=4) and double cart-pole (D=6) states, one action,
// 2 x 200 hidden units; plain / per-step / in-kernel moment matching.
#define PM_FAST_SHAPED_CASES                                  \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_LEAN, 4, 1, 216, 3, 13)      \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_EXT, 4, 1, 216, 3, 13)       \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_LEAN, 5, 1, 216, 3, 13)      \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_LEAN, 6, 1, 216, 3, 13)      \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_EXT, 5, 1, 216, 3, 13)       \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_EXT, 6, 1, 216, 3, 13)       \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_MM, 5, 1, 216, 3, 13)        \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_MM, 6, 1, 216, 3, 13)        \
  PM_FAST_SHAPED(2, 4, 3, PF_VAR_MM, 4, 1, 232, 3, 13)        \
  PM_FAST_SHAPED(2, 4, 3, PF_VAR_MM, 6, 1, 232, 3, 13)        \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_MM, 4, 1, 216, 3, 13)        \
  PM_FAST_SHAPED(4, 1, 1, PF_VAR_MM, 6, 1, 232, 3, 13)        \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_MMG, 4, 1, 216, 3, 13)       \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_MMG, 5, 1, 216, 3, 13)       \
  PM_FAST_SHAPED(1, 7, 6, PF_VAR_MMG, 6, 1, 216, 3, 13)
#define PM_FAST_F32_INSTANCES PM_FAST_CASES PM_FAST_SHAPED_CASES

// split bf16 / fp16 operands (pmbrl_split.h): stage pairs in K32 blocks.  64-row workgroups exist with two fp16 piece
// planes only, and only as the shape-specialised instance (the generic ones fail tools/check_inflight.py)
#define PM_SPLIT_CASES PM_FAST_CASE(1, 4, 3) PM_FAST_CASE(1, 1, 1) PM_FAST_CASE(2, 4, 3) PM_FAST_CASE(2, 1, 1)
// shape-specialised split instantiations; LDV: floats per row of an activation buffer = piece planes x 240 / 2
// (three bf16 planes: 360, two fp16 planes: 240)
#define PM_SPLIT_SHAPED_CASES(LDV)                             \
  PM_FAST_SHAPED(1, 4, 3, PF_VAR_LEAN, 4, 1, LDV, 3, 13)       \
  PM_FAST_SHAPED(1, 4, 3, PF_VAR_EXT, 4, 1, LDV, 3, 13)        \
  PM_FAST_SHAPED(1, 4, 3, PF_VAR_LEAN, 5, 1, LDV, 3, 13)       \
  PM_FAST_SHAPED(1, 4, 3, PF_VAR_LEAN, 6, 1, LDV, 3, 13)       \
  PM_FAST_SHAPED(2, 4, 3, PF_VAR_MM, 4, 1, LDV, 3, 13)         \
  PM_FAST_SHAPED(1, 4, 3, PF_VAR_MM, 4, 1, LDV, 3, 13)         \
  PM_FAST_SHAPED(2, 4, 3, PF_VAR_MM, 6, 1, LDV, 3, 13)         \
  PM_FAST_SHAPED(1, 4, 3, PF_VAR_MMG, 5, 1, LDV, 3, 13)
#define PM_SPLIT1_INSTANCES PM_SPLIT_CASES PM_SPLIT_SHAPED_CASES(360)
// ... two fp16 planes: also the 64-row double cart-pole instance and the cart-pole one whose groups are split over more
// than 8 workgroups (two-level sum exchange, PfShapeTree)
#define PM_SPLIT2_INSTANCES                                                                     \
  PM_SPLIT_CASES PM_SPLIT_SHAPED_CASES(240)                                                      \
  PM_FAST_SHAPED(4, 4, 3, PF_VAR_MM, 6, 1, 240, 3, 13) PM_INST(1, 4, 3, PF_VAR_MM, 4, 1, 240, 3, 13, 1)

// general family, by row tiles: exact fp32; split operands (the in-place forms at 64 rows); networks that are not ReLU
#define PM_GENERAL_ROWS(VAR) PM_INST(1, 0, 0, VAR, 0, 0, 0, 0, 0, 0) PM_INST(2, 0, 0, VAR, 0, 0, 0, 0, 0, 0) PM_INST(4, 0, 0, VAR, 0, 0, 0, 0, 0, 0)
#define PM_GENERAL_F32_INSTANCES PM_GENERAL_ROWS(0)
#define PM_GENERAL_SPLIT_INSTANCES \
  PM_GENERAL_ROWS(0) PM_INST(4, 0, 0, 1, 0, 0, 0, 0, 0, 0) PM_INST(4, 0, 0, 2, 0, 0, 0, 0, 0, 0) PM_INST(4, 0, 0, 3, 0, 0, 0, 0, 0, 0)
#define PM_GENERAL_ACT_INSTANCES PM_GENERAL_ROWS(0) PM_GENERAL_ROWS(2)
// register-resident family
#define PM_REG_ROWS(MMD, TREE) PM_INST(1, 0, 0, 0, MMD, 0, 0, 0, 0, TREE) PM_INST(1, 0, 0, 1, MMD, 0, 0, 0, 0, TREE)
#define PM_REG_INSTANCES PM_REG_ROWS(0, 0) PM_REG_ROWS(4, 0) PM_REG_ROWS(5, 0) PM_REG_ROWS(6, 0) PM_REG_ROWS(4, 1)

// ---- the keys of every list
#define PM_INST(RT, CA, CB, VAR, D, U, LD, NL, NT, TREE) {RT, CA, CB, VAR, D, U, LD, NL, NT, TREE},
#define PM_KEYS(NAME, LIST)                                 \
  static constexpr PmInstKey NAME##_keys[] = {LIST}; \
  static constexpr int NAME##_n = (int)(sizeof(NAME##_keys) / sizeof(PmInstKey));
PM_KEYS(pm_fast_f32, PM_FAST_F32_INSTANCES)
PM_KEYS(pm_fast_split1, PM_SPLIT1_INSTANCES)
PM_KEYS(pm_fast_split2, PM_SPLIT2_INSTANCES)
PM_KEYS(pm_general_f32, PM_GENERAL_F32_INSTANCES)
PM_KEYS(pm_general_split, PM_GENERAL_SPLIT_INSTANCES)
PM_KEYS(pm_general_act, PM_GENERAL_ACT_INSTANCES)
PM_KEYS(pm_reg, PM_REG_INSTANCES)
#undef PM_KEYS
#undef PM_INST
// the keys of the latency-optimised family at a PMBRL_PREC_*
static inline PmInstTable pm_fast_keys(int prec) {
  if (prec == PMBRL_PREC_SPLIT_F16) return {pm_fast_split2_keys, nullptr, pm_fast_split2_n};
  if (prec) return {pm_fast_split1_keys, nullptr, pm_fast_split1_n};
  return {pm_fast_f32_keys, nullptr, pm_fast_f32_n};
}

// ---- lookups
// row of the full key (-1: no such instance)
static inline int pm_inst_find(const PmInstTable& T, const PmInstKey& k) {
  for (int i = 0; i < T.n; ++i) {
    const PmInstKey& r = T.key[i];
    if (r.rt == k.rt && r.ca == k.ca && r.cb == k.cb && r.var == k.var && r.d == k.d && r.u == k.u && r.ld == k.ld &&
        r.nl == k.nl && r.nt == k.nt && r.tree == k.tree)
      return i;
  }
  return -1;
}
// does any row match (RT, variant, D, U, NL, NT), whatever its stage pair and leading dimension?
static inline bool pm_inst_any(const PmInstTable& T, int rt, int var, int d, int u, int nl, int nt, int tree = 0) {
  for (int i = 0; i < T.n; ++i) {
    const PmInstKey& r = T.key[i];
    if (r.rt == rt && r.var == var && r.d == d && r.u == u && r.nl == nl && r.nt == nt && r.tree == tree) return true;
  }
  return false;
}
// the stage pairs the table has for RT, in table order; returns how many (at most `max` are written)
struct StagePair { int ca, cb; };
static inline int pm_inst_stage_pairs(const PmInstTable& T, int rt, StagePair* out, int max) {
  int n = 0;
  for (int i = 0; i < T.n; ++i) {
    const PmInstKey& r = T.key[i];
    if (r.rt != rt) continue;
    bool seen = false;
    for (int j = 0; j < n && j < max; ++j) seen = seen || (out[j].ca == r.ca && out[j].cb == r.cb);
    if (seen) continue;
    if (n < max) out[n] = {r.ca, r.cb};
    ++n;
  }
  return n;
}
// ... and, among them, the one for which work(CA + CB) is least: the first listed wins a tie
template <class Work>
static inline StagePair pm_inst_best_stages(const PmInstTable& T, int rt, Work work) {
  StagePair c[8];
  const int n = pm_inst_stage_pairs(T, rt, c, 8);
  StagePair best = n ? c[0] : StagePair{0, 0};
  for (int i = 1; i < n && i < 8; ++i)
    if (work(c[i].ca + c[i].cb) < work(best.ca + best.cb)) best = c[i];
  return best;
}
