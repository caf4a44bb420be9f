// Host-only check of the sweep-kernel instance lists (prob_mbrl_amd/csrc/pmbrl_instances.h); compiled and run by
// tests/test_instances.py.  Prints one line per failed check and returns how many failed.
#include <stdio.h>

#include <initializer_list>

#include "pmbrl_instances.h"

static int failed = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) { ++failed; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
  } while (0)

// (a) the stage pairs a family has for RT, in the order the chooser tries them
static void pairs_are(const char* what, const PmInstTable& T, int rt, const StagePair* want, int n_want) {
  StagePair got[8];
  const int n = pm_inst_stage_pairs(T, rt, got, 8);
  CHECK(n == n_want, "%s RT%d: %d pairs, expected %d", what, rt, n, n_want);
  for (int i = 0; i < n && i < n_want; ++i)
    CHECK(got[i].ca == want[i].ca && got[i].cb == want[i].cb, "%s RT%d pair %d: {%d,%d}, expected {%d,%d}", what, rt, i,
          got[i].ca, got[i].cb, want[i].ca, want[i].cb);
}

// the work LayoutCalc::stream_work (pmbrl.hip) counts for two networks of two hidden layers, nt tiles each
static long stream_work(int nt, int m, int kdiv) {
  const int k = (nt + kdiv - 1) / kdiv;
  return 2L * 2 * nt * ((k + m - 1) / m * m);
}
static bool has(const PmInstTable& T, int rt, StagePair sp, int var) {
  const PmInstKey k = {rt, sp.ca, sp.cb, var, 0, 0, 0, 0, 0, 0};
  return pm_inst_find(T, k) >= 0;
}

int main() {
  const PmInstTable f32 = pm_fast_keys(PMBRL_PREC_F32), s1 = pm_fast_keys(PMBRL_PREC_SPLIT), s2 = pm_fast_keys(PMBRL_PREC_SPLIT_F16);
  {
    const StagePair f1[] = {{8, 8}, {7, 6}, {4, 4}, {2, 2}}, f2[] = {{4, 4}, {4, 3}, {2, 2}}, f4[] = {{2, 2}, {1, 1}};
    const StagePair sp[] = {{4, 3}, {1, 1}}, sp4[] = {{4, 3}};
    pairs_are("fp32", f32, 1, f1, 4);
    pairs_are("fp32", f32, 2, f2, 3);
    pairs_are("fp32", f32, 4, f4, 2);
    pairs_are("split", s1, 1, sp, 2);
    pairs_are("split", s1, 2, sp, 2);
    pairs_are("split", s1, 4, sp, 0);      // 64-row workgroups: fp16 pieces only
    pairs_are("split_f16", s2, 1, sp, 2);
    pairs_are("split_f16", s2, 2, sp, 2);
    pairs_are("split_f16", s2, 4, sp4, 1);
  }
  // (b) whatever pair the chooser returns has the plain and moment-matching instances, at 16 rows the barrier form too
  struct Fam { const char* name; PmInstTable T; int kdiv, n_rt, rt[3]; };
  const Fam fams[] = {{"fp32", f32, 1, 3, {1, 2, 4}}, {"split", s1, 2, 2, {1, 2, 0}}, {"split_f16", s2, 2, 2, {1, 2, 0}}};
  for (const Fam& F : fams)
    for (int i = 0; i < F.n_rt; ++i)
      for (int nt = 1; nt <= 32; ++nt) {
        const int rt = F.rt[i];
        const StagePair sp = pm_inst_best_stages(F.T, rt, [&](int m) { return stream_work(nt, m, F.kdiv); });
        for (int var : {PF_VAR_LEAN, PF_VAR_EXT, PF_VAR_MM})
          CHECK(has(F.T, rt, sp, var), "%s RT%d, %d tiles: no variant %d for {%d,%d}", F.name, rt, nt, var, sp.ca, sp.cb);
        CHECK(has(F.T, rt, sp, PF_VAR_MMG) == (rt == 1), "%s RT%d, %d tiles: barrier form of {%d,%d}", F.name, rt, nt, sp.ca, sp.cb);
      }
  // ... and a 64-row plan on fp16 pieces, which plan_layout takes for 13 tiles only, its shape-specialised instance
  {
    const StagePair sp = pm_inst_best_stages(s2, 4, [&](int m) { return stream_work(13, m, 2); });
    const PmInstKey k = {4, sp.ca, sp.cb, PF_VAR_MM, 6, 1, 240, 3, 13, 0};
    CHECK(sp.ca == 4 && sp.cb == 3 && pm_inst_find(s2, k) >= 0, "split_f16 RT4: {%d,%d}", sp.ca, sp.cb);
    CHECK(!has(s2, 4, {1, 1}, PF_VAR_MM) && !has(s2, 4, {4, 3}, PF_VAR_MM), "split_f16 RT4 has a generic instance");
  }
  // (c) the rows plan_layout's predicates ask for
  CHECK(pm_inst_any(s2, 4, PF_VAR_MM, 6, 1, 3, 13), "rt4_split");
  CHECK(!pm_inst_any(s1, 4, PF_VAR_MM, 6, 1, 3, 13) && !pm_inst_any(s2, 4, PF_VAR_MM, 4, 1, 3, 13), "rt4_split elsewhere");
  CHECK(pm_inst_any(s2, 1, PF_VAR_MM, 4, 1, 3, 13, 1), "shaped_mm1 (tree)");
  CHECK(!pm_inst_any(s2, 1, PF_VAR_MM, 6, 1, 3, 13, 1) && !pm_inst_any(s1, 1, PF_VAR_MM, 4, 1, 3, 13, 1), "tree elsewhere");
  const int lds_rows[][2] = {{PF_VAR_LEAN, 4}, {PF_VAR_EXT, 4}, {PF_VAR_LEAN, 5}, {PF_VAR_LEAN, 6}, {PF_VAR_MM, 4}};
  for (const auto& r : lds_rows) {
    const PmInstKey k = {1, 4, 3, r[0], r[1], 1, 240, 3, 13, 0};
    CHECK(pm_inst_find(s2, k) >= 0, "LDS-tile row: variant %d, D = %d", r[0], r[1]);
  }
  printf("%d checks failed\n", failed);
  return failed;
}
