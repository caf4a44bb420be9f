// Host-only check of the LDS maps (prob_mbrl_amd/csrc/pmbrl_lds_map.h); compiled and run by tests/test_lds_map.py.
// One case per branch of the two walks, at the smallest shape that takes it.  A case lists its regions in the documented
// order as {what the map says, offset worked out by hand, floats worked out by hand}: the offsets must be equal, the
// regions must follow each other without overlap (a gap only where the walk rounds up to 4 floats) and end at the total.
// Every number is worked out by hand from the region list (the sizes stand next to them); none is taken from the walk.
// Prints one line per failed check and returns how many failed.
#include <stdio.h>

#include <vector>

#include "pmbrl_lds_map.h"

static int failed = 0;
static const char* now = "";
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { ++failed; printf("FAILED [%s] %s (line %d)\n", now, #cond, __LINE__); } \
  } while (0)

struct Region {
  const char* name;
  long got, want;      // offset: the map's, by hand
  size_t floats;       // by hand; 0: a region that takes no room in this case
  bool aligned;        // starts at a multiple of 4 floats (mm, and whatever follows a round-up)
};
static void regions_ok(const std::vector<Region>& rs, size_t total, size_t want_total) {
  size_t end = 0;
  for (const Region& r : rs) {
    if (r.got != r.want) { ++failed; printf("FAILED [%s] %s at %ld, by hand %ld\n", now, r.name, r.got, r.want); }
    if (r.want < 0) continue;      // absent (aliased)
    if (r.aligned && r.want % 4) { ++failed; printf("FAILED [%s] %s at %ld is not 16-byte aligned\n", now, r.name, r.want); }
    // a region that takes no room in this case: its offset is where it would be, which the regions behind it do not count
    if (!r.floats) { if ((size_t)r.want >= end && (size_t)r.want <= end + 3) end = (size_t)r.want; continue; }
    if ((size_t)r.want < end || (size_t)r.want > end + 3) { ++failed; printf("FAILED [%s] %s at %ld, the regions before it end at %zu\n", now, r.name, r.want, end); }
    end = (size_t)r.want + r.floats;
  }
  if (end != want_total || total != want_total) { ++failed; printf("FAILED [%s] total %zu, regions end at %zu, by hand %zu\n", now, total, end, want_total); }
}

// the latency-optimised family's offsets by hand, in the order of the walk
struct FastWant {
  long bufA, bufB, xa, xb, av, gad, rr, gr, hp;
  std::vector<long> pbias, dbias, pmask, dmask;
  long zp, zd, mx, iSx, my, Sy, lSy, psc, pbi, jx, stg, zs, xin, ovf, tp, tcnt, tw, mm, xch, xch_zt, xch_sets, rows;
  size_t total;
};
static void fast_ok(const char* name, const PmFastMap& m, const FastWant& w, int R, int LD, int D, int U, int RT, const int* pnt,
                    int pnl, const int* dnt, int dnl, int mm_d, int prec, size_t tails, int mm_waves, int group_rows, int steps) {
  now = name;
  const size_t r = R, scr = 2 * ((size_t)3 * mm_d * mm_d + 5 * mm_d);      // floats of one wave's fp64 scratch: 3 d^2 + 5 d doubles
  std::vector<Region> rs = {{"bufA", (long)m.bufA, w.bufA, r * LD, true}, {"bufB", (long)m.bufB, w.bufB, r * LD, false},
                            {"xa", (long)m.xa, w.xa, r * D, false}, {"xb", (long)m.xb, w.xb, r * D, false},
                            {"av", (long)m.av, w.av, r * U, false}, {"gad", (long)m.gad, w.gad, r * 16, false},
                            {"rr", (long)m.rr, w.rr, r, false}, {"gr", (long)m.gr, w.gr, r, false},
                            {"hp", m.hp_off, w.hp, (size_t)8 * RT * 256, false}};
  CHECK((int)w.pbias.size() == pnl && (int)w.dbias.size() == dnl && (int)w.pmask.size() == pnl - 1 && (int)w.dmask.size() == dnl - 1);
  for (int l = 0; l < pnl; ++l) rs.push_back({"pbias", (long)m.pbias[l], w.pbias[l], (size_t)pnt[l + 1] * 16, false});
  for (int l = 0; l < dnl; ++l) rs.push_back({"dbias", (long)m.dbias[l], w.dbias[l], (size_t)dnt[l + 1] * 16, false});
  for (int l = 0; l < pnl - 1; ++l) rs.push_back({"pmask", (long)m.pmask[l], w.pmask[l], (r * pnt[l + 1] + 1) / 2, false});   // 16 bits per (row, tile)
  for (int l = 0; l < dnl - 1; ++l) rs.push_back({"dmask", (long)m.dmask[l], w.dmask[l], (r * dnt[l + 1] + 1) / 2, false});
  const std::vector<Region> rest = {
      {"zp", (long)m.zp, w.zp, r * U, false}, {"zd", (long)m.zd, w.zd, r * D, false},
      {"mx", (long)m.mx, w.mx, (size_t)D + U, false}, {"iSx", (long)m.iSx, w.iSx, (size_t)D + U, false},
      {"my", (long)m.my, w.my, (size_t)D, false}, {"Sy", (long)m.Sy, w.Sy, (size_t)D, false}, {"lSy", (long)m.lSy, w.lSy, (size_t)D, false},
      {"psc", (long)m.psc, w.psc, (size_t)U, false}, {"pbi", (long)m.pbi, w.pbi, (size_t)U, false},
      {"jx", (long)m.jx, w.jx, r * 16, true}, {"stg", (long)m.stg, w.stg, r * (1 + 2 * D + 3 * U), false}, {"zs", (long)m.zs, w.zs, r * D, false},
      {"xin", (long)m.xin, w.xin, prec ? r * 24 : 0, true}, {"ovf", (long)m.ovf, w.ovf, prec ? 4u : 0u, false},
      {"tp", (long)m.tp, w.tp, tails ? (size_t)8 * RT * 256 : 0, false}, {"tcnt", (long)m.tcnt, w.tcnt, tails ? 4u : 0u, false},
      {"tw", (long)m.tw, w.tw, tails, false},
      {"mm scratch", (long)m.mm, w.mm, mm_waves * scr, true},
      {"xch ref", (long)m.m.xch, w.xch, group_rows ? 8u : 0u, false},
      {"xch zt", (long)m.m.xch_zt, w.xch_zt, group_rows ? (size_t)2 * steps * 2 * mm_d : 0, false},      // doubles [steps][zm (d) | zi (d)]
      {"xch sets", (long)m.m.xch_sets, w.xch_sets, group_rows ? 2 * (scr + 2 * r * mm_d) : 0, false},      // [scratch | rows | z rows] x 2
      {"rows", (long)m.m.rows, w.rows, (size_t)4 * group_rows * mm_d, true}};
  rs.insert(rs.end(), rest.begin(), rest.end());
  regions_ok(rs, m.total, w.total);
  CHECK(m.m.total == m.total && m.m.mm == m.mm && m.base == 0 && m.m.mm_wave == scr && m.m.tile_base == (size_t)(w.rows + 3) / 4 * 4);
}

int main() {
  const int n13[] = {1, 13, 13, 1}, n14[] = {1, 14, 14, 1}, n5[] = {1, 5, 5, 1};

  // ---- K-split tails: 16 rows, exact fp32, both nets 1-13-13-1 tiles, D = 4, U = 1, LD = 232
  // 2 x 16 x 232 | 2 x 64 | 16 | 256 | 16 | 16 -> 7856; hp 8 x 256 -> 9904; biases 208 208 16 twice -> 10768; masks
  // (16 x 13 + 1) / 2 = 104, two per net -> 11184; zp 16, zd 64, mx 5, iSx 5, my / Sy / lSy 4, psc / pbi 1 -> 11288 (= 0 mod 4);
  // jx 256, stg 16 x 12 = 192, zs 64 -> 11800; no xin; tails: 13 = 4 x 3 + 1 tiles, 13 k-blocks x 256 per net and direction
  // = 6656: tp 2048, tcnt 4, tw 6656 -> 20508
  const FastWant tails = {0, 3712, 7424, 7488, 7552, 7568, 7824, 7840, 7856, {9904, 10112, 10320}, {10336, 10544, 10752},
                          {10768, 10872}, {10976, 11080}, 11184, 11200, 11264, 11269, 11274, 11278, 11282, 11286, 11287, 11288,
                          11544, 11736, 11800, 12184, 11800, 13848, 13852, 20508, 20508, 20516, 20516, 20508, 20508};
  fast_ok("K-split tails", pm_fast_map(16, 232, 4, 1, 1, n13, 3, n13, 3, 0), tails, 16, 232, 4, 1, 1, n13, 3, n13, 3, 0, 0, 6656, 8, 0, 0);
  CHECK(pm_fast_ksplit(13, 1) && !pm_fast_ksplit(14, 1) && !pm_fast_ksplit(13, 4) && !pm_fast_ksplit(13, 1, 2) && pm_fast_ksplit(5, 2));
  CHECK(pm_fast_tail_floats(n13, 3, n13, 3, false, 1) == 6656 && pm_fast_tail_floats(n13, 3, n13, 3, true, 1) == 6656);

  // ---- whole groups moment matched in the sweep (same shape, d = 4: 3 x 16 + 5 x 4 = 68 doubles = 136 floats per wave):
  // groups of 8 rows in a 16-row workgroup = 2 waves -> 20508 + 272; eight waves -> 20508 + 1088
  FastWant whole = tails;
  whole.xch = whole.rows = 20780; whole.xch_zt = whole.xch_sets = 20788; whole.total = 20780;
  fast_ok("whole groups, 2 waves", pm_fast_map(16, 232, 4, 1, 1, n13, 3, n13, 3, 4, 0, 2), whole, 16, 232, 4, 1, 1, n13, 3, n13, 3, 4, 0, 6656, 2, 0, 0);
  whole.xch = whole.rows = 21596; whole.xch_zt = whole.xch_sets = 21604; whole.total = 21596;
  fast_ok("whole groups, 8 waves", pm_fast_map(16, 232, 4, 1, 1, n13, 3, n13, 3, 4, 0, 8), whole, 16, 232, 4, 1, 1, n13, 3, n13, 3, 4, 0, 6656, 8, 0, 0);
  {
    double scr[4 * 68];
    CHECK(pm_mm_scratch_doubles(4) == 68 && pm_mm_scratch_doubles(0) == 0 && pm_mm_scratch_of(scr, 3, 4) == scr + 204);
  }

  // ---- no tails: the same with 14 hidden tiles -- biases 224 224 16 twice -> 10832; masks 112 x 4 -> 11280; ... -> 11384;
  // jx, stg, zs -> 11896, and nothing behind
  const FastWant notails = {0, 3712, 7424, 7488, 7552, 7568, 7824, 7840, 7856, {9904, 10128, 10352}, {10368, 10592, 10816},
                            {10832, 10944}, {11056, 11168}, 11280, 11296, 11360, 11365, 11370, 11374, 11378, 11382, 11383, 11384,
                            11640, 11832, 11896, 12280, 11896, 13944, 13948, 11896, 11896, 11904, 11904, 11896, 11896};
  fast_ok("no tails", pm_fast_map(16, 232, 4, 1, 1, n14, 3, n14, 3, 0), notails, 16, 232, 4, 1, 1, n14, 3, n14, 3, 0, 0, 0, 8, 0, 0);

  // ---- hp alias: 64 rows (RT = 4), nets 1-5-5-1 tiles (5 = 4 + 1, yet no tails: RT = 4), LD = 136: 64 x 136 = 8704 >= 8 x 4 x 256
  // 2 x 8704 | 2 x 256 | 64 | 1024 | 64 | 64 -> 19136, no hp; biases 80 80 16 twice -> 19488; masks 160 x 4 -> 20128; zp 64,
  // zd 256, 24 -> 20472; jx 1024, stg 64 x 12 = 768, zs 256 -> 22520
  CHECK(pm_fast_hp_alias(64, 136, 4) && !pm_fast_hp_alias(64, 120, 4) && !pm_fast_hp_alias(32, 512, 2));
  const FastWant alias = {0, 8704, 17408, 17664, 17920, 17984, 19008, 19072, -1, {19136, 19216, 19296}, {19312, 19392, 19472},
                          {19488, 19648}, {19808, 19968}, 20128, 20192, 20448, 20453, 20458, 20462, 20466, 20470, 20471, 20472,
                          21496, 22264, 22520, 24056, 22520, 30712, 30716, 22520, 22520, 22528, 22528, 22520, 22520};
  fast_ok("hp alias", pm_fast_map(64, 136, 4, 1, 4, n5, 3, n5, 3, 0), alias, 64, 136, 4, 1, 4, n5, 3, n5, 3, 0, 0, 0, 8, 0, 0);
  // ... and LD = 120, 64 x 120 = 7680 < 8192: 2 x 7680 | ... -> 17088; hp 8192 -> 25280; -> 25632; -> 26272; -> 26616; -> 28664
  const FastWant noalias = {0, 7680, 15360, 15616, 15872, 15936, 16960, 17024, 17088, {25280, 25360, 25440}, {25456, 25536, 25616},
                            {25632, 25792}, {25952, 26112}, 26272, 26336, 26592, 26597, 26602, 26606, 26610, 26614, 26615, 26616,
                            27640, 28408, 28664, 30200, 28664, 36856, 36860, 28664, 28664, 28672, 28672, 28664, 28664};
  fast_ok("hp present at 64 rows", pm_fast_map(64, 120, 4, 1, 4, n5, 3, n5, 3, 0), noalias, 64, 120, 4, 1, 4, n5, 3, n5, 3, 0, 0, 0, 8, 0, 0);

  // ---- split precision (fp16 pieces): 16 rows, 1-13-13-1 tiles, LD = 240
  // 2 x 3840 | 128 | 16 | 256 | 32 -> 8112; hp -> 10160; biases -> 11024; masks -> 11440; -> 11544; -> 12056; xin 16 x 24 = 384,
  // ovf 4 -> 12444; no tails in split precision
  const FastWant split = {0, 3840, 7680, 7744, 7808, 7824, 8080, 8096, 8112, {10160, 10368, 10576}, {10592, 10800, 11008},
                          {11024, 11128}, {11232, 11336}, 11440, 11456, 11520, 11525, 11530, 11534, 11538, 11542, 11543, 11544,
                          11800, 11992, 12056, 12440, 12444, 14492, 14496, 12444, 12444, 12452, 12452, 12444, 12444};
  fast_ok("split precision", pm_fast_map(16, 240, 4, 1, 1, n13, 3, n13, 3, 0, 2), split, 16, 240, 4, 1, 1, n13, 3, n13, 3, 0, 2, 0, 8, 0, 0);

  // ---- split groups, <= 8 parts: 2 parts of a 30-row group, 3 steps, d = 4, the shape above: wave 0's scratch 136 -> 12580;
  // reference point 8 -> 12588; z table 2 x 3 x 2 x 4 = 48 floats -> 12636; two sets of 136 + 64 + 64 = 264 -> 13164
  // (8 + 48 + 528 = 584 = 0 mod 4); four blocks of 30 x 4 = 120 -> 13644
  FastWant parts = split;
  parts.xch = 12580; parts.xch_zt = 12588; parts.xch_sets = 12636; parts.rows = 13164; parts.total = 13644;
  {
    const PmFastMap m = pm_fast_map(16, 240, 4, 1, 1, n13, 3, n13, 3, 4, 2, 1, 30, 3);
    fast_ok("split groups, 2 parts", m, parts, 16, 240, 4, 1, 1, n13, 3, n13, 3, 4, 2, 0, 1, 30, 3);
    CHECK(pm_fast_xch_floats(16, 4, 3) == 584);
    CHECK(m.m.xch_zset == 64 && m.m.xch_set == 264 && m.m.xch_set_rows == 136 && m.m.rows_block == 120);
    CHECK(pm_mm_rows_block(m.m, 3) == 13164 + 360 && m.m.xch_sets + 1 * m.m.xch_zset == 12636 + 64 && pm_mm_xch_set(m.m, 1) == 12636 + 264);
    // LDS tiles: from the rows area's offset rounded up to 16 bytes, in place of the row blocks
    CHECK(m.m.tile_base == 13164);
  }
  // ---- split groups, > 8 parts: row blocks of 16 rows, 4 x 16 x 4 = 256 -> 13420
  parts.total = 13420;
  {
    const PmFastMap m = pm_fast_map(16, 240, 4, 1, 1, n13, 3, n13, 3, 4, 2, 1, 16, 3);
    fast_ok("split groups, > 8 parts", m, parts, 16, 240, 4, 1, 1, n13, 3, n13, 3, 4, 2, 0, 1, 16, 3);
    CHECK(m.m.rows_block == 64 && m.m.tile_base == 13164);
  }
  // ---- LDS tiles: 8 tiles of 14 loads of 256 floats, the last K32 block (2 pieces) of 32 lanes x 4 floats (13 hidden tiles:
  // 208 - 192 = 16 k-values = 2 k-blocks) or 64 lanes (14: 32 k-values); 12 x 256 + 2 x 128 = 3328 / 12 x 256 + 2 x 256 = 3584
  now = "LDS tiles";
  CHECK(pm_lds_tile_last_lanes(13) == 32 && pm_lds_tile_last_lanes(14) == 64);
  CHECK(pm_lds_tile_floats(14, 2, 32) == 3328 && pm_lds_tile_floats(14, 2, 64) == 3584);
  CHECK(pm_lds_tiles_bytes(13) == 106496 && pm_lds_tiles_bytes(14) == 114688);
  CHECK(pm_lds_tile_at(0, 13164, 3, 14, 2, 32) == 13164 + 9984);
  // (without split groups the tiles start behind everything: the total, which is a multiple of 4 floats)
  CHECK(pm_fast_map(16, 240, 4, 1, 1, n13, 3, n13, 3, 0, 2).m.tile_base == 12444);

  // ---- networks of different depth: policy 1-3-1 tiles, dynamics 1-3-3-3-1, D = 5, U = 2, 16 rows, LD = 56
  // 2 x 896 | 2 x 80 | 32 | 256 | 32 -> 2272; hp -> 4320; pbias 48 16, dbias 48 48 48 16 -> 4544; masks 24: one, three -> 4640;
  // zp 32, zd 80, mx / iSx 7, my / Sy / lSy 5, psc / pbi 2 -> 4785, rounded up to 4788; jx 256, stg 16 x 17 = 272, zs 80 -> 5396
  {
    const int p2[] = {1, 3, 1}, d4[] = {1, 3, 3, 3, 1};
    const FastWant depth = {0, 896, 1792, 1872, 1952, 1984, 2240, 2256, 2272, {4320, 4368}, {4384, 4432, 4480, 4528}, {4544},
                            {4568, 4592, 4616}, 4640, 4672, 4752, 4759, 4766, 4771, 4776, 4781, 4783, 4788, 5044, 5316, 5396,
                            5780, 5396, 7444, 7448, 5396, 5396, 5404, 5404, 5396, 5396};
    fast_ok("networks of different depth", pm_fast_map(16, 56, 5, 2, 1, p2, 2, d4, 4, 0), depth, 16, 56, 5, 2, 1, p2, 2, d4, 4, 0, 0, 0, 8, 0, 0);
  }

  // ---- general family: 16 rows, LD = 40 (no free columns for the partials: 40 - 48 < 0), D = 4, U = 1
  // 2 x 640 | 2 x 64 | 16 | 256 | 16 | 16 -> 1712; part 8 x 3 x 256 = 6144 -> 7856
  CHECK(!pm_part_alias_ok(16, 40, 1));
  for (int mm_d : {0, 4}) {      // ... and with moment matching in the sweep, d = 4: eight waves of 136 floats -> 8944
    now = mm_d ? "general, mm_d > 0" : "general, two buffers";
    const PmLdsMap m = pm_lds_map(0, 16, 40, 4, 1, 1, mm_d);
    regions_ok({{"bufA", (long)m.bufA, 0, 640, true}, {"bufB", (long)m.bufB, 640, 640, false}, {"xa", (long)m.xa, 1280, 64, false},
                {"xb", (long)m.xb, 1344, 64, false}, {"av", (long)m.av, 1408, 16, false}, {"gad", (long)m.gad, 1424, 256, false},
                {"rr", (long)m.rr, 1680, 16, false}, {"gr", (long)m.gr, 1696, 16, false}, {"part", m.has_part ? m.part : -1L, 1712, 6144, false},
                {"mm", (long)m.mm, 7856, mm_d ? 1088u : 0u, true}}, m.total, mm_d ? 8944 : 7856);
  }
  // ---- partials aliased: LD = 440, (440 - 48) & ~3 = 392 free columns, 16 x 392 = 6272 >= 6144
  // 2 x 7040 | 128 | 16 | 256 | 32 -> 14512, no part
  {
    now = "general, partials aliased";
    CHECK(pm_part_alias_w(440) == 392 && pm_part_alias_ok(16, 440, 1) && !pm_part_alias_ok(16, 424, 1));
    const PmLdsMap m = pm_lds_map(0, 16, 440, 4, 1, 1, 0);
    regions_ok({{"bufA", (long)m.bufA, 0, 7040, true}, {"bufB", (long)m.bufB, 7040, 7040, false}, {"xa", (long)m.xa, 14080, 64, false},
                {"xb", (long)m.xb, 14144, 64, false}, {"av", (long)m.av, 14208, 16, false}, {"gad", (long)m.gad, 14224, 256, false},
                {"rr", (long)m.rr, 14480, 16, false}, {"gr", (long)m.gr, 14496, 16, false}, {"part", m.has_part ? m.part : -1L, -1, 0, false},
                {"mm", (long)m.mm, 14512, 0, true}}, m.total, 14512);
  }
  // ---- in-place layers: 64 rows, LD = 520, ONE buffer 64 x 520 = 33280 | 2 x 256 | 64 | 1024 | 64 | 64 -> 35008; table 64 -> 35072
  {
    now = "general, in-place";
    const PmLdsMap m = pm_lds_map(0, 64, 520, 4, 1, 4, 0, true);
    CHECK(m.bufB == 0);
    regions_ok({{"bufA", (long)m.bufA, 0, 33280, true}, {"xa", (long)m.xa, 33280, 256, false}, {"xb", (long)m.xb, 33536, 256, false},
                {"av", (long)m.av, 33792, 64, false}, {"gad", (long)m.gad, 33856, 1024, false}, {"rr", (long)m.rr, 34880, 64, false},
                {"gr", (long)m.gr, 34944, 64, false}, {"tbl", (long)m.tbl, 35008, 64, false}, {"part", m.has_part ? m.part : -1L, -1, 0, false},
                {"mm", (long)m.mm, 35072, 0, true}}, m.total, 35072);
  }
  printf(failed ? "%d checks failed\n" : "lds map: all checks passed\n", failed);
  return failed;
}
