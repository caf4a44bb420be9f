// The LDS maps of the two sweep families that carve their LDS at run time: ONE walk per family over the list of regions,
// in order.  On the host the walk runs on ints and returns every region's offset (floats from the LDS base) and the total:
// the launch's size (LayoutCalc::lds), the per-layer offsets in the kernel arguments (FastOff) and where the LDS-resident
// weight tiles go are read from it.  In a kernel the same walk runs on float* and returns the regions themselves
// (pm_fast_carve, pm_lds_carve, the moment-matching areas): the chain of pointer additions it has always been, which
// folds to immediates where the arguments are compile-time constants (the shape-specialised instances).  A new region is
// one more line of the walk.  Pure arithmetic, host compiler alone: tests/lds_map_check.cpp holds every branch to offsets
// worked out by hand.  (The register-resident family's map is the PR_LDS_* list of pmbrl_reg.h.)
#pragma once
#include <stddef.h>

#include "pmbrl.h"

#ifdef __HIPCC__
#define PM_HD __host__ __device__
#define PM_HD_FI __host__ __device__ __forceinline__      // (where a kernel's carve-up must fold into it)
#else
#define PM_HD
#define PM_HD_FI inline
#endif

#define PM_MAXL PMBRL_MAX_LAYERS      // (as pmbrl_dw.h)
#define PM_NW 8                 // waves per workgroup (two per SIMD), general family
#define PM_KS_NT 3              // max out tiles handled by the K-split GEMM (< PM_NW)
#define PF_NW 8                 // waves per workgroup of the latency-optimised family (pmbrl_fast.h)
#define PM_XIN_LD 24            // = 8 (mod 16): conflict-free ds_read_b128 of the MFMA B operand
#define PM_IP_NOFF 64           // in-place layers: narrow GEMM outputs at this column of the one activation buffer

// fp64 scratch of one wave's moment matching of d-wide rows (pm_mm_carve, pmbrl_mm.h), and wave w's in an area of them
PM_HD inline size_t pm_mm_scratch_doubles(int d) {
  return d > 0 ? (size_t)3 * d * d + 5 * d : 0;
}
PM_HD inline double* pm_mm_scratch_of(double* mm, int w, int d) { return mm + (size_t)w * pm_mm_scratch_doubles(d); }

// ---------------------------------------------------------------------------
// latency-optimised family (pmbrl_fast.h)
// ---------------------------------------------------------------------------
// Tile balance: tile ot runs on wave ot mod 8, i.e. SIMD ot mod 4.  A layer with 4m+1 output
// tiles (13 for a 200-wide layer) would put m+1 tiles on SIMD 0 and m on the others: the phase
// then lasts as long as SIMD 0's extra tile (+25 % at m = 3).  Instead the LAST tile of such a
// layer is K-split over all 8 waves (<= 2 k-blocks each, weights LDS-resident for the launch):
// every wave adds its partial tile to LDS at the START of the phase and bumps a counter; the
// last wave, which owns at most one regular tile, waits for the 8 partials after its tile,
// sums them in fixed order and runs the tile's normal epilogue before the phase barrier.
// (not with 64-row workgroups: LDS is the constraint there)
// (split-bf16 precision: the tiles are short enough that the imbalance costs less than the K-split's
// partial / gather round trip -- every tile is a regular tile there)
PM_HD constexpr bool pm_fast_ksplit(int n_ot, int RT, int prec = 0) {
  return !prec && RT < 4 && n_ot >= 5 && (n_ot % 4) == 1;
}
// LDS floats for the K-split tail weights of one sweep direction (bwd: transposed layers)
PM_HD inline size_t pm_fast_tail_floats(const int* pnt, int pnl, const int* dnt, int dnl,
                                        bool bwd, int RT, int prec = 0) {
  size_t n = 0;
  if (prec) return 0;
  for (int l = 1; l <= pnl - 2; ++l) {
    const int n_ot = bwd ? pnt[l] : pnt[l + 1], n_kb = bwd ? pnt[l + 1] : pnt[l];
    if (pm_fast_ksplit(n_ot, RT)) n += (size_t)n_kb * 256;
  }
  for (int l = 1; l <= dnl - 2; ++l) {
    const int n_ot = bwd ? dnt[l] : dnt[l + 1], n_kb = bwd ? dnt[l + 1] : dnt[l];
    if (pm_fast_ksplit(n_ot, RT)) n += (size_t)n_kb * 256;
  }
  return n;
}
// The partial head tiles are written while one activation buffer (the head's input) is being
// read and the other is dead: when that buffer is large enough they live there and cost no LDS.
PM_HD inline bool pm_fast_hp_alias(int R, int LD, int RT) {
  return RT >= 4 && (size_t)R * LD >= (size_t)PF_NW * RT * 256;   // only where LDS is the constraint (64-row workgroups)
}

// The moment-matching areas behind the other regions (mm: where they start).  Per-wave fp64 scratch for mm_waves waves
// (waves that do in-kernel moment matching at once = whole groups per workgroup, at most PF_NW; a split group: wave 0).
// Then, for a group split over workgroups (mm_group_rows: rows of a row block, 0: whole groups), what the statistics
// exchange keeps -- the reference point (8), the z standardisation [zm | zi] of every step of the launch, and two
// staging sets, alternating between steps, of what wave 1 fetches a step ahead while wave 0 works: the part's noise
// rows [R][d] (forward sweep, set s at xch_sets + s * xch_zset, formed in the kernel); scratch with the factor, the part's pre-mm rows and
// noise rows (adjoint, set s at xch_sets + s * xch_set) -- rounded up to 4 floats; then -- LAST, so that the
// LDS-resident weight tiles of the instances that never exchange rows can take its place (tile_base) -- four row
// blocks of the whole group for the rows + flags form.
// (P: what an offset is -- int, floats from an LDS base of 0, on the host; float*, the region itself, in a kernel, where
//  the walk then is the chain of pointer additions the compiler folds best)
template <class P>
struct PmMmAreasT {
  P mm;                             // scratch of wave w: mm + w * mm_wave floats (pm_mm_scratch_of on the doubles)
  P xch, xch_zt, xch_sets;          // reference point, z table (doubles), staging sets
  P rows;                           // block k of the rows + flags form: rows + k * rows_block
  P tile_base;                      // first 16-byte boundary at or behind `rows`: where LDS-resident tiles may start
  P total;
  size_t mm_wave;                   // floats of one wave's scratch
  int xch_zset;                     // floats of a forward staging set = of a block of the part's rows, [R][d]
  size_t xch_set;                   // floats of an adjoint staging set: scratch (xch_set_rows floats), then two such blocks
  size_t xch_set_rows;
  int rows_block;
};
typedef PmMmAreasT<int> PmMmAreas;
// floats of the statistics exchange's area: reference point, z table, two adjoint staging sets; a multiple of 4
// (= rows - xch below: the check's region list ends the second set where the row blocks start)
PM_HD inline size_t pm_fast_xch_set_floats(int R, int d) { return 2 * pm_mm_scratch_doubles(d) + 2 * (size_t)R * d; }
PM_HD inline size_t pm_fast_xch_floats(int R, int d, int steps) {
  const size_t n = 8 + 2 * (size_t)steps * 2 * d + 2 * pm_fast_xch_set_floats(R, d);
  return (n + 3) & ~(size_t)3;
}
// n doubles behind p
PM_HD inline int pm_skip_doubles(int p, size_t n) { return p + (int)(2 * n); }
PM_HD inline float* pm_skip_doubles(float* p, size_t n) { return (float*)((double*)p + n); }
template <class P>
PM_HD inline PmMmAreasT<P> pm_fast_mm_areas(P base, P mm, int R, int mm_d, int mm_waves, int mm_group_rows, int mm_steps) {
  PmMmAreasT<P> a;
  a.mm = mm;
  a.mm_wave = 2 * pm_mm_scratch_doubles(mm_d);
  a.xch = pm_skip_doubles(mm, (size_t)mm_waves * pm_mm_scratch_doubles(mm_d));
  a.xch_zt = a.xch + 8;
  a.xch_sets = pm_skip_doubles(a.xch_zt, (size_t)mm_steps * 2 * mm_d);
  a.xch_zset = R * mm_d;
  a.xch_set = pm_fast_xch_set_floats(R, mm_d);
  a.xch_set_rows = a.mm_wave;
  a.rows = a.xch + (mm_group_rows ? pm_fast_xch_floats(R, mm_d, mm_steps) : 0);
  a.rows_block = mm_group_rows * mm_d;
  a.tile_base = base + (((size_t)(a.rows - base) + 3) & ~(size_t)3);
  a.total = a.rows + 4 * (size_t)a.rows_block;
  return a;
}
// block k of the rows + flags form; staging set s of the adjoint (the forward sweep forms the base of its two sets of
// noise rows, [2][R][d] at xch_sets, itself: the one value whose place in the kernel its register allocation hangs on)
template <class P> PM_HD inline P pm_mm_rows_block(const PmMmAreasT<P>& a, int k) { return a.rows + k * a.rows_block; }
template <class P> PM_HD inline P pm_mm_xch_set(const PmMmAreasT<P>& a, int s) { return a.xch_sets + (size_t)s * a.xch_set; }

// The host's record of the walk below: every region's offset in floats from the LDS base (the kernels' record of the same
// walk is FastLds, pmbrl_fast.h: the regions themselves)
struct PmFastMap {
  static constexpr bool kLayers = true;
  int bufA, bufB, xa, xb, av, gad, rr, gr;
  int hp_off;                    // head / tail partial tiles [PF_NW][RT][64][4]: offset from bufA, or -1 when
                                 // they live in whichever activation buffer is idle (pm_fast_hp_alias)
  int base;                      // 0
  int pbias[PM_MAXL], dbias[PM_MAXL], pmask[PM_MAXL], dmask[PM_MAXL];   // per layer (FastOff)
  int zp, zd, mx, iSx, my, Sy, lSy, psc, pbi;
  int jx;                        // backward: dL/dx~ rows [R][16]
  int stg;                       // backward: staged per-row inputs of one step [R][1+2D+3U]
  int zs;                        // in-kernel moment matching: this step's noise rows [R][D]
  int xin, ovf;                  // split precision: fp32 input tile of the resident first layers [R][PM_XIN_LD],
                                 // range-overflow flag of the launch (4); no room taken in exact fp32
  int tp, tcnt, tw;              // K-split last tile: partial tiles [PF_NW][RT][64][4], arrival counter (4), the
                                 // LDS-resident weight k-blocks of those tiles; no room taken without such a tile
  int mm;                        // the moment-matching areas (4-float aligned) ...
  PmMmAreas m;                   // ... and what they hold
  int total;
};
// THE list of regions, in order.  M: the record it fills (PmFastMap: offsets, P = int, base 0; FastLds: pointers, P = float*);
// a field's type is the record's business.  (pnt / dnt: 16-wide tile counts of layer inputs / outputs, nl + 1 entries each)
template <class M, class P>
PM_HD_FI M pm_fast_walk(P base, int R, int LD, int D, int U, int RT, const int* pnt, int pnl, const int* dnt, int dnl,
                        int prec = 0) {
  M m{};
  P p = base;
  m.bufA = p; p += (size_t)R * LD;
  m.bufB = p; p += (size_t)R * LD;
  m.xa = p; p += (size_t)R * D;
  m.xb = p; p += (size_t)R * D;
  m.av = p; p += (size_t)R * U;
  m.gad = p; p += (size_t)R * 16;
  m.rr = p; p += R;
  m.gr = p; p += R;
  m.hp_off = -1;
  if (!pm_fast_hp_alias(R, LD, RT)) {
    m.hp_off = (int)(p - base);
    p += (size_t)PF_NW * RT * 256;
  }
  m.base = base;
  for (int l = 0; l < pnl; ++l) { if constexpr (M::kLayers) m.pbias[l] = p; p += (size_t)pnt[l + 1] * 16; }
  for (int l = 0; l < dnl; ++l) { if constexpr (M::kLayers) m.dbias[l] = p; p += (size_t)dnt[l + 1] * 16; }
  for (int l = 0; l < pnl - 1; ++l) { if constexpr (M::kLayers) m.pmask[l] = p; p += ((size_t)R * pnt[l + 1] + 1) / 2; }
  for (int l = 0; l < dnl - 1; ++l) { if constexpr (M::kLayers) m.dmask[l] = p; p += ((size_t)R * dnt[l + 1] + 1) / 2; }
  m.zp = p; p += (size_t)R * U;
  m.zd = p; p += (size_t)R * D;
  m.mx = p; p += D + U;
  m.iSx = p; p += D + U;
  m.my = p; p += D;
  m.Sy = p; p += D;
  m.lSy = p; p += D;
  m.psc = p; p += U;
  m.pbi = p; p += U;
  size_t n = ((size_t)(p - base) + 3) & ~(size_t)3;
  p = base + n;
  m.jx = p; p += (size_t)R * 16;
  m.stg = p; p += (size_t)R * (1 + 2 * D + 3 * U);
  m.zs = p; p += (size_t)R * D;
  n = ((size_t)(p - base) + 3) & ~(size_t)3;
  p = base + n;
  m.xin = p;
  m.ovf = (decltype(m.ovf))(p + (size_t)R * PM_XIN_LD);
  if (prec) p += (size_t)R * PM_XIN_LD + 4;
  {
    const size_t tf = pm_fast_tail_floats(pnt, pnl, dnt, dnl, false, RT, prec), tb = pm_fast_tail_floats(pnt, pnl, dnt, dnl, true, RT, prec);
    const size_t tw = tf > tb ? tf : tb;
    m.tp = p;
    m.tcnt = (decltype(m.tcnt))(p + (size_t)PF_NW * RT * 256);
    m.tw = p + (size_t)PF_NW * RT * 256 + 4;
    if (tw) p += (size_t)PF_NW * RT * 256 + 4 + tw;
  }
  m.mm = (decltype(m.mm))(p);
  return m;
}
// ... with the moment-matching areas behind it, and the total
PM_HD inline PmFastMap pm_fast_map(int R, int LD, int D, int U, int RT, const int* pnt, int pnl, const int* dnt, int dnl,
                                   int mm_d, int prec = 0, int mm_waves = PF_NW, int mm_group_rows = 0, int mm_steps = 0) {
  PmFastMap m = pm_fast_walk<PmFastMap>(0, R, LD, D, U, RT, pnt, pnl, dnt, dnl, prec);
  m.m = pm_fast_mm_areas(0, m.mm, R, mm_d, mm_waves, mm_group_rows, mm_steps);
  m.total = m.m.total;
  return m;
}

// LDS-resident weight tiles (pmbrl_fast.h, lds_tile_s): one tile per wave of a streamed layer of 13 or 14 hidden tiles on
// two fp16 pieces, a tile one stage pair of 7 K32 blocks = 14 loads of 1 KiB; of the last block only the lanes that hold
// real k-blocks are stored
PM_HD inline size_t pm_lds_tile_floats(int n_loads, int np, int last_lanes) {
  return (size_t)(n_loads - np) * 256 + (size_t)np * last_lanes * 4;
}
PM_HD inline int pm_lds_tile_last_lanes(int ht) { return 16 * ((16 * ht - 32 * 6) / 8); }
// bytes of the tile area for ht hidden tiles, and where wave w's tile starts
PM_HD inline size_t pm_lds_tiles_bytes(int ht) {
  return (size_t)PF_NW * pm_lds_tile_floats(14, 2, pm_lds_tile_last_lanes(ht)) * sizeof(float);
}
template <class P>
PM_HD inline P pm_lds_tile_at(P base, int tile_base, int w, int n_loads, int np, int last_lanes) {
  return base + tile_base + (size_t)w * pm_lds_tile_floats(n_loads, np, last_lanes);
}

// ---------------------------------------------------------------------------
// general family (pmbrl_rollout.h)
// ---------------------------------------------------------------------------
// Where the K-split GEMM's partial tiles live: a dedicated LDS region (`part`), or -- wide networks, where LDS is
// what limits the workgroups per CU -- the columns >= 16 * PM_KS_NT of the OUTPUT buffer's rows,
// which a narrow GEMM leaves untouched (element e of the region sits at row e / W, column 16 * PM_KS_NT + e % W with
// W = the free columns rounded down to 4).
PM_HD inline int pm_part_alias_w(int ld) { return (ld - 16 * PM_KS_NT) & ~3; }
PM_HD inline bool pm_part_alias_ok(int R, int ld, int RT) {
  const int w = pm_part_alias_w(ld);
  return w > 0 && (size_t)R * w >= (size_t)PM_NW * PM_KS_NT * RT * 256;
}

template <class P>
struct PmLdsMapT {
  P bufA, bufB, xa, xb, av, gad, rr, gr;
  P part;         // K-split partials [PM_NW][PM_KS_NT][RT][64][4]; has_part false: in the output buffer (aliased, in-place)
  bool has_part;
  P tbl;          // in-place layers: nibble -> multipliers (pmbrl_wide.h), 64 floats; no room taken otherwise
  P mm;           // per-wave fp64 scratch, PM_NW waves (4-float aligned)
  P total;
};
typedef PmLdsMapT<int> PmLdsMap;
// ip: in-place layers (gemm_layer_inplace_s) -- ONE activation buffer (bufB = bufA)
template <class P>
PM_HD inline PmLdsMapT<P> pm_lds_map(P base, int R, int LD, int D, int U, int RT, int mm_d, bool ip = false) {
  PmLdsMapT<P> m;
  m.bufA = base;
  m.bufB = ip ? m.bufA : m.bufA + (size_t)R * LD;
  m.xa = m.bufB + (size_t)R * LD;
  m.xb = m.xa + (size_t)R * D;
  m.av = m.xb + (size_t)R * D;
  m.gad = m.av + (size_t)R * U;
  m.rr = m.gad + (size_t)R * 16;      // (gad: action gradient, U <= 16)
  m.gr = m.rr + R;
  m.part = m.tbl = m.gr + R;
  size_t n = (size_t)(m.part - base);
  if (ip) n += 64;
  m.has_part = true;
  if (ip || pm_part_alias_ok(R, LD, RT)) m.has_part = false;
  else n += (size_t)PM_NW * PM_KS_NT * RT * 256;
  n = (n + 3) & ~(size_t)3;
  m.mm = base + n;
  m.total = m.mm + 2 * (size_t)PM_NW * pm_mm_scratch_doubles(mm_d);
  return m;
}
