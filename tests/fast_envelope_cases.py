"""The envelope of the latency-optimised sweep family (csrc/pmbrl_fast.h, pmbrl_split.h, pmbrl_mm_w.h, the pm_xch_*
exchange; the host side's plan_layout / plan_groups / plain_row_tiles / LayoutCalc in csrc/pmbrl.hip) as a table of small
synthetic problems:

  tests/test_fast_envelope_cases.py  (CPU) every case is well conditioned -- the oracle's own fp32 run stays within a
                                     quarter of each bar of its fp64 run -- and the table's expectations together name
                                     every generic instance of the family (FAST_ROWS, SPLIT_ROWS below)
  tests/test_gpu_fast_envelope.py    (GPU) every case against the fp64 oracle in every arithmetic, on the family (plain
                                     call, call with optional outputs, step ranges) and on the general family

The arithmetic both tests judge with (oracle, global_errors, slice_errors, worst, BARS, SLICE_FLOOR, the saturation and
drift modifications of `problem`) is tests/reg_envelope_cases.py's, imported.

One axis varies per case around D = 4, U = 1, 2 x 96 hidden units, 40 rows, H = 5 (moment-matching cases: H = 4), plus
combined corners.  Cases are generated (prob_mbrl_amd.problem.synthetic_problem from a shape dictionary), nothing is
stored.  No case has two equal hidden layers of 193..208 units in both networks with D + U <= 8, so the
register-resident family takes none of them.

`expect` is what Engine.info must report, per arithmetic asked for, WRITTEN DOWN BY HAND from the rules of pmbrl.hip --
never from a run:

  * row tiles RT: rows_per_wg_hint >= 64 -> 4, >= 32 -> 2, else 1; halved while the LDS map of RT exceeds 160 KiB
    (plain_row_tiles).  64-row workgroups run in exact fp32 whatever was asked for (LayoutCalc::prec: the generic 64-row
    split instances are not compiled), so `precision` reads 'f32' there.
  * stage pair (CA, CB): among the pairs the arithmetic has for RT, in the order of pmbrl_instances.h, the first that
    minimises stream_work(m = CA + CB) = sum over the hidden -> hidden layers of both networks of
    nt_out * roundup(k_in, m) + nt_in * roundup(k_out, m), k = tiles (fp32) or ceil(tiles / 2) (split: K32 blocks).
    For equal hidden layers of n tiles:
      fp32, 16 rows   (2,2) n = 1..4, 9..12;  (4,4) n = 5..8;  (7,6) n = 13;  (8,8) n = 14..16
      fp32, 32 rows   (2,2) n = 1..4, 9..12;  (4,3) n = 5..7, 13, 14;  (4,4) n = 8, 15, 16
      fp32, 64 rows   (2,2) n = 3, 4, 7, 8, 11, 12, 15;  (1,1) n = 1, 2, 5, 6, 9, 10, 13, 14;  n = 16 does not fit:
                      LD = 264, two 64-row buffers 135 168 B, the whole map 164 068 B > 163 840 -> 32 rows.
                      (n = 15: the same LD, 163 296 B -- fits by 544 B.)
      split, 16 / 32  (4,3) n = 13, 14;  (1,1) otherwise
    One hidden layer: nothing is streamed, every pair ties, the first listed wins -- (8,8) / (4,4) / (2,2) in fp32 at
    16 / 32 / 64 rows, (4,3) on split operands.
  * moment matching (plan_groups): a whole number of groups in the first of 16 / 32 / 64 rows that holds one (mm_mode 1,
    rows_per_wg = floor(R / M) M); groups of more than 16 rows are split over the fewest 2..8 workgroups that bring a part
    to <= 16 rows (M <= 128; mm_parts, rows_per_wg = ceil(M / parts), n_wg = G parts) unless PMBRL_MM_PARTS=1; a group
    no form takes (M > 128) runs per step with the moment matching in the sweeps' prologue for D = 4..6 (mm_mode 3) -- as
    one launch with a device-wide barrier (mm_grid 1) when the workgroups fit the chip and PMBRL_MM_PERSTEP is unset --
    and between the launches otherwise (mm_mode 2).
"""
from tests.reg_envelope_cases import (BARS, SLICE_FLOOR, TOL_GRAD, TOL_TRAJ, DRIFT_DIM, global_errors, ids, oracle,  # noqa: F401
                                      problem, rel, saturation_shares, slice_errors, split_drift, worst)
import torch  # noqa: F401  (the envelope tests use it through this module)

# The generic instances of the family: (row tiles, CA, CB) of PM_FAST_CASES (exact fp32) and PM_SPLIT_CASES (both split
# arithmetics) in csrc/pmbrl_instances.h.  Each is compiled as LEAN, EXT and MM; the rt = 1 rows also as MMG (the
# device-wide-barrier form).  Every row is reached by some accepted shape: none is listed as unreachable.
FAST_ROWS = [(1, 8, 8), (1, 7, 6), (1, 4, 4), (1, 2, 2), (2, 4, 4), (2, 4, 3), (2, 2, 2), (4, 2, 2), (4, 1, 1)]
SPLIT_ROWS = [(1, 4, 3), (1, 1, 1), (2, 4, 3), (2, 1, 1)]
ROWS_OF = {'f32': FAST_ROWS, 'split_f16': SPLIT_ROWS, 'split': SPLIT_ROWS}

BOTH = ('split_f16', 'f32')
ALL3 = ('split_f16', 'f32', 'split')
WHOLE = (('PMBRL_MM_PARTS', '1'),)         # one workgroup per group
PERSTEP = (('PMBRL_MM_PERSTEP', '1'),)     # the per-step prologue form instead of the device-wide barrier


def _e(rt, rpw, nwg, f16, f32, mode=0, parts=1, grid=0):
    """expectation per arithmetic ASKED FOR: f16 / f32 are the stage pairs on split operands / in exact fp32"""
    out = {}
    for prec in ALL3:
        split = prec != 'f32' and rt < 4
        out[prec] = dict(fast=1, row_tiles=rt, rows_per_wg=rpw, n_wg=nwg, stages=f16 if split else f32,
                         precision=prec if split else 'f32', mm_mode=mode, mm_parts=parts, mm_grid=grid)
    return out


def _case(cid, seed, expect, pol=(96, 96), dyn=None, D=4, U=1, rows=40, groups=0, H=5, hint=0, env=(), precs=BOTH,
          mods=(), mm_rewards=None, reward=None):
    """rows: the batch; groups > 0: moment matching of the states in that many groups of rows / groups.  expect None: just
    outside the envelope (fast == 0)"""
    if reward is None:
        reward = {4: 'cartpole', 5: 'cartpole', 6: 'double_cartpole'}.get(D, 'generic') if U == 1 else 'generic'
    mm = groups > 0
    P = groups if mm else rows
    assert rows % P == 0
    cfg = dict(D=D, U=U, pol_hid=list(pol), dyn_hid=list(pol if dyn is None else dyn), P=P, S=rows // P, H=H, mm=mm,
               reward=reward, maxU={'cartpole': 10.0, 'double_cartpole': 20.0, 'generic': 2.0}[reward])
    if mm_rewards is not None:
        cfg['mm_rewards'] = mm_rewards
    return dict(id=cid, seed=seed, inside=expect is not None, hint=hint, precision=tuple(precs), mods=tuple(mods),
                env=tuple(env), expect=expect, cfg=cfg)


def _mm(cid, seed, expect, D, M, G, pol, H=4, **kw):
    return _case(cid, seed, expect, pol=pol, D=D, rows=M * G, groups=G, H=H, **kw)


def w(x, n=2):
    return (x,) * n


P11, P22, P43, P44, P76, P88 = (1, 1), (2, 2), (4, 3), (4, 4), (7, 6), (8, 8)

CASES = [
    _case('centre', 1, _e(1, 16, 3, P11, P44)),
    # ---- hidden width, equal layers, 16 rows: both ends of every band of the stage-pair table
    #      (1, 4 | 5, 8 | 9, 12 | 14, 16 tiles)
    _case('w16', 0, _e(1, 16, 3, P11, P22), pol=w(16)),
    _case('w64', 2, _e(1, 16, 3, P11, P22), pol=w(64)),
    _case('w80', 0, _e(1, 16, 3, P11, P44), pol=w(80)),        # 5 tiles: the K-split last tile (4 m + 1)
    _case('w128', 3, _e(1, 16, 3, P11, P44), pol=w(128)),
    _case('w144', 0, _e(1, 16, 3, P11, P22), pol=w(144)),      # 9 tiles: K-split, padded to 12 k-blocks
    _case('w192', 4, _e(1, 16, 3, P11, P22), pol=w(192)),
    _case('w224', 103, _e(1, 16, 3, P43, P88), pol=w(224)),
    _case('w256', 5, _e(1, 16, 3, P11, P88), pol=w(256)),
    # ... ragged last tiles
    _case('w1', 0, _e(1, 16, 3, P11, P22), pol=w(1)),
    _case('w17', 6, _e(1, 16, 3, P11, P22), pol=w(17)),
    _case('w65', 0, _e(1, 16, 3, P11, P44), pol=w(65)),
    _case('w100', 7, _e(1, 16, 3, P11, P44), pol=w(100)),      # 7 tiles: a half-empty K32 block on split operands
    _case('w113', 0, _e(1, 16, 3, P11, P44), pol=w(113)),
    _case('w129', 8, _e(1, 16, 3, P11, P22), pol=w(129)),
    _case('w177', 0, _e(1, 16, 3, P11, P22), pol=w(177)),
    _case('w209', 9, _e(1, 16, 3, P43, P88), pol=w(209), precs=ALL3),
    _case('w241', 0, _e(1, 16, 3, P11, P88), pol=w(241)),
    _case('w96-bf16', 10, _e(1, 16, 3, P11, P44), precs=('split',)),
    # 13 tiles without the compile-time shape (three hidden layers): the only tile count that takes (7,6)
    _case('w208x3', 0, _e(1, 16, 3, P43, P76), pol=w(208, 3)),
    # ... at 32 rows
    _case('w17-r32', 11, _e(2, 32, 2, P11, P22), pol=w(17), hint=32),
    _case('w100-r32', 0, _e(2, 32, 2, P11, P43), pol=w(100), hint=32),
    _case('w128-r32', 12, _e(2, 32, 2, P11, P44), pol=w(128), hint=32, precs=ALL3),
    _case('w177-r32', 0, _e(2, 32, 2, P11, P22), pol=w(177), hint=32),
    _case('w209-r32', 13, _e(2, 32, 2, P43, P43), pol=w(209), hint=32, precs=ALL3),
    _case('w256-r32', 0, _e(2, 32, 2, P11, P44), pol=w(256), hint=32),
    # ... at 64 rows (exact fp32 whatever is asked for); 16 tiles do not fit 64 rows and fall back to 32
    _case('w64-r64', 14, _e(4, 64, 1, P11, P22), pol=w(64), hint=64),
    _case('w80-r64', 0, _e(4, 64, 1, P11, P11), pol=w(80), hint=64),
    _case('w209-r64', 101, _e(4, 64, 1, P11, P11), pol=w(209), hint=64),
    _case('w225-r64', 0, _e(4, 64, 1, P11, P22), pol=w(225), hint=64),      # 15 tiles: 163 296 of 163 840 B
    _case('w241-r64', 16, _e(2, 32, 2, P11, P44), pol=w(241), hint=64),
    _case('w257-out', 0, None, pol=w(257)),                                   # 17 tiles
    # ---- unequal layers: the pair that minimises stream_work over both networks
    # (fp32, per network: stream_work 100 / 152 / 208 / 256 at m = 4 / 8 / 13 / 16)
    _case('u48-200', 17, _e(1, 16, 3, P11, P22), pol=(48, 200)),
    _case('u256-16', 0, _e(1, 16, 3, P11, P22), pol=(256, 16)),
    _case('u16-256', 18, _e(1, 16, 3, P11, P22), pol=(16, 256)),
    _case('u112-144', 0, _e(1, 16, 3, P11, P22), pol=(112, 144)),            # 7 and 9 tiles: fp32 156 / 184 at m = 4 / 8
    _case('pol64-dyn176-80', 19, _e(1, 16, 3, P11, P22), pol=(64, 64), dyn=(176, 80)),
    _case('pol64-dyn176-80-r32', 0, _e(2, 32, 2, P11, P22), pol=(64, 64), dyn=(176, 80), hint=32),
    # ---- depth
    _case('l1-80-112', 20, _e(1, 16, 3, P43, P88), pol=(80,), dyn=(112,)),   # nothing streamed: the first listed pair
    _case('l3-64-112-48', 0, _e(1, 16, 3, P11, P22), pol=(64, 112, 48)),
    _case('l4-48-96-32-64', 21, _e(1, 16, 3, P11, P22), pol=(48, 96, 32, 64)),
    _case('l7-32', 0, _e(1, 16, 3, P11, P22), pol=w(32, 7)),                 # PMBRL_MAX_LAYERS
    _case('l-pol1-dyn3', 22, _e(1, 16, 3, P11, P22), pol=(96,), dyn=(64, 64, 64)),
    _case('l-pol3-dyn1', 0, _e(1, 16, 3, P11, P22), pol=(64, 128, 64), dyn=(144,)),
    # ---- state and action widths: first-layer K <= 16, heads <= 16 outputs (pm_fast_net_ok, PM_HJ)
    _case('d1u1', 23, _e(1, 16, 3, P11, P44), D=1, U=1),
    _case('d8u8', 0, _e(1, 16, 3, P11, P44), D=8, U=8),
    _case('d8u1', 24, _e(1, 16, 3, P11, P44), D=8, U=1),
    _case('d1u8', 0, _e(1, 16, 3, P11, P44), D=1, U=8),
    _case('d7u2', 25, _e(1, 16, 3, P11, P44), D=7, U=2),
    _case('d9u1-out', 0, None, D=9, U=1),                                     # dynamics head 2 D = 18
    _case('d4u9-out', 26, None, D=4, U=9),                                    # policy head 2 U = 18
    # ---- rows: ragged last workgroup at every row-tile count
    _case('rows1', 0, _e(1, 16, 1, P11, P44), rows=1),
    _case('rows15', 27, _e(1, 16, 1, P11, P44), rows=15),
    _case('rows16', 0, _e(1, 16, 1, P11, P44), rows=16),
    _case('rows17', 28, _e(1, 16, 2, P11, P44), rows=17),
    _case('rows33', 0, _e(1, 16, 3, P11, P44), rows=33),
    _case('rows65', 29, _e(1, 16, 5, P11, P44), rows=65),
    _case('rows33-r32', 0, _e(2, 32, 2, P11, P43), rows=33, hint=32),
    _case('rows33-r64', 30, _e(4, 64, 1, P11, P11), rows=33, hint=64),
    _case('rows65-r32', 0, _e(2, 32, 3, P11, P43), rows=65, hint=32),
    _case('rows65-r64', 31, _e(4, 64, 2, P11, P11), rows=65, hint=64),
    # ---- horizon
    _case('h1', 0, _e(1, 16, 3, P11, P44), H=1),
    _case('h2', 32, _e(1, 16, 3, P11, P44), H=2),
    _case('h3', 0, _e(1, 16, 3, P11, P44), H=3),
    _case('h12', 33, _e(1, 16, 3, P11, P44), H=12),
    # ---- moment matching of the states: whole groups in a workgroup
    _mm('mm4-m5', 0, _e(1, 15, 2, P11, P44, 1), 4, 5, 6, w(112)),                        # three groups per workgroup
    _mm('mm4-m7', 34, _e(1, 14, 2, P11, P22, 1), 4, 7, 4, w(64)),
    _mm('mm4-m16', 0, _e(1, 16, 3, P11, P22, 1), 4, 16, 3, w(144), precs=ALL3),
    _mm('mm4-m8-hint8', 35, _e(1, 8, 4, P11, P88, 1), 4, 8, 4, w(256), hint=8),        # one group per workgroup on request
    _mm('mm4-m16-w224', 104, _e(1, 16, 2, P43, P88, 1), 4, 16, 2, w(224), precs=ALL3),
    _mm('mm4-m16-w208x3', 36, _e(1, 16, 2, P43, P76, 1), 4, 16, 2, w(208, 3)),
    _mm('mm5-m16', 0, _e(1, 16, 3, P11, P44, 1), 5, 16, 3, w(112)),
    _mm('mm6-m16', 37, _e(1, 16, 3, P11, P22, 1), 6, 16, 3, w(64)),
    # D = 2 and D = 8: whole groups stay inside the sweep (plan_groups asks nothing of D there), on the routines of
    # run-time width
    _mm('mm2-m16', 0, _e(1, 16, 3, P11, P44, 1), 2, 16, 3, w(112)),
    _mm('mm8-m16', 38, _e(1, 16, 3, P11, P22, 1), 8, 16, 3, w(144)),
    _mm('mm4-m16-norr', 0, _e(1, 16, 3, P11, P88, 1), 4, 16, 3, w(256), mm_rewards=False),
    # ---- groups split over workgroups, rows + flags form
    _mm('mm4-m17', 39, _e(1, 9, 4, P11, P44, 1, 2), 4, 17, 2, w(112)),                  # 9 + 8
    _mm('mm4-m25', 0, _e(1, 13, 6, P11, P22, 1, 2), 4, 25, 3, w(144), precs=ALL3),      # 13 + 12
    _mm('mm4-m50', 105, _e(1, 13, 8, P11, P88, 1, 4), 4, 50, 2, w(256)),                 # 13 + 13 + 13 + 11
    _mm('mm4-m100', 0, _e(1, 15, 7, P11, P22, 1, 7), 4, 100, 1, w(64)),                 # 6 x 15 + 10
    _mm('mm4-m128', 41, _e(1, 16, 8, P11, P44, 1, 8), 4, 128, 1, w(112)),               # the last size the form takes
    # ... M = 129 lies outside the split forms, not outside the family: the device-wide-barrier form, 9 workgroups
    _mm('mm4-m129-barrier', 0, _e(1, 16, 9, P11, P44, 3, 1, 1), 4, 129, 1, w(112)),
    _mm('mm5-m17', 42, _e(1, 9, 4, P11, P22, 1, 2), 5, 17, 2, w(144)),
    _mm('mm6-m25', 0, _e(1, 13, 4, P11, P88, 1, 2), 6, 25, 2, w(256)),
    _mm('mm6-m50', 43, _e(1, 13, 4, P11, P44, 1, 4), 6, 50, 1, w(112)),
    _mm('mm2-m25', 0, _e(1, 13, 4, P11, P22, 1, 2), 2, 25, 2, w(64)),                   # (D = 2, 8: split like any width)
    _mm('mm8-m25', 44, _e(1, 13, 4, P11, P44, 1, 2), 8, 25, 2, w(112)),
    _mm('mm4-m25-norr', 0, _e(1, 13, 4, P11, P44, 1, 2), 4, 25, 2, w(112), mm_rewards=False),
    # ---- PMBRL_MM_PARTS=1: one 32- or 64-row workgroup per group (64 rows: exact fp32)
    _mm('mm4-m25-whole-w64', 45, _e(2, 25, 2, P11, P22, 1), 4, 25, 2, w(64), env=WHOLE),
    _mm('mm4-m25-whole-w112', 0, _e(2, 25, 2, P11, P43, 1), 4, 25, 2, w(112), env=WHOLE),
    _mm('mm4-m25-whole-w144', 46, _e(2, 25, 2, P11, P22, 1), 4, 25, 2, w(144), env=WHOLE, precs=ALL3),
    _mm('mm4-m25-whole-w224', 0, _e(2, 25, 2, P43, P43, 1), 4, 25, 2, w(224), env=WHOLE, precs=ALL3),
    _mm('mm4-m25-whole-w256', 47, _e(2, 25, 2, P11, P44, 1), 4, 25, 2, w(256), env=WHOLE),
    _mm('mm4-m50-whole-w64', 0, _e(4, 50, 1, P11, P22, 1), 4, 50, 1, w(64), env=WHOLE),
    _mm('mm4-m50-whole-w80', 48, _e(4, 50, 1, P11, P11, 1), 4, 50, 1, w(80), env=WHOLE),
    _mm('mm4-m50-whole-w112', 0, _e(4, 50, 1, P11, P22, 1), 4, 50, 1, w(112), env=WHOLE),
    _mm('mm4-m50-whole-w144', 49, _e(4, 50, 1, P11, P11, 1), 4, 50, 1, w(144), env=WHOLE),
    _mm('mm6-m50-whole-w112', 0, _e(4, 50, 1, P11, P22, 1), 6, 50, 1, w(112), env=WHOLE),
    # ---- one group of 160 rows: the device-wide-barrier form (10 workgroups of 16 rows) ...
    _mm('mm4-b160-w112', 50, _e(1, 16, 10, P11, P44, 3, 1, 1), 4, 160, 1, w(112), precs=ALL3),
    _mm('mm4-b160-w144', 106, _e(1, 16, 10, P11, P22, 3, 1, 1), 4, 160, 1, w(144)),
    _mm('mm4-b160-w224', 102, _e(1, 16, 10, P43, P88, 3, 1, 1), 4, 160, 1, w(224), precs=ALL3),
    _mm('mm4-b160-w256', 0, _e(1, 16, 10, P11, P88, 3, 1, 1), 4, 160, 1, w(256)),
    _mm('mm4-b160-w208x3', 108, _e(1, 16, 10, P43, P76, 3, 1, 1), 4, 160, 1, w(208, 3)),
    _mm('mm6-b160-w112', 0, _e(1, 16, 10, P11, P44, 3, 1, 1), 6, 160, 1, w(112)),
    _mm('mm5-b160-w144', 53, _e(1, 16, 10, P11, P22, 3, 1, 1), 5, 160, 1, w(144)),
    # ... the per-step prologue form of the same group ...
    _mm('mm4-b160-perstep', 0, _e(1, 16, 10, P11, P44, 3, 1, 0), 4, 160, 1, w(112), env=PERSTEP),
    _mm('mm6-b160-perstep', 54, _e(1, 16, 10, P11, P44, 3, 1, 0), 6, 160, 1, w(112), env=PERSTEP),
    # ... and D = 3: outside the in-sweep forms, the sweeps run between the external moment-matching launches
    _mm('mm3-b160-external', 0, _e(1, 16, 10, P11, P44, 2, 1, 0), 3, 160, 1, w(112)),
    # ---- combined corners
    _mm('w113-mm6-m25-h2', 55, _e(1, 13, 4, P11, P44, 1, 2), 6, 25, 2, w(113), H=2),
    _case('u16-256-d8u8-rows17-h1', 0, _e(1, 16, 2, P11, P22), pol=(16, 256), D=8, U=8, rows=17, H=1),
    _mm('l7-mm4-m7', 56, _e(1, 14, 2, P11, P22, 1), 4, 7, 4, w(32, 7)),
    _case('w209-d7u2-rows33-r32-h2', 0, _e(2, 32, 2, P43, P43), pol=w(209), D=7, U=2, rows=33, hint=32, H=2),
    _case('mm5-m17-pol64-dyn176-80', 57, _e(1, 9, 4, P11, P22, 1, 2), pol=(64, 64), dyn=(176, 80), D=5, rows=34, groups=2, H=4),
    _mm('l4-mm4-b160', 0, _e(1, 16, 10, P11, P22, 3, 1, 1), 4, 160, 1, (48, 96, 32, 64)),
    _case('w241-rows65-r64-h3', 58, _e(2, 32, 3, P11, P44), pol=w(241), rows=65, hint=64, H=3),
]

# ---- saturation of the family's transcendentals (the modifications of tests/reg_envelope_cases.problem), on one plain
# case at width 112 and one split-group case (seeds drawn until the oracle's head values cover the range: the CPU test)
SAT_CASES = [
    _case('sat-tanh-w112', 70, _e(1, 16, 3, P11, P44), pol=w(112), rows=48, H=6, mods=('sat_policy',)),
    _mm('sat-tanh-mm4-m25', 60, _e(1, 13, 4, P11, P44, 1, 2), 4, 25, 2, w(112), H=6, mods=('sat_policy',)),
    _case('sat-logstd-w112-d4u3', 61, _e(1, 16, 3, P11, P44), pol=w(112), U=3, rows=48, H=6, mods=('sat_logstd',)),
    _mm('sat-logstd-mm4u3-m25', 62, _e(1, 13, 4, P11, P44, 1, 2), 4, 25, 2, w(112), H=6, U=3, mods=('sat_logstd',)),
]
# ---- a non-finite value mid horizon: state dimension 3, decoupled from both networks and the reward, drifts by 5e37 a
# step and overflows fp32 while step 6 computes x_7.  The family keeps 6 steps in either arithmetic: its first layers
# take their input tile in fp32 on split operands too (the map's `xin` region), the decoupled dimension meets only zero
# weights there, and the fp16 range check (pmbrl_fast.h: an activation beyond 65504 after the epilogue) sees hidden
# activations only -- so nothing reports before the non-finite state itself.
# (tests/test_gpu_full_size.py::test_device_detects_a_mid_horizon_failure_... pins the 6 on a recorded fixture.)
OVERFLOW_STEPS = 6
OVERFLOW_CASES = [
    _case('overflow-plain-w112', 63, _e(1, 16, 3, P11, P44), pol=w(112), H=12, mods=('drift',)),
    _mm('overflow-mm4-m25', 107, _e(1, 13, 4, P11, P22, 1, 2), 4, 25, 2, w(144), H=12, mods=('drift',)),
]

ALL_CASES = CASES + SAT_CASES + OVERFLOW_CASES
assert len({c['id'] for c in ALL_CASES}) == len(ALL_CASES)
assert 2 * sum(c['seed'] != 0 for c in ALL_CASES) >= len(ALL_CASES)

INSIDE = [c for c in CASES if c['inside']] + SAT_CASES
OUTSIDE = [c for c in CASES if not c['inside']]
# the adjoint in two step ranges: one plain case per row-tile count and the seven-layer one
RANGE_CASES = ('centre', 'w128-r32', 'w80-r64', 'l7-32')
# run twice, bit for bit: a split-group case and a barrier-form case (both exchange through HBM)
TWICE_CASES = ('mm4-m25', 'mm4-b160-w112')


def by_id(cid):
    return next(c for c in ALL_CASES if c['id'] == cid)


def pairs(cases):
    """(case, arithmetic) of every arithmetic a case runs in"""
    return [(c, p) for c in cases for p in c['precision']]


def pair_ids(cases):
    return ['%s-%s' % (c['id'], p) for c, p in pairs(cases)]


def form(case):
    """'plain' | 'mm' (moment matching inside one launch per sweep, or in the prologue of per-step launches: the MM
    instances) | 'barrier' (MMG) | 'external' (mm_mode 2: the EXT instances between moment-matching launches)"""
    e = case['expect']['f32']
    return {0: 'plain', 1: 'mm', 2: 'external', 3: 'barrier' if e['mm_grid'] else 'mm'}[e['mm_mode']]


def action_grad_norms(st):
    """oracle/adjoint_np.backward's per-step dL/da_t -> their row norms [H, B]"""
    import numpy as np
    return np.stack([np.linalg.norm(g, axis=1) for g in st['grad_actions']])


# A hidden unit whose pre-activation is zero to within fp32 rounding has its ReLU's side -- and with it that unit's whole
# contribution to the gradient, 1e-3 of it at these sizes -- decided by the order of additions: the forward results do not
# move, the gradient does, in any fp32 implementation (seen on the first draw of w209-r64: 8.4e-9 against a mean of
# 0.07; the general family on fp16 pieces took the other side from the fp64 oracle, gradient off by 9.6e-4).  A case must
# keep every unmasked pre-activation of both networks further from zero than the rounding of an fp32 dot product of the
# widest layer: unit roundoff 2^-24 = 6e-8 times sqrt(K = 256) = 16 -> 1e-6 of the layer's rms pre-activation.
RELU_MARGIN = 1e-6


def relu_margin(d, o64):
    """fp64 oracle run o64 of problem d -> (smallest |pre-activation| / rms pre-activation over the unmasked hidden units
    of both networks and every step, where)"""
    import numpy as np
    f = lambda k: np.asarray(d[k], dtype=np.float64)      # noqa: E731
    best = (np.inf, None)
    for t in range(o64['actions'].shape[0]):
        x, a = o64['states'][t].astype(np.float64), o64['actions'][t].astype(np.float64)
        for net, h in (('pol', x), ('dyn', (np.concatenate([x, a], 1) - f('dyn_mx')) * f('dyn_iSx'))):
            keep = f(net + '_keep')
            for i in range(int(d[net + '_n_layers']) - 1):
                v = h @ f('%s_W%d' % (net, i)).T + f('%s_b%d' % (net, i))
                m = f('%s_mask%d' % (net, i))
                m = m[t] if m.ndim == 3 else m
                rms = float(np.sqrt(np.mean(v * v)))
                live = np.abs(v)[m > 0]
                if live.size and live.min() / rms < best[0]:
                    best = (float(live.min() / rms), '%s layer %d step %d' % (net, i, t))
                h = np.where(v > 0, v, 0.0) * m / keep[i]
    return best
