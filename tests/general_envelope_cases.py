"""The envelope of the general sweep family (csrc/pmbrl_rollout.h, pmbrl_rollout_sweeps.h, the GEMMs of pmbrl_dev.h and
pmbrl_gsplit.h, the 512-wide layers of pmbrl_wide.h, the moment matching of pmbrl_mm.h and pmbrl_mm_wide.h; the host side's
plan_layout / plain_row_tiles / plan_groups in csrc/pmbrl.hip and pm_lds_map in csrc/pmbrl_lds_map.h) as a table of small
synthetic problems:

  tests/test_general_envelope_cases.py  (CPU) every case is well conditioned -- the oracle's own fp32 run stays within a
                                        quarter of each bar of its fp64 run --, the table's expectations together name
                                        every instance of PM_GENERAL_F32 / _SPLIT / _ACT_INSTANCES, and the LDS figures
                                        are those of pm_lds_map (tests/general_lds_check.cpp, host compiler alone)
  tests/test_gpu_general_envelope.py    (GPU) every case against the fp64 oracle in both arithmetics of the family

The arithmetic both tests judge with (oracle, global_errors, slice_errors, worst, BARS, SLICE_FLOOR, the saturation and
drift modifications of `problem`) is tests/reg_envelope_cases.py's, imported.  The modifications synthetic_problem has no
key for -- angle features, per-step masks, infer_ns, moment matching of the rewards alone, activations -- are made here
(`problem`), from a case's `extra`.

One axis varies per case around D = 12, U = 3, policy 2 x 272, dynamics model 3 x 272, 20 rows, H = 4 -- hidden layers
beyond 256 and a dynamics head beyond 16 outputs, which neither other family takes --, plus combined corners.  The
moment-matching cases, the 16 35x-row cases and a few others sit on networks the latency-optimised family would take and
ask for this family (`generic`: force_generic).  Cases are generated, nothing is stored.

`expect` is what Engine.info must report, per arithmetic asked for ('f32', 'split_f16': the family's two), from figures
WRITTEN DOWN BY HAND per case -- row tiles, rows per workgroup, the widest activation in 16-wide tiles, where the moment
matching runs, the in-place form -- never from a run.  LD, n_wg and lds_bytes are NOT per-case literals: `_ld` and `_lds`
below restate the three rules marked (*) in Python and work them out from the hand-written figures; the restatement is
held to pm_lds_map by tests/general_lds_check.cpp on the CPU and to Engine.info on the GPU.  The rules of pmbrl.hip:

  * the family takes what the others decline (plan_layout: fast = 0): force_generic, infer_ns, per-step masks, angle
    features, an activation other than ReLU, a network of fewer than two Linear layers, a first layer of more than 16
    inputs, a head of more than 16 outputs, a hidden layer of more than 256 units.
  * (*) LD (ld_generic), from the widest activation of either network, inputs and heads included, in tiles n:
    exact fp32 16 n + 8; split operands 16 n rounded up to 32, + 16.
  * row tiles RT without moment matching inside the sweep (plain_row_tiles): rows_per_wg_hint >= 64 -> 4, >= 32 -> 2,
    a hint of 0 -> 2 from (B + 31) / 32 >= 512 on, else 1; halved while the two-buffer map of RT exceeds 160 KiB.
    rows_per_wg = 16 RT, (*) n_wg = ceil(B / rows_per_wg).
  * in-place layers (split operands only, on request: hint >= 64) where RT came out below 4, no angle features, every
    layer ReLU, the widest activation <= 32 tiles, 2 D, 2 U, D + U <= 64 and the one-buffer map of 64 rows fits:
    RT = 4, inplace = 2 if every hidden layer of both networks is 512 wide (unless PMBRL_WIDE=0), else 1.
    (D <= 32 and U <= 16 are refused before any of this, so 2 D, 2 U and D + U never exceed 64 and a one-buffer map of
    <= 512-wide layers always fits: of the fall-backs to two buffers only "wider than 512" can be reached.)
  * moment matching (plan_groups, fast = 0): a whole number of groups in the first of 16 / 32 / 64 rows that holds a group
    of M rows AND whose two-buffer map with eight waves' scratch fits (mm_mode 1, rows_per_wg = floor(16 RT / M) M, or M
    times floor(hint / M) on request); otherwise between per-step launches (mm_mode 2, row tiles as without moment
    matching).  Which kernels do the per-step moment matching is not in Engine.info: for 6 < D <= 32, no infer_ns and
    pm_mmw_lds_bytes(M, D) <= 160 KiB the multi-wave pm_mmw_* kernels, the one-wave routines otherwise (beyond 64 rows
    they walk the rows in strides).  MM_PER_STEP_WIDE below says which, by hand, for every case that runs per step;
    tests/general_mmw_check.cpp evaluates pm_mmw_ok for those (M, D, infer_ns) on the CPU (nothing reports it on the GPU).
  * (*) lds_bytes (pm_lds_map), R = 16 RT rows:  floats = nbuf R LD + R (2 D + U + 18), nbuf = 2, or 1 in place;
    + 64 in place; + 6144 RT for the K-split partials unless in place or R ((LD - 48) & ~3) >= 6144 RT (they then live in
    the output buffer's free columns); rounded up to 4;  bytes = 4 floats + 64 (3 d^2 + 5 d) with d = D under mm_mode 1.
    The centre in fp32: LD = 280, 2 x 16 x 280 + 16 x 45 + 6144 = 15 824 floats = 63 296 B.
  * the instance (resolve_sweeps): exact fp32 pm_rollout_fwd<RT, 0, 0, false>; split operands <RT, 2, form, false> with
    form = inplace, or 3 where inplace = 2 and the policy has a 512 x 512 layer (its stashes are then pre-split for the
    dW GEMM: pm_dw_plan_blocks); a plan with an activation other than ReLU <RT, planes, 0, true>.

What the table cannot reach, and why: 65 input features, D + U = 64 and 2 D = 66 (D <= 32, U <= 16 and at most 8 angle
features: 56 is the widest input).  The mixture and learned-reward heads and the span form keep their own suites."""
import numpy as np

from tests.reg_envelope_cases import (BARS, SLICE_FLOOR, TOL_GRAD, TOL_TRAJ, DRIFT_DIM, global_errors, ids, oracle,  # noqa: F401
                                      rel, saturation_shares, slice_errors, split_drift, worst)
from tests.reg_envelope_cases import problem as _base_problem
from tests.fast_envelope_cases import RELU_MARGIN, action_grad_norms  # noqa: F401

# The instances of the family (csrc/pmbrl_instances.h), as (list, row tiles, third template argument): exact fp32 by row
# tiles; split operands by row tiles and form (0 two buffers, 1 / 2 in place, 3 = 2 on pre-split stashes); the networks
# that are not ReLU by row tiles and piece planes.  Every one is reached by some accepted shape: none is unreachable.
GENERAL_F32 = [('f32', 1, 0), ('f32', 2, 0), ('f32', 4, 0)]
GENERAL_SPLIT = [('split', 1, 0), ('split', 2, 0), ('split', 4, 0), ('split', 4, 1), ('split', 4, 2), ('split', 4, 3)]
GENERAL_ACT = [('act', 1, 0), ('act', 2, 0), ('act', 4, 0), ('act', 1, 2), ('act', 2, 2), ('act', 4, 2)]
INSTANCES = GENERAL_F32 + GENERAL_SPLIT + GENERAL_ACT

BOTH = ('split_f16', 'f32')
F16 = ('split_f16',)
F32 = ('f32',)
NOWIDE = (('PMBRL_WIDE', '0'),)
LDS_CAP = 160 * 1024
RELU, TANH, SILU = 0, 1, 2      # prob_mbrl_amd.activations


def _ld(n, prec):
    return 16 * n + 8 if prec == 'f32' else (16 * n + 31) // 32 * 32 + 16


def _lds(R, LD, D, U, RT, mmd=0, ip=False):
    """the lds_bytes rule of the docstring"""
    n = (1 if ip else 2) * R * LD + R * (2 * D + U + 18)
    if ip:
        n += 64
    elif R * ((LD - 48) & ~3) < 6144 * RT:
        n += 6144 * RT
    n = (n + 3) & ~3
    return 4 * n + 64 * (3 * mmd * mmd + 5 * mmd)


def _e(D, U, rows, n, f32, f16=None, form=0, act=False, precs=BOTH):
    """f32, f16: (row tiles, rows per workgroup, mm_mode, inplace) as written down for the case in exact fp32 / on split
    operands (f16 None: the same, two buffers); n: tiles of the widest activation; form: the split instance's third
    template argument (the in-place form, 3 on pre-split stashes)"""
    out = {}
    for prec, v in (('f32', f32), ('split_f16', f16 if f16 is not None else f32)):
        if prec not in precs:
            continue
        rt, rpw, mode, ip = (tuple(v) + (0, 0))[:4]
        LD = _ld(n, prec)
        out[prec] = dict(fast=0, reg=0, row_tiles=rt, rows_per_wg=rpw, n_wg=-(-rows // rpw), LD=LD,
                         lds_bytes=_lds(16 * rt, LD, D, U, rt, D if mode == 1 else 0, ip != 0), inplace=ip, mm_mode=mode,
                         precision=prec)
        assert prec == 'split_f16' or ip == 0
        out[prec]['_inst'] = (('act', rt, 0 if prec == 'f32' else 2) if act else
                              ('f32', rt, 0) if prec == 'f32' else ('split', rt, form if ip else 0))
    return out


CENTRE = dict(pol=(272, 272), dyn=(272, 272, 272), D=12, U=3, rows=20, H=4)


def _case(cid, seed, f32, f16=None, n=17, form=0, hint=0, env=(), precs=BOTH, mods=(), generic=False, groups=0,
          mm_rewards=None, reward=None, z_orth=False, refused=None, **kw):
    """rows: the batch; groups > 0: moment matching in that many groups of rows / groups; n: tiles of the widest
    activation; extra keys (pol_ang, dyn_ang, pol_step_masks, dyn_step_masks, infer_ns, no_mm_states, pol_act, dyn_act,
    pol_acts, dyn_acts):
    see `problem`.  refused: (code, part of the message) of a case plan creation must refuse"""
    shape = dict(CENTRE)
    extra = {k: kw.pop(k) for k in list(kw) if k not in shape}
    shape.update(kw)
    D, U, rows, H = shape['D'], shape['U'], shape['rows'], shape['H']
    if reward is None:
        reward = {4: 'cartpole', 6: 'double_cartpole'}.get(D, 'generic') if U == 1 else 'generic'
    mm = groups > 0
    P = groups if mm else rows
    assert rows % P == 0
    cfg = dict(D=D, U=U, pol_hid=list(shape['pol']), dyn_hid=list(shape['dyn']), P=P, S=rows // P, H=H, mm=mm, reward=reward,
               maxU={'cartpole': 10.0, 'double_cartpole': 20.0, 'generic': 2.0}[reward])
    if mm_rewards is not None:
        cfg['mm_rewards'] = mm_rewards
    if z_orth:
        cfg['z_orth'] = True
    act = bool(extra.get('pol_act') or extra.get('dyn_act') or extra.get('pol_acts') or extra.get('dyn_acts'))
    expect = None if refused else _e(D, U, rows, n, f32, f16, form, act, precs)
    return dict(id=cid, seed=seed, inside=refused is None, refused=refused, hint=hint, precision=tuple(precs),
                mods=tuple(mods), env=tuple(env), expect=expect, cfg=cfg, generic=generic, extra=extra)


def w(x, n=2):
    return (x,) * n


R16, R32, R64 = (1, 16), (2, 32), (4, 64)
IP1, IP2 = (4, 64, 0, 1), (4, 64, 0, 2)
SMALL = dict(pol=(32, 32), dyn=(32, 32), D=4, U=1)      # the latency-optimised family's shape: `generic` asks for this one


def _mm(cid, seed, D, M, G, f32, f16=None, n=2, H=4, **kw):
    """G groups of M rows on 2 x 32 networks with one action; f32 / f16: (row tiles, rows per workgroup, mm_mode)"""
    shape = dict(SMALL, D=D)
    shape.update(kw)
    return _case(cid, seed, f32, f16, n=n, rows=M * G, groups=G, H=H, generic=True, **shape)


CASES = [
    # the widest activation is a 272-wide layer: 17 tiles, LD = 280 / 304; 20 rows in two 16-row workgroups
    _case('centre', 1, R16),
    # ---- hidden width, equal layers in both networks, 16 rows.  gemm_tiles: the branch-free group form at a multiple of
    # 8 k-blocks (384 = 24, 512 = 32 tiles), the general form otherwise; ragged last groups of output tiles
    _case('w257', 0, R16, n=17, pol=w(257), dyn=w(257)),            # 17 tiles, the last one column wide
    _case('w258', 2, R16, n=17, pol=w(258), dyn=w(258)),
    _case('w384', 0, R16, n=24, pol=w(384), dyn=w(384)),            # split: LD = 400, the partials in a region of their own
    _case('w385', 101, R16, n=25, pol=w(385), dyn=w(385)),            # 25 tiles: a half-empty K32 block; split LD = 432
    _case('w400', 0, R16, n=25, pol=w(400), dyn=w(400)),
    # the partials' aliasing boundary 16 ((LD - 48) & ~3) >= 6144, i.e. LD >= 432: fp32 LD = 424 (26 tiles) against 440
    # (27); split 432 (25 or 26 tiles: aliased) against 400 (w384 above)
    _case('w416', 4, R16, n=26, pol=w(416), dyn=w(416)),
    _case('w432', 0, R16, n=27, pol=w(432), dyn=w(432)),
    _case('w512', 5, R16, n=32, pol=w(512), dyn=w(512)),
    _case('w513', 0, R16, n=33, pol=w(513), dyn=w(513)),
    # gemm_tiles_s: four tiles at once for an input of at most two K32 blocks (64 wide), the ring beyond
    _case('in64', 101, R16, pol=(64, 272), dyn=(64, 272, 272)),
    _case('in65', 0, R16, pol=(65, 272), dyn=(65, 272, 272)),
    # the widest network two 16-row buffers hold: D = 4, U = 1, 32 LD + 16 x 27 <= 40 960 floats (partials aliased)
    # -> LD <= 1266: 78 tiles in either arithmetic (fp32 1256, split 1264); 79 tiles (1272 / 1296) are refused
    _case('w1248', 102, R16, n=78, pol=w(1248), dyn=w(1248), D=4, U=1, H=2),
    _case('w1249-refused', 0, None, pol=w(1249), dyn=w(1249), D=4, U=1, H=2, refused=(-3, 'LDS')),
    # ---- unequal layers, in each network separately: transposed adjoint layers, K-permuted weight packing
    _case('pol-48-512-32', 8, R16, n=32, pol=(48, 512, 32)),
    _case('pol-400-16-288', 0, R16, n=25, pol=(400, 16, 288)),
    _case('dyn-48-512-32', 9, R16, n=32, dyn=(48, 512, 32)),
    _case('dyn-400-16-288', 0, R16, n=25, dyn=(400, 16, 288)),
    # two adjacent policy layers of 128 .. 208 units: on split operands the dW GEMM of the 160 -> 192 layer is the
    # whole-layer kernel (pm_dw_plan_blocks: layer13, at most 13 x 13 tiles)
    _case('pol-160-192', 64, R16, pol=(160, 192)),
    # ---- depth (net_plan: 1 .. 8 Linear layers per network)
    _case('l1', 10, R16, pol=(272,), dyn=(272,)),
    _case('l3', 0, R16, pol=w(272, 3), dyn=w(272, 3)),
    _case('l7', 11, R16, pol=w(272, 7), dyn=w(272, 7), H=3),
    _case('l-pol1-dyn3', 0, R16, pol=(272,)),
    _case('l-pol3-dyn1', 12, R16, pol=w(272, 3), dyn=(272,)),
    # no hidden layer at all: the linear policy (widest activation: the dynamics model's), a linear dynamics model, both
    # (widest: the 24-wide dynamics head, 2 tiles)
    _case('l0-pol', 13, R16, pol=()),
    _case('l0-dyn', 0, R16, dyn=()),
    _case('l0-both', 14, R16, n=2, pol=(), dyn=()),
    # ---- state, action and input widths.  Heads: gemm_narrow K-splits <= 3 output tiles (2 D, 2 U <= 48) and tile-splits
    # beyond; the first layers' adjoints (D, D + U wide) likewise
    _case('d1', 0, R16, D=1),
    _case('d16', 15, R16, D=16),
    _case('d17', 0, R16, D=17),
    _case('d24', 16, R16, D=24),                                    # 2 D = 48: the last K-split head
    _case('d25', 0, R16, D=25),                                     # 2 D = 50: tile-split
    _case('d32', 17, R16, D=32),
    _case('u1', 0, R16, U=1),
    _case('u8', 18, R16, U=8),
    _case('u9', 0, R16, U=9),
    _case('u16', 19, R16, U=16),
    _case('d32u16', 0, R16, D=32, U=16),                            # D + U = 48
    _case('d33-refused', 20, None, D=33, refused=(-2, 'D <= 32')),
    _case('u17-refused', 0, None, U=17, refused=(-2, 'U <= 16')),
    _case('l9-refused', 21, None, refused=(-2, 'n_layers')),        # (the test sets n_layers = 9 in the C configuration)
    # ---- angle features: [others | sin | cos], first layers and input normalisation of the expanded width
    _case('ang-pol', 22, R16, pol_ang=(2,)),
    _case('ang-dyn', 101, R16, dyn_ang=(0, 11)),                      # an angle at dimension 0 and at D - 1
    _case('ang-both', 23, R16, pol_ang=(0,), dyn_ang=(11, 5)),
    _case('ang-in49', 0, R16, D=32, U=9, dyn_ang=(0, 4, 8, 12, 16, 20, 24, 31)),       # 32 + 9 + 8 = 49: four input tiles
    _case('ang-in56', 24, R16, D=32, U=16, pol_ang=(31, 0), dyn_ang=(1, 3, 5, 7, 9, 11, 13, 15)),   # the widest input there is
    # ---- rows: a ragged last workgroup at every row-tile count.  A hint of 64: two 64-row buffers of LD = 280 / 304 do
    # not fit (35 840 + 2880 + 24 576 floats), two 32-row ones do (17 920 + 1440 + 12 288 = 31 648; split 33 184) -- fp32
    # stays there, split operands take the in-place form (64 x 304 + 2880 + 64 = 22 400 floats)
    _case('rows1', 0, R16, rows=1),
    _case('rows15', 25, R16, rows=15),
    _case('rows16', 0, R16, rows=16),
    _case('rows17', 26, R16, rows=17),
    _case('rows77', 102, R16, rows=77),
    _case('rows1-r32', 27, R32, rows=1, hint=32),
    _case('rows15-r32', 0, R32, rows=15, hint=32),
    _case('rows16-r32', 28, R32, rows=16, hint=32),
    _case('rows17-r32', 0, R32, rows=17, hint=32),
    _case('rows77-r32', 102, R32, rows=77, hint=32),
    _case('rows1-r64', 0, R32, IP1, form=1, rows=1, hint=64),
    _case('rows15-r64', 30, R32, IP1, form=1, rows=15, hint=64),
    _case('rows16-r64', 0, R32, IP1, form=1, rows=16, hint=64),
    _case('rows17-r64', 31, R32, IP1, form=1, rows=17, hint=64),
    _case('rows77-r64', 102, R32, IP1, form=1, rows=77, hint=64),
    # 64-row workgroups on two buffers: 2 x 64 narrow enough (LD = 72 / 80: 9216 + 2880 + 24 576 = 36 672 floats; 37 696)
    _case('w64-r64', 32, R64, n=4, pol=w(64), dyn=w(64), rows=77, hint=64, generic=True),
    # 32 rows by default from (B + 31) / 32 >= 512 on: B = 16 353 (16 352: 511)
    _case('rows16352', 0, R16, n=2, pol=(32,), dyn=(32,), D=4, U=1, rows=16352, H=2, generic=True),
    _case('rows16353', 33, R32, n=2, pol=(32,), dyn=(32,), D=4, U=1, rows=16353, H=2, generic=True),
    # ---- horizon
    _case('h1', 0, R16, H=1),
    _case('h2', 34, R16, H=2),
    _case('h3', 0, R16, H=3),
    _case('h5', 35, R16, H=5),                                      # (the step-range test's)
    _case('h12', 36, R16, H=12),
    # ---- per-step masks [H, B, h]
    _case('masks-pol', 0, R16, pol_step_masks=True),
    _case('masks-dyn', 37, R16, dyn_step_masks=True),
    _case('masks-both', 38, R16, pol_step_masks=True, dyn_step_masks=True),
    # ---- activations: one point per row of PM_GENERAL_ACT_INSTANCES (no in-place form: split stays at 32 rows too)
    _case('act-tanh-silu', 0, R16, pol_act=TANH, dyn_act=SILU),
    _case('act-silu-relu-r32', 39, R32, pol_act=SILU, rows=77, hint=32),
    _case('act-relu-tanh-w64-r64', 40, R64, n=4, pol=w(64), dyn=w(64), dyn_act=TANH, rows=77, hint=64),
    _case('act-tanh-r64', 0, R32, pol_act=TANH, dyn_act=TANH, rows=77, hint=64),
    # ... and one code per hidden layer (PMBRL_ACT_PER_LAYER): the per-layer dispatch of the ACT instances at 16 rows on
    # the centre, at 32 rows on ragged 258-wide layers, at 64 rows
    _case('act-layers', 62, R16, pol_acts=(TANH, RELU), dyn_acts=(SILU, TANH, RELU)),
    _case('act-layers-w258-r32', 63, R32, pol=w(258), dyn=w(258, 3), pol_acts=(RELU, SILU), dyn_acts=(TANH, RELU, SILU),
          rows=77, hint=32),
    _case('act-layers-w64-r64', 0, R64, n=4, pol=w(64), dyn=w(64), pol_acts=(SILU, TANH), dyn_acts=(RELU, TANH), rows=77, hint=64),
]

# ---- the in-place forms: split operands, a hint of 64, 64-row workgroups on one buffer.  gemm_layer_inplace_s runs 1 / 2 /
# 4 tiles per wave for <= 8 / <= 16 / <= 32 output tiles: 96 (6), 128 (8) | 129 (9), 256 (16) | 257 (17), 500, 512 (32)
IP_CASES = [
    _case('ip1-96-500-128', 41, IP1, IP1, n=32, form=1, pol=(96, 500, 128), dyn=(129, 256, 257, 512), rows=77, hint=64, precs=F16),
    _case('ip1-d32u16', 0, IP1, IP1, n=32, form=1, pol=(500, 96), dyn=(256, 129, 512), D=32, U=16, rows=65, hint=64, precs=F16),   # 2 D = 64
    # a 513-wide layer (33 tiles, LD = 560): two buffers -- 64 rows do not fit, 32 do (35 840 + 1440, partials aliased)
    _case('ip0-513', 42, R32, R32, n=33, pol=(513, 96), rows=77, hint=64, precs=F16),
    # every hidden layer 512 wide: the layers of pmbrl_wide.h -- <4, 2, 3> where the policy has a 512 x 512 layer (every
    # 512-wide stash pre-split for the dW GEMM), <4, 2, 2> where its one hidden layer has none; PMBRL_WIDE=0: <4, 2, 1>
    _case('ip2-512x3', 0, IP2, IP2, n=32, form=3, pol=w(512, 3), dyn=w(512, 3), rows=77, hint=64, precs=F16),
    # D = 32, U = 16: the policy's first layer has two input tiles and its head two output tiles -- the pre-split narrow dW
    # kernel's second form (pm_dw_narrow_pre_kernel<2>) on both sides of the 512 x 512 layer
    _case('ip2-512x2-d32u16', 101, IP2, IP2, n=32, form=3, pol=w(512), dyn=w(512), D=32, U=16, rows=65, hint=64, precs=F16),
    _case('ip1-512x3-nowide', 101, IP1, IP1, n=32, form=1, pol=w(512, 3), dyn=w(512, 3), rows=77, hint=64, env=NOWIDE, precs=F16),
    _case('ip2-512x1', 0, IP2, IP2, n=32, form=2, pol=(512,), dyn=(512,), rows=77, hint=64, precs=F16),
    _case('ip2-pol1-dyn3', 101, IP2, IP2, n=32, form=2, pol=(512,), dyn=w(512, 3), D=32, U=1, rows=65, hint=64, precs=F16),   # D + U = 33: 3 input tiles
]

# ---- moment matching in this family, on 2 x 32 networks (`generic`).  Two 16-row buffers of LD = 40 (48 on split operands)
# and the partials' region: 5 KiB + 24 KiB; at 32 / 64 rows 10 + 48 / 20 + 96 KiB -- plus 64 (3 D^2 + 5 D) bytes of scratch
MM_CASES = [
    _mm('mm1-m2', 45, 1, 2, 8, (1, 16, 1)),                                     # eight groups per workgroup
    _mm('mm4-m16', 0, 4, 16, 3, (1, 16, 1)),
    _mm('mm4-m7-hint7', 46, 4, 7, 4, (1, 7, 1), hint=7),                        # one group per workgroup on request (default: two)
    _mm('mm4-m17', 0, 4, 17, 2, (2, 17, 1)),
    _mm('mm4-m32', 47, 4, 32, 2, (2, 32, 1)),
    _mm('mm6-m33', 0, 6, 33, 2, (4, 33, 1)),
    _mm('mm4-m64', 48, 4, 64, 2, (4, 64, 1)),
    _mm('mm4-m16-states-only', 0, 4, 16, 3, (1, 16, 1), mm_rewards=False),
    _mm('mm4-m16-rewards-only', 49, 4, 16, 3, (1, 16, 1), no_mm_states=True),
    _mm('mm4-m16-infer-ns', 50, 4, 16, 3, (1, 16, 1), infer_ns=True),           # (mm4-m16 is the same problem without)
    _mm('mm4-m65-infer-ns', 0, 4, 65, 2, (1, 16, 2), infer_ns=True),
    _mm('mm7-m65-infer-ns', 66, 7, 65, 1, (1, 16, 2), infer_ns=True, reward='generic'),   # infer_ns keeps D = 7 off the multi-wave kernels
    # the largest D whose eight-wave scratch fits beside a 32-row workgroup (groups of 32 rows, z_orth: D close to M).
    # The widest activation is the 2 D-wide head, 3 tiles: LD = 56 / 80.
    # fp32:  4 (64 x 56 + 32 (2 D + 19)) + 49 152 + 64 (3 D^2 + 5 D) = 162 688 at D = 21, 171 520 at D = 22
    # split: 4 (64 x 80 + 32 (2 D + 19)) + ...                       = 160 384 at D = 20, 168 832 at D = 21
    # -- and a group that fits no workgroup goes to the per-step multi-wave kernels (6 < D <= 32)
    _mm('mm20-m32', 51, 20, 32, 2, (2, 32, 1), n=3, reward='generic', z_orth=True),
    _mm('mm21-m32', 0, 21, 32, 2, (2, 32, 1), (1, 16, 2), n=3, reward='generic', z_orth=True),
    _mm('mm22-m32', 52, 22, 32, 2, (1, 16, 2), n=3, reward='generic', z_orth=True),
    # per-step forms.  Multi-wave kernels at D = 7, 16, 32 ...
    _mm('mm7-m200', 0, 7, 200, 1, (1, 16, 2), reward='generic'),
    _mm('mm16-m80', 53, 16, 80, 2, (1, 16, 2), reward='generic', z_orth=True),
    # ... both sides of their LDS bound at D = 32: 8 x 6880 + 12 x 32 M <= 163 840 -> M <= 283; M = 284 runs on the
    # one-wave routines (4-tile head: LD = 72 / 80)
    _mm('mm32-m283', 0, 32, 283, 1, (1, 16, 2), n=4, H=2, reward='generic', z_orth=True),
    _mm('mm32-m284', 54, 32, 284, 1, (1, 16, 2), n=4, H=2, reward='generic', z_orth=True),
    # ... the one-wave routines at D = 4 and 6, rows walked in strides
    _mm('mm4-m65', 0, 4, 65, 2, (1, 16, 2)),
    _mm('mm4-m200', 55, 4, 200, 1, (1, 16, 2)),
    _mm('mm6-m65', 0, 6, 65, 1, (1, 16, 2)),
    _mm('mm6-m200', 56, 6, 200, 1, (1, 16, 2)),
    # the centre's networks: 16-row groups inside the sweep (2 x 16 x LD + 720 + 6144 floats + 64 x 492 B)
    _case('mm12-m16-centre', 57, (1, 16, 1), rows=32, groups=2, z_orth=True),
]

# ---- combined corners
CORNERS = [
    _case('l7-w258-rows17-h1', 58, R16, pol=w(258, 7), dyn=w(258, 7), rows=17, H=1),
    _case('d32u16-ang-r64', 0, R32, D=32, U=16, pol_ang=(5,), dyn_ang=(0, 31), rows=77, hint=64),      # angles: no in-place form
    _case('masks-ang-act-rows33-r32', 59, R32, pol_step_masks=True, dyn_ang=(3,), pol_act=TANH, rows=33, hint=32, H=3),
    _case('mm4-m17-masks-h1', 60, (2, 17, 1), n=2, rows=34, groups=2, H=1, dyn_step_masks=True, **SMALL),
    _case('l0-pol-ang-d25', 61, R16, pol=(), D=25, pol_ang=(24,)),
]
CASES = CASES + IP_CASES + MM_CASES + CORNERS

# ---- saturation of the family's transcendentals (the modifications of tests/reg_envelope_cases.problem need two hidden
# layers in both networks), on one wide and one moment-matching case (seeds in the hundreds: drawn again until the
# conditions of the CPU test held, here and above)
SAT_CASES = [
    _case('sat-tanh-w272', 102, R16, pol=w(272), dyn=w(272), D=4, U=1, rows=48, H=6, mods=('sat_policy',)),
    _mm('sat-tanh-mm4-m16', 104, 4, 16, 3, (1, 16, 1), H=6, mods=('sat_policy',)),
    _case('sat-logstd-w272-d4u3', 101, R16, pol=w(272), dyn=w(272), D=4, U=3, rows=48, H=6, mods=('sat_logstd',)),
    _mm('sat-logstd-mm4u3-m16', 73, 4, 16, 3, (1, 16, 1), H=6, U=3, mods=('sat_logstd',)),
]
# ---- a non-finite value mid horizon: state dimension 3, decoupled from both networks and the reward, drifts by 5e37 a
# step and overflows fp32 while step 6 computes x_7.  In exact fp32 the family keeps 6 steps.  On split operands it splits
# its network INPUTS into fp16 pieces too (pm_rollout_fwd: `an INPUT out of fp16's range ... reported like an activation
# out of range`) and answers at the first step whose input holds the 5e37: step 1 (tests/test_gpu_reg_envelope.py pins the
# same for the register-resident family)
OVERFLOW_STEPS = {'f32': 6, 'split_f16': 1}
OVERFLOW_CASES = [
    _case('overflow-w272', 74, R16, pol=w(272), dyn=w(272), D=4, U=1, rows=40, H=12, mods=('drift',)),
    _mm('overflow-mm4-m16', 75, 4, 16, 3, (1, 16, 1), H=12, mods=('drift',)),
]

ALL_CASES = CASES + SAT_CASES + OVERFLOW_CASES
assert len({c['id'] for c in ALL_CASES}) == len(ALL_CASES)
assert 2 * sum(c['seed'] != 0 for c in ALL_CASES) >= len(ALL_CASES)

PLAIN_INSIDE = [c for c in CASES if c['inside']]      # (inside, without the saturation cases)
INSIDE = PLAIN_INSIDE + SAT_CASES
REFUSED = [c for c in CASES if not c['inside']]
# the adjoint in two step ranges (H = 5)
RANGE_CASE = 'h5'
# run twice, bit for bit: one case per form -- two buffers, in place 1 and 2, moment matching in a workgroup, the per-step
# one-wave routines and multi-wave kernels
TWICE_CASES = ('centre', 'ip1-96-500-128', 'ip2-512x3', 'mm4-m16', 'mm4-m65', 'mm7-m200')
# what oracle/adjoint_np.py does not cover: activations other than ReLU
NO_ADJOINT_ORACLE = tuple(c['id'] for c in ALL_CASES
                          if any(c['extra'].get(k) for k in ('pol_act', 'dyn_act', 'pol_acts', 'dyn_acts')))
# Every case whose moment matching runs per step (mm_mode 2) in some arithmetic: do the multi-wave pm_mmw_* kernels run it
# (pm_mmw_ok: 6 < D <= 32, no infer_ns, 8 (5 D + 2 D (D + 1) + 3 D^2 + 1536) + 12 M D <= 163 840 bytes), or the one-wave
# routines?  By hand; D = 32: 8 x 6880 + 384 M <= 163 840 -> M <= 283
MM_PER_STEP_WIDE = {
    'mm4-m65-infer-ns': False, 'mm7-m65-infer-ns': False, 'mm21-m32': True, 'mm22-m32': True, 'mm7-m200': True,
    'mm16-m80': True, 'mm32-m283': True, 'mm32-m284': False, 'mm4-m65': False, 'mm4-m200': False, 'mm6-m65': False,
    'mm6-m200': False,
}


def by_id(cid):
    return next(c for c in ALL_CASES if c['id'] == cid)


def pairs(cases):
    """(case, arithmetic) of every arithmetic a case runs in"""
    return [(c, p) for c in cases for p in c['precision']]


def pair_ids(cases):
    return ['%s-%s' % (c['id'], p) for c, p in pairs(cases)]


def kernel_head(inst):
    """the template arguments of pm_rollout_fwd / _bwd <RT, planes, form, ACT> in the runtime's names"""
    kind, rt, third = inst
    planes, form, act = {'f32': (0, 0, 0), 'split': (2, third, 0), 'act': (third, 0, 1)}[kind]
    return 'ILi%dELi%dELi%dELb%dEE' % (rt, planes, form, act)


def expand_angles(x, dims):
    """utils/angles.py: [others | sin | cos]"""
    dims = [int(a) for a in dims]
    others = [i for i in range(x.shape[-1]) if i not in dims]
    return np.concatenate([x[..., others], np.sin(x[..., dims]), np.cos(x[..., dims])], -1)


def problem(case, drift=5e37):
    """tests/reg_envelope_cases.problem, then what a case's `extra` asks for"""
    from prob_mbrl_amd import problem as PB
    d = _base_problem(case, drift)
    x = case['extra']
    D, U = case['cfg']['D'], case['cfg']['U']
    B, H = d['x0'].shape[0], int(d['H'])
    rng = np.random.default_rng([case['seed'], 2718])
    # angle features: the first layer of the expanded width, drawn like any other (models/core.py:20-22), and for the
    # dynamics model the normalisation of the expanded input from a synthetic dataset, as synthetic_problem's
    if x.get('pol_ang'):
        d['pol_angle_dims'] = np.asarray(x['pol_ang'], dtype=np.int64)
        d['pol_W0'], d['pol_b0'] = PB._xavier(rng, d['pol_W0'].shape[0], D + len(x['pol_ang']))
    if x.get('dyn_ang'):
        d['dyn_angle_dims'] = np.asarray(x['dyn_ang'], dtype=np.int64)
        d['dyn_W0'], d['dyn_b0'] = PB._xavier(rng, d['dyn_W0'].shape[0], D + U + len(x['dyn_ang']))
        X = expand_angles(rng.standard_normal((300, D + U)), x['dyn_ang'])
        d['dyn_mx'] = X.mean(0).astype(np.float32)
        d['dyn_iSx'] = (1.0 / (4.0 * X.std(0, ddof=1))).astype(np.float32)
    # [H, B, h] masks: a fresh draw at every step
    for net in ('pol', 'dyn'):
        if x.get(net + '_step_masks'):
            for i in range(int(d[net + '_n_layers']) - 1):
                d['%s_mask%d' % (net, i)] = (rng.random((H,) + d['%s_mask%d' % (net, i)].shape) < 0.9).astype(np.float32)
        if x.get(net + '_act'):
            d[net + '_act'] = int(x[net + '_act'])
        if x.get(net + '_acts'):
            # one code per hidden layer: prob_mbrl_amd reads the list, the oracle the index of a callable that applies the
            # codes in turn (tests/act_layers.py: layered)
            from tests import act_layers as AL
            d[net + '_acts'] = np.asarray(x[net + '_acts'], dtype=np.int64)
            d[net + '_act'] = AL.layered(x[net + '_acts'])
    if x.get('infer_ns'):
        d['infer_ns'] = True
    if x.get('no_mm_states'):
        d['mm_states'] = False
    return d


def relu_margin_angles(d, o64):
    """tests/fast_envelope_cases.relu_margin for networks with angle features: the same walk from the expanded inputs"""
    f = lambda k: np.asarray(d[k], dtype=np.float64)      # noqa: E731
    best = (np.inf, None)
    for t in range(o64['actions'].shape[0]):
        x, a = o64['states'][t].astype(np.float64), o64['actions'][t].astype(np.float64)
        xp = expand_angles(x, d['pol_angle_dims'])
        xa = (expand_angles(np.concatenate([x, a], 1), d['dyn_angle_dims']) - f('dyn_mx')) * f('dyn_iSx')
        for net, h in (('pol', xp), ('dyn', xa)):
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
