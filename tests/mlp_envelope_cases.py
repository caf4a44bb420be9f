"""The envelope of the stand-alone network calls (csrc/pmbrl_mlp.h, pmbrl_mlp.hip, pmbrl_mlp_ln.hip: pmbrl_mlp_forward,
_grad_input, _backward, _backward_concrete and the three _ln entry points) as a table of small generated problems, and the
arithmetic both envelope tests judge them with:

  tests/test_mlp_envelope_cases.py   (CPU) the LDS rule restated here agrees with the library's workspace queries, the table
                                     reaches every branch it names, every ReLU / hhSinLU case is clear of the kink, every
                                     case is well conditioned: the reference's own fp32 run stays within a quarter of each
                                     bar of its fp64 run
  tests/test_gpu_mlp_envelope.py     (GPU) every call of every case against the fp64 reference, the refusals, the bits

One axis varies per case around [6, 40, 56, 6], B = 45, where the existing tests sit.  Cases are generated from a seed
(tests/layer_norm_ref.py::standalone, which draws every input of a call), nothing is stored.  The reference is
tests/layer_norm_ref.py::standalone_reference: the one plain-torch statement of the formula, at any dtype.

A case names the calls it is for: 'fwd' (pmbrl_mlp_forward), 'gx' (pmbrl_mlp_grad_input), 'bwd' (pmbrl_mlp_backward), and
with them 'conc' where a hidden layer is train-mode concrete dropout (the backward is then pmbrl_mlp_backward_concrete) and
'ln' where one is layer-normalised (all three are then the _ln entry points).  `refused` maps a call to the code it is
refused with; a call that is named and not refused is inside.

The envelope (mlp_layout, pm_mlp_bwd_lds_floats, pm_mlp_bwdp_lds_floats):
  nl = number of Linear layers, 2 .. 8; every entry of dims 1 .. 1024; dims[nl] even        else -2
  LD = 16 ceil(widest / 16) + 8, widest over ALL of dims
  a call needs n_buf * 16 * LD * 4 + 24 576 bytes of LDS, refused with -3 beyond 163 840:  n_buf * LD <= 2176
    fwd   2                                           (156 672 B at 1024: never refused)
    gx    nl + 2, + 1 if a hidden layer is not ReLU, + 1 per layer-norm layer
    bwd   nl + 2, + nl - 1 if a hidden layer is not ReLU, + 1 per concrete layer, + 1 per layer-norm layer
  widest accepted layer by n_buf:   4: 528   5: 416   6: 352   7: 288   8: 256   9: 224   10: 208   11: 176   17: 112"""
import functools

import numpy as np
import torch

from tests import common
from tests import grad_bars
from tests import layer_norm_ref as LN

MLS = float(np.log(5.0))
# the project's bars: tests/test_gpu_mlp_backward.py::test_forward_matches_fp64, tests/grad_bars.py
FWD_RTOL, FWD_ATOL = 2e-5, 2e-6
GRAD_BAR = grad_bars.BAR
KINK_MARGIN = 1e-4               # tests/test_gpu_mlp_backward.py::test_relu_cases_stay_clear_of_the_kink

RELU, TANH, SILU, SIN, EXP, SINLU, HHSINLU, NONE = range(8)
KINKED = (RELU, HHSINLU)         # the activations whose derivative jumps at 0
OUTS = ('sample', 'mean', 'log_std')
FWD, GX, BWD = 'fwd', 'gx', 'bwd'
ALL = (FWD, GX, BWD)
CENTRE = [6, 40, 56, 6]
BLOCK_CAP, SLAB_CAP = 'block_cap', 'slab_cap'
MLP_BWD_MAX_BLOCKS, MLP_BWD_SLAB_BYTES = 256, 64 << 20       # include/pmbrl.h
RANGE, LDS = -2, -3
# the optional inputs of a call, by the pointers that come together
OPTIONAL = {'in': ('shift', 'iscale'), 'out': ('osc', 'osh'), 'sq': ('sqs', 'sqb'), 'z': ('z',)}


def _case(cid, seed, dims, B=45, act=RELU, layers=None, calls=ALL, refused=None, opts=tuple(OPTIONAL), bits=False):
    """dims: the Linear layers' widths, input first.  B: rows, or BLOCK_CAP / SLAB_CAP (rows()).  act: one code, or one per
    hidden layer.  layers: per hidden layer a string of 'L' (layer norm) and at most one of 'c' (train-mode concrete
    dropout), 'b' (a constant mask, keep 0.8), or '-' (nothing); default: a constant mask on the first hidden layer.
    refused: {call: code}.  opts: the optional inputs that are given (OPTIONAL).  bits: the case is one of those on which
    the GPU test also compares the calls' bits with each other."""
    nh = len(dims) - 2
    layers = list(layers) if layers is not None else (['b'] + ['-'] * (nh - 1))[:max(nh, 0)]
    refused = dict(refused or {})
    assert set(refused) <= set(calls) and set(calls) <= set(ALL) and set(opts) <= set(OPTIONAL)
    names = tuple(calls) + (('conc',) if any('c' in s for s in layers) else ()) + (('ln',) if any('L' in s for s in layers) else ())
    return dict(id=cid, seed=seed, dims=list(dims), B=B, act=act, layers=layers, calls=names, refused=refused,
                opts=tuple(opts), bits=bits)


def _h(w, n):
    return [6] + [w] * n + [6]


NO_GRAD = {GX: LDS, BWD: LDS}
OUTSIDE = {FWD: RANGE, GX: RANGE, BWD: RANGE}
T2 = [TANH, TANH]

CASES = [
    # ---- width of a hidden layer.  n_kb % 8 == 0 takes gemm_tiles_group_full (128, 256, 512, 1024); 17, 33 and 49 output
    #      tiles start a wave's second, third and fourth tile group (272, 520 / 528, 1024).  Three Linear layers hold 5
    #      buffers in both gradient calls (<= 416), so 512 .. 528 run them behind one hidden layer (4 buffers).
    _case('w1', 1, [6, 1, 56, 6]),
    _case('w15', 2, [6, 15, 56, 6]),
    _case('w16', 3, [6, 16, 56, 6]),
    _case('w17', 4004, [6, 17, 56, 6]),
    _case('w128', 1005, [6, 128, 56, 6], 13),
    _case('w136', 1006, [6, 136, 56, 6], 13),
    _case('w256', 2007, [6, 256, 56, 6], 13),
    _case('w264', 8, [6, 264, 56, 6], 13),
    _case('w272', 1009, [6, 272, 56, 6], 13),
    _case('w512', 10, [6, 512, 6], 5),
    _case('w512_fwd', 11, [6, 512, 56, 6], 13, refused=NO_GRAD),      # K = 512 into a hidden layer: 32 k-blocks, full form
    _case('w520', 12, [6, 520, 6], 5),
    _case('w528', 13, [6, 528, 6], 5, bits=True),                     # n_buf 4: the last accepted
    _case('w529', 1014, [6, 529, 6], 5, refused=NO_GRAD),               # ... the first refused; the forward still serves it
    _case('w1024', 6015, [6, 1024, 1024, 6], 5, refused=NO_GRAD),       # 64 tiles by 64 k-blocks
    _case('w1025', 0, [6, 1025, 56, 6], refused=OUTSIDE),
    # ---- unequal layers: LD comes from the widest, a narrow layer's tiles must not read the wide layer's stale columns
    _case('wide_first', 16, [6, 416, 24, 6], 5, bits=True),
    _case('wide_last', 1017, [6, 24, 416, 6], 5),
    _case('wide_middle', 18, [6, 24, 352, 24, 6], 5),
    _case('wide_first_512', 19, [6, 512, 24, 6], 5, refused=NO_GRAD),
    _case('wide_last_512', 2020, [6, 24, 512, 6], 5, refused=NO_GRAD),
    # ---- input width
    _case('in1', 1021, [1, 40, 56, 6]),
    _case('in16', 1022, [16, 40, 56, 6]),
    _case('in17', 23, [17, 40, 56, 6]),
    _case('in64', 24, [64, 40, 56, 6]),
    _case('in1024', 25, [1024, 40, 6], 13, refused=NO_GRAD),
    # ---- head 2 n_out: 48 is the last K-split head (PM_KS_NT = 3 tiles), 50 the first tile-split one
    _case('head2', 1026, [6, 40, 56, 2]),
    _case('head48', 4027, [6, 40, 56, 48]),
    _case('head50', 28, [6, 40, 56, 50]),
    _case('head64', 2029, [6, 40, 56, 64]),
    _case('head512', 10030, [6, 40, 512], 13),
    _case('head1024', 1031, [6, 40, 1024], 13, refused=NO_GRAD),
    _case('head_odd', 0, [6, 40, 56, 5], refused=OUTSIDE),
    #      the K-split head behind 1, 8, 9, 17 and 64 k-blocks: a wave's K slice is ceil(n_kb / 8) blocks -- empty slices
    #      (1, 9, 17), single ones (8), part-filled ones (9, 17) and two whole chunks (64)
    _case('ks_kb1', 32, [6, 40, 16, 6]),
    _case('ks_kb8', 1033, [6, 40, 128, 48], 13),
    _case('ks_kb9', 1034, [6, 40, 144, 6], 13),
    _case('ks_kb17', 35, [6, 40, 272, 48], 13),
    _case('ks_kb64', 36, [6, 1024, 34], 5, refused=NO_GRAD),
    # ---- depth
    _case('nl2', 37, [6, 40, 6]),
    _case('nl8', 38, [6, 40, 56, 24, 40, 32, 48, 24, 6], 13, layers=['b'] * 7),      # keep < 1 on every hidden layer
    _case('nl1', 0, [6, 6], refused=OUTSIDE),
    _case('nl9', 0, [6, 8, 8, 8, 8, 8, 8, 8, 8, 6], refused=OUTSIDE),
    # ---- the LDS edges: on every n_buf line the last accepted width runs and the next tile count is refused by that call,
    #      while the calls that need less still serve it
    _case('e5_relu', 39, _h(416, 2), 5, bits=True),                                   # gx 5, bwd 5
    _case('e5_relu_out', 40, [6, 417, 416, 6], 5, refused=NO_GRAD),
    _case('e5_tanh', 41, _h(416, 1), 21, TANH, bits=True),                            # gx 3 + 1 + 1, bwd 3 + 1 + 1
    _case('e5_tanh_out', 1042, _h(417, 1), 21, TANH, refused=NO_GRAD),
    _case('e5_conc', 43, _h(416, 1), 5, layers=['c'], bits=True),                     # gx 4, bwd 4 + 1: a concrete layer at its widest
    _case('e5_conc_out', 1044, _h(417, 1), 5, layers=['c'], refused={BWD: LDS}),
    _case('e5_ln', 45, _h(416, 1), 5, layers=['L'], bits=True),                       # gx 5, bwd 5: layer norm at its widest
    _case('e5_ln_out', 46, _h(417, 1), 5, layers=['L'], refused=NO_GRAD),
    _case('e6_relu', 47, _h(352, 3), 5),                                              # gx 6, bwd 6
    _case('e6_relu_out', 48, _h(353, 3), 5, refused=NO_GRAD),
    _case('e6_tanh_gx', 49, _h(352, 2), 21, T2, refused={BWD: LDS}),                  # gx 6; bwd 7 is beyond 288
    _case('e6_tanh_gx_out', 2050, _h(353, 2), 21, T2, refused=NO_GRAD),
    _case('e6_ln_conc', 51, _h(352, 1), 5, layers=['Lc'], bits=True),                 # gx 5, bwd 6
    _case('e6_ln_conc_out', 52, _h(353, 1), 5, layers=['Lc'], refused={BWD: LDS}),
    _case('e6_ln_narrow', 53, [6, 352, 40, 6], 5, layers=['-', 'L']),                 # layer norm on a narrower layer: gx 6, bwd 6
    _case('e7_tanh', 54, _h(288, 2), 21, T2, bits=True),                              # gx 6, bwd 7
    _case('e7_tanh_out', 55, _h(289, 2), 21, T2, refused={BWD: LDS}),
    _case('e7_ln2', 1056, _h(288, 2), 5, layers=['L', 'L']),                            # gx 7, bwd 7
    _case('e7_ln2_out', 57, _h(289, 2), 5, layers=['L', 'L'], refused=NO_GRAD),
    _case('e8_ln2_conc', 58, _h(256, 2), 5, layers=['Lc', 'L'], bits=True),           # gx 7, bwd 8
    _case('e8_ln2_conc_out', 1059, _h(257, 2), 5, layers=['Lc', 'L'], refused={BWD: LDS}),
    _case('e8_tanh_ln2_gx', 60, _h(256, 2), 21, T2, layers=['L', 'L'], refused={BWD: LDS}),      # gx 8; bwd 9 is beyond 224
    _case('e8_tanh_ln2_gx_out', 1061, _h(257, 2), 21, T2, layers=['L', 'L'], refused=NO_GRAD),
    _case('e9_ln2_conc2', 62, _h(224, 2), 5, layers=['Lc', 'Lc'], bits=True),         # gx 7, bwd 9
    _case('e9_ln2_conc2_out', 1063, _h(225, 2), 5, layers=['Lc', 'Lc'], refused={BWD: LDS}),
    _case('e9_tanh_ln2', 64, _h(224, 2), 21, T2, layers=['L', 'L']),                  # gx 8, bwd 9
    _case('e9_tanh_ln2_out', 65, _h(225, 2), 21, T2, layers=['L', 'L'], refused={BWD: LDS}),
    _case('e9_deep', 1066, _h(224, 6), 5, layers=['-'] * 6),                            # six hidden layers: gx 9, bwd 9
    _case('e9_deep_out', 4067, _h(225, 6), 5, layers=['-'] * 6, refused=NO_GRAD),
    _case('e10_deep', 2068, _h(208, 7), 5, layers=['-'] * 7, bits=True),                # seven hidden layers: gx 10, bwd 10
    _case('e10_deep_out', 4069, _h(209, 7), 5, layers=['-'] * 7, refused=NO_GRAD),
    _case('e10_tanh_ln2_conc', 70, _h(208, 2), 21, T2, layers=['Lc', 'L'], bits=True),            # gx 8, bwd 10
    _case('e10_tanh_ln2_conc_out', 1071, _h(209, 2), 21, T2, layers=['Lc', 'L'], refused={BWD: LDS}),
    _case('e11_tanh_ln2_conc2_at208', 72, _h(208, 2), 21, T2, layers=['Lc', 'Lc'], refused={BWD: LDS}),   # one more concrete layer
    _case('e11_tanh_ln2_conc2', 73, _h(176, 2), 21, T2, layers=['Lc', 'Lc'], bits=True),          # gx 8, bwd 11
    _case('e11_tanh_ln2_conc2_out', 74, _h(177, 2), 21, T2, layers=['Lc', 'Lc'], refused={BWD: LDS}),
    _case('e11_deep_tanh_gx', 75, _h(176, 7), 21, [TANH] * 7, layers=['-'] * 7, refused={BWD: LDS}),      # gx 11; bwd 17 is beyond 112
    _case('e11_deep_tanh_gx_out', 76, _h(177, 7), 21, [TANH] * 7, layers=['-'] * 7, refused=NO_GRAD),
    _case('e11_deep_ln', 2077, _h(176, 7), 5, layers=['L'] + ['-'] * 6),                # gx 11, bwd 11
    _case('e17_deep_tanh', 78, _h(112, 7), 21, [TANH] * 7, layers=['-'] * 7, bits=True),          # gx 11, bwd 17
    _case('e17_deep_tanh_out', 79, _h(113, 7), 21, [TANH] * 7, layers=['-'] * 7, refused={BWD: LDS}),
    _case('e17_deep_ln7', 2080, _h(112, 7), 5, layers=['L'] * 7),                       # gx 17, bwd 17
    _case('e17_deep_ln7_out', 81, _h(113, 7), 5, layers=['L'] * 7, refused=NO_GRAD),
    # ---- rows
    _case('b1', 82, CENTRE, 1),
    _case('b15', 83, CENTRE, 15),
    _case('b16', 84, CENTRE, 16),
    _case('b17', 1085, CENTRE, 17),
    # (1.7 million and 0.3 million hidden units: too many for any seed to keep them all 1e-4 from 0, so these run Tanh; what
    #  they are there for -- a workgroup's stride over its tiles, the slab reduction -- does not depend on the activation)
    #  The gradient calls only: the largest of 12 000 and more forward outputs of the reference's own fp32 run is 0.3 to 1.5
    #  of the forward bar from its fp64 run, whatever the seed -- nothing a kernel could be held to.)
    _case('many_rows_w416', 86, _h(416, 1), BLOCK_CAP, TANH, calls=(GX, BWD), bits=True),
    _case('slab_cap_w416', 87, [416, 416, 416], SLAB_CAP, TANH, calls=(GX, BWD), bits=True),     # 347 000 parameters: 48 slabs of the 256
    # ---- activations: each code once at a width >= 272 (ReLU: w272), and a per-layer list with None
    _case('act_tanh', 88, [6, 272, 40, 6], 21, T2),
    _case('act_silu', 2089, [6, 272, 40, 6], 21, [SILU, SILU]),
    _case('act_sin', 90, [6, 272, 40, 6], 21, [SIN, SIN]),
    _case('act_exp', 91, [6, 272, 40, 6], 21, [EXP, EXP]),
    _case('act_sinlu', 2092, [6, 272, 40, 6], 21, [SINLU, SINLU]),
    _case('act_hhsinlu', 93, [6, 272, 40, 6], 5, [HHSINLU, HHSINLU]),
    _case('act_list_none', 94, [6, 40, 56, 24, 40, 32, 6], 21, [TANH, NONE, SIN, RELU, SILU]),
    # ---- dropout (keep < 1 on every layer of a deep network: nl8; a concrete layer at its widest: e5_conc; the logits are
    #      per unit in every concrete case)
    _case('null_mask_between', 95, [7, 32, 48, 16, 4], 37, layers=['b', '-', 'b']),
    _case('conc_two', 96, CENTRE, 45, layers=['c', 'c']),
    _case('nl8_conc', 2106, [6, 40, 56, 24, 40, 32, 48, 24, 6], 13, layers=['b', 'c', '-', 'b', 'c', '-', 'b'], bits=True),
    _case('conc_tanh_first', 97, CENTRE, 45, T2, layers=['c', 'b']),
    # ---- layer norm at 16, 17 (208, 224 and the widest: the edges above)
    _case('ln16', 98, [6, 16, 56, 6], 45, layers=['L', '-']),
    _case('ln17', 99, [6, 17, 56, 6], 45, layers=['L', 'L']),
    _case('ln17_conc', 100, [6, 17, 56, 6], 45, T2, layers=['Lc', 'Lb']),
    # ---- optional pointers: all null at a wide shape, each group alone
    _case('plain_w272', 101, [6, 272, 56, 6], 13, layers=['-', '-'], opts=()),
    _case('only_in', 1102, CENTRE, opts=('in',)),
    _case('only_out', 103, CENTRE, opts=('out',)),
    _case('only_sq', 2104, CENTRE, opts=('sq',)),
    _case('only_z', 1105, CENTRE, opts=('z',)),
]
assert len({c['id'] for c in CASES}) == len(CASES)


def ids(cases):
    return [c['id'] for c in cases]


def by_id(cid):
    return next(c for c in CASES if c['id'] == cid)


def inside(case, call=None):
    """Does the case run `call` (None: any call)?"""
    runs = [k for k in ALL if k in case['calls'] and k not in case['refused']]
    return bool(runs) if call is None else call in runs


INSIDE = [c for c in CASES if inside(c)]
OUTSIDE_CASES = [c for c in CASES if c['refused']]


# ---- the envelope's arithmetic, restated (csrc/pmbrl_mlp.hip: mlp_layout; csrc/pmbrl_mlp.h: pm_mlp_*_lds_floats;
#      csrc/pmbrl_dev.h: gemm_tiles, gemm_narrow)
PM_NW, PM_KS_NT, PM_CK, GEMM_NT = 8, 3, 4, 2
LDS_LIMIT = 160 * 1024
SCRATCH = PM_NW * PM_KS_NT * 256 * 4             # the K-split scratch: 24 576 bytes
MAX_LINEAR, MAX_WIDTH = 8, 1024
WIDEST = {4: 528, 5: 416, 6: 352, 7: 288, 8: 256, 9: 224, 10: 208, 11: 176, 17: 112}


def tiles(w):
    return (w + 15) // 16


def codes(case):
    nh = len(case['dims']) - 2
    return [int(a) for a in case['act']] if isinstance(case['act'], (list, tuple)) else [int(case['act'])] * nh


def leading_dim(dims):
    return 16 * max(tiles(w) for w in dims) + 8


def n_buf(case, call):
    """The 16-row LDS buffers of a call."""
    nl = len(case['dims']) - 1
    smooth = any(a != RELU for a in codes(case))
    n_ln, n_conc = sum('L' in s for s in case['layers']), sum('c' in s for s in case['layers'])
    if call == FWD:
        return 2
    if call == GX:
        return nl + 2 + (1 if smooth else 0) + n_ln
    return nl + 2 + (nl - 1 if smooth else 0) + n_conc + n_ln


def lds_bytes(case, call):
    return n_buf(case, call) * 16 * leading_dim(case['dims']) * 4 + SCRATCH


def verdict(case, call):
    """0, or the code the call is refused with, by the restated rule."""
    dims = case['dims']
    nl = len(dims) - 1
    if not 2 <= nl <= MAX_LINEAR or any(not 1 <= w <= MAX_WIDTH for w in dims) or dims[nl] % 2:
        return RANGE
    return LDS if lds_bytes(case, call) > LDS_LIMIT else 0


def rows(case):
    """B of a case: a number; BLOCK_CAP: five rows past the last tile that gets a workgroup (gradient slab) of its own;
    SLAB_CAP: the same where the slab limit, not PMBRL_MLP_BWD_MAX_BLOCKS, caps the workgroups."""
    B, dims = case['B'], case['dims']
    if B == BLOCK_CAP:
        return 16 * MLP_BWD_MAX_BLOCKS + 5
    if B == SLAB_CAP:
        blocks = MLP_BWD_SLAB_BYTES // (4 * n_params(dims))
        assert 1 < blocks < MLP_BWD_MAX_BLOCKS
        return 16 * blocks + 5
    return B


def n_params(dims):
    return sum(dims[i + 1] * dims[i] + dims[i + 1] for i in range(len(dims) - 1))


def regimes(case):
    """The names of the branches the calls of a case take, from its dims alone."""
    dims = case['dims']
    nl = len(dims) - 1
    out = set()
    if verdict(case, FWD) == RANGE:
        return {'out_of_range'}
    nt = [tiles(w) for w in dims]
    gemms = {FWD: [(nt[l + 1], nt[l]) for l in range(nl - 1)]}
    if nt[nl] > PM_KS_NT:
        gemms[FWD].append((nt[nl], nt[nl - 1]))
        out.add('head_tile_split')
    else:
        out.add('head_k_split')
        per = -(-nt[nl - 1] // PM_NW)
        slices = [max(0, min(nt[nl - 1], (w + 1) * per) - w * per) for w in range(PM_NW)]
        out.add('k_split_%d_blocks' % nt[nl - 1])
        out.update('k_slice_' + ('empty' if s == 0 else 'single' if s == 1 else 'chunks' if s > PM_CK else 'several') for s in slices)
    # the dX chain of both gradient calls: every layer but the first, then the first
    gemms[BWD] = [(nt[l], nt[l + 1]) for l in range(nl)]
    for name, calls in gemms.items():
        ran = inside(case, name) if name == FWD else (inside(case, GX) or inside(case, BWD))
        if not ran:
            continue
        for n_ot, n_kb in calls:
            out.add('tile_groups_%d_%s' % (-(-n_ot // (GEMM_NT * PM_NW)), name))
            out.add(('gemm_full_' if n_kb % (2 * PM_CK) == 0 else 'gemm_general_') + name)
            if n_kb % (2 * PM_CK) == 0 and n_kb > 16:
                out.add('gemm_full_gt16_' + name)
    for call in (GX, BWD):
        if call not in case['calls']:
            continue
        n, LD = n_buf(case, call), leading_dim(dims)
        if n * LD <= 2176 < n * (LD + 16):
            out.add('last_accepted_%s_%d' % (call, n))
        if n * (LD - 16) <= 2176 < n * LD:
            out.add('first_refused_%s_%d' % (call, n))
            out.update('served_by_' + k for k in ALL if inside(case, k))
    if nt[0] > 1:
        out.add('input_tiles_gt1')
    if nt[0] > 4 or nt[nl] > 4:
        out.add('input_or_head_gt64')
    out.add('nl%d' % nl)
    return out


# ---- the problems and their reference
def generate(case, seed=None):
    """The inputs of the case's calls (CPU tensors, fp32 values): tests/layer_norm_ref.py::standalone's dict, with the
    optional inputs that the case leaves out set to None."""
    seed = case['seed'] if seed is None else seed
    c = LN.standalone(case['dims'], codes(case), rows(case), seed, [s.replace('-', '') for s in case['layers']])
    for group, keys in OPTIONAL.items():
        if group not in case['opts']:
            c.update(dict.fromkeys(keys))
    return c


@functools.lru_cache(maxsize=None)
def _problem(cid):
    return generate(by_id(cid))


def problem(case):
    """The case's inputs, generated once and shared (leave them unchanged)."""
    return _problem(case['id'])


def reference_of(c, dtype=torch.float64):
    return LN.standalone_reference(c, dtype, MLS)


@functools.lru_cache(maxsize=None)
def _reference(cid):
    return reference_of(_problem(cid))


def reference(case):
    """The fp64 reference of the case (shared, leave it unchanged): LN.standalone_reference's dict."""
    return _reference(case['id'])


def kink_margin(case, ref):
    """The smallest kept |y| over the hidden layers whose activation has a kink (inf: there is none)."""
    return min([m for m, a in zip(ref['margins'], codes(case)) if a in KINKED], default=float('inf'))


def forward_figures(got, ref):
    """[(output, np.allclose's criterion at the forward bar as one number: it holds at <= 1)]"""
    out = []
    for k in OUTS:
        g, w = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        out.append((k, float(np.max(np.abs(g - w) / (FWD_ATOL + FWD_RTOL * np.abs(w))))))
    return out


def param_tensors(c, flat):
    """A flat parameter-order vector as [W0, b0, W1, b1, ...]."""
    out, off = [], 0
    for t in (t for pair in zip(c['Ws'], c['bs']) for t in pair):
        out.append(np.asarray(flat[off:off + t.numel()]).reshape(tuple(t.shape)))
        off += t.numel()
    assert off == len(flat)
    return out


def gradient_figures(got, ref):
    """[(tensor, error)] of a gradient dict (grad_x, and where the call gives them params: [W0, b0, ...], logit / gamma /
    beta: per hidden layer or None) against the reference dict: grad_x and every parameter tensor by tests/grad_bars.py,
    every logit, gamma and beta gradient on its own norm."""
    errs = grad_bars.errors([np.asarray(got['grad_x'])], [ref['grad_x'].numpy()], ['grad_x'])
    if got.get('params') is not None:
        errs += grad_bars.errors([np.asarray(t) for t in got['params']], [r.numpy() for r in ref['params']])
    for key, label in (('logit', 'logit_p'), ('gamma', 'gamma'), ('beta', 'beta')):
        if got.get(key) is None:
            continue
        for l, r in enumerate(ref[key]):
            if r is not None:
                errs.append(('%s%d' % (label, l), common.rel(np.asarray(got[key][l]), r.numpy())))
    return errs


def hold(what, fwd_figs, grad_figs, share=1.0):
    """Print every figure, then hold each to `share` of its bar."""
    print('%s: %s' % (what, ', '.join(['%s %.3f of its bar' % e for e in fwd_figs] + ['%s %.2e' % e for e in grad_figs])))
    for key, e in fwd_figs:
        assert e <= share, (what, key, e)
    for key, e in grad_figs:
        assert e < share * GRAD_BAR, (what, key, e)


def conditioning(case, c=None, ref=None):
    """The reference's own fp32 run against its fp64 run: (forward figures, gradient figures) of what the case's inside
    calls are judged on."""
    c = problem(case) if c is None else c
    ref = reference(case) if ref is None else ref
    r32 = reference_of(c, torch.float32)
    fwd = forward_figures({k: r32[k].numpy() for k in OUTS}, {k: ref[k].numpy() for k in OUTS}) if inside(case, FWD) else []
    got = dict(grad_x=r32['grad_x'].numpy())
    if inside(case, BWD):
        got.update(params=[t.numpy() for t in r32['params']],
                   **{k: [None if t is None else t.numpy() for t in r32[k]] for k in ('logit', 'gamma', 'beta')})
    grads = gradient_figures(got, ref) if inside(case, GX) or inside(case, BWD) else []
    return fwd, grads
