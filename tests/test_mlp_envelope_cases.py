"""CPU: the table of tests/mlp_envelope_cases.py.  Its restatement of the stand-alone network calls' envelope agrees with the
library's workspace queries (validation comes before the first device call), it reaches every branch it names (by the
kernels' own arithmetic, mirrored), its ReLU / hhSinLU cases are clear of the kink, and every case is well conditioned: the
reference's own fp32 run stays within a quarter of each bar the GPU test holds."""
import ctypes

import pytest

from tests import mlp_envelope_cases as ME

RANGE_TEXT = (b'2..8 layers', b'layer width out of range', b'2 x n_out wide')


def call_struct(case, layers=None):
    """(pmbrl_mlp_call, pmbrl_mlp_concrete or None, pmbrl_mlp_layer_norm or None) of a case, as a workspace query reads
    them: the pointers only say which layers are concrete / layer-normalised.  layers: instead of the case's own."""
    from prob_mbrl_amd import _lib
    from prob_mbrl_amd import activations as ACT
    dims = case['dims']
    layers = case['layers'] if layers is None else layers
    call = _lib.MlpCall()
    call.B = ME.rows(case)
    call.net.n_layers = len(dims) - 1
    for i, w in enumerate(dims[:_lib.MAX_LAYERS + 1]):
        call.net.dims[i] = w
    for l, s in enumerate(layers[:_lib.MAX_LAYERS]):
        call.net.keep[l] = 0.8 if 'b' in s else 1.0
    call.max_log_std = ME.MLS
    call.act = ACT.pack(ME.codes(case)[:ACT.MAX_HIDDEN])
    conc = ln = None
    if any('c' in s for s in layers):
        conc = _lib.MlpConcrete()
        for l, s in enumerate(layers):
            if 'c' in s:
                conc.u_d[l], conc.logit_d[l], conc.temp[l] = 16, 16, 0.1
    if any('L' in s for s in layers):
        ln = _lib.MlpLayerNorm()
        for l, s in enumerate(layers):
            if 'L' in s:
                ln.gamma_d[l], ln.beta_d[l], ln.eps[l] = 16, 16, 1e-5
    return call, conc, ln


def variant(case, drop):
    """The case with the layer kinds in `drop` ('c', 'L') taken off its hidden layers: the network the narrower calls see."""
    return dict(case, layers=[''.join(k for k in s if k not in drop) or '-' for s in case['layers']])


def test_mirrors_of_the_envelope():
    assert [ME.tiles(w) for w in (1, 16, 17, 528, 529, 1024)] == [1, 1, 2, 33, 34, 64]
    assert ME.leading_dim([6, 40, 56, 6]) == 72 and ME.leading_dim([1024, 40, 6]) == 1032 and ME.leading_dim([6, 40, 1024]) == 1032
    assert ME.SCRATCH == 24576 and ME.LDS_LIMIT == 163840
    # the forward at the widest layer the range check lets through: never refused
    assert ME.lds_bytes(ME.by_id('w1024'), ME.FWD) == 156672 <= ME.LDS_LIMIT
    # n_buf * LD <= 2176: the widest accepted layer on every line of the table, and the next tile count refused
    for n, widest in ME.WIDEST.items():
        assert n * (widest + 8) <= 2176 < n * (widest + 16 + 8), n
        assert n * 16 * (widest + 8) * 4 + ME.SCRATCH <= ME.LDS_LIMIT < n * 16 * (widest + 24) * 4 + ME.SCRATCH
    # the slab rule's "at least one" branch: more than 16 M parameters, and the largest network a backward accepts has 0.56 M
    assert ME.MLP_BWD_SLAB_BYTES // 4 == 16 << 20 and ME.n_params([528, 528, 528]) == 558624
    # pm_mlp_bwdp_lds_floats' own example (two hidden layers of 200)
    two200 = dict(dims=[5, 200, 200, 2], act=ME.TANH)
    assert ME.lds_bytes(dict(two200, layers=['Lc', 'L']), ME.BWD) == 162816
    assert ME.lds_bytes(dict(two200, layers=['Lc', 'Lc']), ME.BWD) == 176640


def test_table_is_what_it_claims():
    from prob_mbrl_amd import _lib
    assert (ME.MLP_BWD_MAX_BLOCKS, ME.MLP_BWD_SLAB_BYTES) == (_lib.MLP_BWD_MAX_BLOCKS, _lib.MLP_BWD_SLAB_BYTES)
    assert len(set(ME.ids(ME.CASES))) == len(ME.CASES)
    seeds = [c['seed'] for c in ME.CASES]
    assert 2 * sum(1 for s in seeds if s) >= len(seeds)
    for case in ME.CASES:
        for call in ME.ALL:
            if call in case['calls']:
                assert ME.verdict(case, call) == case['refused'].get(call, 0), (case['id'], call)
        assert ('conc' in case['calls']) == any('c' in s for s in case['layers'])
        assert ('ln' in case['calls']) == any('L' in s for s in case['layers'])
        # rows stay small except where they are the axis
        assert 1 <= ME.rows(case) <= 45 or case['B'] in (ME.BLOCK_CAP, ME.SLAB_CAP), case['id']
    assert ME.rows(ME.by_id('many_rows_w416')) == 16 * 256 + 5 and ME.rows(ME.by_id('slab_cap_w416')) == 16 * 48 + 5


@pytest.mark.parametrize('case', ME.CASES, ids=lambda c: c['id'])
def test_restated_rule_agrees_with_the_library(case):
    """Every workspace query, served or refused: pmbrl_mlp_workspace_bytes and pmbrl_mlp_ln_workspace_bytes know the range
    only (the forward and the input gradient share them), the three backward queries each their own LDS need."""
    from prob_mbrl_amd import _lib
    lib = _lib.load()

    def agrees(nbytes, want, what):
        msg = lib.pmbrl_last_error() if nbytes == 0 else b''
        assert (nbytes == 0) == (want != 0), (case['id'], what, nbytes, want, msg)
        if want == ME.LDS:
            assert b'LDS' in msg, (what, msg)
        if want == ME.RANGE:
            assert any(t in msg for t in RANGE_TEXT), (what, msg)

    call, conc, ln = call_struct(case)
    in_range = ME.RANGE if ME.verdict(case, ME.FWD) == ME.RANGE else 0
    agrees(lib.pmbrl_mlp_workspace_bytes(ctypes.byref(call)), in_range, 'pmbrl_mlp_workspace_bytes')
    agrees(lib.pmbrl_mlp_ln_workspace_bytes(ctypes.byref(call), None), in_range, 'pmbrl_mlp_ln_workspace_bytes(NULL)')
    # the backward of the same network without its concrete and layer-norm layers
    plain = variant(case, 'cL')
    agrees(lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(call)), ME.verdict(plain, ME.BWD), 'pmbrl_mlp_backward_workspace_bytes')
    agrees(lib.pmbrl_mlp_backward_ln_workspace_bytes(ctypes.byref(call), None, None), ME.verdict(plain, ME.BWD),
           'pmbrl_mlp_backward_ln_workspace_bytes(NULL, NULL)')
    if conc is not None:
        want = ME.verdict(variant(case, 'L'), ME.BWD)
        agrees(lib.pmbrl_mlp_backward_concrete_workspace_bytes(ctypes.byref(call), ctypes.byref(conc)), want,
               'pmbrl_mlp_backward_concrete_workspace_bytes')
        agrees(lib.pmbrl_mlp_backward_ln_workspace_bytes(ctypes.byref(call), ctypes.byref(conc), None), want,
               'pmbrl_mlp_backward_ln_workspace_bytes(conc, NULL)')
    if ln is not None:
        agrees(lib.pmbrl_mlp_ln_workspace_bytes(ctypes.byref(call), ctypes.byref(ln)), in_range, 'pmbrl_mlp_ln_workspace_bytes')
        agrees(lib.pmbrl_mlp_backward_ln_workspace_bytes(ctypes.byref(call), ctypes.byref(conc) if conc else None, ctypes.byref(ln)),
               ME.verdict(case, ME.BWD), 'pmbrl_mlp_backward_ln_workspace_bytes')
        if conc is not None:      # ... and with the layer norm alone
            agrees(lib.pmbrl_mlp_backward_ln_workspace_bytes(ctypes.byref(call), None, ctypes.byref(ln)),
                   ME.verdict(variant(case, 'c'), ME.BWD), 'pmbrl_mlp_backward_ln_workspace_bytes(NULL, ln)')


def test_accepted_workspace_sizes_follow_the_slab_rule():
    """pmbrl_mlp_backward_workspace_bytes of the two many-row cases: min(256, slab limit / slab, tiles) slabs behind the
    packed weights; one row more than a tile boundary adds a slab until the cap, none behind it."""
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    for cid, slabs in (('many_rows_w416', 256), ('slab_cap_w416', 48)):
        case = ME.by_id(cid)
        call = call_struct(case)[0]
        slab = 4 * ME.n_params(case['dims'])
        fwd = lib.pmbrl_mlp_workspace_bytes(ctypes.byref(call))
        at = lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(call))
        assert at == ((fwd + 255) & ~255) + slabs * slab, cid
        call.B = 16 * (slabs - 1)
        assert lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(call)) == at - slab
        call.B = 16 * slabs + 4000
        assert lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(call)) == at


# what each case is in the table for (regimes it must reach), beyond the LDS edges below
REACHES = {
    'w16': {'tile_groups_1_fwd', 'gemm_general_fwd'}, 'w17': {'tile_groups_1_bwd'},
    'w128': {'gemm_full_fwd', 'gemm_full_bwd'}, 'w256': {'gemm_full_fwd', 'tile_groups_1_fwd', 'tile_groups_1_bwd'},
    'w264': {'tile_groups_2_fwd', 'tile_groups_2_bwd', 'gemm_general_fwd'}, 'w272': {'tile_groups_2_fwd', 'tile_groups_2_bwd'},
    'w512': {'tile_groups_2_fwd', 'gemm_full_gt16_bwd'}, 'w512_fwd': {'gemm_full_gt16_fwd'},
    'w520': {'tile_groups_3_fwd', 'tile_groups_3_bwd'}, 'w528': {'tile_groups_3_fwd', 'tile_groups_3_bwd'},
    'w1024': {'tile_groups_4_fwd', 'gemm_full_gt16_fwd'},
    'in17': {'input_tiles_gt1'}, 'in64': {'input_tiles_gt1'}, 'in1024': {'input_or_head_gt64', 'gemm_full_gt16_fwd'},
    'head2': {'head_k_split'}, 'head48': {'head_k_split'}, 'head50': {'head_tile_split'}, 'head64': {'head_tile_split'},
    'head512': {'head_tile_split', 'input_or_head_gt64', 'tile_groups_2_fwd', 'gemm_full_gt16_bwd'},
    'head1024': {'head_tile_split', 'tile_groups_4_fwd'},
    'ks_kb1': {'k_split_1_blocks', 'k_slice_empty', 'k_slice_single'}, 'ks_kb8': {'k_split_8_blocks', 'k_slice_single'},
    'ks_kb9': {'k_split_9_blocks', 'k_slice_empty', 'k_slice_single', 'k_slice_several'},
    'ks_kb17': {'k_split_17_blocks', 'k_slice_empty', 'k_slice_several'}, 'ks_kb64': {'k_split_64_blocks', 'k_slice_chunks'},
    'nl2': {'nl2'}, 'nl8': {'nl8'}, 'e10_deep': {'nl8'}, 'e17_deep_tanh': {'nl8'}, 'act_list_none': {'nl6'},
    'w1025': {'out_of_range'}, 'head_odd': {'out_of_range'}, 'nl1': {'out_of_range'}, 'nl9': {'out_of_range'},
}
REGIMES = ['tile_groups_%d_%s' % (n, k) for n in (1, 2, 3) for k in ('fwd', 'bwd')] + [
    'tile_groups_4_fwd', 'gemm_full_fwd', 'gemm_full_bwd', 'gemm_general_fwd', 'gemm_general_bwd', 'gemm_full_gt16_fwd',
    'gemm_full_gt16_bwd', 'head_k_split', 'head_tile_split', 'k_slice_empty', 'k_slice_single', 'k_slice_several',
    'k_slice_chunks', 'input_tiles_gt1', 'input_or_head_gt64', 'nl2', 'nl8', 'out_of_range']


def test_table_reaches_every_regime():
    reached = {c['id']: ME.regimes(c) for c in ME.CASES}
    for cid, want in REACHES.items():
        assert want <= reached[cid], (cid, sorted(want - reached[cid]))
    for regime in REGIMES:
        assert any(regime in r for r in reached.values()), regime
    # (a fourth tile group in a gradient call would need a layer of 769 or more, beyond the 528 a gradient call accepts)
    assert not any('tile_groups_4_bwd' in r for r in reached.values())
    # the shape the existing tests sit at reaches none of the GEMM regimes the table is there for
    centre = ME.regimes(ME._case('centre', 0, ME.CENTRE))
    assert not centre & {r for r in REGIMES if 'tile_groups_1' not in r and 'general' not in r and
                         r not in ('head_k_split', 'k_slice_empty', 'k_slice_single')}
    # every n_buf line of the table: the last accepted width runs, in both gradient calls where both reach the line, the
    # first refused width is refused by that call
    every = set().union(*reached.values())
    for n in ME.WIDEST:
        for call in (ME.GX, ME.BWD):
            assert 'last_accepted_%s_%d' % (call, n) in every, (call, n)
            assert 'first_refused_%s_%d' % (call, n) in every, (call, n)
    for case in ME.CASES:
        r = reached[case['id']]
        for call in (ME.GX, ME.BWD):
            if call in case['calls'] and 'last_accepted_%s_%d' % (call, ME.n_buf(case, call)) in r:
                assert ME.tiles(max(case['dims'])) == ME.tiles(ME.WIDEST[ME.n_buf(case, call)]) and ME.inside(case, call), case['id']
    # ... while the calls that need less still serve it: the forward alone, the forward and the input gradient
    served = [frozenset(k for k in r if k.startswith('served_by_')) for r in reached.values() if any('first_refused' in k for k in r)]
    assert frozenset({'served_by_fwd'}) in served and frozenset({'served_by_fwd', 'served_by_gx'}) in served
    # the configurations: ReLU and smooth, 0 to 2 concrete layers, 0 to 2 layer-norm layers, at an edge each
    edge = [c for c in ME.CASES if any(k.startswith('last_accepted') for k in reached[c['id']])]
    kinds = {(any(a != ME.RELU for a in ME.codes(c)), sum('c' in s for s in c['layers']), sum('L' in s for s in c['layers'])) for c in edge}
    assert {(False, 0, 0), (True, 0, 0), (False, 1, 0), (False, 0, 1), (False, 1, 1), (False, 0, 2), (False, 2, 2), (True, 0, 2),
            (True, 1, 2), (True, 2, 2)} <= kinds, kinds


def test_activations_and_optional_inputs_are_all_there():
    wide = {a for c in ME.INSIDE if max(c['dims'][1:-1]) >= 272 and ME.inside(c, ME.BWD) for a in ME.codes(c)}
    assert wide >= {ME.RELU, ME.TANH, ME.SILU, ME.SIN, ME.EXP, ME.SINLU, ME.HHSINLU}
    assert ME.NONE in ME.codes(ME.by_id('act_list_none')) and len(ME.by_id('act_list_none')['dims']) == 7
    opts = {frozenset(c['opts']) for c in ME.INSIDE}
    assert {frozenset(), frozenset(ME.OPTIONAL)} | {frozenset({g}) for g in ME.OPTIONAL} <= opts
    assert max(ME.by_id('plain_w272')['dims']) >= 272
    # a null mask between masked layers, keep < 1 on every layer of a deep network, per-unit logits, layer norm with and
    # without a concrete mask on the same layer
    assert ME.by_id('null_mask_between')['layers'] == ['b', '-', 'b'] and ME.by_id('nl8')['layers'] == ['b'] * 7
    c = ME.problem(ME.by_id('e5_conc'))
    assert c['logit'][0].numel() == 416 and float(c['logit'][0].std()) > 0.1
    assert ME.by_id('e8_ln2_conc')['layers'] == ['Lc', 'L']
    ln_widths = {c['dims'][l + 1] for c in ME.INSIDE if ME.inside(c, ME.BWD) for l, s in enumerate(c['layers']) if 'L' in s}
    assert ln_widths >= {16, 17, 40, 208, 224, 416}
    assert ME.by_id('ln16')['dims'][1] == 16 and ME.by_id('ln17')['dims'][1] == 17


@pytest.mark.parametrize('case', ME.INSIDE, ids=lambda c: c['id'])
def test_cases_are_clear_of_the_kink_and_well_conditioned(case):
    """Every kept pre-activation of a ReLU or hhSinLU layer at least 1e-4 from 0 in the fp64 run; the forward outputs and
    every gradient tensor of the reference's fp32 run within a quarter of the bars of its fp64 run."""
    ref = ME.reference(case)
    margin = ME.kink_margin(case, ref)
    print(case['id'], 'smallest kept |pre-activation| at a kink: %.2e' % margin)
    assert margin > ME.KINK_MARGIN == 1e-4
    fwd, grads = ME.conditioning(case)
    assert (len(fwd) == 3) == ME.inside(case, ME.FWD) and bool(grads) == (ME.inside(case, ME.GX) or ME.inside(case, ME.BWD))
    ME.hold(case['id'] + ', fp32 reference', fwd, grads, share=0.25)


def test_cases_come_from_the_seed_alone():
    case = ME.by_id('e8_ln2_conc')
    a, b = ME.generate(case), ME.problem(case)
    assert all(a[k].equal(b[k]) for k in ('x', 'z', 'shift')) and all(s.equal(t) for s, t in zip(a['Ws'] + a['u'][:1], b['Ws'] + b['u'][:1]))
    assert a['x'].dtype == a['Ws'][0].dtype == a['gamma'][0].dtype
    plain = ME.problem(ME.by_id('plain_w272'))
    assert all(plain[k] is None for keys in ME.OPTIONAL.values() for k in keys) and plain['hard'] == [None, None]
