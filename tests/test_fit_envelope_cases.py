"""CPU: the table of tests/fit_envelope_cases.py reaches every branch of the fit kernels it is there for (by the kernels'
own arithmetic, mirrored), its ReLU cases are clear of the kink, every case is well conditioned -- the oracle's own fp32
run stays within a quarter of each bar the GPU test holds -- and plan creation refuses what lies behind the LDS edge
(validation comes before the first device call)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from tests import common
from tests import fit_envelope_cases as FE
from tests.test_bernoulli_fit_oracle import KINK_MARGIN

# what each case is in the table for
REACHES = {
    'in20': {'input_tiles_gt1'},
    'one_hidden': {'nl2', 'm_mod16_1'},
    'eight_linear': {'nl8', 'nl_gt4', 'bernoulli', 'concrete', 'no_dropout'},
    'kb8': {'gemm_group_full_fwd', 'gemm_group_full_bwd'},
    'w256_edge': {'gemm_group_full_fwd', 'gemm_group_full_bwd', 'lds_edge', 'dw_from_16_tiles', 'dw_n_it5', 'dw_n_it6'},
    'w272_relu': {'gemm_second_group_fwd', 'gemm_second_group_bwd', 'tail_second_group', 'dw_from_17_tiles', 'dw_n_it5',
                  'dw_n_it6', 'input_tiles_gt1', 'relu'},
    'w272_silu': {'gemm_second_group_fwd', 'gemm_second_group_bwd', 'tail_second_group', 'dw_from_17_tiles', 'silu', 'concrete'},
    'nt4': {'dw_n_it4'},
    'nt5': {'dw_n_it5'},
    'head64': {'head_tile_split', 'gaussian'},
    'gmm_head53': {'head_tile_split', 'mixture', 'mixture_gt2'},
    'gmm_8comp': {'mixture', 'mixture_gt2', 'mixture_max_comp'},
    'm1_bern': {'m1', 'relu'},
    'm1_tanh': {'m1', 'tanh'},
    'm16': {'m_mod16_0'},
    'm17': {'m_mod16_1'},
    'm144': {'tail_chunks_9_16'},
    'm272': {'tail_chunks_gt16'},
    'm144_w144': {'tail_chunks_9_16', 'tail_restore'},
}
# every regime the fit path has and the recorded fixtures do not reach
REGIMES = ['gemm_group_full_fwd', 'gemm_group_full_bwd', 'gemm_second_group_fwd', 'gemm_second_group_bwd', 'head_tile_split',
           'tail_chunks_9_16', 'tail_chunks_gt16', 'tail_second_group', 'tail_restore', 'input_tiles_gt1',
           'nl2', 'nl8', 'nl_gt4', 'm1', 'm_mod16_0', 'm_mod16_1', 'dw_n_it4', 'dw_n_it5', 'dw_from_16_tiles', 'dw_from_17_tiles', 'mixture_gt2',
           'mixture_max_comp', 'lds_edge', 'bernoulli', 'concrete', 'no_dropout', 'relu', 'tanh', 'silu', 'gaussian', 'mixture']


def test_mirrors_of_the_kernels_arithmetic():
    assert [FE.tiles(w) for w in (1, 16, 17, 112, 113, 128, 256, 257, 272)] == [1, 1, 2, 7, 8, 8, 16, 17, 17]
    # build_dw_blocks: split(n, 7) of the input tiles, split(n, 4) of the output tiles
    assert FE.split(4, 7) == [4] and FE.split(5, 7) == [5] and FE.split(8, 7) == [4, 4]
    assert FE.split(16, 7) == [6, 5, 5] and FE.split(17, 7) == [6, 6, 5] and FE.split(17, 4) == [4, 4, 3, 3, 3]
    assert FE.split(13, 7) == [7, 6] and FE.split(1, 7) == [1]
    # pm_bnn_lds_floats at the edge the issue quotes: 161 792 of 163 840 bytes
    assert FE.lds_bytes([6, 256, 256, 8], FE.RELU) == 161792 <= FE.LDS_LIMIT
    assert FE.lds_bytes([6, 256, 256, 8], FE.TANH) > FE.LDS_LIMIT and FE.lds_bytes([6, 272, 272, 8], FE.RELU) > FE.LDS_LIMIT


def test_table_reaches_every_regime():
    reached = {c['id']: FE.regimes(c) for c in FE.CASES}
    assert set(REACHES) == set(reached)
    for cid, want in REACHES.items():
        assert want <= reached[cid], (cid, sorted(want - reached[cid]))
    for regime in REGIMES:
        assert any(regime in r for r in reached.values()), regime
    # the recorded fixtures' own shape reaches none of the GEMM, tail and dW regimes the table is there for
    centre = FE.regimes(FE._case('centre', 0, FE.CENTRE, 24, FE.RELU, [FE.B, FE.C]))
    assert not centre & set(REGIMES[:10]) and not centre & {'dw_n_it4', 'dw_n_it5', 'lds_edge', 'nl2', 'nl8', 'm1'}


def test_cases_are_fits_the_helpers_understand():
    for case in FE.CASES:
        d = FE.problem(case)
        dims = [d['W0_init'].shape[1]] + [d['W%d_init' % l].shape[0] for l in range(int(d['n_layers']))]
        assert dims == case['dims'] and int(d['iters']) == 2 and len(d['idx_it1']) == case['M'] == int(d['M'])
        assert d['Yn'].shape[0] == d['Xn'].shape[0] == int(d['N']) >= case['M']
        for l, kind in enumerate(case['kinds']):
            for it in range(2):
                if kind != FE.N:
                    hard = d['hard%d_it%d' % (l, it)]
                    assert hard.shape == (case['M'], dims[l + 1]) and set(np.unique(hard)) <= {0.0, 1.0}
                if kind == FE.C:
                    assert d['u%d_it%d' % (l, it)].dtype == np.float32
        assert all(np.asarray(v).dtype != np.float64 for k, v in d.items() if isinstance(v, np.ndarray) and 'idx' not in k)
        assert np.array_equal(FE.generate(case)['W0_init'], d['W0_init'])      # from the seed alone


def test_oracle_hands_back_every_iterations_gradient():
    """bnn_train's `grads` list: its first entry is the first-iteration gradient the call returns anyway, and the call
    without the list gives what it gave."""
    d = FE.problem(FE.by_id('one_hidden'))
    grads = []
    p1, l1, g1 = R.bnn_train(d, torch.float64, grads=grads)
    p0, l0, g0 = R.bnn_train(d, torch.float64)
    assert len(grads) == 2 and l0 == l1
    assert all(torch.equal(a, b) for a, b in zip(g0, g1)) and all(torch.equal(a, b) for a, b in zip(g0, grads[0]))
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    assert any(not torch.equal(a, b) for a, b in zip(grads[0], grads[1]))


@pytest.mark.parametrize('case', [c for c in FE.CASES if c['act'] == FE.RELU], ids=lambda c: c['id'])
def test_relu_cases_stay_clear_of_the_kink(case):
    """In the fp64 replay of both iterations, and where the second iteration of the comparisons starts (the fp64 run's
    parameters after its first step, cast to fp32)."""
    d = FE.problem(case)
    margins = common.kink_margin(d), common.kink_margin(FE.reference(case)['second'])
    print(case['id'], 'smallest kept |pre-activation|: %.2e, %.2e' % margins)
    assert min(margins) > KINK_MARGIN == FE.KINK_MARGIN == 1e-5


@pytest.mark.parametrize('case', FE.CASES, ids=lambda c: c['id'])
def test_cases_are_well_conditioned(case):
    """Losses and per-tensor gradients of both iterations: the oracle's fp32 run within a quarter of the bars of its fp64 run."""
    d = FE.problem(case)
    for it, loss_fig, grad_figs in FE.conditioning(d, FE.reference(case)):
        FE.hold('%s iteration %d, fp32 oracle' % (case['id'], it), loss_fig, grad_figs, share=0.25)


def _config(dims, act):
    from prob_mbrl_amd import _lib
    cfg = _lib.BnnConfig()
    cfg.M, cfg.N = 20, 60
    cfg.net.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        cfg.net.dims[i] = v
    cfg.reg_weight, cfg.act = 1.0, act
    for l in range(len(dims) - 2):
        cfg.drop_kind[l], cfg.bern_keep[l] = _lib.DROP_BERNOULLI, 0.9
    return cfg


@pytest.mark.parametrize('dims, act', [([6, 272, 272, 8], FE.RELU), ([6, 256, 256, 8], FE.TANH)])
def test_plan_creation_refuses_behind_the_lds_edge(dims, act):
    """One tile wider than w256_edge, and w256_edge with an activation that keeps a derivative buffer: -3 and a message
    before any device call.  (The accepted side, w256_edge itself, is the GPU test's.)"""
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    assert FE.lds_bytes(dims, act) > FE.LDS_LIMIT
    plan = ctypes.c_void_p()
    assert lib.pmbrl_bnn_plan_create(ctypes.byref(_config(dims, act)), 0, ctypes.byref(plan)) == -3
    assert b'LDS' in lib.pmbrl_last_error() and not plan
