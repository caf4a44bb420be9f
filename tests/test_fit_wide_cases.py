"""CPU: the table of tests/fit_wide_cases.py holds only fits the resident form's LDS map refuses and the spill form's
takes, its ReLU cases are clear of the kink, and every case is well conditioned -- the oracle's own fp32 run stays within a
quarter of each bar the GPU test holds (tests/test_gpu_fit_spill.py), at the widths' longer sums too."""
import numpy as np
import pytest

from tests import common
from tests import fit_envelope_cases as FE
from tests import fit_wide_cases as FW


def test_every_case_is_spill_only():
    for case in FW.CASES:
        act = FE.TANH if 'acts' in case else case['act']      # (anything but ReLU keeps the derivative buffer)
        assert FE.lds_bytes(case['dims'], act) > FE.LDS_LIMIT, case['id']
        assert FW.spill_fits(case['dims']), case['id']
        assert case['M'] <= 33 and case['N'] == 60


def test_table_holds_the_cases_it_is_there_for():
    by = {c['id']: c for c in FW.CASES}
    assert by['w272_refused']['dims'] == [6, 272, 272, 8] and by['w272_refused']['kinds'] == (FE.B, FE.C)
    assert by['w256_tanh_refused']['dims'] == [6, 256, 256, 8] and by['w256_tanh_refused']['act'] == FE.TANH
    wide = [c for c in FW.CASES if c['dims'] == [40, 512, 512, 512, 64]]
    assert sorted(c['M'] for c in wide) == [1, 20, 33]
    assert any(c['act'] == FE.SILU and c['kinds'] == (FE.C, FE.B, FE.C) and c['M'] == 20 for c in wide)
    assert any(c['act'] == FE.RELU and c['kinds'] == (FE.B, FE.N, FE.C) and c['M'] == 33 for c in wide)
    layered = [c for c in FW.CASES if 'acts' in c]
    assert layered and all(c['acts'][-1] == FW.ACT.HHSINLU and FE.N in c['kinds'] for c in layered)
    assert by['gmm_w320']['dims'] == [6, 320, 320, 53] and by['gmm_w320']['n_components'] == 4
    edge = by['w688_edge']
    assert max(edge['dims']) == FW.WIDEST and len(edge['dims']) == 3
    assert not FW.spill_fits([6, FW.WIDEST + 1, 8])


def test_cases_are_fits_the_helpers_understand():
    for case in FW.CASES:
        d = FW.problem(case)
        dims = [d['W0_init'].shape[1]] + [d['W%d_init' % l].shape[0] for l in range(int(d['n_layers']))]
        assert dims == case['dims'] and int(d['iters']) == 2 and len(d['idx_it1']) == case['M'] == int(d['M'])
        assert np.array_equal(FW.generate(case)['W0_init'], d['W0_init'])      # from the seed alone
        dev = FW.for_device(case, d)
        if 'acts' in case:
            assert FW.ACT.unpack(dev['act'], len(dims) - 2) == case['acts'] and dev['act'] != d['act']
            assert dev['W0_init'] is d['W0_init']
        else:
            assert dev is d


@pytest.mark.parametrize('case', [c for c in FW.CASES if FW.all_relu(c)], ids=lambda c: c['id'])
def test_relu_cases_stay_clear_of_the_kink(case):
    d = FW.problem(case)
    margins = common.kink_margin(d), common.kink_margin(FW.reference(case)['second'])
    print(case['id'], 'smallest kept |pre-activation|: %.2e, %.2e' % margins)
    assert min(margins) > FE.KINK_MARGIN == 1e-5


@pytest.mark.parametrize('case', FW.CASES, ids=lambda c: c['id'])
def test_cases_are_well_conditioned(case):
    """Losses and per-tensor gradients of both iterations: the oracle's fp32 run within a quarter of the bars of its fp64 run."""
    d = FW.problem(case)
    for it, loss_fig, grad_figs in FE.conditioning(d, FW.reference(case)):
        FE.hold('%s iteration %d, fp32 oracle' % (case['id'], it), loss_fig, grad_figs, share=0.25)
