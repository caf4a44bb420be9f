"""CPU: the fp64 restatement of a learned reward head on a Gaussian-mixture dynamics model (tests/gmm_reward_ref.py)
against the reference's own runs (tests/golden/gmm_reward, tools/make_golden_gmm_reward.py), at the bar
tests/test_oracle_golden.py holds fp64 to; the fit fixture through oracle.ref_torch.bnn_train at that file's bars."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from tests import common
from tests import gmm_reward_ref as GR


@pytest.mark.parametrize('name', GR.ROLLOUTS)
def test_restatement_matches_reference_fp64(name):
    d = GR.load(name)
    D = d['x0'].shape[1]
    n = int(d['dyn_gmm_n'])
    assert d['dyn_W%d' % (int(d['dyn_n_layers']) - 1)].shape[0] == (2 * (D + 1) + 1) * n + 1
    assert d['dyn_z'].shape == (int(d['H']), d['x0'].shape[0], D + 1) and d['dyn_my'].shape == (D + 1,)
    loss, g, S, Rw = GR.reference(name)
    assert common.rel(S, d['ref64_states']) < 1e-6
    assert common.rel(Rw, d['ref64_rewards']) < 1e-6
    assert abs(loss - float(d['ref64_loss'])) <= 1e-6 * abs(float(d['ref64_loss']))
    assert common.rel(g, d['ref64_grad']) < 1e-6


@pytest.mark.parametrize('name', GR.ROLLOUTS)
def test_component_intervals_are_wide(name):
    """The device draws the component by inverse CDF from the midpoint of the recorded component's interval: no interval
    may be so narrow that rounding could flip a draw."""
    d = GR.load(name)
    assert d['min_interval'] >= GR.MIN_INTERVAL, d['min_interval']
    assert d['dyn_ucat'].shape == d['dyn_kidx'].shape
    if name == 'gr_8comp':
        assert int(d['dyn_gmm_n']) == 8 and len(np.unique(d['dyn_kidx'])) > 2


def test_exact_noise_gradient_is_another_gradient():
    d = GR.load('gr_d4')
    _, g, _ = GR.iteration(d, dyn_update=dict(exact_noise_grad=True))
    assert common.rel(g.numpy(), d['ref64_grad']) > 1e-2


def test_fit_on_d_plus_one_targets_matches_reference():
    """utils.train_regressor's iteration body with the mixture log-likelihood on D + 1 = 5 targets."""
    d = np.load(os.path.join(GR.DIR, GR.FIT + '.npz'))
    assert d['Yn'].shape[1] == 5 and int(d['n_components']) == 3 and d['W2_init'].shape[0] == (2 * 5 + 1) * 3 + 1
    params, losses, g0 = R.bnn_train(d, torch.float32)
    nl = int(d['n_layers'])
    assert np.allclose(np.array(losses), d['losses'], rtol=2e-5, atol=1e-6)
    k = 0
    for l in range(nl):
        for key in ('W%d' % l, 'b%d' % l) + (('logit_p%d' % l,) if l < nl - 1 else ()):
            assert common.rel(g0[k].numpy(), d['g' + key + '_it0']) < 2e-5, key
            assert np.allclose(params[k].detach().numpy(), d[key + '_final'], rtol=1e-5, atol=2e-7), key
            k += 1
