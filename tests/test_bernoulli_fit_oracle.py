"""CPU: the fp64 oracle (oracle/ref_torch.py: fit_loss, critic_loss over layers of any dropout kind) on fits with
fixed-rate Bernoulli dropout, alone or mixed with concrete dropout and with layers that have none, against the reference's fixtures
(tests/golden/bdropout, tools/make_golden_bdropout.py; recorded with the reference's modules in double precision), the C
ABI additions, and the Bernoulli model behind the statistical GPU test."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from prob_mbrl_amd import activations as ACT
from tests import common
from tests.common import rel

TOL = 1e-6


@pytest.mark.parametrize('name', common.BD_FIT)
def test_oracle_fit_matches_reference(name):
    """Losses of every iteration, gradients of iteration 0 and the parameters after the last Adam step."""
    d = common.load(name)
    params, losses, g0 = R.bnn_train(d, torch.float64)
    assert np.allclose(losses, d['losses'], rtol=TOL, atol=0), np.abs(np.asarray(losses) / d['losses'] - 1).max()
    keys = R.fit_problem_from_npz(d)[3]
    assert len(keys) == len(params) == len(g0)
    for k, p, g in zip(keys, params, g0):
        assert rel(g.numpy(), d['g%s_it0' % k]) < TOL, k
        assert rel(p.detach().numpy(), d[k + '_final']) < TOL, k


def test_oracle_critic_fit_matches_reference():
    d = common.load('bd_critic')
    keys = R.fit_problem_from_npz(d)[3]
    updates = R.critic_train(d, torch.float64)
    assert len(updates) == int(d['n_updates']) and all(len(got) == len(keys) for got in updates)
    for it, got in enumerate(updates):
        for k, v in zip(keys, got):
            assert rel(v.numpy(), d['%s_it%d' % (k, it)]) < TOL, (it, k)


def test_fixture_shapes_are_the_tabulated_ones():
    """What the cases are there for: a partial 16-row tile, widths that are no multiple of 16, mixed kinds, per-unit rates,
    one stored mask when resample is off."""
    shape = lambda d: [d['W0_init'].shape[1]] + [d['W%d_init' % l].shape[0] for l in range(int(d['n_layers']))]  # noqa: E731
    kinds = lambda d: [int(d['kind%d' % l]) for l in range(int(d['n_layers']) - 1)]  # noqa: E731
    d = common.load('bd_nll_relu')
    assert shape(d) == [6, 40, 24, 8] and kinds(d) == [2, 2] and int(d['M']) == 24 and int(d['N']) == 60 and int(d['iters']) == 4
    assert np.allclose(d['keep0'], 0.9) and np.allclose(d['keep1'], 0.75)
    d = common.load('bd_unit_tanh')
    assert shape(d) == [6, 40, 40, 8] and kinds(d) == [2, 2] and int(d['act']) == ACT.TANH
    assert np.allclose(d['keep0'], 1 - np.linspace(0.05, 0.5, 40)) and np.allclose(d['keep1'], 0.9)
    d = common.load('bd_mixed_silu')
    assert shape(d) == [5, 32, 40, 16, 6] and kinds(d) == [2, 1, 0] and int(d['act']) == ACT.SILU and int(d['M']) == 20
    d = common.load('bd_gmm')
    assert shape(d) == [6, 40, 24, (2 * 4 + 1) * 2 + 1] and int(d['n_components']) == 2 and int(d['iters']) == 3
    d = common.load('bd_critic')
    assert shape(d) == [4, 40, 24, 1] and kinds(d) == [2, 2] and d['states0'].shape[0] == 24 and int(d['n_updates']) == 2
    d = common.load('bd_resample_off')
    assert int(d['resample']) == 0 and int(d['iters']) == 3
    m = [len(d['idx_it%d' % it]) for it in range(3)]
    for l in range(2):      # every iteration applies the leading rows of ONE mask
        for it in range(1, 3):
            assert np.array_equal(d['hard%d_it%d' % (l, it)], d['hard%d_it0' % l][:m[it]])
    for name in common.BD_FIT + common.BD_OPTS + common.BD_CRITIC:
        path = common.path_of(name)
        assert os.path.getsize(path) < 100 * 1024
        raw = np.load(path, allow_pickle=False)
        assert all(raw[k].dtype.kind in 'biuf' for k in raw.files), name


def test_library_exports_unit_keep_and_config_mirror_has_the_fields():
    from prob_mbrl_amd import _lib
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'pmbrl_bnn_plan_set_unit_keep')
    assert 'pmbrl_bnn_plan_set_unit_keep' in _lib.EXPORTS
    names = [f[0] for f in _lib.BnnConfig._fields_]
    assert names[-3:] == ['act', 'drop_kind', 'bern_keep']
    assert _lib.BnnConfig.drop_kind.size == 4 * _lib.MAX_LAYERS == _lib.BnnConfig.bern_keep.size
    assert _lib.BnnConfig.drop_kind.offset == _lib.BnnConfig.act.offset + 4
    assert _lib.load().pmbrl_version() == 8 and ctypes.sizeof(_lib.MLP) == 4 + 4 * 9 + 4 * 8


def _config(**kw):
    from prob_mbrl_amd import _lib
    cfg = _lib.BnnConfig()
    cfg.M, cfg.N = 8, 16
    cfg.net.n_layers = 2
    for i, v in enumerate([5, 16, 8]):
        cfg.net.dims[i] = v
    cfg.reg_weight = 1.0
    cfg.drop_kind[0] = kw.get('kind', 1)
    cfg.bern_keep[0] = kw.get('keep', 0.9)
    return cfg


@pytest.mark.parametrize('kw, text', [(dict(keep=0.0), b'(0, 1]'), (dict(keep=1.5), b'(0, 1]'),
                                      (dict(keep=float('nan')), b'(0, 1]'), (dict(kind=7), b'unknown dropout kind')])
def test_plan_creation_rejects_bad_bernoulli_fields(kw, text):
    """Validation comes before the first device call: -2 and a message, with no GPU."""
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    plan = ctypes.c_void_p()
    assert lib.pmbrl_bnn_plan_create(ctypes.byref(_config(**kw)), 0, ctypes.byref(plan)) == -2
    assert text in lib.pmbrl_last_error() and not plan


def binomial_moments(h, p):
    """Mean and variance of o^2 for o = K / (p h), K ~ Binomial(h, p): the squared output of a network whose h hidden
    units are 1 and whose output weights are 1 / h, under Bernoulli dropout with keep probability p."""
    from math import comb
    k = np.arange(h + 1, dtype=np.float64)
    pmf = np.array([comb(h, int(i)) for i in k], dtype=np.float64) * p**k * (1 - p)**(h - k)
    o2 = (k / (p * h))**2
    mean = float((pmf * o2).sum())
    return mean, float((pmf * o2**2).sum() - mean**2)


STAT = dict(M=256, h=40, p=0.8, iters=8, seeds=(11, 12, 13))


def test_bernoulli_model_of_the_statistical_test():
    """E[o^2] = 1 + (1 - p) / (p h); torch.bernoulli masks through the oracle's MSE term stay within 5 standard deviations
    of it, per iteration (M rows) and over the 8 iterations, for the seeds tests/test_gpu_bernoulli_fit.py uses."""
    M, h, p, iters = STAT['M'], STAT['h'], STAT['p'], STAT['iters']
    mean, var = binomial_moments(h, p)
    assert abs(mean - (1 + (1 - p) / (p * h))) < 1e-12
    weights = [(torch.zeros(h, 6, dtype=torch.float64), torch.ones(h, dtype=torch.float64)),
               (torch.cat([torch.full((1, h), 1.0 / h, dtype=torch.float64), torch.zeros(1, h, dtype=torch.float64)]),
                torch.zeros(2, dtype=torch.float64))]
    layers = [dict(kind=R.BERNOULLI, keep=torch.full((h,), p, dtype=torch.float64), reg_scale=0.5)]
    x, y = torch.randn(M, 6, dtype=torch.float64), torch.zeros(M, 1, dtype=torch.float64)

    def mse_term(hard):      # mean squared error of the mean head (pmbrl_bnn_config.loss_kind 1)
        o = R.bnn_forward(x, weights, layers, [None], [None], [hard], ACT.RELU)
        return ((o[:, :y.shape[1]] - y)**2).mean()

    for seed in STAT['seeds']:
        torch.manual_seed(seed)
        mse = [float(mse_term(torch.bernoulli(torch.full((M, h), p, dtype=torch.float64)))) for _ in range(iters)]
        assert all(abs(v - mean) < 5 * np.sqrt(var / M) for v in mse), mse
        assert abs(np.mean(mse) - mean) < 5 * np.sqrt(var / (M * iters)), mse


# The example's width against the oracle (tests/test_gpu_bernoulli_fit.py): ReLU's derivative jumps at 0, so a kept unit
# whose pre-activation is closer to 0 than single precision resolves it may fall on either side, and then no fp32 gradient
# can be held to the fp64 one.  A pre-activation of the 200-wide layers is a sum of 200 products of size ~0.1 of
# parameters that carry a rounding of 6e-8 each (and, after an Adam step, the step's own rounding, a few 1e-8): an
# error of about sqrt(200) * 0.1 * 6e-8 ~ 1e-7, at the worst 200 * 0.1 * 6e-8 ~ 1e-6.  The case keeps ten times the
# latter between every kept pre-activation and 0.
KINK_MARGIN = 1e-5
EXAMPLE_SEEDS = (72, 72)      # numpy's (weights, data, minibatches), torch's (masks)


def example_width_case(seeds=EXAMPLE_SEEDS):
    """6 -> 200 -> 200 -> 10, B(0.1) twice, M = 100, N = 300, two iterations, as a fixture-like dict for ref_torch.bnn_train."""
    rs = np.random.RandomState(seeds[0])
    dims, M, N = [6, 200, 200, 10], 100, 300
    d = dict(n_layers=3, act=ACT.RELU, N=N, M=M, iters=2, lr=1e-3, reg_weight=1.0, max_log_std=1.0)
    for l in range(3):
        d['W%d_init' % l] = (rs.randn(dims[l + 1], dims[l]) * np.sqrt(2.0 / dims[l])).astype(np.float32)
        d['b%d_init' % l] = rs.uniform(-0.1, 0.1, dims[l + 1]).astype(np.float32)
    for l in range(2):
        d['kind%d' % l], d['keep%d' % l], d['reg_scale%d' % l] = R.BERNOULLI, np.array([np.float32(0.9)]), 0.5
    d['Xn'] = rs.randn(N, 6).astype(np.float32)
    d['Yn'] = (0.3 * rs.randn(N, 5) + 0.5 * d['Xn'][:, :5] * d['Xn'][:, 5:]).astype(np.float32)
    torch.manual_seed(seeds[1])
    for it in range(2):
        d['idx_it%d' % it] = rs.permutation(N)[:M]
        for l in range(2):
            d['hard%d_it%d' % (l, it)] = torch.bernoulli(torch.full((M, 200), 0.9)).numpy()
    return d


def test_example_width_case_is_clear_of_the_relu_kink():
    """The seeds of the example-width case are the first pair of (71, 72), (72, 72), ... whose fp64 replay keeps every kept
    pre-activation KINK_MARGIN away from 0: with (71, 72) a unit of the second layer sits at -2.6e-8 in iteration 1."""
    assert common.kink_margin(example_width_case()) > KINK_MARGIN
    assert EXAMPLE_SEEDS == (72, 72) and common.kink_margin(example_width_case((71, 72))) < 1e-7
