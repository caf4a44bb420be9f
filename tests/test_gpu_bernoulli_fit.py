"""GPU (-m gpu): fits of networks with fixed-rate Bernoulli dropout (BDropout), alone and mixed with concrete dropout and
with layers that have none: pmbrl_bnn_loss_grad, pmbrl_bnn_train_steps, train_regressor and the critic fit against the
reference's fixtures (tests/golden/bdropout, tools/make_golden_bdropout.py) and the fp64 oracle (oracle/ref_torch.py).
Bars: those of tests/test_gpu_activations.py::test_bnn_loss_grad_matches_reference / test_bnn_train_steps_matches_reference
and of tests/test_gpu_api.py::test_critic_fit_matches_reference."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from tests import common
from tests.common import rel
from tests.test_bernoulli_fit_oracle import STAT, binomial_moments, example_width_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)  # noqa: E731


def keeps(d):
    """BnnStep's bernoulli_keep of a fixture: None, a float, or a tensor of the layer's width."""
    out = []
    for l in range(int(d['n_layers']) - 1):
        k = np.asarray(d['keep%d' % l], np.float32) if int(d['kind%d' % l]) == R.BERNOULLI else None
        out.append(None if k is None else (float(k[0]) if k.size == 1 else torch.tensor(k)))
    return out


def bnn_step(d, M, **kw):
    from prob_mbrl_amd import engine as E
    nl = int(d['n_layers'])
    dims = [d['W0_init'].shape[1]] + [d['W%d_init' % l].shape[0] for l in range(nl)]
    kind = [int(d['kind%d' % l]) for l in range(nl - 1)]
    n_comp = int(d['n_components']) if 'n_components' in d else 0
    return E.BnnStep(dims, [float(d['temp%d' % l]) if kind[l] == R.CONCRETE else 0.0 for l in range(nl - 1)],
                     [float(d['reg_scale%d' % l]) if kind[l] else 0.0 for l in range(nl - 1)],
                     [float(d['drop_reg%d' % l]) if kind[l] == R.CONCRETE else 0.0 for l in range(nl - 1)], M, int(d['N']),
                     float(d['reg_weight']), max_log_std=float(d['max_log_std']), device=torch.device(DEV),
                     loss_kind='gmm' if n_comp > 1 else 'nll', n_components=n_comp, act=int(d['act']),
                     bernoulli_keep=kw.get('bernoulli_keep', keeps(d)))


def flat_params(d, suffix='_init'):
    keys = R.fit_problem_from_npz(d)[3]
    parts = [T(d[k + suffix]).reshape(-1) for k in keys]
    return torch.cat(parts).contiguous(), keys, [p.numel() for p in parts]


def noise(d, it):
    """u / bvar of an iteration: one [M, h] block per dropout layer of either kind (a Bernoulli layer's u block is not read)."""
    us, bs = [], []
    for l in range(int(d['n_layers']) - 1):
        kind = int(d['kind%d' % l])
        if kind == R.NONE:
            continue
        hard = T(d['hard%d_it%d' % (l, it)]).reshape(-1)
        us.append(T(d['u%d_it%d' % (l, it)]).reshape(-1) if kind == R.CONCRETE else torch.full_like(hard, 0.5))
        bs.append(1.0 - hard)
    return torch.cat(us).contiguous(), torch.cat(bs).contiguous()


def blocks(flat, keys, sizes):
    off = 0
    for key, n in zip(keys, sizes):
        yield key, flat[off:off + n].cpu().numpy()
        off += n


def replay_loss_grad(d, want_losses, want_g0, want_final):
    from prob_mbrl_amd import engine as E
    flat, keys, sizes = flat_params(d)
    Xn, Yn = T(d['Xn']), T(d['Yn'])
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    steps = {}
    for it in range(len(want_losses)):
        idx = torch.tensor(np.asarray(d['idx_it%d' % it]).astype(np.int32), device=DEV)
        M = idx.numel()
        step = steps.get(M) or steps.setdefault(M, bnn_step(d, M))
        u, bvar = noise(d, it)
        grad, loss = step.loss_grad(Xn, Yn, idx, flat, u, bvar)
        print(it, loss.cpu().numpy(), want_losses[it])
        assert np.allclose(loss.cpu().numpy(), want_losses[it], rtol=3e-5, atol=2e-6), (it, loss, want_losses[it])
        if it == 0:
            for key, g in blocks(grad, keys, sizes):
                want = np.asarray(want_g0[key]).reshape(-1)
                print(key, rel(g, want))
                assert rel(g, want) < 5e-5, key
        E.clip_adam(flat, grad, m, v, it + 1, float(d['lr']), max_norm=None)
    for key, p in blocks(flat, keys, sizes):
        assert np.allclose(p, np.asarray(want_final[key]).reshape(-1), rtol=2e-5, atol=5e-7), (key, np.abs(p - np.asarray(want_final[key]).reshape(-1)).max())


@pytest.mark.parametrize('name', common.BD_FIT)
def test_loss_grad_matches_reference(name):
    """pmbrl_bnn_loss_grad + pmbrl_clip_adam replaying every nll / mixture fixture (a plan per minibatch size: the third
    minibatch of an epoch is short)."""
    d = common.load(name)
    keys = R.fit_problem_from_npz(d)[3]
    replay_loss_grad(d, d['losses'], {k: d['g%s_it0' % k] for k in keys}, {k: d[k + '_final'] for k in keys})


@pytest.mark.parametrize('name', ['bd_nll_relu', 'bd_unit_tanh', 'bd_mixed_silu'])
def test_train_steps_match_reference(name):
    """pmbrl_bnn_train_steps with the recorded draws, one iteration per call."""
    d = common.load(name)
    flat, keys, sizes = flat_params(d)
    Xn, Yn = T(d['Xn']), T(d['Yn'])
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    stepc = torch.zeros(1, dtype=torch.int64, device=DEV)
    steps = {}
    iters = int(d['iters'])
    for it in range(iters):
        idx = torch.tensor(np.asarray(d['idx_it%d' % it]).astype(np.int32), device=DEV).reshape(1, -1).contiguous()
        M = idx.numel()
        step = steps.get(M) or steps.setdefault(M, bnn_step(d, M))
        u, bvar = noise(d, it)
        loss = step.train_steps(Xn, Yn, idx, flat, m, v, stepc, float(d['lr']), u=u, bvar=bvar)
        assert np.allclose(loss.cpu().numpy(), d['losses'][it], rtol=3e-5, atol=2e-6), (it, loss, d['losses'][it])
    assert int(stepc.item()) == iters
    for key, p in blocks(flat, keys, sizes):
        want = d[key + '_final'].reshape(-1)
        assert np.allclose(p, want, rtol=1e-4, atol=2e-6), (key, np.abs(p - want).max())


def dynamics_from_fixture(d):
    import prob_mbrl_amd as pm
    n = int(d['n_layers'])
    hid = [d['W%d_init' % i].shape[0] for i in range(n - 1)]
    Din, Dout = d['W0_init'].shape[1], d['W%d_init' % (n - 1)].shape[0] // 2
    drops = []
    for l, h in enumerate(hid):
        kind = int(d['kind%d' % l])
        if kind == R.BERNOULLI:
            k = np.asarray(d['keep%d' % l], np.float32)
            drops.append(pm.models.BDropout(float(1 - k[0]) if k.size == 1 else torch.tensor(1 - k)))
        else:
            drops.append(pm.models.CDropout(0.1 * np.ones(h)) if kind == R.CONCRETE else None)
    dyn = pm.models.DynamicsModel(pm.models.mlp(Din, 2 * Dout, hid, dropout_layers=drops, nonlin=common.act_module(d['act'])),
                                  reward_func=None,
                                  output_density=pm.models.DiagGaussianDensity(Dout)).float()
    lins = [m for m in dyn.model._modules.values() if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for i, lin in enumerate(lins):
            lin.weight.copy_(torch.tensor(d['W%d_init' % i], dtype=torch.float32))
            lin.bias.copy_(torch.tensor(d['b%d_init' % i], dtype=torch.float32))
    dyn.set_dataset(torch.tensor(d['X'], dtype=torch.float32), torch.tensor(d['Y'], dtype=torch.float32))
    return dyn, lins


class Scalars:
    def __init__(self):
        self.rows = {}

    def add_scalar(self, name, value, i):
        self.rows.setdefault(int(i), {})[name] = float(value)


@pytest.mark.parametrize('name', ['bd_nll_relu', 'bd_resample_off', 'bd_nll_relu_decoupled', 'bd_nll_relu_prioritized'])
def test_train_regressor_matches_reference(name):
    """utils.train_regressor end to end with the recorded masks (_replay), numpy seeded like the reference's run:
    bd_nll_relu on the fused path, resample=False, decoupled_reg and prioritized_sampling."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import train_regressor as TR
    d = common.load(name)
    dyn, lins = dynamics_from_fixture(d)
    opt = torch.optim.Adam([p for p in dyn.parameters() if p.requires_grad], float(d['lr']))
    dyn = dyn.to(DEV)
    n, iters = int(d['n_layers']), int(d['iters'])
    replay = dict(u=[[None] * (n - 1) for _ in range(iters)],
                  hard=[[d['hard%d_it%d' % (l, it)] for l in range(n - 1)] for it in range(iters)])
    calls = []
    from prob_mbrl_amd import engine as E
    orig = E.BnnStep.train_steps
    E.BnnStep.train_steps = lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1]
    writer = Scalars()
    TR.priority_tree.clear()
    np.random.seed(int(d['np_seed']))
    try:
        pm.utils.train_regressor(dyn, iters - 1, int(d['M']), bool(d['resample']), opt, summary_writer=writer,
                                 decoupled_reg=name.endswith('decoupled'), prioritized_sampling=name.endswith('prioritized'),
                                 _replay=replay, _warmup_iters=int(d['warmup']))
    finally:
        E.BnnStep.train_steps = orig
    assert bool(calls) == (name in ('bd_nll_relu', 'bd_resample_off'))      # the fused path where it is offered
    got = np.array([[writer.rows[it]['training_loss'], -writer.rows[it]['E_lml']] for it in range(iters)])
    want = d['losses'][:, :2]
    print(got, want)
    assert np.allclose(got[:, 1], want[:, 1], rtol=3e-5, atol=2e-6)
    if not name.endswith('decoupled'):
        assert np.allclose(got[:, 0], want[:, 0], rtol=3e-5, atol=2e-6)
    for i, lin in enumerate(lins):
        for t, key in ((lin.weight, 'W%d_final' % i), (lin.bias, 'b%d_final' % i)):
            assert np.allclose(t.detach().cpu().numpy(), d[key], rtol=1e-4, atol=2e-6), (key, np.abs(t.detach().cpu().numpy() - d[key]).max())
    if name.endswith('prioritized'):
        tree, N = TR.priority_tree[dyn], int(d['N'])
        assert np.array_equal(tree.counts[:N], d['tree_counts'])
        assert np.allclose(tree.sum_tree[tree.max_size - 1:tree.max_size - 1 + N], d['tree_leaves'], rtol=1e-3)


def test_train_regressor_applies_the_stored_mask_without_resample():
    """resample=False and no replay: the leading rows of the modules' stored masks serve every iteration (set here to the
    fixture's), and are still there afterwards."""
    import prob_mbrl_amd as pm
    d = common.load('bd_resample_off')
    dyn, lins = dynamics_from_fixture(d)
    opt = torch.optim.Adam([p for p in dyn.parameters() if p.requires_grad], float(d['lr']))
    dyn = dyn.to(DEV)
    masks = [T(d['hard%d_it0' % l]) for l in range(2)]
    for l in range(2):
        getattr(dyn.model, 'drop%d' % l).noise.data = masks[l].clone()
    np.random.seed(int(d['np_seed']))
    pm.utils.train_regressor(dyn, int(d['iters']) - 1, int(d['M']), False, opt)
    for i, lin in enumerate(lins):
        assert np.allclose(lin.weight.detach().cpu().numpy(), d['W%d_final' % i], rtol=1e-4, atol=2e-6), i
    assert all(torch.equal(getattr(dyn.model, 'drop%d' % l).noise, masks[l]) for l in range(2))


def test_critic_fit_matches_reference():
    """critic.update_value_function on a critic with Bernoulli layers, the recorded masks through _bernoulli."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd.critic import update_value_function
    d = common.load('bd_critic')
    C = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))  # noqa: E731
    n = int(d['n_layers'])
    hid = [d['W%d_init' % i].shape[0] for i in range(n - 1)]
    V = pm.models.Regressor(pm.models.mlp(d['W0_init'].shape[1], 1, hid, nonlin=torch.nn.ReLU, dropout_layers=[
        pm.models.BDropout(float(1 - np.float32(d['keep%d' % l][0]))) for l in range(n - 1)])).float()
    lins = [m for m in V.model._modules.values() if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for i, lin in enumerate(lins):
            lin.weight.copy_(C(d['W%d_init' % i]))
            lin.bias.copy_(C(d['b%d_init' % i]))
        for k in ('mx', 'iSx', 'my', 'Sy'):
            getattr(V, k).data = C(d[k]).reshape(1, -1)
    V = V.to(DEV)
    opt = torch.optim.Adam(V.parameters(), float(d['lr']))
    H, gam = int(d['H']), float(d['gamma'])
    states = [None] * (H + 1)
    states[0], states[H] = C(d['states0']).to(DEV), C(d['statesH']).to(DEV)
    rewards = [C(r).to(DEV) for r in d['rewards']]
    for it in range(int(d['n_updates'])):
        draws = [d['hard%d_it%d' % (k, it)] for k in range(2 * (n - 1))]
        update_value_function(V, opt, H, it, states, None, rewards, lambda i: gam**i, reg_weight=float(d['reg_weight']),
                              _bernoulli=draws)
        for i, lin in enumerate(lins):
            assert np.allclose(lin.weight.detach().cpu().numpy(), d['W%d_it%d' % (i, it)], rtol=5e-4, atol=5e-6), (it, i)
            assert np.allclose(lin.bias.detach().cpu().numpy(), d['b%d_it%d' % (i, it)], rtol=5e-4, atol=5e-6), (it, i)
    assert not V.training


def test_example_width_against_the_oracle():
    """6 -> 200 -> 200 -> 10, B(0.1) twice, M = 100, N = 300, two iterations: no fixture, the fp64 oracle is the reference.
    (The seeds keep every kept pre-activation clear of ReLU's kink: tests/test_bernoulli_fit_oracle.py says how far and why.)"""
    d = example_width_case()
    params, losses, g0 = R.bnn_train(d, torch.float64)
    keys = R.fit_problem_from_npz(d)[3]
    replay_loss_grad(d, np.asarray(losses), {k: g.numpy() for k, g in zip(keys, g0)},
                     {k: p.detach().numpy() for k, p in zip(keys, params)})


def _two_layer(keep, seed, n_steps=3, u=False):
    """train_steps on a 6 -> 40 -> 24 -> 8 ReLU network with Bernoulli layers of keep probability `keep`; returns the
    parameters after n_steps iterations (draws in the kernel, or bvar = 0 handed in when `u`)."""
    from prob_mbrl_amd import engine as E
    rs = np.random.RandomState(5)
    dims, M, N = [6, 40, 24, 8], 24, 60
    flat = torch.cat([T(rs.randn(dims[l + 1] * dims[l] + dims[l + 1]) * 0.3) for l in range(3)]).contiguous()
    Xn, Yn = T(rs.randn(N, 6)), T(rs.randn(N, 4))
    idx = torch.tensor(np.stack([rs.permutation(N)[:M] for _ in range(n_steps)]).astype(np.int32), device=DEV).contiguous()
    step = E.BnnStep(dims, [0.0, 0.0], [0.5, 0.5], [0.0, 0.0], M, N, device=torch.device(DEV), bernoulli_keep=[keep, keep])
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    stepc = torch.zeros(1, dtype=torch.int64, device=DEV)
    z = torch.zeros(n_steps * M * 64, device=DEV) if u else None
    step.train_steps(Xn, Yn, idx, flat, m, v, stepc, 1e-3, seed=seed, u=z, bvar=z)
    assert int(stepc.item()) == n_steps
    return flat.cpu().numpy()


def test_in_kernel_draws_with_rate_zero_are_the_replay_bits():
    """p = 1: every unit is kept whatever the variate, so the in-kernel draws give the bits of the replay form with bvar = 0."""
    assert np.array_equal(_two_layer(1.0, seed=3), _two_layer(1.0, seed=0, u=True))


def test_in_kernel_draws_repeat_under_a_seed():
    a, b, c = _two_layer(0.8, seed=3), _two_layer(0.8, seed=3), _two_layer(0.8, seed=4)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and np.isfinite(a).all()


@pytest.mark.parametrize('seed', STAT['seeds'])
def test_in_kernel_draws_keep_the_right_fraction(seed):
    """Hidden units all 1 (zero W0, b0 = 1), output weights 1 / h, targets 0, lr = 0: the mean head is K / (p h) with K the
    number of kept units, so the MSE term -- read back from the reported -E[lml], whose log-std is a constant -- has mean
    1 + (1 - p) / (p h).  Within 5 standard deviations of it, per iteration and over the 8 iterations; the standard deviation
    from the Binomial(h, p) model (tests/test_bernoulli_fit_oracle.py holds torch.bernoulli masks to the same interval)."""
    from prob_mbrl_amd import engine as E
    M, h, p, iters = STAT['M'], STAT['h'], STAT['p'], STAT['iters']
    mean, var = binomial_moments(h, p)
    dims, N, mls = [6, h, 2], 300, 1.0
    W1 = torch.zeros(2, h)
    W1[0] = 1.0 / h
    flat = torch.cat([torch.zeros(h * 6), torch.ones(h), W1.reshape(-1), torch.zeros(2)]).to(DEV).contiguous()
    before = flat.clone()
    Xn, Yn = torch.randn(N, 6, device=DEV), torch.zeros(N, 1, device=DEV)
    idx = torch.randint(0, N, (iters, M), dtype=torch.int32, device=DEV)
    step = E.BnnStep(dims, [0.0], [0.5], [0.0], M, N, max_log_std=mls, device=torch.device(DEV), bernoulli_keep=[p])
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    stepc = torch.zeros(1, dtype=torch.int64, device=DEV)
    hist = torch.empty(iters, 3, device=DEV)
    step.train_steps(Xn, Yn, idx, flat, m, v, stepc, 0.0, seed=seed, loss_hist=hist)
    assert torch.equal(flat, before)
    # -E[lml] = 1/2 exp(-2 lsc) mse + lsc + 1/2 log 2 pi, lsc = mls - softplus(mls - 0) (losses.py:16-37, densities.py:87-121)
    lsc = mls - np.log1p(np.exp(mls))
    mse = (hist[:, 1].double().cpu().numpy() - lsc - 0.5 * np.log(2 * np.pi)) * 2.0 * np.exp(2.0 * lsc)
    print(mse, mean, np.sqrt(var / M))
    assert len(set(mse.tolist())) > 1      # a fresh mask every iteration
    assert all(abs(x - mean) < 5 * np.sqrt(var / M) for x in mse), (mse, mean)
    assert abs(mse.mean() - mean) < 5 * np.sqrt(var / (M * iters)), (mse.mean(), mean)


def test_all_concrete_plan_keeps_its_bits():
    """A concrete plan created through the old BnnStep call and one created with explicit (empty) Bernoulli fields give
    bit-identical pmbrl_bnn_loss_grad output on act_bnn_tanh."""
    from prob_mbrl_amd import engine as E
    d = common.load('act_bnn_tanh')
    nl = int(d['n_layers'])
    parts = []
    for l in range(nl):
        parts += [T(d['W%d_init' % l]).reshape(-1), T(d['b%d_init' % l]).reshape(-1)]
        if l < nl - 1:
            parts.append(T(d['logit_p%d_init' % l]).reshape(-1))
    flat = torch.cat(parts).contiguous()
    dims = [d['W0_init'].shape[1]] + [d['W%d_init' % l].shape[0] for l in range(nl)]
    args = (dims, [float(d['temp%d' % l]) for l in range(nl - 1)], [float(d['reg_scale%d' % l]) for l in range(nl - 1)],
            [float(d['drop_reg%d' % l]) for l in range(nl - 1)], int(d['M']), int(d['N']), float(d['reg_weight']),
            float(d['max_log_std']), torch.device(DEV), 'nll', 0, int(d['act']))
    u = torch.cat([T(d['u%d_it0' % l]).reshape(-1) for l in range(nl - 1)]).contiguous()
    bvar = torch.cat([1.0 - T(d['hard%d_it0' % l]).reshape(-1) for l in range(nl - 1)]).contiguous()
    idx = torch.tensor(d['idx_it0'].astype(np.int32), device=DEV)
    out = []
    for kw in ({}, dict(bernoulli_keep=[None] * (nl - 1))):
        step = E.BnnStep(*args, **kw)
        assert step.n_params == flat.numel()
        grad, loss = step.loss_grad(T(d['Xn']), T(d['Yn']), idx, flat, u, bvar)
        out.append((grad.cpu().numpy().copy(), loss.cpu().numpy().copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.allclose(out[0][1], d['losses'][0], rtol=3e-5, atol=2e-6)


def test_calls_alternating_on_one_plan_are_those_of_fresh_plans():
    """Both BNN calls start from a copy of the records their plan filled when it was created.  Seven calls alternating on ONE
    BnnStep against the same calls each on a FRESH one, started from the state the shared sequence had: every output
    bit-equal.  Calls 5 and 6 would read a field call 4 (row weights) or call 5 (the generator switch) left in the plan."""
    from prob_mbrl_amd import activations
    from prob_mbrl_amd import engine as E
    rs = np.random.RandomState(11)
    dims, M, N, h = [3, 20, 20, 4], 24, 60, 40
    CALLS = (1, 2, 1, 2, 1, 2, 1)      # iterations per call: 1 is a loss_grad, 2 a train_steps
    fresh = lambda: E.BnnStep(dims, [0.7, 0.0], [0.5, 0.5], [1.0, 0.0], M, N, device=torch.device(DEV),  # noqa: E731
                              act=activations.SILU, bernoulli_keep=[None, 0.8])
    n = (3 * 20 + 20 + 20) + (20 * 20 + 20) + (20 * 4 + 4)
    Xn, Yn = T(rs.randn(N, 3)), T(rs.randn(N, 2))
    idx = [torch.tensor(np.stack([rs.permutation(N)[:M] for _ in range(k)]).astype(np.int32), device=DEV).contiguous()
           for k in CALLS]
    u = [T(rs.rand(k * M * h)) for k in CALLS]
    bvar = [T(rs.rand(k * M * h)) for k in CALLS]
    row_w = T(rs.rand(M) + 0.5)

    def call(i, step, flat, m, v, stepc):
        """Call i on `step`; the state is updated in place.  Returns every output of the call."""
        if CALLS[i] == 2:
            kw = dict(seed=7, first_step=3 + i) if i in (1, 5) else dict(u=u[i], bvar=bvar[i])
            out = [step.train_steps(Xn, Yn, idx[i], flat, m, v, stepc, 1e-2, **kw)]
        else:
            lp = torch.zeros(M, device=DEV)
            kw = {0: {}, 2: dict(terms=2), 4: dict(row_weight=row_w, row_logprob=lp), 6: {}}[i]
            out = list(step.loss_grad(Xn, Yn, idx[i].reshape(-1), flat, u[i], bvar[i], **kw)) + [lp]
        return [t.clone() for t in out + [flat, m, v, stepc]]

    shared = fresh()
    assert shared.n_params == n
    state = [T(rs.randn(n) * 0.3), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV),
             torch.zeros(1, dtype=torch.int64, device=DEV)]
    for i in range(len(CALLS)):
        start, before = [t.clone() for t in state], state[0].clone()
        got = call(i, shared, *state)
        want = call(i, fresh(), *start)
        bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t  # noqa: E731
        assert all(torch.isfinite(t).all() for t in got), i
        assert len(got) == len(want) and all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want)), i
        if CALLS[i] == 2:
            assert not torch.equal(state[0], before)      # the iterations did step
    assert int(state[3].item()) == 6


def test_bad_bernoulli_fields_are_rejected():
    from prob_mbrl_amd import _lib
    from prob_mbrl_amd import engine as E
    mk = lambda k: E.BnnStep([5, 16, 8], [0.0], [0.5], [0.0], 8, 16, device=torch.device(DEV), bernoulli_keep=[k])  # noqa: E731
    for k in (0.0, 1.5):
        with pytest.raises(_lib.PmbrlError, match=r'\(-2\).*\(0, 1\]'):
            mk(k)
    with pytest.raises(_lib.PmbrlError, match=r'\(-2\).*n must be the layer'):
        mk(torch.full((15,), 0.9))
    lib = _lib.load()
    cfg = _lib.BnnConfig()
    cfg.M, cfg.N, cfg.net.n_layers, cfg.reg_weight = 8, 16, 2, 1.0
    for i, w in enumerate([5, 16, 8]):
        cfg.net.dims[i] = w
    cfg.drop_kind[0] = 7
    plan = ctypes.c_void_p()
    assert lib.pmbrl_bnn_plan_create(ctypes.byref(cfg), 0, ctypes.byref(plan)) == -2
    assert b'unknown dropout kind' in lib.pmbrl_last_error()
    # per-unit rates on a layer that is not Bernoulli
    step = E.BnnStep([5, 16, 8], [0.1], [0.5], [1.0], 8, 16, device=torch.device(DEV))
    k = (ctypes.c_float * 16)(*([0.9] * 16))
    assert lib.pmbrl_bnn_plan_set_unit_keep(step.plan, 0, k, 16) == -2
    assert step.n_params == 5 * 16 + 16 + 16 + 16 * 8 + 8 and mk(0.9).n_params == 5 * 16 + 16 + 16 * 8 + 8


def test_deep_pilco_with_bernoulli_dynamics_runs(tmp_path):
    """examples/deep_pilco.py --dyn_dropout bernoulli at tiny sizes: one policy-search iteration ends with the checkpoints
    on disk (a dynamics model with BDropout layers fitted by train_regressor)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import sys; sys.path.insert(0, %r); import json; from examples import deep_pilco; '
            'folder, hist = deep_pilco.main(sys.argv[1:]); print("RESULT", json.dumps([folder, hist]))' % root)
    args = ['--dyn_dropout', 'bernoulli', '--ps_iters', '1', '--pol_opt_iters', '3', '--dyn_opt_iters', '20', '--control_H', '20',
            '--pred_H', '8', '--pol_batch_size', '20', '--dyn_shape', '32,32', '--pol_shape', '32,32', '-o', str(tmp_path)]
    r = subprocess.run([sys.executable, '-c', code] + args, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import json
    folder, hist = json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
    for f in ('experience.pth.tar', 'latest_dynamics.pth.tar', 'latest_policy.pth.tar'):
        assert os.path.exists(os.path.join(folder, f)), f
    assert len(hist) == 1 and all(np.isfinite(h['first_loss']) and np.isfinite(h['last_loss']) for h in hist)
