"""`models.param_grad()`: stand-alone Policy / DynamicsModel / critic calls that are differentiable in the network's own
Parameters (pmbrl_mlp_backward behind an autograd node), against fp64 torch autograd over the oracle's step functions.

For every case: the values inside the context are torch.equal to the call outside it (the same forward kernel), the
output requires grad inside and has no grad_fn outside, and the gradient of a fixed linear functional of the outputs
meets the per-tensor bar of tests/grad_bars.py.  The masks and the noise are the fixture's frozen ones."""
import functools

import numpy as np
import pytest
import torch

from tests import common, grad_bars

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def linears(net):
    return [m for m in net._modules.values() if isinstance(m, torch.nn.Linear)]


def params_of(net):
    return [t for lin in linears(net) for t in (lin.weight, lin.bias)]


def grads_of(net):
    return [t.grad.cpu().numpy() for t in params_of(net)]


def zero(net):
    for t in params_of(net):
        t.grad = None


@functools.lru_cache(maxsize=None)
def problem(name):
    """The fixture, its fp64 oracle networks (leaf parameters requiring grad) and a fixed set of functional weights."""
    from oracle import ref_torch as R
    d = common.load(name)
    x0, pol, dyn, spec, meta, _, _, _ = R.problem_from_npz(d, torch.float64)
    for i in range(len(pol['masks'])):
        if 'pol_rate%d' % i in d:      # per-unit rates: (h * mask) / p_j (models/modules.py:55-61)
            pol['masks'][i] = pol['masks'][i] / (1.0 - torch.tensor(np.asarray(d['pol_rate%d' % i]), dtype=torch.float64))
    for net in (pol, dyn):
        net['weights'] = [(W.requires_grad_(True), b.requires_grad_(True)) for W, b in net['weights']]
    g = torch.Generator().manual_seed(3)
    B, D = x0.shape
    U = pol['z'].shape[1]
    w = dict(u=torch.randn(B, U, generator=g), s=torch.randn(B, D, generator=g), r=torch.randn(B, 1, generator=g),
             m=torch.randn(B, D, generator=g), l=torch.randn(B, D, generator=g), a=torch.tanh(torch.randn(B, U, generator=g)),
             y=torch.randn(B, D, generator=g), x=torch.randn(B, D, generator=g))
    return d, x0, pol, dyn, spec, w


def oracle_grads(loss, net, extra=()):
    ps = [t for pair in net['weights'] for t in pair]
    gs = torch.autograd.grad(loss, ps + list(extra))
    return [g.numpy() for g in gs]


def dev(t):
    return t.float().to(DEV)


def inside_outside(fn, fn_outside=None):
    """fn() outside the context and inside it, with the checks every case shares."""
    import prob_mbrl_amd as pm
    out0 = (fn_outside or fn)()
    with pm.models.param_grad():
        out1 = fn()
    t0 = out0 if isinstance(out0, (tuple, list)) else [out0]
    t1 = out1 if isinstance(out1, (tuple, list)) else [out1]
    for a, b in zip(t0, t1):
        assert a.grad_fn is None and not a.requires_grad
        assert b.requires_grad
        assert torch.equal(a, b.detach())
    return out1


@pytest.mark.parametrize('name', ['standalone_fwd', 'standalone_fwd_u4', 'act_tanh_d4', 'unit_rates_d4'])
def test_policy_samples(name):
    """(unit_rates_d4: per-unit BDropout rates -- the gradient of a row scaled by 1 / p_j is scaled back.)"""
    from oracle import ref_torch as R
    d, x0, pol64, _, _, w = problem(name)
    _, pol = common.modules_from_fixture(d, name, DEV)
    zero(pol.model)
    u = inside_outside(lambda: pol(dev(x0), resample=False, resample_noise=False))
    (u * dev(w['u'])).sum().backward()
    ref = oracle_grads((R.policy_forward(x0, pol64) * w['u'].double()).sum(), pol64)
    grad_bars.hold(name + ' policy', grad_bars.errors(grads_of(pol.model), ref))


@pytest.mark.parametrize('name', ['standalone_fwd', 'standalone_fwd_u4'])
def test_dynamics_mean_and_log_std(name):
    from oracle import ref_torch as R
    d, x0, _, dyn64, _, w = problem(name)
    dyn, _ = common.modules_from_fixture(d, name, DEV)
    zero(dyn.model)
    a = w['a'].double()
    mean, log_std = inside_outside(lambda: dyn((dev(x0), dev(a)), return_samples=False, resample=False))
    ((mean * dev(w['m'])).sum() + (log_std * dev(w['l'])).sum()).backward()
    o = R.mlp_forward((torch.cat([x0, a], -1) - dyn64['mx']) * dyn64['iSx'], dyn64['weights'], dyn64['masks'], dyn64['keep'],
                      act=dyn64.get('act', 0))
    m64, l64 = o.split(o.shape[-1] // 2, -1)
    l64 = R.clamp_log_std(l64) + dyn64['Sy'].log()
    m64 = m64 * dyn64['Sy'] + dyn64['my']
    ref = oracle_grads((m64 * w['m'].double()).sum() + (l64 * w['l'].double()).sum(), dyn64)
    grad_bars.hold(name + ' dynamics mean / log-std', grad_bars.errors(grads_of(dyn.model), ref))


@pytest.mark.parametrize('name', ['standalone_fwd', 'standalone_fwd_u4'])
def test_dynamics_samples_with_the_analytic_reward(name):
    """... and x.requires_grad: one backward gives the parameter gradients and the input gradient."""
    from oracle import ref_torch as R
    d, x0, _, dyn64, spec, w = problem(name)
    dyn, _ = common.modules_from_fixture(d, name, DEV)
    zero(dyn.model)
    a = w['a'].double()
    x = dev(x0).requires_grad_(True)
    call = lambda xx: dyn((xx, dev(a)), return_samples=True, separate_outputs=True, deltas=False,  # noqa: E731
                          resample=False, resample_noise=False)
    nxt, rew = inside_outside(lambda: call(x), lambda: call(x.detach()))
    ((nxt * dev(w['s'])).sum() + (rew * dev(w['r'])).sum()).backward()
    x64 = x0.clone().requires_grad_(True)
    n64, r64 = R.dynamics_forward(x64, a, dyn64, spec)
    ref = oracle_grads((n64 * w['s'].double()).sum() + (r64 * w['r'].double()).sum(), dyn64, extra=[x64])
    grad_bars.hold(name + ' dynamics samples + reward',
                   grad_bars.errors(grads_of(dyn.model), ref[:-1]) + grad_bars.errors([x.grad.cpu().numpy()], ref[-1:], ['x']))


def test_critic_value():
    """A network without an output density: the zero log-std rows the kernel's head is padded with are sliced away."""
    from oracle import ref_torch as R
    d = common.load('ext_value')
    V = common.value_from_fixture(d, DEV)
    val64 = R.value_from_npz(d, torch.float64)
    val64['weights'] = [(W.requires_grad_(True), b.requires_grad_(True)) for W, b in val64['weights']]
    x0 = torch.tensor(np.asarray(d['x0']), dtype=torch.float64)
    w = torch.randn(x0.shape[0], 1, generator=torch.Generator().manual_seed(4))
    zero(V.model)
    v = inside_outside(lambda: V(dev(x0), resample=False))
    assert v.shape == (x0.shape[0], 1)
    (v * dev(w)).sum().backward()
    assert [tuple(t.grad.shape) for t in params_of(V.model)] == [tuple(t.shape) for t in params_of(V.model)]
    ref = oracle_grads((R.value_forward(x0, val64) * w.double()).sum(), val64)
    grad_bars.hold('critic', grad_bars.errors(grads_of(V.model), ref))


def test_mixture_head_log_likelihood():
    """return_samples=False of the mixture head into losses.gaussian_mixture_log_likelihood: the head's torch formulas
    carry the gradient into the raw head rows."""
    import prob_mbrl_amd as pm
    from oracle import ref_torch as R
    name = 'gmm_d4'
    d, x0, _, dyn64, _, w = problem(name)
    dyn, _ = common.modules_from_fixture(d, name, DEV)
    zero(dyn.model)
    a, y = w['a'].double(), w['y'].double()
    outs = inside_outside(lambda: dyn((dev(x0), dev(a)), return_samples=False, resample=False, normalize=False))
    pm.losses.gaussian_mixture_log_likelihood(dev(y), *outs).mean().backward()
    o = R.mlp_forward(torch.cat([x0, a], -1), dyn64['weights'], dyn64['masks'], dyn64['keep'], act=dyn64.get('act', 0))
    ref = oracle_grads(R.row_log_likelihood(o, y, n_components=dyn64['gmm_n']).mean(), dyn64)
    grad_bars.hold('mixture log-likelihood', grad_bars.errors(grads_of(dyn.model), ref))


def test_autograd_contract():
    """.grad accumulates over backward calls; torch.autograd.grad on a subset; a frozen parameter gets None; numpy in
    gives numpy out; no graph under torch.no_grad()."""
    import prob_mbrl_amd as pm
    name = 'standalone_fwd'
    d, x0, _, _, _, w = problem(name)
    _, pol = common.modules_from_fixture(d, name, DEV)
    ps = params_of(pol.model)
    zero(pol.model)
    with pm.models.param_grad():
        u = pol(dev(x0), resample=False, resample_noise=False)
        (u * dev(w['u'])).sum().backward()
        once = [t.grad.clone() for t in ps]
        u = pol(dev(x0), resample=False, resample_noise=False)
        (u * dev(w['u'])).sum().backward()
        for t, g in zip(ps, once):
            assert torch.equal(t.grad, g + g)
        # a subset, through torch.autograd.grad: the same bits, and .grad is left alone
        u = pol(dev(x0), resample=False, resample_noise=False)
        gW1, gb0 = torch.autograd.grad((u * dev(w['u'])).sum(), [ps[2], ps[1]])
        assert torch.equal(gW1, once[2]) and torch.equal(gb0, once[1])
        for t, g in zip(ps, once):
            assert torch.equal(t.grad, g + g)
        # a frozen parameter
        zero(pol.model)
        ps[0].requires_grad_(False)
        u = pol(dev(x0), resample=False, resample_noise=False)
        (u * dev(w['u'])).sum().backward()
        assert ps[0].grad is None
        for t, g in zip(ps[1:], once[1:]):
            assert torch.equal(t.grad, g)
        # all frozen and a plain x: nothing to differentiate
        for t in ps:
            t.requires_grad_(False)
        assert not pol(dev(x0), resample=False, resample_noise=False).requires_grad
        for t in ps:
            t.requires_grad_(True)
        un = pol(x0.float().numpy(), resample=False, resample_noise=False)
        assert isinstance(un, np.ndarray) and np.array_equal(un, u.detach().cpu().numpy())
        with torch.no_grad():
            assert not pol(dev(x0), resample=False, resample_noise=False).requires_grad
