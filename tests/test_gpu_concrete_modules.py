"""models.param_grad() with concrete dropout in train() mode: a stand-alone Regressor / Policy / critic call is
differentiable in drop*.logit_p as well as in the Linear parameters (pmbrl_mlp_backward_concrete behind the autograd node
of BSequential.device_forward).  With the draws forced (CDropout._forced_samples), every gradient is held to the fp64
restatement (tests/concrete_policy_ref.py) at the bar of tests/grad_bars.py, each tensor on its own.

eval() mode and calls outside param_grad() are what they were: no logit gradient, the same outputs."""
from functools import partial

import numpy as np
import pytest
import torch

from tests import common, grad_bars
from tests import concrete_policy_ref as CP

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MLS = float(np.log(5.0))
RELU, TANH, SILU = 0, 1, 2


def case(act, seed, B=21, dims=(5, 24, 40, 4), kinds=('c', 'c')):
    return CP.standalone(list(dims), act, B, seed, 0.1, list(kinds))


def build(c, kind, scalar_logit=False):
    """The module of a case: 'gauss' Regressor with a DiagGaussianDensity, 'policy', or 'plain' (a critic: no output
    density, one output: the first row of the case's head).  Its draws are forced: one recorded hard sample per call."""
    import prob_mbrl_amd as pm
    dims, n = c['dims'], c['n_out']
    hid = dims[1:-1]
    drops = []
    for l, k in enumerate(c['kinds']):
        if k == 'c':
            drops.append(pm.models.CDropout(0.1 if scalar_logit else 0.1 * np.ones(hid[l]), temperature=c['temp'][l]))
        else:
            drops.append(pm.models.BDropout(0.2) if k == 'b' else None)
    density = partial(pm.models.DiagGaussianDensity, n) if kind == 'policy' else None
    net = pm.models.mlp(dims[0], n if kind == 'plain' else 2 * n, hid, dropout_layers=drops,
                        nonlin=common.act_module(c['act']), output_nonlin=density)
    if kind == 'policy':
        mod = pm.models.Policy(net, c['sqs'] + c['sqb'], c['sqb'] - c['sqs'])
    else:
        mod = pm.models.Regressor(net, output_density=pm.models.DiagGaussianDensity(n) if kind == 'gauss' else None)
    lins = [m for m in net._modules.values() if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for i, lin in enumerate(lins):
            last = kind == 'plain' and i == len(lins) - 1
            lin.weight.copy_(c['Ws'][i][:n] if last else c['Ws'][i])
            lin.bias.copy_(c['bs'][i][:n] if last else c['bs'][i])
        for l, dr in enumerate(drops):
            if c['kinds'][l] == 'c':
                if scalar_logit:
                    dr.logit_p.fill_(float(c['logit'][l].mean()))
                else:
                    dr.logit_p.copy_(c['logit'][l])
                dr.noise.data = c['u'][l].clone()
                dr.concrete_noise = torch.zeros_like(c['u'][l])
            elif c['kinds'][l] == 'b':
                dr.noise.data = c['hard'][l].clone()
        if kind == 'policy':
            net.fc_nonlin.z.data = c['z'].clone()
        else:
            mod.mx.data, mod.iSx.data = c['shift'][None].clone(), c['iscale'][None].clone()
            mod.my.data, mod.Sy.data = c['osh'][None].clone(), c['osc'][None].clone()
    mod = mod.float().to(DEV)
    return mod, lins, drops


def force(c, drops, calls=1):
    for l, dr in enumerate(drops):
        if c['kinds'][l] == 'c':
            dr._forced_samples = [c['hard'][l] for _ in range(calls)]


def call(mod, kind, x):
    if kind == 'policy':
        return (mod(x, resample=False, return_samples=True, resample_noise=False),)
    if kind == 'plain':
        return (mod(x, resample=False),)
    return mod(x, resample=False)


def reference(c, kind, scalar_logit=False):
    """fp64: (outputs, [grad W0, grad b0, ...], [grad logit_p or None], smallest kept |pre-activation|) of
    sum(out_k * up_k)."""
    d = lambda t: t.double()  # noqa: E731
    weights = [(d(W).requires_grad_(True), d(b).requires_grad_(True)) for W, b in zip(c['Ws'], c['bs'])]
    logits = [None if t is None else (d(t).mean() if scalar_logit else d(t)).requires_grad_(True) for t in c['logit']]
    us = [d(t) if t is not None else None for t in c['u']]
    hards = [None if h is None else (d(h) if k == 'c' else d(h) / keep) for h, k, keep in zip(c['hard'], c['kinds'], c['keep'])]
    x, n, margin = d(c['x']), c['n_out'], []
    if kind == 'policy':
        o = CP.mlp(x, weights, c['act'], logits, us, c['temp'], hards, margin)
        mu, ls = o[:, :n], -torch.nn.functional.softplus(-o[:, n:] + MLS) + MLS
        outs = (d(c['sqs']) * torch.tanh(mu + d(c['z']) * ls.exp()) + d(c['sqb']),)
    else:
        o = CP.mlp((x - d(c['shift'])) * d(c['iscale']), weights, c['act'], logits, us, c['temp'], hards, margin)
        if kind == 'plain':
            outs = (o[:, :n] * d(c['osc']) + d(c['osh']),)
        else:
            ls = -torch.nn.functional.softplus(-o[:, n:] + MLS) + MLS
            outs = (o[:, :n] * d(c['osc']) + d(c['osh']), ls + d(c['osc']).log())
    sum((o_ * d(up)).sum() for o_, up in zip(outs, c['up'])).backward()
    gp = [t.grad for pair in weights for t in pair]
    if kind == 'plain':      # (the module has the first n rows of the head only)
        gp[-2], gp[-1] = gp[-2][:n], gp[-1][:n]
    return [o_.detach() for o_ in outs], gp, [None if t is None else t.grad for t in logits], min(margin)


def hold(what, c, kind, lins, drops, ref, outs):
    r_out, r_gp, r_gl = ref[:3]
    for k, (o, r) in enumerate(zip(outs, r_out)):
        assert np.allclose(o.detach().cpu().numpy(), r.numpy(), rtol=2e-5, atol=2e-6), (what, 'output', k)
    got = [t.grad.cpu().numpy() for lin in lins for t in (lin.weight, lin.bias)]
    errs = grad_bars.errors(got, [r.numpy() for r in r_gp])
    for l, dr in enumerate(drops):
        if c['kinds'][l] == 'c':
            assert dr.logit_p.grad is not None, (what, 'drop%d.logit_p.grad is None' % l)
            assert dr.logit_p.grad.shape == dr.logit_p.shape
            errs.append(('logit_p%d' % l, common.rel(dr.logit_p.grad.cpu().numpy(), r_gl[l].numpy())))
    grad_bars.hold(what, errs)


@pytest.mark.parametrize('kind,act,seed', [('gauss', TANH, 31), ('gauss', RELU, 132), ('policy', SILU, 33), ('policy', RELU, 131),
                                           ('plain', TANH, 35), ('plain', RELU, 133)])
def test_train_mode_gradients_match_fp64(kind, act, seed):
    import prob_mbrl_amd as pm
    c = case(act, seed)
    ref = reference(c, kind)
    if act == RELU:
        assert ref[3] > 1e-4      # (the seed keeps the kept units clear of ReLU's kink)
    mod, lins, drops = build(c, kind)
    mod.train()
    force(c, drops)
    x = c['x'].to(DEV)
    with pm.models.param_grad():
        outs = call(mod, kind, x)
    sum((o * up.to(DEV)).sum() for o, up in zip(outs, c['up'])).backward()
    hold('%s act %d' % (kind, act), c, kind, lins, drops, ref, outs)


def test_mixed_layers_and_a_scalar_logit():
    """A Bernoulli layer behind a concrete one keeps the constant-mask path; a scalar logit_p gets the sum over its units."""
    import prob_mbrl_amd as pm
    c = case(SILU, 37, kinds=('c', 'b'))
    mod, lins, drops = build(c, 'gauss')
    mod.train()
    force(c, drops)
    with pm.models.param_grad():
        outs = mod(c['x'].to(DEV), resample=False)
    sum((o * up.to(DEV)).sum() for o, up in zip(outs, c['up'])).backward()
    hold('concrete + Bernoulli', c, 'gauss', lins, drops, reference(c, 'gauss'), outs)

    c = case(TANH, 38)
    # (the hard samples of the case were drawn for per-unit logits; any {0,1} draw is a valid input)
    mod, lins, drops = build(c, 'gauss', scalar_logit=True)
    assert all(dr.logit_p.dim() == 0 for dr in drops)
    mod.train()
    force(c, drops)
    with pm.models.param_grad():
        outs = mod(c['x'].to(DEV), resample=False)
    sum((o * up.to(DEV)).sum() for o, up in zip(outs, c['up'])).backward()
    hold('scalar logit_p', c, 'gauss', lins, drops, reference(c, 'gauss', scalar_logit=True), outs)


def test_eval_mode_and_calls_outside_param_grad_are_unchanged():
    import prob_mbrl_amd as pm
    c = case(TANH, 39)
    mod, lins, drops = build(c, 'gauss')
    x = c['x'].to(DEV)
    # eval(): the stored hard sample is a constant
    mod.eval()
    for l, dr in enumerate(drops):
        dr.concrete_noise = c['hard'][l].to(DEV)
    plain = mod(x, resample=False)
    assert all(o.grad_fn is None for o in plain)
    with pm.models.param_grad():
        outs = mod(x, resample=False)
    assert all(torch.equal(a, b) for a, b in zip(outs, plain))
    sum((o * up.to(DEV)).sum() for o, up in zip(outs, c['up'])).backward()
    assert all(dr.logit_p.grad is None for dr in drops)
    assert all(lin.weight.grad is not None for lin in lins)
    # train(), outside param_grad(): the value of a fresh hard sample, no graph
    mod.train()
    force(c, drops, calls=2)
    outs_t = mod(x, resample=False)
    assert all(o.grad_fn is None for o in outs_t)
    assert all(torch.equal(a, b) for a, b in zip(outs_t, plain))      # (the same forced sample: the same values)
    with pm.models.param_grad():
        outs_g = mod(x, resample=False)
    assert all(torch.equal(a, b) for a, b in zip(outs_g, plain)) and all(o.grad_fn is not None for o in outs_g)
