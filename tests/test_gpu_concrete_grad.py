"""pmbrl_mlp_backward_concrete (the stand-alone network's backward with train-mode concrete-dropout layers: the gradient
of their logit_p beside grad_x and grad_params) against fp64 torch autograd of the same formula
(tests/concrete_policy_ref.py).

Bars: tests/grad_bars.py -- common.rel < 2e-5 for grad_x, for every parameter tensor and for every layer's logit gradient
on its own.  (fp32 torch against fp64 on these shapes is 2e-7 .. 1.3e-6 off in grad_logit; the logit gradient is a few per
cent of the next layer's weight gradient in norm, so an output of zeros fails by five decades.)

Conditions beside the measurements: grad_x and grad_params are the bits pmbrl_mlp_backward gives on the same inputs;
two calls give the same bits; a unit whose noise saturates probs in every row has a gradient of exactly 0."""
import functools

import numpy as np
import pytest
import torch

from tests import common, grad_bars  # noqa: F401
from tests import concrete_policy_ref as CP

MLS = float(np.log(5.0))
RELU, TANH, SILU = 0, 1, 2
RAGGED = [6, 40, 56, 6]
MANY = 'block_cap'      # B = 16 * PMBRL_MLP_BWD_MAX_BLOCKS + 5: tiles strided over the workgroups, every slab summed

# (the seeds of the ReLU cases: test_relu_cases_stay_clear_of_the_kink)
# name: (seed, B, dims, act, temp, kind per hidden layer: 'c' concrete, 'b' Bernoulli keep 0.8, None)
CASES = {
    'relu_t01': (103, 45, RAGGED, RELU, 0.1, 'cc'),
    'relu_t05': (102, 45, RAGGED, RELU, 0.5, 'cc'),
    'tanh_t01': (3, 45, RAGGED, TANH, 0.1, 'cc'),
    'tanh_t05': (4, 45, RAGGED, TANH, 0.5, 'cc'),
    'silu_t01': (5, 45, RAGGED, SILU, 0.1, 'cc'),
    'silu_t05': (6, 45, RAGGED, SILU, 0.5, 'cc'),
    'one_row': (100, 1, RAGGED, RELU, 0.1, 'cc'),
    'one_tile': (8, 16, RAGGED, SILU, 0.1, 'cc'),
    'one_hidden': (101, 21, [4, 24, 2], RELU, 0.1, 'c'),
    'three_hidden': (10, 37, [7, 32, 48, 16, 4], TANH, 0.1, 'ccc'),
    'conc_then_bern': (103, 45, RAGGED, RELU, 0.1, 'cb'),
    'bern_then_conc': (12, 45, RAGGED, SILU, 0.1, 'bc'),
    'conc_then_none': (13, 45, RAGGED, TANH, 0.1, 'c-'),
    'none_then_conc': (102, 45, RAGGED, RELU, 0.1, '-c'),
    'many_rows': (15, MANY, [5, 200, 200, 2], TANH, 0.1, 'cc'),
}
SATURATED = (1, 17)      # tanh_t01: hidden layer 1, unit 17 has u = 0 in every row


@functools.lru_cache(maxsize=None)
def inputs(name):
    from prob_mbrl_amd import _lib
    seed, B, dims, act, temp, kinds = CASES[name]
    B = 16 * _lib.MLP_BWD_MAX_BLOCKS + 5 if B == MANY else B
    return CP.standalone(dims, act, B, seed, temp, [None if k == '-' else k for k in kinds],
                         saturate=SATURATED if name == 'tanh_t01' else None)


@functools.lru_cache(maxsize=None)
def reference(name):
    return CP.standalone_reference(inputs(name), torch.float64, MLS)


def device_call(name):
    from prob_mbrl_amd import engine as E
    c = inputs(name)
    dev = torch.device('cuda:0')
    flat = torch.cat([t.reshape(-1) for pair in zip(c['Ws'], c['bs']) for t in pair]).to(dev)
    bits = [E.pack_mask(m.to(dev)) if m is not None else None for m in c['hard']]
    call = E._MlpCall(c['x'].to(dev), flat, c['dims'], c['keep'], bits, c['z'].to(dev), c['shift'], c['iscale'], c['osc'],
                      c['osh'], c['sqs'], c['sqb'], MLS, act=c['act'])
    conc = [None if k != 'c' else (c['u'][l].to(dev), c['logit'][l].to(dev), c['temp'][l]) for l, k in enumerate(c['kinds'])]
    return call, [t.to(dev) for t in c['up']], conc


def split(c, flat):
    out, off = [], 0
    for t in (t for pair in zip(c['Ws'], c['bs']) for t in pair):
        out.append(flat[off:off + t.numel()].reshape(t.shape))
        off += t.numel()
    return out


def test_relu_cases_stay_clear_of_the_kink():
    for name, case in CASES.items():
        if case[3] == RELU:
            assert reference(name)[3] > 1e-4, (name, reference(name)[3])


def test_the_logit_gradient_is_not_small():
    """... against the weight gradient behind it: 2 to 10 % (0.1 % with a single row), far above fp32 rounding of the
    sums it shares a kernel with; each logit gradient is measured on its own norm, so zeros miss the bar whatever it is."""
    for name in CASES:
        c, (rx, rp, rl, _) = inputs(name), reference(name)
        for l, g in enumerate(rl):
            if g is not None:
                assert float(g.norm()) > 1e-3 * float(rp[2 * (l + 1)].norm()), (name, l)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_backward_matches_fp64_autograd(name):
    call, ups, conc = device_call(name)
    gx, gp, gl = call.backward(*ups, concrete=conc)
    c, (rx, rp, rl, _) = inputs(name), reference(name)
    assert [g is None for g in gl] == [r is None for r in rl]
    errs = grad_bars.errors([gx.cpu().numpy()], [rx.numpy()], ['grad_x'])
    errs += grad_bars.errors([t.numpy() for t in split(c, gp.cpu())], [r.numpy() for r in rp])
    # each logit gradient on its own scale (grad_bars.errors measures a list against its largest member)
    errs += [('logit_p%d' % l, common.rel(g.cpu().numpy(), r.numpy())) for l, (g, r) in enumerate(zip(gl, rl)) if g is not None]
    grad_bars.hold(name, errs)
    # the other outputs are pmbrl_mlp_backward's, bit for bit
    gx0, gp0 = call.backward(*ups)
    assert torch.equal(gx, gx0) and torch.equal(gp, gp0)
    if name == 'tanh_t01':
        l, j = SATURATED
        assert float(gl[l][j]) == 0.0 and float(rl[l][j].abs()) < 1e-30


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['silu_t01', 'many_rows'])
def test_two_calls_give_the_same_bits(name):
    call, ups, conc = device_call(name)
    a = call.backward(*ups, concrete=conc)
    b = call.backward(*ups, concrete=conc)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(s, t) for s, t in zip(a[2], b[2]) if s is not None)


@pytest.mark.gpu
def test_logit_gradient_alone():
    """Neither grad_x nor grad_params wanted: the logit gradient is still what the full call gives."""
    call, ups, conc = device_call('relu_t01')
    full = call.backward(*ups, concrete=conc)
    gx, gp, gl = call.backward(*ups, want_x=False, want_params=False, concrete=conc)
    assert gx is None and gp is None
    assert all(torch.equal(s, t) for s, t in zip(full[2], gl))
