"""pmbrl_mlp_forward_ln / pmbrl_mlp_grad_input_ln / pmbrl_mlp_backward_ln (the stand-alone network calls with
layer-normalised hidden layers) against fp64 torch autograd of the same formula (tests/layer_norm_ref.py).

Bars.  Gradients: tests/grad_bars.py -- common.rel < 2e-5 for grad_x, every W / b, every gamma, every beta and every logit
gradient on its own (fp32 torch autograd of the same network is 2.7e-7 .. 1.1e-6 from fp64 on these shapes).  Forward
values: rtol 2e-5, atol 2e-6, the bar of the existing stand-alone forward tests (tests/test_gpu_concrete_modules.py,
tests/common.py).  The cancellation case (layer 0's bias shifted by +300, v = 300 +- 1) is beyond fp32 itself -- torch's
fp32 autograd is some 7e-5 off there --, so it is held to 4 x the error of torch's fp32 autograd on the same inputs (the
largest over the tensors: the two differ in summation order, a tensor on which torch happens to be lucky says nothing
about the kernel); a single-pass variance E[v^2] - mu^2 would be about 1e-2 off.

Conditions beside the measurements: two calls give the same bits; with no layer-norm layer the new entry points give the
bits of pmbrl_mlp_forward / _grad_input / _backward / _backward_concrete; a row of constant v leaves everything finite."""
import functools

import numpy as np
import pytest
import torch

from tests import common, grad_bars  # noqa: F401
from tests import layer_norm_ref as LN

MLS = float(np.log(5.0))
RELU, TANH, SILU, HHSINLU = LN.RELU, LN.TANH, LN.SILU, LN.HHSINLU
RAGGED = [6, 40, 56, 6]
MANY = 'block_cap'      # B = 16 * PMBRL_MLP_BWD_MAX_BLOCKS + 5: tiles strided over the workgroups, every slab summed
ZERO_VAR_ROW = 7
ZERO_GAMMA = (1, 17)

# (the seeds of the ReLU and hhSinLU cases: test_relu_cases_stay_clear_of_the_kink)
# name: (seed, B, dims, act, per hidden layer: 'L' layer norm, 'c' concrete, 'b' Bernoulli keep 0.8, '-' nothing)
CASES = {}
for _act, _name, _seeds in ((RELU, 'relu', (1211, 202, 203)), (TANH, 'tanh', (211, 212, 213)), (SILU, 'silu', (221, 222, 223)),
                            (HHSINLU, 'hhsinlu', (231, 232, 233))):
    CASES['ragged_' + _name] = (_seeds[0], 45, RAGGED, _act, ['L', 'L'])
    CASES['one_row_' + _name] = (_seeds[1], 1, RAGGED, _act, ['L', 'L'])
    CASES['one_tile_' + _name] = (_seeds[2], 16, RAGGED, _act, ['L', 'L'])
CASES.update({
    'one_hidden': (241, 21, [4, 24, 2], RELU, ['L']),
    'three_hidden': (242, 37, [7, 32, 48, 16, 4], TANH, ['L', 'L', 'L']),
    'first_only': (243, 45, RAGGED, SILU, ['L', '-']),
    'second_only': (244, 45, RAGGED, RELU, ['-', 'L']),
    'bernoulli': (245, 45, RAGGED, TANH, ['Lb', 'Lb']),
    'concrete_same_layer': (246, 45, RAGGED, RELU, ['Lc', 'Lc']),
    'concrete_same_layer_silu': (247, 45, RAGGED, SILU, ['Lc', 'L']),
    'concrete_other_layer': (248, 45, RAGGED, TANH, ['L', 'c']),
    'zero_variance_row': (249, 45, RAGGED, TANH, ['L', 'L']),
    'zero_gamma': (250, 45, RAGGED, SILU, ['L', 'L']),
    'block_cap': (251, MANY, [5, 200, 200, 2], TANH, ['L', 'L']),
})
CANCEL = 'cancellation'
CASES[CANCEL] = (252, 45, RAGGED, TANH, ['L', 'L'])
KINKED = (RELU, HHSINLU)


@functools.lru_cache(maxsize=None)
def inputs(name):
    from prob_mbrl_amd import _lib
    seed, B, dims, act, layers = CASES[name]
    B = 16 * _lib.MLP_BWD_MAX_BLOCKS + 5 if B == MANY else B
    return LN.standalone(dims, act, B, seed, [s.replace('-', '') for s in layers],
                         bias_shift=300.0 if name == CANCEL else 0.0,
                         zero_var_row=ZERO_VAR_ROW if name == 'zero_variance_row' else None,
                         zero_gamma=ZERO_GAMMA if name == 'zero_gamma' else None)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64):
    return LN.standalone_reference(inputs(name), dtype, MLS)


def device_call(name, layer_norm=True):
    from prob_mbrl_amd import activations as ACT
    from prob_mbrl_amd import engine as E
    c = inputs(name)
    dev = torch.device('cuda:0')
    flat = torch.cat([t.reshape(-1) for pair in zip(c['Ws'], c['bs']) for t in pair]).to(dev)
    bits = [E.pack_mask(m.to(dev)) if m is not None else None for m in c['hard']]
    ln = [None if g is None else (g.to(dev), b.to(dev), e) for g, b, e in zip(c['gamma'], c['beta'], c['eps'])]
    call = E._MlpCall(c['x'].to(dev), flat, c['dims'], c['keep'], bits, c['z'].to(dev), c['shift'], c['iscale'], c['osc'],
                      c['osh'], c['sqs'], c['sqb'], MLS, act=ACT.pack([c['act']] * (c['nl'] - 1)), layer_norm=ln if layer_norm else None)
    conc = [None if k != 'c' else (c['u'][l].to(dev), c['logit'][l].to(dev), c['temp'][l]) for l, k in enumerate(c['kinds'])]
    return call, [t.to(dev) for t in c['up']], conc if any(k == 'c' for k in c['kinds']) else None


def split(c, flat):
    out, off = [], 0
    for t in (t for pair in zip(c['Ws'], c['bs']) for t in pair):
        out.append(flat[off:off + t.numel()].reshape(t.shape))
        off += t.numel()
    return out


def tensor_errors(c, got, ref):
    """[(label, common.rel)] of a device backward (grad_x, grad_params, logit parts, ln pairs) against a reference dict,
    every tensor on its own norm."""
    gx, gp, gl, gn = got
    errs = grad_bars.errors([gx.cpu().numpy()], [ref['grad_x'].numpy()], ['grad_x'])
    errs += grad_bars.errors([t.numpy() for t in split(c, gp.cpu())], [r.numpy() for r in ref['params']])
    pairs = iter(gn)
    for l, (rg, rb) in enumerate(zip(ref['gamma'], ref['beta'])):
        if rg is not None:
            g, b = next(pairs)
            errs += [('gamma%d' % l, common.rel(g.cpu().numpy(), rg.numpy())), ('beta%d' % l, common.rel(b.cpu().numpy(), rb.numpy()))]
    for l, r in enumerate(ref['logit']):
        if r is not None:
            errs.append(('logit_p%d' % l, common.rel(gl[l].cpu().numpy(), r.numpy())))
    return errs


def test_relu_cases_stay_clear_of_the_kink():
    for name, case in CASES.items():
        if case[3] in KINKED:
            assert reference(name)['margin'] > 1e-4, (name, reference(name)['margin'])


def test_the_gamma_gradient_is_not_small():
    """... beside the weight gradient behind it (the next Linear's), so that an output of zeros cannot pass; every gamma and
    beta gradient is measured on its own norm anyway."""
    for name in CASES:
        ref = reference(name)
        for l, g in enumerate(ref['gamma']):
            if g is not None:
                assert float(g.norm()) > 1e-2 * float(ref['params'][2 * (l + 1)].norm()), (name, l)
                assert float(ref['beta'][l].norm()) > 1e-2 * float(ref['params'][2 * (l + 1)].norm()), (name, l)


def test_the_special_inputs_are_what_they_claim():
    v = reference('zero_variance_row')['pre'][0]
    assert float(v[ZERO_VAR_ROW].max() - v[ZERO_VAR_ROW].min()) == 0.0 and float(v.std(-1).min()) == 0.0
    assert float((v.std(-1) > 0.1).sum()) == v.shape[0] - 1
    assert float(inputs('zero_gamma')['gamma'][ZERO_GAMMA[0]][ZERO_GAMMA[1]]) == 0.0
    assert abs(float(reference('zero_gamma')['gamma'][ZERO_GAMMA[0]][ZERO_GAMMA[1]])) > 1e-3
    v = reference(CANCEL)['pre'][0]
    assert 295 < float(v.min()) and float(v.max()) < 305


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n in CASES if n != CANCEL])
def test_backward_matches_fp64_autograd(name):
    call, ups, conc = device_call(name)
    got = call.backward(*ups, concrete=conc)
    c, ref = inputs(name), reference(name)
    assert all(bool(torch.isfinite(t).all()) for t in (got[0], got[1]))
    grad_bars.hold(name, tensor_errors(c, got, ref))
    if name == 'zero_gamma':
        l, j = ZERO_GAMMA
        g = got[3][l][0][j]
        assert abs(float(g) - float(ref['gamma'][l][j])) < grad_bars.BAR * float(ref['gamma'][l].norm())
    # the input gradient alone (pmbrl_mlp_grad_input_ln) is held to the same bar
    gx = call.grad_input(*ups)
    grad_bars.hold(name + ' grad_input', grad_bars.errors([gx.cpu().numpy()], [ref['grad_x'].numpy()], ['grad_x']))


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n in CASES if n != CANCEL])
def test_forward_matches_fp64(name):
    call, _, _ = device_call(name)
    out, ref = call.forward(('sample', 'mean', 'log_std')), reference(name)
    for k, o in out.items():
        got, want = o.cpu().numpy(), ref[k].numpy()
        print('%s %s: max |got - want| / (2e-6 + 2e-5 |want|) = %.3f' % (name, k, float((np.abs(got - want) / (2e-6 + 2e-5 * np.abs(want))).max())))
        assert np.allclose(got, want, rtol=2e-5, atol=2e-6), (name, k)


@pytest.mark.gpu
def test_cancellation_case_is_as_good_as_fp32_allows():
    call, ups, conc = device_call(CANCEL)
    c, r64, r32 = inputs(CANCEL), reference(CANCEL), reference(CANCEL, torch.float32)
    lists = lambda r: [r['grad_x']] + r['params'] + [t for t in r['gamma'] + r['beta'] if t is not None]  # noqa: E731
    fp32 = max(common.rel(a.numpy(), b.numpy()) for a, b in zip(lists(r32), lists(r64)))
    errs = tensor_errors(c, call.backward(*ups, concrete=conc), r64)
    print('cancellation: torch fp32 against fp64 %.2e (worst tensor)' % fp32)
    grad_bars.hold(CANCEL, errs, bar=4 * fp32)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['ragged_silu', 'concrete_same_layer', 'block_cap'])
def test_two_calls_give_the_same_bits(name):
    call, ups, conc = device_call(name)
    a = call.backward(*ups, concrete=conc)
    b = call.backward(*ups, concrete=conc)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(s, t) for p, q in zip(a[3], b[3]) for s, t in zip(p, q))
    if conc is not None:
        assert all(torch.equal(s, t) for s, t in zip(a[2], b[2]) if s is not None)
    assert torch.equal(call.forward(('sample',))['sample'], call.forward(('sample',))['sample'])


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['ragged_relu', 'ragged_tanh', 'concrete_same_layer', 'concrete_other_layer', 'block_cap'])
def test_without_a_layer_norm_layer_the_new_calls_give_the_old_bits(name):
    """The same network with its LayerNorms left out, through pmbrl_mlp_*_ln with ln = NULL and through the calls they
    extend."""
    old, ups, conc = device_call(name, layer_norm=False)
    new, _, _ = device_call(name, layer_norm=False)
    new.ln_entry = True
    want = ('sample', 'mean', 'log_std')
    assert all(torch.equal(a, b) for a, b in zip(old.forward(want).values(), new.forward(want).values()))
    assert torch.equal(old.grad_input(*ups), new.grad_input(*ups))
    a, b = old.backward(*ups, concrete=conc), new.backward(*ups, concrete=conc)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and b[3] is None
    if conc is not None:
        assert all(torch.equal(s, t) for s, t in zip(a[2], b[2]) if s is not None)


@pytest.mark.gpu
def test_ln_gradient_alone_and_not_wanted():
    call, ups, conc = device_call('ragged_tanh')
    full = call.backward(*ups)
    gx, gp, _, gn = call.backward(*ups, want_x=False, want_params=False)
    assert gx is None and gp is None
    assert all(torch.equal(s, t) for p, q in zip(full[3], gn) for s, t in zip(p, q))
    gx, gp, _, gn = call.backward(*ups, want_ln=False)
    assert gn is None and torch.equal(gx, full[0]) and torch.equal(gp, full[1])
