"""pmbrl_mlp_backward (the stand-alone network's gradient with respect to its input rows AND its parameters) against
fp64 torch autograd of the same formula (the one of test_gpu_kernels.test_mlp_input_gradient_matches_torch).

Bars (tests/grad_bars.py): common.rel < 2e-5 -- the input-gradient bar of this kernel family -- for grad_x and for EVERY
parameter tensor on its own.

ReLU's derivative jumps at 0, and a kept unit whose pre-activation is closer to 0 than fp32 resolves may take either
side there (common.kink_margin): the seeds of the ReLU cases are chosen so that the fp64 run's smallest kept
|pre-activation| exceeds 1e-4 (test_relu_cases_stay_clear_of_the_kink, no device needed).  The many-row cases have
1.6 and 1.9 million hidden units, too many for any seed to keep them all that far from 0, and run Tanh: what they are
there for -- the tile stride of a workgroup and the slab reduction -- does not depend on the activation.

pmbrl_mlp_forward on the same cases: the three outputs against the same fp64 evaluation (test_forward_matches_fp64)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import common, grad_bars  # noqa: F401
from tests import layer_norm_ref as LN

MLS = float(np.log(5.0))
RELU, TANH, SILU = 0, 1, 2
ACT = {RELU: torch.relu, TANH: torch.tanh, SILU: torch.nn.functional.silu}
ALL = ('sample', 'mean', 'log_std')


BLOCK_CAP, SLAB_CAP, PLAIN = 'block_cap', 'slab_cap', 'plain'


def _rows(B, dims):
    """B of a case: a number, or five rows past the last tile that still gets a workgroup (gradient slab) of its own."""
    from prob_mbrl_amd import _lib
    if B == BLOCK_CAP:
        return 16 * _lib.MLP_BWD_MAX_BLOCKS + 5
    if B == SLAB_CAP:      # a network whose MAX_BLOCKS slabs would exceed the slab limit gets as many as fit
        n_params = sum(dims[i + 1] * dims[i] + dims[i + 1] for i in range(len(dims) - 1))
        blocks = _lib.MLP_BWD_SLAB_BYTES // (4 * n_params)
        assert 1 < blocks < _lib.MLP_BWD_MAX_BLOCKS
        return 16 * blocks + 5
    return B


# name: (seed, B, dims, act[, PLAIN: no masks, no input / output scaling, no squashing, no noise -- every optional pointer null])
CASES = {
    'ragged_relu': (7, 45, [6, 40, 56, 6], RELU),
    'ragged_tanh': (7, 45, [6, 40, 56, 6], TANH),
    'ragged_silu': (7, 45, [6, 40, 56, 6], SILU),
    'one_row': (11, 1, [6, 40, 56, 6], RELU),
    'one_tile': (12, 16, [6, 40, 56, 6], SILU),
    'one_hidden': (13, 21, [4, 24, 2], RELU),
    'three_hidden_relu': (14, 37, [7, 32, 48, 16, 4], RELU),
    'three_hidden_tanh': (14, 37, [7, 32, 48, 16, 4], TANH),
    'many_rows': (15, BLOCK_CAP, [5, 200, 200, 2], TANH),      # B = 16 * PMBRL_MLP_BWD_MAX_BLOCKS + 5
    # the GEMM branches the fit kernels share (tests/fit_envelope_cases.py), in these calls' instances
    'kb8': (16, 45, [6, 128, 120, 6], TANH),             # gemm_tiles_group_full: 8 k-tiles forward (128) and backward (120)
    'w272': (17, 21, [6, 272, 272, 4], RELU),            # 17 output tiles: a wave's second tile group
    'head64': (18, 45, [6, 40, 56, 64], SILU),           # gemm_narrow's tile-split head
    'in20': (20, 45, [20, 40, 56, 6], RELU),             # two input tiles
    'plain': (20, 45, [6, 40, 56, 6], RELU, PLAIN),      # the ragged shape, every unit kept
    'slab_cap': (21, SLAB_CAP, [8, 264, 264, 4], TANH),  # about 3 650 rows on 228 workgroups: the block cap from the slab limit
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The fp32 inputs of a case (CPU tensors), drawn once."""
    seed, B, dims, act = CASES[name][:4]
    B = _rows(B, dims)
    g = torch.Generator().manual_seed(seed)
    nl, n_out = len(dims) - 1, dims[-1] // 2
    c = dict(B=B, dims=dims, act=act, nl=nl, n_out=n_out)
    c['Ws'] = [torch.randn(dims[i + 1], dims[i], generator=g) / np.sqrt(dims[i]) for i in range(nl)]
    c['bs'] = [0.1 * torch.randn(dims[i + 1], generator=g) for i in range(nl)]
    c['masks'] = [(torch.rand(B, dims[i + 1], generator=g) < 0.8).float() for i in range(nl - 1)]
    c['keep'] = [0.8] + [1.0] * (nl - 2)
    c['x'] = torch.randn(B, dims[0], generator=g)
    c['z'] = torch.randn(B, n_out, generator=g)
    c['shift'], c['iscale'] = torch.randn(dims[0], generator=g), 0.5 + torch.rand(dims[0], generator=g)
    c['osc'], c['osh'] = 0.5 + torch.rand(n_out, generator=g), torch.randn(n_out, generator=g)
    c['sqs'], c['sqb'] = 1.0 + torch.rand(n_out, generator=g), 0.1 * torch.randn(n_out, generator=g)
    c['up'] = dict(zip(ALL, (torch.randn(B, n_out, generator=g) for _ in range(3))))
    if PLAIN in CASES[name][4:]:
        c['masks'], c['keep'] = [None] * (nl - 1), [1.0] * (nl - 1)
        c.update(dict.fromkeys(('z', 'shift', 'iscale', 'osc', 'osh', 'sqs', 'sqb')))
    return c


@functools.lru_cache(maxsize=None)
def reference(name, up=ALL, use_z=True, dtype=torch.float64):
    """(grad_x, [grad W0, grad b0, ...], smallest kept |pre-activation|, the three outputs) by torch autograd in `dtype`
    on the CPU.  An input that is None is a null pointer of the call: that step of the formula is left out."""
    c = inputs(name)
    d = lambda t: t.to(dtype)  # noqa: E731
    x = d(c['x']).requires_grad_(True)
    params = [d(t).requires_grad_(True) for pair in zip(c['Ws'], c['bs']) for t in pair]
    h = (x - d(c['shift'])) * d(c['iscale']) if c['shift'] is not None else x
    margin = math.inf
    for i in range(c['nl'] - 1):
        v = h @ params[2 * i].t() + params[2 * i + 1]
        h = ACT[c['act']](v)
        if c['masks'][i] is not None:
            margin = min(margin, float(v.detach().abs()[c['masks'][i] > 0].min()))
            h = h * d(c['masks'][i]) / c['keep'][i]
        else:
            margin = min(margin, float(v.detach().abs().min()))
    smp, mu, ls = LN.head(h @ params[-2].t() + params[-1], c, MLS, d, use_z)
    outs = dict(sample=smp, mean=mu, log_std=ls)
    sum((outs[k] * d(c['up'][k])).sum() for k in up).backward()
    return x.grad, [p.grad for p in params], margin, {k: v.detach() for k, v in outs.items()}


def device_call(name, use_z=True):
    from prob_mbrl_amd import engine as E
    c = inputs(name)
    dev = torch.device('cuda:0')
    flat = torch.cat([t.reshape(-1) for pair in zip(c['Ws'], c['bs']) for t in pair]).to(dev)
    bits = [E.pack_mask(m.to(dev)) if m is not None else None for m in c['masks']]
    z = c['z'].to(dev) if use_z and c['z'] is not None else None
    return E._MlpCall(c['x'].to(dev), flat, c['dims'], c['keep'], bits, z, c['shift'],
                      c['iscale'], c['osc'], c['osh'], c['sqs'], c['sqb'], MLS, act=c['act'])


def upstream(name, up):
    c = inputs(name)
    return [c['up'][k].to('cuda:0') if k in up else None for k in ALL]


def split(name, flat):
    c = inputs(name)
    out, off = [], 0
    for t in (t for pair in zip(c['Ws'], c['bs']) for t in pair):
        out.append(flat[off:off + t.numel()].reshape(t.shape))
        off += t.numel()
    assert off == flat.numel()
    return out


def check(name, gx, gp, ref, what=''):
    rx, rp = ref[:2]
    errs = []
    if gx is not None:
        errs += grad_bars.errors([gx.cpu().numpy()], [rx.numpy()], ['grad_x'])
    if gp is not None:
        errs += grad_bars.errors([t.numpy() for t in split(name, gp.cpu())], [r.numpy() for r in rp])
    grad_bars.hold('%s %s' % (name, what), errs)


def test_relu_cases_stay_clear_of_the_kink():
    for name, case in CASES.items():
        if case[3] == RELU:
            assert reference(name)[2] > 1e-4, name


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_backward_matches_fp64_autograd(name):
    """Masks (keep 0.8 on the first hidden layer, 1 behind it), noise, input / output scaling, squashing and all three
    upstream gradients, over ragged rows and widths, one row, one full tile, one and three hidden layers, and more
    tiles than workgroups."""
    call = device_call(name)
    gx, gp = call.backward(*upstream(name, ALL))
    check(name, gx, gp, reference(name))


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_forward_matches_fp64(name):
    """pm_mlp_fwd_kernel (a kernel of its own, not the backward's recomputed forward) on the same cases: all three outputs
    at the bar of tests/test_gpu_kernels.py::test_mlp_forward_matches_torch."""
    out = device_call(name).forward(ALL)
    want = reference(name)[3]
    for k in ALL:
        got, ref = out[k].cpu().numpy().astype(np.float64), want[k].numpy()
        worst = float((np.abs(got - ref) / (2e-6 + 2e-5 * np.abs(ref))).max())
        print('%s %s: max |got - want| / (2e-6 + 2e-5 |want|) = %.3f' % (name, k, worst))
        assert np.allclose(got, ref, rtol=2e-5, atol=2e-6), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize('up,use_z', [(('mean',), True), (('log_std',), True), (('sample',), False)])
def test_upstream_subsets(up, use_z):
    name = 'ragged_relu'
    call = device_call(name, use_z)
    gx, gp = call.backward(*upstream(name, up))
    check(name, gx, gp, reference(name, up, use_z), '+'.join(up))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['ragged_relu', 'ragged_silu'])
def test_one_output_only_and_nan_prefill(name):
    """Either output alone is what both together give, bit for bit; outputs are overwritten, not accumulated into."""
    call = device_call(name)
    ups = upstream(name, ALL)
    gx, gp = call.backward(*ups)
    gx1, none = call.backward(*ups, want_params=False)
    assert none is None and torch.equal(gx1, gx)
    none, gp1 = call.backward(*ups, want_x=False)
    assert none is None and torch.equal(gp1, gp)
    out = (torch.full_like(gx, math.nan), torch.full_like(gp, math.nan))
    call.backward(*ups, out=out)
    assert torch.equal(out[0], gx) and torch.equal(out[1], gp)
    check(name, out[0], out[1], reference(name), 'NaN prefill')


@pytest.mark.gpu
def test_no_upstream_gradient_is_refused():
    from prob_mbrl_amd import _lib
    call = device_call('one_hidden')
    with pytest.raises(_lib.PmbrlError, match='upstream'):
        call.backward(None, None, None)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['ragged_tanh', 'many_rows', 'slab_cap'])
def test_two_calls_give_the_same_bits(name):
    call = device_call(name)
    ups = upstream(name, ALL)
    a = call.backward(*ups)
    b = call.backward(*ups)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_input_gradient_is_the_input_gradient_kernels():
    """grad_x of the backward against pmbrl_mlp_grad_input: the same chain, so the same bits."""
    for name in ('ragged_relu', 'ragged_tanh'):
        call = device_call(name)
        ups = upstream(name, ALL)
        assert torch.equal(call.backward(*ups, want_params=False)[0], call.grad_input(*ups))
