"""GPU (-m gpu): the stand-alone network calls over every shape they accept (the table of tests/mlp_envelope_cases.py)
against the fp64 reference (tests/layer_norm_ref.py::standalone_reference), through engine._MlpCall.

Every inside case, every call it names:
  forward      sample, mean, log_std at rtol 2e-5, atol 2e-6 (tests/test_gpu_mlp_backward.py::test_forward_matches_fp64)
  grad_input   grad_x at tests/grad_bars.py (common.rel < 2e-5)
  backward     grad_x, every parameter tensor, every concrete layer's d logit_p, every layer-norm layer's d gamma / d beta,
               each on its own norm at the same bar; its grad_x has the bits of grad_input's
Every output sits inside a larger NaN-filled tensor: no NaN is left in it, the bands in front of it and behind it are
untouched.  On the edge and many-row cases two calls give the same bits.  The _ln entry points with ln = NULL and
pmbrl_mlp_backward_concrete's grad_x / grad_params give the bits of the calls they extend.  Every refused call returns its
code with its message, launches nothing and leaves its outputs alone."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mlp_envelope_cases as ME
from tests.test_mlp_envelope_cases import RANGE_TEXT, call_struct

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BAND = 64


def device_call(case, ln_entry=False):
    """(_MlpCall, upstream gradients, concrete argument or None).  ln_entry: take the _ln entry points whatever the layers."""
    from prob_mbrl_amd import activations as ACT
    from prob_mbrl_amd import engine as E
    c = ME.problem(case)
    dev = torch.device(DEV)
    flat = torch.cat([t.reshape(-1) for pair in zip(c['Ws'], c['bs']) for t in pair]).to(dev)
    bits = [E.pack_mask(m.to(dev)) if m is not None else None for m in c['hard']]
    ln = [None if g is None else (g.to(dev), b.to(dev), e) for g, b, e in zip(c['gamma'], c['beta'], c['eps'])]
    call = E._MlpCall(c['x'].to(dev), flat, c['dims'], c['keep'], bits, c['z'].to(dev) if c['z'] is not None else None,
                      c['shift'], c['iscale'], c['osc'], c['osh'], c['sqs'], c['sqb'], ME.MLS, act=ACT.pack(ME.codes(case)),
                      layer_norm=ln)
    call.ln_entry = ln_entry
    conc = None
    if any(k == 'c' for k in c['kinds']):
        conc = [None if k != 'c' else (c['u'][l].to(dev), c['logit'][l].to(dev), c['temp'][l]) for l, k in enumerate(c['kinds'])]
    return call, [t.to(dev) for t in c['up']], conc


class Banded:
    """An output [shape] inside a larger NaN-filled tensor."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * BAND,), float('nan'), device=DEV)
        self.t = self.buf[BAND:BAND + n].view(*shape)

    def written(self):
        return not bool(torch.isnan(self.t).any()) and self.untouched_bands()

    def untouched_bands(self):
        return bool(torch.isnan(self.buf[:BAND]).all()) and bool(torch.isnan(self.buf[-BAND:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def backward_outputs(case, call):
    """Banded (grad_x, grad_params, grad_logit or None, grad_ln or None) of the case's backward."""
    c = ME.problem(case)
    n_logit = sum(c['dims'][l + 1] for l, k in enumerate(c['kinds']) if k == 'c')
    n_ln = 2 * sum(c['dims'][l + 1] for l, g in enumerate(c['gamma']) if g is not None)
    return (Banded(*call.x.shape), Banded(call.pf.numel()), Banded(n_logit) if n_logit else None, Banded(n_ln) if n_ln else None)


def run_backward(case, call, ups, conc, outs=None):
    """The case's backward as the dict tests/mlp_envelope_cases.py::gradient_figures reads (device tensors)."""
    c = ME.problem(case)
    res = call.backward(*ups, concrete=conc, out=None if outs is None else tuple(None if o is None else o.t for o in outs))
    got = dict(grad_x=res[0], flat=res[1])
    if len(res) > 2 and res[2] is not None:
        got['logit'] = list(res[2])
    if len(res) > 3 and res[3] is not None:
        pairs = iter(res[3])
        got['gamma'], got['beta'] = [], []
        for g in c['gamma']:
            pair = next(pairs) if g is not None else (None, None)
            got['gamma'].append(pair[0]), got['beta'].append(pair[1])
    return got


def to_host(c, got):
    out = {}
    for k, v in got.items():
        if k == 'flat':
            out['params'] = ME.param_tensors(c, v.cpu().numpy())
        elif isinstance(v, list):
            out[k] = [None if t is None else t.cpu().numpy() for t in v]
        else:
            out[k] = v.cpu().numpy()
    return out


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        pairs = zip(a[k], b[k]) if isinstance(a[k], list) else [(a[k], b[k])]
        for s, t in pairs:
            if (s is None) != (t is None) or (s is not None and not torch.equal(s, t)):
                return False
    return True


@pytest.mark.parametrize('case', ME.INSIDE, ids=lambda c: c['id'])
def test_inside_calls_match_the_fp64_reference(case):
    c, ref = ME.problem(case), ME.reference(case)
    call, ups, conc = device_call(case)
    what = case['id']
    fwd_figs, figs = [], []
    gx = None
    if ME.inside(case, ME.FWD):
        outs = {k: Banded(call.B, call.n_out) for k in ME.OUTS}
        call.forward(ME.OUTS, out={k: o.t for k, o in outs.items()})
        assert all(o.written() for o in outs.values()), what
        fwd_figs = ME.forward_figures({k: o.t.cpu().numpy() for k, o in outs.items()}, {k: ref[k].numpy() for k in ME.OUTS})
        if case['bits']:
            again = call.forward(ME.OUTS)
            assert all(torch.equal(again[k], outs[k].t) for k in ME.OUTS), what
    if ME.inside(case, ME.GX):
        out = Banded(*call.x.shape)
        gx = call.grad_input(*ups, out=out.t)
        assert out.written(), what
        figs += [('grad_input ' + k, e) for k, e in ME.gradient_figures(dict(grad_x=gx.cpu().numpy()), ref)]
        if case['bits']:
            assert torch.equal(call.grad_input(*ups), gx), what
    if ME.inside(case, ME.BWD):
        outs = backward_outputs(case, call)
        got = run_backward(case, call, ups, conc, outs)
        assert all(o is None or o.written() for o in outs), what
        figs += ME.gradient_figures(to_host(c, got), ref)
        if gx is not None:      # the same chain, so the same bits
            assert torch.equal(got['grad_x'], gx), what
        if case['bits']:
            assert same_bits(run_backward(case, call, ups, conc), got), what
    ME.hold(what, fwd_figs, figs)


@pytest.mark.parametrize('cid', ['w528', 'e10_deep', 'e17_deep_tanh'])
def test_ln_entry_points_without_layer_norm_are_the_calls_they_extend(cid):
    """pmbrl_mlp_forward_ln / _grad_input_ln / _backward_ln with ln = NULL: the bits of pmbrl_mlp_forward / _grad_input /
    _backward, on a wide and on two deep cases."""
    case = ME.by_id(cid)
    old, ups, _ = device_call(case)
    new, _, _ = device_call(case, ln_entry=True)
    a, b = old.forward(ME.OUTS), new.forward(ME.OUTS)
    assert all(torch.equal(a[k], b[k]) for k in ME.OUTS)
    assert torch.equal(old.grad_input(*ups), new.grad_input(*ups))
    a, b = old.backward(*ups), new.backward(*ups)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and b[2] is None and b[3] is None


@pytest.mark.parametrize('cid', ['e5_conc', 'nl8_conc'])
def test_concrete_backward_extends_the_backward(cid):
    """grad_x and grad_params of pmbrl_mlp_backward_concrete: the bits of pmbrl_mlp_backward on the same inputs (the hard
    samples as constant masks), on a wide and on a deep case; through pmbrl_mlp_backward_ln (ln = NULL) the logits' too."""
    case = ME.by_id(cid)
    call, ups, conc = device_call(case)
    assert conc is not None
    with_logits = call.backward(*ups, concrete=conc)
    plain = call.backward(*ups)
    assert len(plain) == 2 and torch.equal(plain[0], with_logits[0]) and torch.equal(plain[1], with_logits[1])
    call.ln_entry = True
    through_ln = call.backward(*ups, concrete=conc)
    assert torch.equal(through_ln[0], with_logits[0]) and torch.equal(through_ln[1], with_logits[1])
    assert all((s is None) == (t is None) and (s is None or torch.equal(s, t)) for s, t in zip(through_ln[2], with_logits[2]))


def nothing_ran(outs):
    torch.cuda.synchronize()
    return all(o.untouched() for o in outs)


@pytest.mark.parametrize('case', [c for c in ME.OUTSIDE_CASES if ME.inside(c)], ids=lambda c: c['id'])
def test_calls_behind_the_lds_edge_are_refused(case):
    """-3 and "LDS" from the call itself (pmbrl_mlp_grad_input has no workspace query of its own) and from the backward's
    workspace query and entry point; nothing has been launched, the outputs are untouched."""
    from prob_mbrl_amd import _lib
    from prob_mbrl_amd import engine as E
    call, ups, conc = device_call(case)
    lib = _lib.load()
    if ME.GX in case['refused']:
        out = Banded(*call.x.shape)
        with pytest.raises(_lib.PmbrlError, match=r'\(-3\).*LDS'):
            call.grad_input(*ups, out=out.t)
        assert nothing_ran([out])
    assert ME.BWD in case['refused'] and case['refused'][ME.BWD] == ME.LDS
    outs = backward_outputs(case, call)
    with pytest.raises(ValueError, match='LDS'):
        run_backward(case, call, ups, conc, outs)
    # the entry point itself, on the forward's workspace (it is refused before anything is read)
    cs = call_struct(case)[1]
    if cs is not None:
        for l, t in enumerate(conc):
            if t is not None:
                cs.u_d[l], cs.logit_d[l] = t[0].data_ptr(), t[1].data_ptr()
    p = call._p
    gx, gp, gl, gn = (None if o is None else o.t for o in outs)
    rc = lib.pmbrl_mlp_backward_ln(E._stream(), ctypes.byref(call.call), p(call.ws), *call._common(), p(ups[0]), p(ups[1]),
                                   p(ups[2]), p(gx), p(gp), ctypes.byref(cs) if cs is not None else None, p(gl),
                                   call._ln_ref(), p(gn))
    assert rc == ME.LDS and b'LDS' in lib.pmbrl_last_error()
    assert nothing_ran([o for o in outs if o is not None])


@pytest.mark.parametrize('case', [c for c in ME.OUTSIDE_CASES if not ME.inside(c)], ids=lambda c: c['id'])
def test_shapes_out_of_range_are_refused(case):
    """-2 and the range's message from every entry point, before anything is read or launched."""
    from prob_mbrl_amd import _lib
    from prob_mbrl_amd import engine as E
    lib = _lib.load()
    call = call_struct(case)[0]
    B, dims = call.B, case['dims']
    x = torch.zeros(B, dims[0], device=DEV)
    params = torch.zeros(ME.n_params(dims), device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    up = torch.ones(B, max(dims[-1] // 2, 1), device=DEV)
    outs = [Banded(B, max(dims[-1] // 2, 1)) for _ in range(3)] + [Banded(B, dims[0]), Banded(params.numel())]
    masks = (ctypes.c_void_p * 8)()
    p = E._MlpCall._p
    common = [E._stream(), ctypes.byref(call), p(ws), p(x), p(params), masks] + [None] * 7
    ups = [p(up)] * 3

    def refused(rc):
        assert rc == ME.RANGE and any(t in lib.pmbrl_last_error() for t in RANGE_TEXT), (rc, lib.pmbrl_last_error())

    refused(lib.pmbrl_mlp_forward(*common, p(outs[0].t), p(outs[1].t), p(outs[2].t)))
    refused(lib.pmbrl_mlp_forward_ln(*common, p(outs[0].t), p(outs[1].t), p(outs[2].t), None))
    refused(lib.pmbrl_mlp_grad_input(*common, *ups, p(outs[3].t)))
    refused(lib.pmbrl_mlp_grad_input_ln(*common, *ups, p(outs[3].t), None))
    refused(lib.pmbrl_mlp_backward(*common, *ups, p(outs[3].t), p(outs[4].t)))
    refused(lib.pmbrl_mlp_backward_ln(*common, *ups, p(outs[3].t), p(outs[4].t), None, None, None, None))
    assert nothing_ran(outs)
