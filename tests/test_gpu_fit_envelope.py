"""GPU (-m gpu): the network-fit kernels over every shape they accept (the table of tests/fit_envelope_cases.py) against
the fp64 oracle (oracle/ref_torch.py::bnn_train).

pmbrl_bnn_loss_grad: the loss triple and EVERY parameter tensor's gradient of two iterations, at the bars of
tests/test_gpu_bernoulli_fit.py::replay_loss_grad (losses rtol 3e-5, atol 2e-6; common.rel < 5e-5 per tensor).  The second
iteration starts at the oracle's fp64 parameters after its first step, cast to fp32: Adam's first step is g / (|g| + eps),
which no fp32 run -- the oracle's own included -- reproduces for the elements whose gradient is rounding noise, so
parameters after a step are never compared with the oracle here.

pmbrl_bnn_train_steps (the Gaussian cases; the mixture is refused there by design), recorded draws handed in:
  lr = 0       the parameters keep their bits; exp_avg / (1 - beta1) is the tail's gradient: held as above; exp_avg_sq
               against (1 - beta2) g^2 of that gradient and the fused Adam against torch's formula, in fp64 on the device's
               own moments, at the bars of tests/test_gpu_kernels.py::test_clip_adam_matches_torch
  two steps    in ONE call (the tail keeps the weight fragments current) against two calls of one (each re-packs them from
               the parameters): every bit of parameters, moments, step count and losses; the second loss against the
               oracle's at the device's parameters after the first step.
Every call runs twice and gives the same bits."""
import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from tests import fit_envelope_cases as FE
from tests.test_gpu_bernoulli_fit import DEV, bnn_step, flat_params, noise

pytestmark = pytest.mark.gpu

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def minibatch(d, it):
    return torch.tensor(np.asarray(d['idx_it%d' % it]).astype(np.int32), device=DEV)


def split(flat, sizes):
    return [t.cpu().numpy() for t in torch.split(flat, sizes)]


@pytest.mark.parametrize('case', FE.CASES, ids=lambda c: c['id'])
def test_loss_grad_matches_the_oracle(case):
    d, ref = FE.problem(case), FE.reference(case)
    step = bnn_step(d, case['M'])
    Xn, Yn = (torch.tensor(d[k], device=DEV) for k in ('Xn', 'Yn'))
    for it, fit in enumerate((d, ref['second'])):
        flat, keys, sizes = flat_params(fit)
        assert step.n_params == flat.numel()
        u, bvar = noise(fit, 0) if step.sum_h else (None, None)
        runs = []
        for _ in range(2):
            grad, loss = step.loss_grad(Xn, Yn, minibatch(fit, 0), flat, u, bvar, grad=torch.full_like(flat, float('nan')))
            runs.append((grad.clone(), loss.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        FE.hold('%s iteration %d, loss_grad' % (case['id'], it), FE.loss_figure(runs[0][1].cpu().numpy(), ref['losses'][it]),
                FE.grad_figures(split(runs[0][0], sizes), ref['grads'][it], keys))


def train(step, d, its, lr, start=None):
    """pmbrl_bnn_train_steps over the iterations `its` of d in ONE call, from `start` (parameters, moments, step count;
    None: the initial parameters, zero moments) -> (parameters, exp_avg, exp_avg_sq, step count, loss history [n, 3])."""
    if start is None:
        flat = flat_params(d)[0]
        start = (flat, torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros(1, dtype=torch.int64, device=DEV))
    flat, m, v, stepc = (t.clone() for t in start)
    Xn, Yn = (torch.tensor(d[k], device=DEV) for k in ('Xn', 'Yn'))
    idx = torch.stack([minibatch(d, it) for it in its]).contiguous()
    u = bvar = None
    if step.sum_h:
        u, bvar = (torch.cat(ts).contiguous() for ts in zip(*(noise(d, it) for it in its)))
    hist = torch.full((len(its), 3), float('nan'), device=DEV)
    loss = step.train_steps(Xn, Yn, idx, flat, m, v, stepc, lr, betas=(BETA1, BETA2), eps=EPS, u=u, bvar=bvar, loss_hist=hist)
    assert torch.equal(loss, hist[-1])
    return flat, m, v, stepc, hist


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('case', FE.GAUSSIAN, ids=lambda c: c['id'])
def test_train_steps_match_the_oracle(case):
    d, ref = FE.problem(case), FE.reference(case)
    step = bnn_step(d, case['M'])
    flat0, keys, sizes = flat_params(d)
    what = case['id']
    # ---- one step with lr = 0: the tail's gradient and second moment
    still = train(step, d, [0], 0.0)
    assert same_bits(still, train(step, d, [0], 0.0))
    assert torch.equal(still[0], flat0) and int(still[3].item()) == 1
    omb1, omb2 = 1.0 - float(np.float32(BETA1)), 1.0 - float(np.float32(BETA2))
    g = still[1].double() / float(np.float32(omb1))
    FE.hold('%s train_steps, lr = 0' % what, FE.loss_figure(still[4][0].cpu().numpy(), ref['losses'][0]),
            FE.grad_figures(split(g, sizes), ref['grads'][0], keys))
    want_v = float(np.float32(omb2)) * g * g
    print('%s exp_avg_sq: max |got - want| / (1e-12 + 1e-5 |want|) = %.3f'
          % (what, float(((still[2].double() - want_v).abs() / (1e-12 + 1e-5 * want_v.abs())).max())))
    assert np.allclose(still[2].cpu().numpy(), want_v.cpu().numpy(), rtol=1e-5, atol=1e-12)
    # ---- one step with lr = 1e-3: the fused Adam against torch's formula on the device's own moments
    lr = float(d['lr'])
    one = train(step, d, [0], lr)
    assert same_bits(one, train(step, d, [0], lr))
    assert torch.equal(one[1], still[1]) and torch.equal(one[2], still[2]) and torch.equal(one[4], still[4])
    m, v = one[1].double(), one[2].double()
    want_p = flat0.double() - lr / (1.0 - BETA1) * m / (v.sqrt() / np.sqrt(1.0 - BETA2) + EPS)
    print('%s Adam step: max |got - want| / (1e-6 + 1e-5 |want|) = %.3f'
          % (what, float(((one[0].double() - want_p).abs() / (1e-6 + 1e-5 * want_p.abs())).max())))
    assert np.allclose(one[0].cpu().numpy(), want_p.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert not torch.equal(one[0], flat0)
    # ---- two steps: one call against two calls
    two = train(step, d, [1], lr, start=one[:4])
    both = train(step, d, [0, 1], lr)
    assert same_bits(both, train(step, d, [0, 1], lr))
    assert int(both[3].item()) == 2
    assert same_bits(both[:4], two[:4]) and torch.equal(both[4], torch.cat([one[4], two[4]]))
    # the second step's loss: the oracle at the device's parameters after the first step
    at_one = FE.restart(d, 1, [p.reshape(np.asarray(d[k + '_init']).shape) for k, p in zip(keys, split(one[0], sizes))])
    want = R.bnn_train(at_one, torch.float64)[1][0]
    fig = FE.loss_figure(two[4][0].cpu().numpy(), want)
    print('%s train_steps, second step: loss %.3f of its bar' % (what, fig))
    assert fig <= 1.0
