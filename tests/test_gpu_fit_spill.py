"""GPU (-m gpu): the spill form of the training step (csrc/pmbrl_bnn_spill.h: pm_bnn_fwd_bwd_spill).

Where both forms run -- every case of tests/fit_envelope_cases.py -- BnnStep(form='spill') gives the bits of
form='resident': the loss triple and the flat gradient of pmbrl_bnn_loss_grad, and for the Gaussian cases parameters, both
moments, the step count and every loss of two iterations of pmbrl_bnn_train_steps; with an optimiser rule attached, with
row weights, and with the in-kernel generator.

Where only the spill form runs -- tests/fit_wide_cases.py -- form='auto' becomes 'spill' and is held to the fp64 oracle
(oracle/ref_torch.py::bnn_train) at the project's bars exactly as tests/test_gpu_fit_envelope.py holds the resident form;
every call runs twice and gives the same bits."""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from tests import fit_envelope_cases as FE
from tests import fit_wide_cases as FW
from tests.test_gpu_bernoulli_fit import DEV, bnn_step, flat_params, noise
from tests.test_gpu_fit_envelope import BETA1, BETA2, EPS, minibatch, same_bits, split, train

pytestmark = pytest.mark.gpu


def step_of(d, M, form):
    """tests/test_gpu_bernoulli_fit.py::bnn_step with BnnStep's `form` keyword."""
    from prob_mbrl_amd import engine as E
    keep = E.BnnStep
    E.BnnStep = functools.partial(keep, form=form)
    try:
        step = bnn_step(d, M)
    finally:
        E.BnnStep = keep
    assert step.form == form or (form == 'auto' and step.form in ('resident', 'spill'))
    return step


def both_forms(d, M):
    res, spl = step_of(d, M, 'resident'), step_of(d, M, 'spill')
    assert res.form == 'resident' and spl.form == 'spill' and res.n_params == spl.n_params
    assert spl.ws.numel() > res.ws.numel()      # the spill plan's workspace includes its stashes
    return res, spl


# ---- the same bits where both forms run
@pytest.mark.parametrize('case', FE.CASES, ids=lambda c: c['id'])
def test_loss_grad_has_the_resident_forms_bits(case):
    d, ref = FE.problem(case), FE.reference(case)
    steps = both_forms(d, case['M'])
    Xn, Yn = (torch.tensor(d[k], device=DEV) for k in ('Xn', 'Yn'))
    for fit in (d, ref['second']):
        flat = flat_params(fit)[0]
        u, bvar = noise(fit, 0) if steps[0].sum_h else (None, None)
        out = []
        for step in steps:
            grad, loss = step.loss_grad(Xn, Yn, minibatch(fit, 0), flat, u, bvar, grad=torch.full_like(flat, float('nan')))
            out.append((grad.clone(), loss.clone()))
        assert torch.equal(out[0][1], out[1][1]), (out[0][1], out[1][1])
        assert torch.equal(out[0][0], out[1][0]), float((out[0][0] - out[1][0]).abs().max())
        assert bool(torch.isfinite(out[1][0]).all())


@pytest.mark.parametrize('case', FE.GAUSSIAN, ids=lambda c: c['id'])
def test_train_steps_have_the_resident_forms_bits(case):
    d = FE.problem(case)
    res, spl = both_forms(d, case['M'])
    lr = float(d['lr'])
    a, b = train(res, d, [0, 1], lr), train(spl, d, [0, 1], lr)
    assert same_bits(a, b) and int(b[3].item()) == 2
    assert not torch.equal(b[0], flat_params(d)[0])


def test_train_steps_with_a_rule_have_the_resident_forms_bits():
    """AdamW + amsgrad through pmbrl_bnn_plan_set_optimizer: the rule instance of the tail behind either form."""
    from prob_mbrl_amd import _lib, optim as OPT
    case = FE.by_id('nt5')
    d = FE.problem(case)
    out = []
    for step in both_forms(d, case['M']):
        flat = flat_params(d)[0].clone()
        vmax = torch.zeros_like(flat)
        rule = OPT.Rule([dict(lr=float(d['lr']), betas=(BETA1, BETA2), eps=EPS, weight_decay=0.02,
                              flags=_lib.OPT_DECOUPLED | _lib.OPT_AMSGRAD)], [(flat.numel(), 0)], vmax)
        m, v = torch.zeros_like(flat), torch.zeros_like(flat)
        stepc = torch.zeros(1, dtype=torch.int64, device=DEV)
        Xn, Yn = (torch.tensor(d[k], device=DEV) for k in ('Xn', 'Yn'))
        idx = torch.stack([minibatch(d, it) for it in (0, 1)]).contiguous()
        u, bvar = (torch.cat(ts).contiguous() for ts in zip(*(noise(d, it) for it in (0, 1))))
        hist = torch.zeros(2, 3, device=DEV)
        step.train_steps(Xn, Yn, idx, flat, m, v, stepc, float(d['lr']), u=u, bvar=bvar, loss_hist=hist, rule=rule)
        out.append((flat, m, v, vmax, hist))
    assert same_bits(out[0], out[1])
    assert float(out[1][3].max()) > 0      # amsgrad's running maximum was written


def test_row_logprob_has_the_resident_forms_bits():
    case = FE.by_id('m17')
    d = FE.problem(case)
    Xn, Yn = (torch.tensor(d[k], device=DEV) for k in ('Xn', 'Yn'))
    flat = flat_params(d)[0]
    u, bvar = noise(d, 0)
    w = torch.linspace(0.5, 1.5, case['M'], device=DEV).contiguous()
    out = []
    for step in both_forms(d, case['M']):
        lp = torch.full((case['M'],), float('nan'), device=DEV)
        grad, loss = step.loss_grad(Xn, Yn, minibatch(d, 0), flat, u, bvar, row_weight=w, row_logprob=lp)
        out.append((grad.clone(), loss.clone(), lp))
    assert same_bits(out[0], out[1]) and bool(torch.isfinite(out[1][2]).all())


def test_in_kernel_draws_have_the_resident_forms_bits():
    case = FE.by_id('kb8')
    d = FE.problem(case)
    Xn, Yn = (torch.tensor(d[k], device=DEV) for k in ('Xn', 'Yn'))
    idx = torch.stack([minibatch(d, it) for it in (0, 1)]).contiguous()
    out = []
    for step in both_forms(d, case['M']):
        flat = flat_params(d)[0].clone()
        m, v = torch.zeros_like(flat), torch.zeros_like(flat)
        stepc = torch.zeros(1, dtype=torch.int64, device=DEV)
        hist = torch.zeros(2, 3, device=DEV)
        step.train_steps(Xn, Yn, idx, flat, m, v, stepc, float(d['lr']), seed=1234, first_step=5, loss_hist=hist)
        out.append((flat, m, v, hist))
    assert same_bits(out[0], out[1]) and not torch.equal(out[1][0], flat_params(d)[0])


# ---- the cases only the spill form takes, against the fp64 oracle
@pytest.mark.parametrize('case', FW.CASES, ids=lambda c: c['id'])
def test_wide_loss_grad_matches_the_oracle(case):
    d, ref = FW.problem(case), FW.reference(case)
    step = step_of(FW.for_device(case, d), case['M'], 'auto')
    assert step.form == 'spill'
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


@pytest.mark.parametrize('case', FW.GAUSSIAN, ids=lambda c: c['id'])
def test_wide_train_steps_match_the_oracle(case):
    """As tests/test_gpu_fit_envelope.py::test_train_steps_match_the_oracle: lr = 0 gives the tail's gradient through
    exp_avg; two steps in one call are two calls of one; the second loss against the oracle at the device's parameters."""
    d, ref = FW.problem(case), FW.reference(case)
    dev = FW.for_device(case, d)
    step = step_of(dev, case['M'], 'auto')
    assert step.form == 'spill'
    flat0, keys, sizes = flat_params(d)
    what = case['id']
    still = train(step, dev, [0], 0.0)
    assert same_bits(still, train(step, dev, [0], 0.0))
    assert torch.equal(still[0], flat0) and int(still[3].item()) == 1
    g = still[1].double() / float(np.float32(1.0 - float(np.float32(BETA1))))
    FE.hold('%s train_steps, lr = 0' % what, FE.loss_figure(still[4][0].cpu().numpy(), ref['losses'][0]),
            FE.grad_figures(split(g, sizes), ref['grads'][0], keys))
    lr = float(d['lr'])
    one = train(step, dev, [0], lr)
    two = train(step, dev, [1], lr, start=one[:4])
    both = train(step, dev, [0, 1], lr)
    assert same_bits(both, train(step, dev, [0, 1], lr)) and int(both[3].item()) == 2
    assert same_bits(both[:4], two[:4]) and torch.equal(both[4], torch.cat([one[4], two[4]]))
    at_one = FE.restart(d, 1, [p.reshape(np.asarray(d[k + '_init']).shape) for k, p in zip(keys, split(one[0], sizes))])
    fig = FE.loss_figure(two[4][0].cpu().numpy(), R.bnn_train(at_one, torch.float64)[1][0])
    print('%s train_steps, second step: loss %.3f of its bar' % (what, fig))
    assert fig <= 1.0
