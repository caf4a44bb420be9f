"""GPU (-m gpu): the register-resident sweep family (csrc/pmbrl_reg.h, pmbrl_reg_mm.h) over the envelope of shapes its
host side accepts (tests/reg_envelope_cases.py), every case against the fp64 oracle at the project's bars -- on the
whole quantities and on every policy tensor, state dimension and step by itself -- with the family serving both sweeps
(asserted, a case the family declines FAILS) and with the family switched off (PMBRL_REG=0) on the same problem, which
tells a reader of a failure whether the problem or the family is at fault.  Cases just outside the envelope must NOT be
served by the family and meet the same bars.  tests/test_reg_envelope_cases.py (CPU) shows that every case leaves
three quarters of each bar to the kernels."""
import numpy as np
import pytest
import torch

from tests import reg_envelope_cases as EC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _run(case, d, monkeypatch, reg):
    """forward, weighted_sum, the plain backward(gw) -> (engine, dict of what the oracle's dict holds, valid steps)"""
    from prob_mbrl_amd import problem as PB
    if reg:
        monkeypatch.delenv('PMBRL_REG', raising=False)
    else:
        monkeypatch.setenv('PMBRL_REG', '0')        # (the switches are read once, at plan creation)
    eng, args, _ = PB.engine_from_problem(d, torch.device(DEV), rows_per_wg_hint=case['hint'])
    monkeypatch.delenv('PMBRL_REG', raising=False)
    assert eng.info['precision'] == 'split_f16'
    S, A, Rw = eng.forward(**args)
    B = d['x0'].shape[0]
    gw = torch.tensor(PB.loss_weights(d, B), device=DEV)
    loss = float(eng.weighted_sum(Rw, gw))
    g, _, _ = eng.backward(gw)
    torch.cuda.synchronize()
    n = eng.valid_steps()
    got = dict(states=S.cpu().numpy()[:n + 1], actions=A.cpu().numpy()[:n], rewards=Rw.cpu().numpy().reshape(-1, B)[:n],
               loss=loss, grad=g.cpu().numpy().copy())
    return eng, got, n


def _served_by_the_family(case, eng):
    assert eng.info['reg'], 'the family declined %s: %s' % (case['id'], eng.info)
    assert eng.reg_calls() == (1, 1), eng.reg_calls()
    assert eng.info['rows_per_wg'] <= 16
    if case['layout'] is not None:
        assert eng.info['mm_mode'] == 1
        assert {k: eng.info[k] for k in case['layout']} == case['layout'], eng.info
    else:
        assert eng.info['mm_mode'] == 0 and eng.info['rows_per_wg'] == 16
        assert eng.info['n_wg'] == -(-case['cfg']['P'] * case['cfg']['S'] // 16)


def _judge(case, d, tag, got, o64, n_steps=None):
    """the bars: whole quantities, then every slice on its own fp64 norm.  Prints the figures before it asserts."""
    e = EC.global_errors(got, o64)
    sl = EC.slice_errors(d, got, o64)
    print('%s [%s]: states %.2e actions %.2e rewards %.2e loss %.2e grad %.2e | worst tensor %s %.2e, dimension %s %.2e, '
          'step %s %.2e' % ((case['id'], tag, e['states'], e['actions'], e['rewards'], e['loss'], e['grad']) +
                            EC.worst(sl, 'grad.') + EC.worst(sl, 'states.dim') +
                            max((EC.worst(sl, k + '.step') for k in ('states', 'actions', 'rewards')), key=lambda kv: kv[1])))
    assert np.all(np.isfinite(got['grad'])) and all(np.all(np.isfinite(got[k])) for k in ('states', 'actions', 'rewards'))
    for k, bar in EC.BARS.items():
        assert e[k] < bar, (case['id'], tag, k, e[k])
    failing = {k: v for k, v in sl.items() if not v[0] < v[1]}
    if failing:
        # the referee is the oracle's own fp32 run: a slice on which IT stays within a quarter of the bar keeps the bar
        # (tests/test_reg_envelope_cases.py asserts that of every slice of every case)
        o32 = EC.oracle(d, torch.float32, n_steps)
        if 'drift' in o64:
            o32 = EC.split_drift(o32)
        gap = EC.slice_errors(d, o32, o64)
        report = {k: '%.2e (bar %.0e, fp32 oracle %.2e)' % (v[0], v[1], gap[k][0]) for k, v in failing.items()}
        print('%s [%s]: slices beyond their bar: %s' % (case['id'], tag, report))
        kept = [k for k in failing if gap[k][0] <= 0.25 * failing[k][1]]
        assert not kept, (case['id'], tag, {k: report[k] for k in kept})
    return e


def _pair(case, g_reg, g_off):
    bar = EC.TOL_PAIR_MM if case['cfg']['mm'] else EC.TOL_PAIR_PLAIN
    e = EC.rel(g_reg, g_off)
    print('%s: gradient, family on vs off: %.2e' % (case['id'], e))
    assert e < bar, (case['id'], e)


INSIDE = [c for c in EC.CASES if c['inside']] + EC.SAT_CASES
OUTSIDE = [c for c in EC.CASES if not c['inside']]


@pytest.mark.parametrize('case', INSIDE, ids=EC.ids(INSIDE))
def test_family_meets_the_bars_inside_its_envelope(case, monkeypatch):
    """Also the saturation cases: a policy whose head output covers |u| < 2 .. |u| > 44 (pr_tanh: exp(2 u) overflows at
    44, the clamp at 15 is what keeps rcp(inf) out of the Newton step) and log-std heads beyond both ends of
    pr_sigmoid_neg's clamp at +-80 -- everything finite, the whole horizon valid, the same bars."""
    d = EC.problem(case)
    H = case['cfg']['H']
    o64 = EC.oracle(d, torch.float64)
    eng, got, n = _run(case, d, monkeypatch, reg=True)
    _served_by_the_family(case, eng)
    assert n == H, n
    eng0, got0, n0 = _run(case, d, monkeypatch, reg=False)
    assert not eng0.info['reg'] and eng0.reg_calls() == (0, 0) and n0 == H
    e0 = _judge(case, d, 'family off', got0, o64)
    e1 = _judge(case, d, 'family on', got, o64)
    _pair(case, got['grad'], got0['grad'])
    assert e1 and e0


@pytest.mark.parametrize('case', OUTSIDE, ids=EC.ids(OUTSIDE))
def test_family_declines_just_outside_its_envelope(case, monkeypatch):
    d = EC.problem(case)
    o64 = EC.oracle(d, torch.float64)
    eng, got, n = _run(case, d, monkeypatch, reg=True)
    assert eng.info['reg'] == 0 and eng.reg_calls() == (0, 0), eng.info
    assert n == case['cfg']['H']
    _judge(case, d, 'declined', got, o64)


@pytest.mark.parametrize('case', EC.OVERFLOW_CASES, ids=EC.ids(EC.OVERFLOW_CASES))
def test_a_non_finite_value_is_reported_not_laundered(case, monkeypatch):
    """tests/test_gpu_full_size.py::test_device_detects_a_mid_horizon_failure_and_continues_on_the_truncated_horizon on
    this family: a state dimension decoupled from both networks and the reward drifts by 5e37 per step.  The family
    splits its network INPUTS into fp16 pieces too, so it answers with its fp16 range check (amax in pm_reg_fwd_kernel)
    at the first step whose input holds the 5e37 -- step 1 -- long before fp32 overflows at step 6: valid_steps() == 1,
    which is what the general family on fp16 pieces does with the same input, and what rollout() / mc_pilco re-run in
    fp32 for.  Pinned: nothing raises, the step is reported (not rolled over with a NaN that vanishes in a ReLU), the
    gradient is finite, and the kept step, its loss and its gradient are the fp64 oracle's run to that many steps.
    With the family off the latency-optimised kernels (fp32 first layer) keep 6 steps, as that test pins."""
    d = EC.problem(case)
    eng, got, n = _run(case, d, monkeypatch, reg=True)
    _served_by_the_family(case, eng)
    print('%s: the family keeps %d of %d steps' % (case['id'], n, case['cfg']['H']))
    assert n == 1, n
    o64 = EC.split_drift(EC.oracle(d, torch.float64, n_steps=n))
    got = EC.split_drift(got)
    assert EC.rel(got['drift'], o64['drift']) < 1e-6
    _judge(case, EC.problem(case, drift=0.0), 'family on', got, o64, n_steps=n)
    eng0, got0, n0 = _run(case, d, monkeypatch, reg=False)
    assert not eng0.info['reg'] and eng0.reg_calls() == (0, 0)
    print('%s: with the family off %d steps are kept' % (case['id'], n0))
    assert n0 == 6, n0
    o64 = EC.split_drift(EC.oracle(d, torch.float64, n_steps=n0))
    got0 = EC.split_drift(got0)
    assert EC.rel(got0['drift'], o64['drift']) < 1e-6
    _judge(case, EC.problem(case, drift=0.0), 'family off', got0, o64, n_steps=n0)
