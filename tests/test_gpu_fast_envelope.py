"""GPU (-m gpu): the latency-optimised sweep family (csrc/pmbrl_fast.h, pmbrl_split.h, pmbrl_mm_w.h, the pm_xch_*
exchange) over the envelope of shapes its host side accepts (tests/fast_envelope_cases.py), in every arithmetic it
offers.  For every case and arithmetic:

  * the plan is what the table says it must be, field by field (a case the family declines FAILS);
  * the plain call (forward, weighted_sum, backward(gw): the LEAN / MM / MMG instances) meets the project's bars against
    the fp64 oracle on the whole quantities and on every policy tensor, state dimension and step by itself;
  * the call with optional outputs on the same forward sweep (backward(gw, want_x0, want_agn): the EXT instances where
    there is no moment matching) gives the gradient, dL/dx0 and the per-step action-gradient norms of
    oracle/adjoint_np.py in fp64, and the same gradient as the plain call;
  * the general family on the same problem in the same arithmetic meets the same bars -- which tells a reader of a failure
    whether the problem or the family is at fault, and walks the general family over these shapes too.

Cases just outside the envelope must NOT be served by the family and meet the same bars.
tests/test_fast_envelope_cases.py (CPU) shows that every case leaves three quarters of each bar to the kernels."""
import numpy as np
import pytest
import torch

from tests import fast_envelope_cases as EC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# a sweep cut into step ranges against the same sweep in one launch: the same sweeps and products, another order of
# additions in dW (tests/test_gpu_dw_pipeline.py::test_pipelined_dw_matches_one_launch)
TOL_RANGES = 2e-6

_REF = {}


def _ref(case, n_steps=None):
    """the problem and its fp64 oracle, computed once per case and left unchanged"""
    key = (case['id'], n_steps)
    if key not in _REF:
        d = EC.problem(case)
        _REF[key] = (d, EC.oracle(d, torch.float64, n_steps))
    return _REF[key]


def _adjoint_ref(case):
    """oracle/adjoint_np.py in fp64: gradient, dL/dx0, row norms of dL/da_t [H, B]"""
    key = (case['id'], 'adjoint')
    if key not in _REF:
        from oracle import adjoint_np as ADJ
        P = ADJ.Problem(_ref(case)[0], np.float64)
        st = ADJ.forward(P)
        g, gx0, _ = ADJ.backward(P, st)
        _REF[key] = (g, gx0, EC.action_grad_norms(st))
    return _REF[key]


def _engine(case, d, prec, monkeypatch, generic=False, env=()):
    """(the switches are read once, at plan creation)"""
    from prob_mbrl_amd import problem as PB
    env = tuple(case['env']) + tuple(env)
    for k, v in env:
        monkeypatch.setenv(k, v)
    eng, args, _ = PB.engine_from_problem(d, torch.device(DEV), rows_per_wg_hint=case['hint'], precision=prec,
                                          force_generic=generic)
    for k, _ in env:
        monkeypatch.delenv(k, raising=False)
    return eng, args


def _run(case, d, prec, monkeypatch, generic=False, env=(), optional=False):
    """forward, weighted_sum, the plain backward(gw) -> (engine, dict of what the oracle's dict holds, valid steps);
    optional: then the call with optional outputs on the same forward sweep -> got['ext'] = (g, gx0, agn)"""
    from prob_mbrl_amd import problem as PB
    eng, args = _engine(case, d, prec, monkeypatch, generic, env)
    S, A, Rw = eng.forward(**args)
    B = d['x0'].shape[0]
    gw = torch.tensor(PB.loss_weights(d, B), device=DEV)
    loss = float(eng.weighted_sum(Rw, gw))
    g, _, _ = eng.backward(gw)
    torch.cuda.synchronize()
    n = eng.valid_steps()
    got = dict(states=S.cpu().numpy()[:n + 1], actions=A.cpu().numpy()[:n], rewards=Rw.cpu().numpy().reshape(-1, B)[:n],
               loss=loss, grad=g.cpu().numpy().copy())
    if optional:
        g2, gx0, agn = eng.backward(gw, want_x0=True, want_agn=True)
        torch.cuda.synchronize()
        got['ext'] = (g2.cpu().numpy().copy(), gx0.cpu().numpy(), agn.cpu().numpy())
    return eng, got, n


def _served_by_the_family(case, prec, eng):
    want = case['expect'][prec]
    for k, v in want.items():
        assert eng.info[k] == v, 'the plan of %s [%s]: %s is %r, written down as %r (%s)' % (case['id'], prec, k, eng.info[k],
                                                                                         v, eng.info)
    assert eng.info['reg'] == 0 and eng.reg_calls() == (0, 0), eng.info
    # ... and the kernels the plan resolved are the GENERIC instances of that row (tests/test_gpu_call_forms.py: KERNELS
    # shows the names), none of the compile-time shapes
    head = 'fastILi%dELi%dELi%dELi' % ((want['row_tiles'],) + tuple(want['stages']))
    names = {v: n for v, n in eng.sweep_kernels().items() if v in ('lean', 'ext', 'mm', 'mmg')}
    assert names, eng.sweep_kernels()
    for v, (fwd, bwd) in names.items():
        for name, sweep in ((fwd, 'pm_rollout_fwd_'), (bwd, 'pm_rollout_bwd_')):
            assert sweep + head in name and '7PfShapeILi0ELi0ELi0ELi0ELi0EE' in name, (case['id'], prec, v, name)


def _judge(case, d, tag, got, o64, n_steps=None):
    """tests/test_gpu_reg_envelope.py's: whole quantities, then every slice on its own fp64 norm, the oracle's fp32 run
    the referee of a failing slice.  Prints the figures before it asserts."""
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
        o32 = EC.oracle(d, torch.float32, n_steps)
        if 'drift' in o64:
            o32 = EC.split_drift(o32)
        gap = EC.slice_errors(d, o32, o64)
        report = {k: '%.2e (bar %.0e, fp32 oracle %.2e)' % (v[0], v[1], gap[k][0]) for k, v in failing.items()}
        print('%s [%s]: slices beyond their bar: %s' % (case['id'], tag, report))
        kept = [k for k in failing if gap[k][0] <= 0.25 * failing[k][1]]
        assert not kept, (case['id'], tag, {k: report[k] for k in kept})
    return e


def _judge_optional(case, tag, got):
    g_ref, gx0_ref, agn_ref = _adjoint_ref(case)
    g2, gx0, agn = got['ext']
    e = dict(g=EC.rel(g2, g_ref), gx0=EC.rel(gx0, gx0_ref), agn=EC.rel(agn, agn_ref), calls=EC.rel(g2, got['grad']))
    print('%s [%s, optional outputs]: grad %.2e dL/dx0 %.2e action-gradient norms %.2e | against the plain call %.2e' %
          (case['id'], tag, e['g'], e['gx0'], e['agn'], e['calls']))
    assert np.all(np.isfinite(g2)) and np.all(np.isfinite(gx0)) and np.all(np.isfinite(agn))
    for k, v in e.items():
        assert v < EC.TOL_GRAD, (case['id'], tag, k, v)


@pytest.mark.parametrize('case,prec', EC.pairs(EC.INSIDE), ids=EC.pair_ids(EC.INSIDE))
def test_family_meets_the_bars_inside_its_envelope(case, prec, monkeypatch):
    """Also the saturation cases: a policy whose head output covers |u| < 2 .. |u| > 44 and log-std heads beyond both ends
    of the clamp at +-80 -- everything finite, the whole horizon valid, the same bars."""
    d, o64 = _ref(case)
    H = case['cfg']['H']
    eng, got, n = _run(case, d, prec, monkeypatch, optional=True)
    _served_by_the_family(case, prec, eng)
    assert n == H, n
    e1 = _judge(case, d, prec, got, o64)
    _judge_optional(case, prec, got)
    if prec != 'split':      # (the general family has two arithmetics)
        eng0, got0, n0 = _run(case, d, prec, monkeypatch, generic=True)
        assert not eng0.info['fast'] and eng0.info['precision'] == prec and eng0.reg_calls() == (0, 0) and n0 == H
        e0 = _judge(case, d, prec + ', general family', got0, o64)
        # (no bar of the project's for this pair: both are held to fp64 by themselves)
        print('%s [%s]: gradient, this family vs the general one: %.2e' % (case['id'], prec, EC.rel(got['grad'], got0['grad'])))
        assert e0
    assert e1


@pytest.mark.parametrize('case,prec', EC.pairs(EC.OUTSIDE), ids=EC.pair_ids(EC.OUTSIDE))
def test_family_declines_just_outside_its_envelope(case, prec, monkeypatch):
    d, o64 = _ref(case)
    eng, got, n = _run(case, d, prec, monkeypatch)
    assert eng.info['fast'] == 0 and eng.info['reg'] == 0 and eng.reg_calls() == (0, 0), eng.info
    assert n == case['cfg']['H']
    _judge(case, d, prec + ', declined', got, o64)


@pytest.mark.parametrize('prec', EC.BOTH)
@pytest.mark.parametrize('cid', EC.RANGE_CASES)
def test_adjoint_in_two_step_ranges(cid, prec, monkeypatch):
    """PMBRL_DW_PIPE=3,2 at H = 5: the adjoint sweep as two launches over the steps [2, 5) and [0, 2), the state gradient
    carried through HBM between them (the EXT instances: t0 / t1 / gx_from_carry), against the one-launch sweep."""
    case = EC.by_id(cid)
    d, o64 = _ref(case)
    assert case['cfg']['H'] == 5
    eng1, got1, n1 = _run(case, d, prec, monkeypatch, env=(('PMBRL_DW_PIPE', 'off'),))
    eng2, got2, n2 = _run(case, d, prec, monkeypatch, env=(('PMBRL_DW_PIPE', '3,2'),))
    _served_by_the_family(case, prec, eng2)
    assert eng1.info['dw_pipe'] == 1 and eng2.info['dw_pipe'] == 2 and n1 == 5 and n2 == 5
    e = EC.rel(got2['grad'], got1['grad'])
    print('%s [%s]: gradient, two step ranges vs one launch: %.2e' % (cid, prec, e))
    assert e < TOL_RANGES, (cid, prec, e)
    _judge(case, d, prec + ', two step ranges', got2, o64)


@pytest.mark.parametrize('prec', EC.BOTH)
@pytest.mark.parametrize('cid', EC.TWICE_CASES)
def test_exchanging_forms_are_deterministic(cid, prec, monkeypatch):
    """tests/test_gpu_kernels.py::test_deterministic on a group split over workgroups and on the device-wide-barrier form:
    two engines, bit for bit"""
    case = EC.by_id(cid)
    d, _ = _ref(case)
    _, a, na = _run(case, d, prec, monkeypatch, optional=True)
    _, b, nb = _run(case, d, prec, monkeypatch, optional=True)
    assert na == nb == case['cfg']['H']
    for k in ('states', 'actions', 'rewards', 'grad'):
        assert np.array_equal(a[k], b[k]), (cid, prec, k)
    assert all(np.array_equal(x, y) for x, y in zip(a['ext'], b['ext'])) and a['loss'] == b['loss']


@pytest.mark.parametrize('case,prec', EC.pairs(EC.OVERFLOW_CASES), ids=EC.pair_ids(EC.OVERFLOW_CASES))
def test_a_non_finite_value_is_reported_not_laundered(case, prec, monkeypatch):
    """A state dimension decoupled from both networks and the reward drifts by 5e37 per step and overflows fp32 while
    step 6 computes x_7.  Nothing raises, the step is reported -- OVERFLOW_STEPS = 6 in either arithmetic, worked out in
    tests/fast_envelope_cases.py -- the gradient is finite, and the kept steps, their loss and their gradient are the
    fp64 oracle's run to that many steps.  The general family in exact fp32 keeps the same 6 (on fp16 pieces it splits its
    network INPUTS too and answers at the first step: tests/test_gpu_reg_envelope.py pins that)."""
    d = EC.problem(case)
    nodrift = EC.problem(case, drift=0.0)
    for generic in (False, True):
        if generic and prec != 'f32':
            continue
        eng, got, n = _run(case, d, prec, monkeypatch, generic=generic)
        if not generic:
            _served_by_the_family(case, prec, eng)
        else:
            assert not eng.info['fast']
        print('%s [%s%s]: %d of %d steps are kept' % (case['id'], prec, ', general family' if generic else '', n, case['cfg']['H']))
        assert n == EC.OVERFLOW_STEPS, n
        o64 = EC.split_drift(_ref(case, n)[1])
        got = EC.split_drift(got)
        assert EC.rel(got['drift'], o64['drift']) < 1e-6
        _judge(case, nodrift, prec + (', general family' if generic else ''), got, o64, n_steps=n)
