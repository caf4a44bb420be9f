"""GPU (-m gpu): the general sweep family (csrc/pmbrl_rollout.h, pmbrl_rollout_sweeps.h, the GEMMs of pmbrl_dev.h and
pmbrl_gsplit.h, pmbrl_wide.h, pmbrl_mm.h, pmbrl_mm_wide.h) over the envelope of shapes its host side accepts
(tests/general_envelope_cases.py), in exact fp32 and on split operands.  For every case and arithmetic:

  * the plan is what the table says it must be, field by field, and the sweep kernels it resolved are the instance of
    csrc/pmbrl_instances.h the table names;
  * the plain call (forward, weighted_sum, backward(gw)) meets the project's bars against the fp64 oracle on the whole
    quantities and on every policy tensor, state dimension and step by itself (_judge of tests/test_gpu_fast_envelope.py);
  * the call with optional outputs on the same forward sweep (backward(gw, want_x0, want_agn)) gives the gradient, dL/dx0
    and the per-step action-gradient norms of oracle/adjoint_np.py in fp64 -- for every axis but the activations other
    than ReLU, which that oracle does not have (EC.NO_ADJOINT_ORACLE);
  * valid_steps() is the horizon;
  * an in-place case also runs in the 16-row two-buffer form of the same arithmetic, and the two agree within the pair
    tolerances of tests/test_gpu_wide.py.

Shapes just outside are refused at plan creation with the code the table states and a message, and the next plan on the
same process works.  tests/test_general_envelope_cases.py (CPU) shows that every case leaves three quarters of each bar
to the kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import general_envelope_cases as EC
from tests.test_gpu_fast_envelope import TOL_RANGES, _judge

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# an in-place form against the two-buffer form of the same arithmetic (tests/test_gpu_wide.py: hidden layers bit for bit,
# the heads sum their K in another order)
TOL_PAIR_STATES = 2e-6
TOL_PAIR_GRAD = 2e-5

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


def _engine(case, d, prec, monkeypatch, env=(), hint=None):
    """(the switches are read once, at plan creation)"""
    from prob_mbrl_amd import problem as PB
    env = tuple(case['env']) + tuple(env)
    for k, v in env:
        monkeypatch.setenv(k, v)
    eng, args, _ = PB.engine_from_problem(d, torch.device(DEV), rows_per_wg_hint=case['hint'] if hint is None else hint,
                                          precision=prec, force_generic=case['generic'])
    for k, _ in env:
        monkeypatch.delenv(k, raising=False)
    return eng, args


def _run(case, d, prec, monkeypatch, env=(), hint=None, optional=False):
    """forward, weighted_sum, the plain backward(gw) -> (engine, dict of what the oracle's dict holds, valid steps);
    optional: then the call with optional outputs on the same forward sweep -> got['ext'] = (g, gx0, agn)"""
    from prob_mbrl_amd import problem as PB
    eng, args = _engine(case, d, prec, monkeypatch, env, hint)
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


def _served_as_written(case, prec, eng):
    want = case['expect'][prec]
    for k, v in want.items():
        if k != '_inst':
            assert eng.info[k] == v, 'the plan of %s [%s]: %s is %r, written down as %r (%s)' % (case['id'], prec, k,
                                                                                             eng.info[k], v, eng.info)
    assert eng.reg_calls() == (0, 0), eng.reg_calls()
    # ... and the kernels the plan resolved are that instance (tests/test_gpu_call_forms.py: KERNELS shows the names)
    names = eng.sweep_kernels()
    assert set(names) == {'lean'}, names
    head = EC.kernel_head(want['_inst'])
    fwd, bwd = names['lean']
    assert 'pm_rollout_fwd' + head in fwd and 'pm_rollout_bwd' + head in bwd, (case['id'], prec, want['_inst'], names)


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
    covered = case['id'] not in EC.NO_ADJOINT_ORACLE
    eng, got, n = _run(case, d, prec, monkeypatch, optional=covered)
    _served_as_written(case, prec, eng)
    assert n == H, n
    assert _judge(case, d, prec, got, o64)
    if covered:
        _judge_optional(case, prec, got)
    if eng.info['inplace']:
        eng0, got0, n0 = _run(case, d, prec, monkeypatch, hint=0)
        assert eng0.info['inplace'] == 0 and eng0.info['rows_per_wg'] == 16 and eng0.info['precision'] == prec and n0 == H
        assert _judge(case, d, prec + ', two buffers of 16 rows', got0, o64)
        es, eg = EC.rel(got['states'], got0['states']), EC.rel(got['grad'], got0['grad'])
        print('%s [%s]: in place vs two buffers: states %.2e grad %.2e' % (case['id'], prec, es, eg))
        assert es < TOL_PAIR_STATES and eg < TOL_PAIR_GRAD, (case['id'], es, eg)


@pytest.mark.parametrize('case,prec', EC.pairs(EC.REFUSED), ids=EC.pair_ids(EC.REFUSED))
def test_shapes_just_outside_are_refused(case, prec, monkeypatch):
    """... at plan creation, with the code the table states and a message; the next plan on the same process works."""
    from prob_mbrl_amd import _lib
    code, word = case['refused']
    if word == 'n_layers':
        # nine Linear layers: the Engine cannot describe them (its own assert), so the C configuration of a valid plan,
        # with the policy's n_layers set to PMBRL_MAX_LAYERS + 1
        eng, _ = _engine(EC.by_id('centre'), _ref(EC.by_id('centre'))[0], prec, monkeypatch)
        cfg = type(eng.cfg).from_buffer_copy(eng.cfg)
        cfg.pol.n_layers = _lib.MAX_LAYERS + 1
        plan = C.c_void_p()
        rc = eng.lib.pmbrl_plan_create(C.byref(cfg), 0, C.byref(plan))
        msg = (eng.lib.pmbrl_last_error() or b'').decode()
        assert not plan.value
    else:
        with pytest.raises(_lib.PmbrlError) as err:
            _engine(case, EC.problem(case), prec, monkeypatch)
        msg = str(err.value)
        rc = int(msg.split('(')[1].split(')')[0])
        msg = msg.split('):', 1)[1].strip()
    print('%s [%s]: refused with %d: %s' % (case['id'], prec, rc, msg))
    assert rc == code and msg and word in msg, (rc, msg)
    centre = EC.by_id('centre')
    d, o64 = _ref(centre)
    eng, got, n = _run(centre, d, prec, monkeypatch)
    _served_as_written(centre, prec, eng)
    assert n == centre['cfg']['H'] and _judge(centre, d, prec + ', after a refusal', got, o64)


@pytest.mark.parametrize('prec', EC.BOTH)
def test_adjoint_in_two_step_ranges(prec, monkeypatch):
    """PMBRL_DW_PIPE=3,2 at H = 5: the adjoint sweep as two launches over the steps [2, 5) and [0, 2), the state gradient
    carried through HBM between them, against the one-launch sweep."""
    case = EC.by_id(EC.RANGE_CASE)
    d, o64 = _ref(case)
    eng1, got1, n1 = _run(case, d, prec, monkeypatch, env=(('PMBRL_DW_PIPE', 'off'),))
    eng2, got2, n2 = _run(case, d, prec, monkeypatch, env=(('PMBRL_DW_PIPE', '3,2'),))
    _served_as_written(case, prec, eng2)
    assert eng1.info['dw_pipe'] == 1 and eng2.info['dw_pipe'] == 2 and n1 == 5 and n2 == 5, (eng1.info, eng2.info)
    e = EC.rel(got2['grad'], got1['grad'])
    print('%s [%s]: gradient, two step ranges vs one launch: %.2e' % (case['id'], prec, e))
    assert e < TOL_RANGES, (prec, e)
    _judge(case, d, prec + ', two step ranges', got2, o64)


@pytest.mark.parametrize('cid,prec', [(c, p) for c in EC.TWICE_CASES for p in EC.by_id(c)['precision']])
def test_every_form_is_deterministic(cid, prec, monkeypatch):
    """tests/test_gpu_kernels.py::test_deterministic on one case per form -- two buffers, in place 1 and 2, moment matching
    in a workgroup, the per-step one-wave routines and multi-wave kernels: two engines, bit for bit"""
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
    step 6 computes x_7.  Nothing raises, the step is reported -- EC.OVERFLOW_STEPS: 6 in exact fp32; on split operands
    the first step whose network input holds the 5e37, step 1, as tests/test_gpu_reg_envelope.py pins for the
    register-resident family -- the gradient is finite, and the kept steps, their loss and their gradient are the fp64
    oracle's run to that many steps."""
    d = EC.problem(case)
    nodrift = EC.problem(case, drift=0.0)
    eng, got, n = _run(case, d, prec, monkeypatch)
    _served_as_written(case, prec, eng)
    print('%s [%s]: %d of %d steps are kept' % (case['id'], prec, n, case['cfg']['H']))
    assert n == EC.OVERFLOW_STEPS[prec], n
    o64 = EC.split_drift(_ref(case, n)[1])
    got = EC.split_drift(got)
    assert EC.rel(got['drift'], o64['drift']) < 1e-6
    _judge(case, nodrift, prec, got, o64, n_steps=n)
