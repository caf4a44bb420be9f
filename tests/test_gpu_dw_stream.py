"""GPU (-m gpu): the dW GEMM of the policy's second hidden layer BESIDE the one-launch register-resident adjoint sweep
(the streamed form: csrc/pmbrl_dw_plan.h pm_dw_plan_stream, csrc/pmbrl_dw_kernels.h pm_dw_layer_st_kernel, csrc/pmbrl_reg.h the
publication of the policy head's gradient).  Every case is forced with PMBRL_DW_STREAM=<steps>[,<workgroups>] and compared
with PMBRL_DW_STREAM=off on the same problem (tests/reg_envelope_cases.py; policy keep probability 0.9):

  rows17-h1      two chunks, one row in the second workgroup; the reduction reads ONE partial row, so one consumer takes the
                 pair (the `off` form's bits) and every other consumer has no row and leaves
  rows40-h3      the last workgroup has 8 valid rows; every step streamed, a cut in the middle (steps 2..1 streamed, step 0
                 behind the sweep), nothing streamed
  w193 / w208    tile 12 with one valid feature / sixteen
  d3u2 / d1u7    the head gradient spread over lane groups, several granules a lane
  rows200-h40    13 chunks a step: with three consumers, 40 steps of slices of 4-5 chunks (pairs and an odd last chunk);
                 with the plan's consumers, more consumers than chunks a step (130 rows, 13 chunks: most consumers' slices
                 are empty and their rows are written as zeros)
  rows40-h3 with the status word at 2, then 0: the truncated horizon

Each: both sweeps ran on the family; the gradient holds the project's bars against the fp64 oracle
(tests/test_gpu_reg_envelope.py's judgement); everything but the W1 / b1 slices equals the `off` form bit for bit; W1 and
b1 -- the same terms summed in another fixed order -- are within TOL_PAIR_PLAIN of it (a dropped or doubled chunk would be
an error of order 1 at these chunk counts); five repetitions agree bit for bit.

Measured distances of W1 / b1 to the `off` form (relative to its norm; everything else was bit-equal), MI355X:
  rows17-h1@1     0 / 0                    rows40-h3@3    7.005e-08 / 7.121e-08
  rows40-h3@2     6.782e-08 / 8.731e-08    rows40-h3@0    5.278e-08 / 5.749e-08
  w193@3          7.536e-08 / 9.143e-08    w208@2         7.497e-08 / 9.026e-08
  d3u2@3          6.848e-08 / 6.179e-08    d1u7@2         6.661e-08 / 8.019e-08
  rows200-h40@40,3  3.387e-07 / 1.277e-07  rows200-h40@30  1.355e-07 / 1.050e-07
  truncated (rows40-h3, status word 2): 6.951e-08 / 7.407e-08 at @3, 4.829e-08 / 5.515e-08 at @2; status word 0: all zero
"""
import numpy as np
import pytest
import torch

from tests import reg_envelope_cases as EC
from tests.test_gpu_dw_rebuild import BY_ID, _engine, _iteration, _layer1, _weights
from tests.test_gpu_reg_envelope import _judge

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (case, PMBRL_DW_STREAM)
FORCED = [
    ('rows17-h1', '1'),
    ('rows40-h3', '3'),        # every step
    ('rows40-h3', '2'),        # steps 2..1 streamed, step 0 behind the sweep
    ('rows40-h3', '0'),        # nothing streamed: the launch behind the sweep takes every step
    ('w193', '3'),
    ('w208', '2'),
    ('d3u2', '3'),
    ('d1u7', '2'),
    ('rows200-h40', '40,3'),   # three consumers: slices of 4, 4, 5 chunks
    ('rows200-h40', '30'),     # the plan's consumers: more of them than chunks a step
]

_OFF = {}


def _off(cid, monkeypatch):
    """the `off` form's iteration and the oracle's, once per case"""
    if cid not in _OFF:
        case = BY_ID[cid]
        d = EC.problem(case)
        eng, args = _engine(case, d, monkeypatch, env=(('PMBRL_DW_STREAM', 'off'),))
        assert eng.dw_stream() is None
        ref = _iteration(eng, args, _weights(d))
        assert eng.reg_calls() == (1, 1), eng.reg_calls()
        _OFF[cid] = (d, ref, EC.oracle(d, torch.float64))
    return _OFF[cid]


def _compare(cid, d, got, ref, what):
    """everything but W1 / b1 bit for bit; those two within TOL_PAIR_PLAIN"""
    for k in ('states', 'actions', 'rewards'):
        assert np.array_equal(got[k], ref[k]), (cid, what, k)
    assert got['loss'] == ref['loss'], (cid, what)
    layer1 = _layer1(d)
    for name, sl in EC.param_slices(d):
        if name in layer1:
            e = EC.rel(got['grad'][sl], ref['grad'][sl]) if np.any(ref['grad'][sl]) else float(np.abs(got['grad'][sl]).max())
            print('    %s %s: %s %.3e' % (cid, what, name, e))
            assert e < EC.TOL_PAIR_PLAIN, (cid, what, name, e)
        else:
            assert np.array_equal(got['grad'][sl], ref['grad'][sl]), (cid, what, name)


@pytest.mark.parametrize('cid,spec', FORCED, ids=['%s@%s' % f for f in FORCED])
def test_streamed_gemm_gives_the_gradient_of_the_launch_behind_the_sweep(cid, spec, monkeypatch):
    case = BY_ID[cid]
    d, ref, o64 = _off(cid, monkeypatch)
    eng, args = _engine(case, d, monkeypatch, env=(('PMBRL_DW_STREAM', spec),))
    steps = int(spec.split(',')[0])
    st = eng.dw_stream()
    assert st is not None and st[0] == steps and (',' not in spec or st[1] == int(spec.split(',')[1])), (st, spec)
    gw = _weights(d)
    got = _iteration(eng, args, gw)
    assert eng.reg_calls() == (1, 1), eng.reg_calls()
    assert int(eng.status[1]) == 0
    _judge(case, d, 'streamed ' + spec, got, o64)
    _compare(cid, d, got, ref, spec)
    for rep in range(4):
        again = _iteration(eng, args, gw)
        assert np.array_equal(again['grad'], got['grad']), (cid, spec, rep)
    assert eng.reg_calls() == (5, 5)


def test_truncated_horizon_streams_the_valid_steps_only(monkeypatch):
    """rows40-h3, every step streamed; the status word at 2 of 3 steps after a complete iteration, then at 0, then complete
    again: each as the `off` form under the same status word."""
    cid = 'rows40-h3'
    case = BY_ID[cid]
    d = EC.problem(case)
    eng0, args0 = _engine(case, d, monkeypatch, env=(('PMBRL_DW_STREAM', 'off'),))
    outs = {}
    for spec in ('3', '2'):
        eng, args = _engine(case, d, monkeypatch, env=(('PMBRL_DW_STREAM', spec),))
        for nv in (None, 2, 0, None):
            gw = _weights(d, nv)
            if (nv, 'off') not in outs:
                outs[(nv, 'off')] = _iteration(eng0, args0, gw, n_valid=nv)
            got = _iteration(eng, args, gw, n_valid=nv)
            assert np.all(np.isfinite(got['grad'])) and int(eng.status[1]) == 0
            _compare(cid, d, got, outs[(nv, 'off')], 'stream %s, status word %r' % (spec, nv))
            if nv == 0:
                assert np.all(got['grad'] == 0.0)
            if nv == 2:
                d2 = dict(d, H=2, gamma=np.asarray(d['gamma'])[:2])
                _judge(case, d2, 'truncated', got, EC.oracle(d2, torch.float64))
    assert EC.rel(outs[(2, 'off')]['grad'], outs[(None, 'off')]['grad']) > 1e-3


def test_recorded_streamed_call_does_not_meet_its_own_tags(monkeypatch):
    """The adjoint call recorded while the form is forced (rows40-h3, every step streamed) and replayed six times with the
    policy changed in between: a replay repeats the launch generation it was recorded with, so the recording carries the
    fill of the granules -- without it the consumers could take the replay before's head gradients for this one's.  Each
    replay equals the eager call on the same parameters, bit for bit."""
    from prob_mbrl_amd import engine as E
    case = BY_ID['rows40-h3']
    d = EC.problem(case)
    eng, args = _engine(case, d, monkeypatch, env=(('PMBRL_DW_STREAM', '3'),))
    assert eng.dw_stream() is not None and eng.dw_stream()[0] == 3
    gw = _weights(d)
    params = args['pol_flat'].clone()
    args['pol_flat'] = params
    p0 = params.clone()
    scales = [1.0, 0.97, 1.02, 0.99, 1.0, 1.01]

    def eager(sc):
        params.copy_(p0 * sc)
        eng.forward(**args)
        eng.backward(gw)
        torch.cuda.synchronize()
        return eng.grad_flat.cpu().numpy().copy()

    want = [eager(sc) for sc in scales]
    assert not np.array_equal(want[0], want[1])
    params.copy_(p0)
    eng.forward(**args)
    gb = E.Graph(lambda: eng.backward(gw), warmup=1)
    for sc, w in zip(scales, want):
        params.copy_(p0 * sc)
        eng.forward(**args)
        gb.replay()
        torch.cuda.synchronize()
        assert int(eng.status[1]) == 0
        assert np.array_equal(eng.grad_flat.cpu().numpy(), w), sc
    # ... and an eager call behind the replays: a new generation over the recording's leftover tags
    assert np.array_equal(eager(scales[1]), want[1])


def test_plan_rule(monkeypatch):
    """The headline shape (bench.py's cartpole_nomm) streams by default; the 200-row fixture's sweep is too small to hide
    anything; a sweep that moment-matches the states runs another instance, with flag barriers or the statistics exchange
    beside it."""
    from prob_mbrl_amd import problem as PB
    from tests import common
    monkeypatch.delenv('PMBRL_DW_STREAM', raising=False)
    got = {}
    for name in ('cartpole_nomm', 'cartpole_mm'):
        d = PB.synthetic_problem(name, seed=0, data_seed=0)
        eng, _, _ = PB.engine_from_problem(d, torch.device(DEV))
        got[name] = (eng.dw_stream(), dict(eng.info))
        del eng
    eng, _, _ = common.engine_from_fixture(common.load('full200_nomm'), torch.device(DEV))
    got['full200_nomm'] = (eng.dw_stream(), dict(eng.info))
    st, info = got['cartpole_nomm']
    assert info['reg'] and info['precision'] == 'split_f16' and info['dw_pipe'] == 1, info
    assert st is not None and 0 < st[0] <= 40 and st[1] >= 32, st
    assert got['full200_nomm'][1]['reg'] and got['full200_nomm'][0] is None, got['full200_nomm']
    assert got['cartpole_mm'][0] is None, got['cartpole_mm']
