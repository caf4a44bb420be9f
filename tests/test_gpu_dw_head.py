"""GPU (-m gpu): the policy HEAD's dW / db formed by the streamed consumers beside the one-launch adjoint sweep, and the
reduction that reads the consumers' rows only (csrc/pmbrl_dw_plan.h pm_dw_plan_head, csrc/pmbrl_dw_kernels.h pm_dw_layer_body's head
phase and pm_dw_kernel_nh, csrc/pmbrl_tail.hip pm_dw_reduce's column range).  Every forced case runs with
PMBRL_DW_STREAM=<H>[,<workgroups>] plus PMBRL_DW_HEAD=on and is compared with PMBRL_DW_STREAM=off on the same problem
(tests/reg_envelope_cases.py; policy keep probability 0.9):

  rows17-h1      one partial row: one consumer takes the pair, the head's with it
  rows40-h3      the last workgroup has 8 valid rows
  w193 / w208    tile 12 with one valid feature / sixteen; the consumers' column range starts off a multiple of 4
  d3u2 / d1u7    several granules a lane; 4 / 14 head rows
  rows200-h40    13 chunks a step: with three consumers, slices of 4-5 chunks (pairs and an odd last chunk); with the plan's
                 consumers, more of them than chunks a step (empty slices write zeros into W1 .. b2 of their rows)
  rows40-h3 with the status word at 2, then 0, then complete: the truncated horizon
  rows40-h3 recorded and replayed; rows40-h3 with a cut (the head stays in the block kernel); the plan rule

Each forced case: the head form is reported on; both sweeps ran on the family; status[1] == 0; the gradient holds the
project's bars against the fp64 oracle (tests/test_gpu_reg_envelope.py's judgement); trajectory, loss, W0 and b0 equal the
`off` form bit for bit (the block kernel's table without the head deals the same accumulator chains to other waves); W1, b1,
W2 and b2 -- the same terms summed in another fixed order -- are within TOL_PAIR_PLAIN of it; four repetitions agree bit for
bit.

Measured distances of W1 / b1 / W2 / b2 to the `off` form (relative to its norm; everything else was bit-equal), MI355X:
  rows17-h1@1       0 / 0 / 0 / 0
  rows40-h3@3       7.005e-08 / 7.121e-08 / 7.728e-08 / 1.433e-07
  w193@3            7.536e-08 / 9.143e-08 / 1.019e-07 / 7.487e-08
  w208@3            7.964e-08 / 7.763e-08 / 1.233e-07 / 7.918e-08
  d3u2@3            6.848e-08 / 6.179e-08 / 8.694e-08 / 9.648e-08
  d1u7@3            6.805e-08 / 7.134e-08 / 8.729e-08 / 8.448e-08
  rows200-h40@40,3  3.387e-07 / 1.277e-07 / 5.080e-07 / 2.043e-08
  rows200-h40@40    1.735e-07 / 1.115e-07 / 2.110e-07 / 8.425e-08
  truncated (rows40-h3, status word 2): 6.951e-08 / 7.407e-08 / 7.233e-08 / 2.132e-08; status word 0: all zero
(W1 / b1 are the numbers of tests/test_gpu_dw_stream.py where it runs the same spec: the layer's sums are the ones they were.)
"""
import numpy as np
import pytest
import torch

from tests import reg_envelope_cases as EC
from tests.test_gpu_dw_rebuild import BY_ID, _engine, _iteration, _weights
from tests.test_gpu_reg_envelope import _judge

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STREAMED = ('W1', 'b1', 'W2', 'b2')      # the consumers' columns

# (case, PMBRL_DW_STREAM): every step streamed
FORCED = [
    ('rows17-h1', '1'),
    ('rows40-h3', '3'),
    ('w193', '3'),
    ('w208', '3'),
    ('d3u2', '3'),
    ('d1u7', '3'),
    ('rows200-h40', '40,3'),   # three consumers: slices of 4, 4, 5 chunks
    ('rows200-h40', '40'),     # the plan's consumers: more of them than chunks a step
]

_OFF = {}


def _env(spec, head='on'):
    return (('PMBRL_DW_STREAM', spec), ('PMBRL_DW_HEAD', head))


def _off(cid, monkeypatch):
    """the `off` form's iteration and the oracle's, once per case"""
    if cid not in _OFF:
        case = BY_ID[cid]
        d = EC.problem(case)
        eng, args = _engine(case, d, monkeypatch, env=(('PMBRL_DW_STREAM', 'off'),))
        assert eng.dw_stream() is None and not eng.dw_head()
        ref = _iteration(eng, args, _weights(d))
        assert eng.reg_calls() == (1, 1), eng.reg_calls()
        _OFF[cid] = (d, ref, EC.oracle(d, torch.float64))
    return _OFF[cid]


def _compare(cid, d, got, ref, what):
    """everything but the consumers' columns bit for bit; those within TOL_PAIR_PLAIN"""
    for k in ('states', 'actions', 'rewards'):
        assert np.array_equal(got[k], ref[k]), (cid, what, k)
    assert got['loss'] == ref['loss'], (cid, what)
    names = [name for name, _ in EC.param_slices(d)]
    assert names == ['W0', 'b0', 'W1', 'b1', 'W2', 'b2'], names
    for name, sl in EC.param_slices(d):
        if name in STREAMED:
            e = EC.rel(got['grad'][sl], ref['grad'][sl]) if np.any(ref['grad'][sl]) else float(np.abs(got['grad'][sl]).max())
            print('    %s %s: %s %.3e' % (cid, what, name, e))
            assert e < EC.TOL_PAIR_PLAIN, (cid, what, name, e)
        else:
            assert np.array_equal(got['grad'][sl], ref['grad'][sl]), (cid, what, name)


@pytest.mark.parametrize('cid,spec', FORCED, ids=['%s@%s' % f for f in FORCED])
def test_consumers_form_the_head_gradient_of_the_block_kernel(cid, spec, monkeypatch):
    case = BY_ID[cid]
    d, ref, o64 = _off(cid, monkeypatch)
    assert int(spec.split(',')[0]) == int(d['H'])
    eng, args = _engine(case, d, monkeypatch, env=_env(spec))
    st = eng.dw_stream()
    assert st is not None and st[0] == int(d['H']) and (',' not in spec or st[1] == int(spec.split(',')[1])), (st, spec)
    assert eng.dw_head()
    gw = _weights(d)
    got = _iteration(eng, args, gw)
    assert eng.reg_calls() == (1, 1), eng.reg_calls()
    assert int(eng.status[1]) == 0
    _judge(case, d, 'head streamed ' + spec, got, o64)
    _compare(cid, d, got, ref, spec)
    for rep in range(4):
        again = _iteration(eng, args, gw)
        assert np.array_equal(again['grad'], got['grad']), (cid, spec, rep)
    assert eng.reg_calls() == (5, 5)


def test_truncated_horizon_streams_the_head_of_the_valid_steps_only(monkeypatch):
    """rows40-h3, every step and the head streamed; the status word at 2 of 3 steps after a complete iteration, then at 0,
    then complete again: each as the `off` form under the same status word."""
    cid = 'rows40-h3'
    case = BY_ID[cid]
    d = EC.problem(case)
    eng0, args0 = _engine(case, d, monkeypatch, env=(('PMBRL_DW_STREAM', 'off'),))
    eng, args = _engine(case, d, monkeypatch, env=_env('3'))
    assert eng.dw_head()
    outs = {}
    for nv in (None, 2, 0, None):
        gw = _weights(d, nv)
        if nv not in outs:
            outs[nv] = _iteration(eng0, args0, gw, n_valid=nv)
        got = _iteration(eng, args, gw, n_valid=nv)
        assert np.all(np.isfinite(got['grad'])) and int(eng.status[1]) == 0
        _compare(cid, d, got, outs[nv], 'status word %r' % (nv,))
        if nv == 0:
            assert np.all(got['grad'] == 0.0)
        if nv == 2:
            d2 = dict(d, H=2, gamma=np.asarray(d['gamma'])[:2])
            _judge(case, d2, 'truncated', got, EC.oracle(d2, torch.float64))
    assert EC.rel(outs[2]['grad'], outs[None]['grad']) > 1e-3


def test_recorded_call_with_the_head_streamed_replays_the_eager_call(monkeypatch):
    """The adjoint call recorded with the head form on (rows40-h3) and replayed six times with the policy changed in
    between: each replay equals the eager call on the same parameters, bit for bit."""
    from prob_mbrl_amd import engine as E
    case = BY_ID['rows40-h3']
    d = EC.problem(case)
    eng, args = _engine(case, d, monkeypatch, env=_env('3'))
    assert eng.dw_stream() is not None and eng.dw_stream()[0] == 3 and eng.dw_head()
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
    assert np.array_equal(eager(scales[1]), want[1])


def test_cut_keeps_the_head_in_the_block_kernel(monkeypatch):
    """PMBRL_DW_STREAM=2 on rows40-h3 leaves step 0 to the launch behind the sweep: PMBRL_DW_HEAD=on does not apply, and the
    whole gradient is that of PMBRL_DW_STREAM=2 alone, bit for bit."""
    case = BY_ID['rows40-h3']
    d = EC.problem(case)
    gw = _weights(d)
    eng, args = _engine(case, d, monkeypatch, env=_env('2'))
    assert eng.dw_stream() is not None and eng.dw_stream()[0] == 2 and not eng.dw_head()
    got = _iteration(eng, args, gw)
    eng1, args1 = _engine(case, d, monkeypatch, env=(('PMBRL_DW_STREAM', '2'),))
    assert eng1.dw_stream()[0] == 2 and not eng1.dw_head()
    ref = _iteration(eng1, args1, gw)
    assert int(eng.status[1]) == 0 and np.array_equal(got['grad'], ref['grad'])


def test_plan_rule(monkeypatch):
    """The headline shape (bench.py's cartpole_nomm) streams every step and the head by default, not the head under
    PMBRL_DW_HEAD=off; a forced PMBRL_DW_STREAM keeps the head in the block kernel; the shapes that do not stream at all
    do not stream the head."""
    from prob_mbrl_amd import problem as PB
    from tests import common
    monkeypatch.delenv('PMBRL_DW_STREAM', raising=False)
    monkeypatch.delenv('PMBRL_DW_HEAD', raising=False)
    dev = torch.device(DEV)
    d = PB.synthetic_problem('cartpole_nomm', seed=0, data_seed=0)
    eng, _, _ = PB.engine_from_problem(d, dev)
    assert eng.dw_stream() is not None and eng.dw_stream()[0] == int(d['H']) and eng.dw_head(), eng.dw_stream()
    del eng
    monkeypatch.setenv('PMBRL_DW_HEAD', 'off')
    eng, _, _ = PB.engine_from_problem(d, dev)
    assert eng.dw_stream() is not None and not eng.dw_head()
    del eng
    monkeypatch.delenv('PMBRL_DW_HEAD')
    monkeypatch.setenv('PMBRL_DW_STREAM', '%d' % int(d['H']))
    eng, _, _ = PB.engine_from_problem(d, dev)
    assert eng.dw_stream() is not None and not eng.dw_head()
    del eng
    monkeypatch.delenv('PMBRL_DW_STREAM')
    eng, _, _ = PB.engine_from_problem(PB.synthetic_problem('cartpole_mm', seed=0, data_seed=0), dev)
    assert eng.dw_stream() is None and not eng.dw_head()
    del eng
    eng, _, _ = common.engine_from_fixture(common.load('full200_nomm'), dev)
    assert eng.info['reg'] and eng.dw_stream() is None and not eng.dw_head()
