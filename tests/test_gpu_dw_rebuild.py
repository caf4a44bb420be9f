"""GPU (-m gpu): the dW GEMM of the policy's second hidden layer behind a register-resident adjoint sweep REBUILDS its
delta operand (csrc/pmbrl_dw_kernels.h, pm_dw_layer_rc_kernel) -- the sweep no longer stashes it (csrc/pmbrl_reg.h,
head_adjoint).  Small shapes where that kernel can go wrong and the envelope table (tests/reg_envelope_cases.py) is thin:

  rows40-h3      three sweep workgroups, nine chunks, the last workgroup has 8 valid rows; one chunk per partial row
                 (every step of the GEMM is an odd range's last: its second chunk's tiles are zeros); pipelined, most
                 partial rows of a launch are empty and take the zero-writing path
  rows17-h1      two chunks, one row in the second workgroup
  w193 / w208    tile 12 has one valid feature / all sixteen
  d3u2 / d1u7    the head gradient's rows are spread over several lane groups
  rows200-h40    520 chunks in ranges of three: a chunk pair that straddles sweep workgroups and steps (13 a step), then
                 the odd last step, in every GEMM workgroup

All with dropout keep probability 0.9 on the policy (synthetic_problem), so 1 / keep and the activity nibbles matter.
Each case: the family served both sweeps; the gradient against the fp64 oracle at the project's bars (whole and per
tensor, tests/test_gpu_reg_envelope.py's judgement); against the OTHER family's adjoint on the same forward sweep
(PMBRL_REG_BWD=0: it writes the stash and runs the classic kernel) at TOL_PAIR_PLAIN; and, for the second hidden
layer's weight and bias, no further from that adjoint than twice what the parent commit was (PARENT below)."""
import numpy as np
import pytest
import torch

from tests import reg_envelope_cases as EC
from tests.test_gpu_reg_envelope import _judge

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CASES = [
    EC._case('rows40-h3', 41, rows=40, H=3),
    EC._case('rows17-h1', 42, rows=17, H=1),
    EC._case('w193', 43, width=193, rows=40, H=3),
    EC._case('w208', 44, width=208, rows=40, H=3),
    EC._case('d3u2', 45, D=3, U=2, rows=40, H=3),
    EC._case('d1u7', 46, D=1, U=7, rows=40, H=3),
    EC._case('rows200-h40', 47, rows=200, H=40),
]
BY_ID = {c['id']: c for c in CASES}

# Distance of the second hidden layer's gradient slices (W1, b1) between the family's adjoint and the other family's
# adjoint on the same forward sweep, relative to the other's norm, measured on the PARENT commit b089921 (which stashed
# the delta and read it back) in the same GPU visit as this change.  The rebuilt operand is the stash's bits -- the same
# MFMA pair on the same fragments, the product rounded before it is split -- so the weight gradient W1 equals the
# parent's bit for bit on all seven cases and its numbers are the SAME, digit for digit.  The bias gradient b1 is the
# sum of the same values in another fixed order (per row over the range, then a tree over the rows): this change
# measured the parent's numbers to all four digits on six cases and 2.986e-06 on rows200-h40.  The factor of two the
# bound leaves is room for one more rounding of the operand that did not turn out to be needed.
PARENT = {
    'rows40-h3': dict(W1=4.359e-06, b1=3.780e-06),
    'rows17-h1': dict(W1=1.091e-05, b1=1.007e-05),
    'w193': dict(W1=6.117e-06, b1=5.748e-06),
    'w208': dict(W1=4.642e-06, b1=4.007e-06),
    'd3u2': dict(W1=3.609e-06, b1=3.255e-06),
    'd1u7': dict(W1=2.716e-06, b1=2.530e-06),
    'rows200-h40': dict(W1=3.426e-06, b1=2.990e-06),
}


def _engine(case, d, monkeypatch, env=()):
    """the plan's switches are read once, at plan creation"""
    from prob_mbrl_amd import problem as PB
    for k, v in env:
        monkeypatch.setenv(k, v)
    eng, args, _ = PB.engine_from_problem(d, torch.device(DEV), rows_per_wg_hint=case['hint'])
    for k, _v in env:
        monkeypatch.delenv(k, raising=False)
    assert eng.info['precision'] == 'split_f16' and eng.info['reg'], eng.info
    return eng, args


def _weights(d, n_valid=None):
    from prob_mbrl_amd import problem as PB
    gw = torch.tensor(PB.loss_weights(d, d['x0'].shape[0]), device=DEV)
    if n_valid is not None:
        gw[n_valid:] = float('nan')       # nothing may read the weights of the steps that do not count
    return gw


def _iteration(eng, args, gw, n_valid=None, **kw):
    """forward, backward(gw, **kw) -> what tests/test_gpu_reg_envelope.py's _run returns of an iteration"""
    S, A, Rw = eng.forward(**args)
    if n_valid is not None:
        eng.status[0] = n_valid
    ok = torch.nan_to_num(gw, nan=0.0)
    loss = float(eng.weighted_sum(Rw, ok))
    g = eng.backward(gw, **kw)[0]
    torch.cuda.synchronize()
    n = eng.valid_steps()
    B = S.shape[1]
    return dict(states=S.cpu().numpy()[:n + 1], actions=A.cpu().numpy()[:n], rewards=Rw.cpu().numpy().reshape(-1, B)[:n],
                loss=loss, grad=g.cpu().numpy().copy())


def _layer1(d):
    return {k: sl for k, sl in EC.param_slices(d) if k in ('W1', 'b1')}


def measure(case, monkeypatch):
    """-> (problem, the family's iteration, the other family's adjoint on the same kind of forward sweep,
    {W1, b1: distance})"""
    d = EC.problem(case)
    eng, args = _engine(case, d, monkeypatch)
    got = _iteration(eng, args, _weights(d))
    assert eng.reg_calls() == (1, 1), eng.reg_calls()
    eng0, args0 = _engine(case, d, monkeypatch, env=(('PMBRL_REG_BWD', '0'),))
    other = _iteration(eng0, args0, _weights(d))
    assert eng0.reg_calls() == (1, 0), eng0.reg_calls()      # the same forward sweep, the other family's adjoint
    dist = {k: EC.rel(got['grad'][sl], other['grad'][sl]) for k, sl in _layer1(d).items()}
    print("    '%s': dict(W1=%.3e, b1=%.3e)," % (case['id'], dist['W1'], dist['b1']))
    return d, got, other, dist


@pytest.mark.parametrize('case', CASES, ids=EC.ids(CASES))
def test_rebuilt_delta_gives_the_stashed_delta_s_gradient(case, monkeypatch):
    d, got, other, dist = measure(case, monkeypatch)
    assert np.array_equal(got['states'], other['states'])       # (one forward sweep, run twice)
    _judge(case, d, 'rebuilt', got, EC.oracle(d, torch.float64))
    e = EC.rel(got['grad'], other['grad'])
    print('%s: gradient, rebuilt vs the other adjoint: %.2e' % (case['id'], e))
    assert e < EC.TOL_PAIR_PLAIN, (case['id'], e)
    for k, v in dist.items():
        assert v <= 2.0 * PARENT[case['id']][k], (case['id'], k, v, PARENT[case['id']][k])


def test_truncated_horizon_takes_no_chunk_of_an_invalid_step(monkeypatch):
    """rows40-h3 with the status word set to 2 of 3 steps, after a complete iteration that left every stash of step 2
    and every partial row filled: the gradient is that of the same problem with H = 2, bit for bit (the same six
    partial rows; the reduction takes the rows of the valid steps only, in the slices it would cut six rows into)."""
    case = BY_ID['rows40-h3']
    d = EC.problem(case)
    n = 2
    eng, args = _engine(case, d, monkeypatch)
    full = _iteration(eng, args, _weights(d))
    cut = _iteration(eng, args, _weights(d, n), n_valid=n)
    assert eng.reg_calls() == (2, 2) and len(cut['actions']) == n
    d2 = dict(d, H=n, gamma=np.asarray(d['gamma'])[:n])
    eng2, args2 = _engine(case, d2, monkeypatch)
    short = _iteration(eng2, args2, _weights(d)[:n].contiguous())
    assert eng2.reg_calls() == (1, 1)
    e = EC.rel(cut['grad'], short['grad'])
    print('truncated to %d of %d steps vs H = %d: %.2e (complete: %.2e)' % (n, case['cfg']['H'], n, e, EC.rel(full['grad'], short['grad'])))
    assert np.all(np.isfinite(cut['grad'])) and np.array_equal(cut['grad'], short['grad']), e
    assert EC.rel(full['grad'], short['grad']) > 1e-3
    _judge(case, d2, 'truncated', cut, EC.oracle(d2, torch.float64))


@pytest.mark.parametrize('cid,spec', [('rows40-h3', '2,1'), ('rows200-h40', '30,10')])
def test_pipelined_ranges_rebuild_the_delta_too(cid, spec, monkeypatch):
    """PMBRL_DW_PIPE: every range's launch takes the rebuilding form -- 2,1 on rows40-h3: six and three chunks dealt to a
    chip's worth of partial rows, nearly all of them written as zeros; 30,10 on rows200-h40: chunk pairs in the first
    range.  What tests/test_gpu_dw_pipeline.py asserts of the pipelined form: the same products in another order of
    additions."""
    case = BY_ID[cid]
    d = EC.problem(case)
    H = case['cfg']['H']
    eng, args = _engine(case, d, monkeypatch)
    one = _iteration(eng, args, _weights(d))
    engp, argsp = _engine(case, d, monkeypatch, env=(('PMBRL_DW_PIPE', spec), ('PMBRL_MM_PARTS', '1')))
    assert eng.info['dw_pipe'] == 1 and engp.info['dw_pipe'] == 2, engp.info
    piped = _iteration(engp, argsp, _weights(d))
    assert engp.reg_calls() == (1, 2), engp.reg_calls()      # (one adjoint launch a range)
    e = EC.rel(piped['grad'], one['grad'])
    print('%s: pipelined vs one launch: %.2e' % (cid, e))
    assert e < 2e-6, e
    assert EC.rel(piped['grad'], EC.oracle(d, torch.float64)['grad']) < EC.TOL_GRAD
    if H == 3:
        # a truncated horizon through the ranges: the end of the valid steps inside the first range
        cut = _iteration(engp, argsp, _weights(d, 2), n_valid=2)
        ref = _iteration(eng, args, _weights(d, 2), n_valid=2)
        assert np.all(np.isfinite(cut['grad'])) and EC.rel(cut['grad'], ref['grad']) < 2e-6


def test_replayed_calls_carry_the_form_of_their_dw_kernel(monkeypatch):
    """set_replay(2): the plain call eager, recorded, replayed; then a call with want_x0 (still this family's adjoint),
    one with want_agn (the other family's adjoint on the same forward sweep: it writes the stash, the classic kernel
    reads it), then the plain call again -- the note of which form follows the sweep travels with the recording.  Every
    gradient is the eager plan's, bit for bit."""
    case = BY_ID['rows40-h3']
    d = EC.problem(case)
    gw = _weights(d)

    def run(replay):
        eng, args = _engine(case, d, monkeypatch)
        eng.set_replay(replay)
        out = {}
        for k in range(3):
            out['plain%d' % k] = _iteration(eng, args, gw)['grad']
        out['x0'] = _iteration(eng, args, gw, want_x0=True)['grad']
        out['agn'] = _iteration(eng, args, gw, want_agn=True)['grad']
        out['again'] = _iteration(eng, args, gw)['grad']
        assert eng.reg_calls()[0] >= 1
        return eng, out

    eng0, eager = run(0)
    eng2, replayed = run(2)
    assert eng0.replay_count() == (0, 0) and eng0.reg_calls() == (6, 5)
    assert min(eng2.replay_count()) >= 1, eng2.replay_count()
    for k in eager:
        assert np.array_equal(eager[k], replayed[k]), k
    assert np.array_equal(eager['plain0'], eager['again']) and np.array_equal(eager['plain0'], eager['x0'])
    e = EC.rel(eager['agn'], eager['plain0'])
    assert 0.0 < e < EC.TOL_PAIR_PLAIN, e       # (another family's sweep: not the same bits, the same gradient)
