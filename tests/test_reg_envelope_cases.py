"""The envelope cases of the register-resident family (tests/reg_envelope_cases.py) are well conditioned: no kernel
takes part here.  For every case the oracle (oracle/ref_torch.py: iteration) runs in fp32 and in fp64, and the gap
between the two must be at most ONE QUARTER of the bar tests/test_gpu_reg_envelope.py applies to the same quantity.
A case on which plain fp32 arithmetic uses up the tolerance could pass or fail on the GPU for reasons that are not the
kernels'; such a case is re-drawn (another seed, a shorter horizon), not exempted."""
import numpy as np
import pytest

from tests import reg_envelope_cases as EC


def _gaps(case, n_steps=None):
    d = EC.problem(case)
    o64 = EC.oracle(d, EC.torch.float64, n_steps)
    o32 = EC.oracle(d, EC.torch.float32, n_steps)
    return d, o64, o32


def _check(case, d, o64, o32):
    e = EC.global_errors(o32, o64)
    sl = EC.slice_errors(d, o32, o64)
    over = {k: v[0] for k, v in sl.items() if v[0] > 0.25 * v[1]}
    print('%s: fp32 vs fp64 oracle: states %.2e actions %.2e rewards %.2e loss %.2e grad %.2e | worst slices: %s %.2e, %s %.2e, '
          '%s %.2e | slices beyond a quarter of their bar: %s' %
          ((case['id'], e['states'], e['actions'], e['rewards'], e['loss'], e['grad']) + EC.worst(sl, 'grad.') +
           EC.worst(sl, 'states.dim') + EC.worst(sl, 'states.step') + (over or 'none',)))
    for k, bar in EC.BARS.items():
        assert np.isfinite(e[k]) and e[k] <= 0.25 * bar, (case['id'], k, e[k])
    # (what the GPU test does with a slice: one whose oracle gap is beyond a quarter of its bar may fall back to the
    #  global norm there.  None of the cases has such a slice; a new case that does shows up here first)
    assert not over, over


@pytest.mark.parametrize('case', EC.CASES, ids=EC.ids(EC.CASES))
def test_case_is_well_conditioned(case):
    _check(case, *_gaps(case))


def test_the_table_covers_the_axes():
    """one varied axis per case around (width 200, D = 4, U = 1), both sides of every bound"""
    inside = [c['cfg'] for c in EC.CASES if c['inside']]
    outside = [c['cfg'] for c in EC.CASES if not c['inside']]
    assert {c['pol_hid'][0] for c in inside} == {193, 194, 200, 207, 208}
    assert {192, 209} <= {c['pol_hid'][0] for c in outside}
    plain = {(c['D'], c['U']) for c in inside if not c['mm']}
    assert {(1, 1), (2, 1), (3, 2), (4, 4), (7, 1), (1, 7), (5, 3)} <= plain
    assert {(8, 1), (5, 4)} <= {(c['D'], c['U']) for c in outside if not c['mm']}
    assert {1, 15, 16, 17, 77} <= {c['P'] * c['S'] for c in inside if not c['mm']}
    assert {1, 2, 3, 12} <= {c['H'] for c in inside if not c['mm']}
    for D in (4, 5, 6):
        lay = [(c['layout']['mm_parts'], c['layout']['rows_per_wg']) for c in EC.CASES
               if c['inside'] and c['cfg']['mm'] and c['cfg']['D'] == D]
        assert {(1, 16), (2, 13), (2, 9), (8, 16)} <= set(lay), (D, lay)
        assert {c.get('mm_rewards', True) for c in inside if c['mm'] and c['D'] == D} == {True, False}
    assert {(c['D']) for c in outside if c['mm']} >= {3, 5, 7}
    assert {c['reward'] for c in inside if c['D'] in (4, 5) and c['U'] == 1} == {'cartpole'}
    assert {c['reward'] for c in inside if c['D'] == 6} == {'double_cartpole'}


@pytest.mark.parametrize('case', EC.SAT_CASES, ids=EC.ids(EC.SAT_CASES))
def test_saturation_case_covers_the_range_and_is_well_conditioned(case):
    """The conditions are on the fp64 ORACLE's head values.  Saturating policy: at least 10 % of the (step, row, action)
    entries beyond pr_tanh's overflow point of old (|u| > 44), 10 % between its clamp and that point, 10 % where tanh
    is far from flat.  Log-std heads: at least 10 % of the entries of either head beyond each end of pr_sigmoid_neg's
    clamp (|ls - max_log_std| > 80)."""
    d, o64, o32 = _gaps(case)
    shares = EC.saturation_shares(case, o64)
    print(case['id'], {k: round(v, 3) for k, v in shares.items()})
    assert shares and all(v >= 0.10 for v in shares.values()), shares
    _check(case, d, o64, o32)


@pytest.mark.parametrize('case', EC.OVERFLOW_CASES, ids=EC.ids(EC.OVERFLOW_CASES))
def test_overflow_case_is_well_conditioned_on_the_steps_before_it(case):
    """The drifting dimension overflows fp32 while step 6 computes x_7 (7 x 5e37 > 3.4e38).  It is decoupled from
    everything the bars are applied to, so the conditioning of the kept steps is that of the same problem without the
    drift -- which, unlike the drifting one, the oracle can run in fp32 under moment matching too (the fp32 mean of 16
    values of 5e37 overflows in its sum).  Checked at both ends of what the device may keep: 1 step (the fp16 range
    check of the family's network inputs) and 6 (the overflow itself)."""
    for n in (1, 6):
        d = EC.problem(case, drift=0.0)
        o64, o32 = (EC.split_drift(EC.oracle(d, t, n)) for t in (EC.torch.float64, EC.torch.float32))
        _check(case, d, o64, o32)
        # ... and in fp64 the drift changes nothing but its own dimension -- and the gradient of the policy's first-layer
        # weights ON that dimension (zero weights, but dL/dW0[:, k] = sum of dL/dh x_k); every other tensor of the
        # gradient is judged by itself on the GPU (slice_errors)
        o64d = EC.split_drift(EC.oracle(EC.problem(case), EC.torch.float64, n))
        assert np.all(np.isfinite(o64d['grad']))
        D, hid = case['cfg']['D'], case['cfg']['pol_hid'][0]
        col = np.arange(hid) * D + EC.DRIFT_DIM
        o64d['grad'] = o64d['grad'].copy()
        o64d['grad'][col] = o64['grad'][col]
        e = EC.global_errors(o64d, o64)
        assert max(e.values()) < 1e-9, e
    if not case['cfg']['mm']:
        x = EC.oracle(EC.problem(case), EC.torch.float32, n_steps=8)['states'][..., EC.DRIFT_DIM]
        assert np.all(np.isfinite(x[:7])) and not np.any(np.isfinite(x[7]))
