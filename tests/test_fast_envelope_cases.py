"""The envelope cases of the latency-optimised family (tests/fast_envelope_cases.py): no kernel takes part here.

Conditioning, as tests/test_reg_envelope_cases.py: for every case the oracle (oracle/ref_torch.py: iteration) runs in
fp32 and in fp64, and the gap between the two must be at most ONE QUARTER of the bar tests/test_gpu_fast_envelope.py
applies to the same quantity, on the whole quantities and on every slice.  A condition on the inputs, not a measurement:
a case that misses it is re-drawn (another seed, a shorter horizon), not exempted.  The same holds for the
second condition: no unmasked hidden unit of either network has a pre-activation within fp32 rounding of zero
(RELU_MARGIN), where the side of its ReLU, and 1e-3 of the gradient with it, would be decided by the order of additions.

Coverage: the hand-written expectations of the table together name every generic instance of the family
(csrc/pmbrl_instances.h: PM_FAST_CASES, PM_SPLIT_CASES) in every variant it is compiled in."""
import numpy as np
import pytest

from tests import fast_envelope_cases as EC


def _gaps(case, n_steps=None, drift=None):
    d = EC.problem(case) if drift is None else EC.problem(case, drift=drift)
    o64 = EC.oracle(d, EC.torch.float64, n_steps)
    o32 = EC.oracle(d, EC.torch.float32, n_steps)
    return d, o64, o32


def _check(case, d, o64, o32, whole=None):
    """whole: o64 with every state dimension (an overflow case's is judged without the drifting one)"""
    e = EC.global_errors(o32, o64)
    sl = EC.slice_errors(d, o32, o64)
    over = {k: v[0] for k, v in sl.items() if v[0] > 0.25 * v[1]}
    print('%s: fp32 vs fp64 oracle: states %.2e actions %.2e rewards %.2e loss %.2e grad %.2e | worst slices: %s %.2e, %s %.2e, '
          '%s %.2e | slices beyond a quarter of their bar: %s' %
          ((case['id'], e['states'], e['actions'], e['rewards'], e['loss'], e['grad']) + EC.worst(sl, 'grad.') +
           EC.worst(sl, 'states.dim') + EC.worst(sl, 'states.step') + (over or 'none',)))
    for k, bar in EC.BARS.items():
        assert np.isfinite(e[k]) and e[k] <= 0.25 * bar, (case['id'], k, e[k])
    assert not over, over
    # ... and no hidden unit's ReLU is decided by rounding (tests/fast_envelope_cases.py: RELU_MARGIN)
    margin, where = EC.relu_margin(d, whole or o64)
    print('%s: smallest unmasked pre-activation: %.2e of the rms of its layer (%s)' % (case['id'], margin, where))
    assert margin >= EC.RELU_MARGIN, (case['id'], margin, where)


@pytest.mark.parametrize('case', EC.CASES, ids=EC.ids(EC.CASES))
def test_case_is_well_conditioned(case):
    _check(case, *_gaps(case))


@pytest.mark.parametrize('case', EC.SAT_CASES, ids=EC.ids(EC.SAT_CASES))
def test_saturation_case_covers_the_range_and_is_well_conditioned(case):
    """The conditions of tests/test_reg_envelope_cases.py on the fp64 ORACLE's head values.  Saturating policy: at least
    10 % of the (step, row, action) entries with |u| > 44, 10 % with 15 < |u| <= 44, 10 % where tanh is far from flat.
    Log-std heads: at least 10 % of the entries of either head beyond each end of the clamp (|ls - max_log_std| > 80)."""
    d, o64, o32 = _gaps(case)
    shares = EC.saturation_shares(case, o64)
    print(case['id'], {k: round(v, 3) for k, v in shares.items()})
    assert shares and all(v >= 0.10 for v in shares.values()), shares
    _check(case, d, o64, o32)


@pytest.mark.parametrize('case', EC.OVERFLOW_CASES, ids=EC.ids(EC.OVERFLOW_CASES))
def test_overflow_case_is_well_conditioned_on_the_steps_it_keeps(case):
    """The drifting dimension overflows fp32 while step 6 computes x_7 (7 x 5e37 > 3.4e38); the family keeps
    OVERFLOW_STEPS = 6 steps in either arithmetic (tests/fast_envelope_cases.py says why).  The dimension is decoupled
    from everything the bars are applied to, so the conditioning of the kept steps is that of the same problem without
    the drift -- which the oracle can run in fp32 under moment matching too."""
    n = EC.OVERFLOW_STEPS
    d, o64, o32 = _gaps(case, n, drift=0.0)
    whole = o64
    o64, o32 = EC.split_drift(o64), EC.split_drift(o32)
    _check(case, d, o64, o32, whole)
    # in fp64 the drift changes nothing but its own dimension and the gradient of the policy's first-layer weights ON
    # that dimension (zero weights, but dL/dW0[:, k] = sum of dL/dh x_k); every other tensor is judged by itself on the GPU
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


def test_no_case_is_the_register_resident_family_s():
    """pm_reg_shape_ok: three-layer networks with ONE hidden width of 13 tiles in both"""
    for c in EC.ALL_CASES:
        hid = c['cfg']['pol_hid'], c['cfg']['dyn_hid']
        tiles = {-(-x // 16) for h in hid for x in h}
        assert not (len(hid[0]) == 2 and len(hid[1]) == 2 and tiles == {13}), c['id']


def test_the_table_covers_the_axes():
    inside = [c for c in EC.CASES if c['inside']]
    plain = [c['cfg'] for c in inside if not c['cfg']['mm']]
    mm = [c for c in inside if c['cfg']['mm']]
    equal = [c for c in plain if c['pol_hid'] == c['dyn_hid'] and len(set(c['pol_hid'])) == 1 and len(c['pol_hid']) == 2]
    at16 = {c['cfg']['pol_hid'][0] for c in inside if c['cfg'] in equal and c['hint'] == 0}
    assert {16, 64, 80, 128, 144, 192, 224, 256} <= at16                       # 1, 4 | 5, 8 | 9, 12 | 14, 16 tiles
    assert {1, 17, 65, 100, 113, 129, 177, 209, 241, 256} <= at16              # ragged last tiles
    assert {c['hint'] for c in inside if c['cfg'] in equal} >= {0, 32, 64}
    assert all(h in [c['pol_hid'] for c in plain] for h in ([48, 200], [256, 16], [16, 256], [112, 144]))
    assert any(c['pol_hid'] == [64, 64] and c['dyn_hid'] == [176, 80] for c in plain)
    depths = {(len(c['pol_hid']), len(c['dyn_hid'])) for c in plain}
    assert {(1, 1), (2, 2), (3, 3), (4, 4), (7, 7), (1, 3), (3, 1)} <= depths
    assert {(1, 1), (8, 8), (8, 1), (1, 8), (7, 2)} <= {(c['D'], c['U']) for c in plain}
    out = [c['cfg'] for c in EC.OUTSIDE]
    assert {(9, 1), (4, 9)} <= {(c['D'], c['U']) for c in out} and any(c['pol_hid'] == [257, 257] for c in out)
    rows = {(c['cfg']['P'] * c['cfg']['S'], c['hint']) for c in inside if not c['cfg']['mm']}
    assert {(1, 0), (15, 0), (16, 0), (17, 0), (33, 0), (65, 0), (33, 32), (65, 32), (33, 64), (65, 64)} <= rows
    assert {1, 2, 3, 12} <= {c['H'] for c in plain}
    # moment matching: widths among 64, 112, 144, 256 except where a stage pair needs 13 or 14 tiles (208, 224) and in
    # the corners; group sizes and forms
    lay = {(c['cfg']['D'], c['cfg']['S'], c['expect']['f32']['mm_parts'], c['expect']['f32']['mm_mode'],
            c['expect']['f32']['mm_grid']) for c in mm}
    assert {(4, 5, 1, 1, 0), (4, 7, 1, 1, 0), (4, 16, 1, 1, 0), (4, 8, 1, 1, 0), (5, 16, 1, 1, 0), (6, 16, 1, 1, 0),
            (2, 16, 1, 1, 0), (8, 16, 1, 1, 0)} <= lay
    assert {(4, 17, 2, 1, 0), (4, 25, 2, 1, 0), (4, 50, 4, 1, 0), (4, 100, 7, 1, 0), (4, 128, 8, 1, 0),
            (4, 129, 1, 3, 1)} <= lay
    assert {(4, 25, 1, 1, 0), (4, 50, 1, 1, 0)} <= lay                         # PMBRL_MM_PARTS=1
    assert {(4, 160, 1, 3, 1), (6, 160, 1, 3, 1), (4, 160, 1, 3, 0), (6, 160, 1, 3, 0), (3, 160, 1, 2, 0)} <= lay
    norr = [c for c in mm if c['cfg'].get('mm_rewards') is False]
    assert {c['expect']['f32']['mm_parts'] > 1 for c in norr} == {True, False}
    # every split or barrier case keeps its workgroups far below the CU count (they spin on partners)
    for c in EC.ALL_CASES:
        if c['inside'] and (c['expect']['f32']['mm_parts'] > 1 or c['expect']['f32']['mm_grid']):
            assert c['expect']['f32']['n_wg'] <= 16, c['id']
    # what the GPU test looks up by name
    for cid in EC.RANGE_CASES + EC.TWICE_CASES:
        assert EC.by_id(cid)['inside']
    assert {EC.by_id(cid)['expect']['f32']['row_tiles'] for cid in EC.RANGE_CASES} == {1, 2, 4}
    assert [EC.form(EC.by_id(cid)) for cid in EC.TWICE_CASES] == ['mm', 'barrier']
    assert EC.by_id(EC.TWICE_CASES[0])['expect']['f32']['mm_parts'] > 1


def test_the_expectations_name_every_generic_instance():
    """Every (arithmetic, rt, CA, CB) of PM_FAST_CASES / PM_SPLIT_CASES is what SOME case's expectation reports: by a
    case without moment matching (the LEAN and EXT instances), by a case with moment matching inside the sweeps (MM)
    and, for rt = 1, by a device-wide-barrier case (MMG).  The split rows in both split arithmetics."""
    seen = {}
    for c in EC.INSIDE:
        for prec in c['precision']:
            e = c['expect'][prec]
            key = (e['precision'], e['row_tiles']) + tuple(e['stages'])
            seen.setdefault(key, set()).add(EC.form(c))
    missing = []
    for prec, rows in EC.ROWS_OF.items():
        for row in rows:
            forms = seen.get((prec,) + row, set())
            need = {'plain', 'mm'} | ({'barrier'} if row[0] == 1 else set())
            if not need <= forms:
                missing.append((prec, row, sorted(need - forms)))
    assert not missing, missing
    # ... and no expectation names an instance that does not exist
    for key in seen:
        assert key[1:] in EC.ROWS_OF[key[0]], key


def test_an_expectation_holds_every_field_the_gpu_test_compares():
    fields = {'fast', 'row_tiles', 'rows_per_wg', 'n_wg', 'stages', 'precision', 'mm_mode', 'mm_parts', 'mm_grid'}
    for c in EC.INSIDE + EC.OVERFLOW_CASES:
        for prec in c['precision']:
            assert set(c['expect'][prec]) == fields
