"""The envelope cases of the general family (tests/general_envelope_cases.py): no kernel takes part here.

Conditioning, as tests/test_fast_envelope_cases.py: for every case the oracle (oracle/ref_torch.py: iteration) runs in
fp32 and in fp64, and the gap between the two must be at most ONE QUARTER of the bar tests/test_gpu_general_envelope.py
applies to the same quantity, on the whole quantities and on every slice -- a condition on the inputs, not a measurement:
a case that misses it is re-drawn, not exempted.  Likewise no unmasked ReLU unit of either network has a pre-activation
within fp32 rounding of zero.  This table's margin is NOT literally the fast table's RELU_MARGIN: that figure is
2^-24 sqrt(K) at K = 256, and _margin_bar applies the same rule at each case's widest layer (1e-6 up to 256 units, 2.2e-6
at 1248).  Not asked: the cases with an activation other than ReLU in some layer, and the two 16 35x-row cases (why:
_check).

Coverage: the hand-written expectations together name every instance of the three general-family lists of
csrc/pmbrl_instances.h.  LDS: the table's lds_bytes are those of pm_lds_map (tests/general_lds_check.cpp, compiled by
the host compiler alone), and the row tiles written down are the ones whose map fits where the next size does not."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import general_envelope_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'


def _gaps(case, n_steps=None, drift=None):
    d = EC.problem(case) if drift is None else EC.problem(case, drift=drift)
    o64 = EC.oracle(d, torch.float64, n_steps)
    o32 = EC.oracle(d, torch.float32, n_steps)
    return d, o64, o32


def _margin_bar(case):
    """RELU_MARGIN is 2^-24 sqrt(K) at K = 256, the latency-optimised family's widest layer: the same rule at this
    case's widest"""
    K = max([256] + case['cfg']['pol_hid'] + case['cfg']['dyn_hid'])
    return EC.RELU_MARGIN * (K / 256.0) ** 0.5


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
    if case['id'] in EC.NO_ADJOINT_ORACLE:
        return      # (an activation other than ReLU in one of the networks)
    if d['x0'].shape[0] > 1000:
        # the two 16 35x-row cases: 16 352 rows x 2 steps x 32 units are a million unit activations per layer, one of
        # which lies within 1e-6 of zero more often than not -- and carries a millionth of the gradient, two decades
        # below the bar, whichever side its ReLU takes
        return
    margin, where = EC.relu_margin_angles(d, whole or o64)
    bar = _margin_bar(case)
    print('%s: smallest unmasked pre-activation: %.2e of the rms of its layer (%s; asked: %.1e)' % (case['id'], margin, where, bar))
    assert margin >= bar, (case['id'], margin, where)


@pytest.mark.parametrize('case', EC.PLAIN_INSIDE, ids=EC.ids(EC.PLAIN_INSIDE))
def test_case_is_well_conditioned(case):
    _check(case, *_gaps(case))


@pytest.mark.parametrize('case', EC.SAT_CASES, ids=EC.ids(EC.SAT_CASES))
def test_saturation_case_covers_the_range_and_is_well_conditioned(case):
    """The conditions of tests/test_reg_envelope_cases.py on the fp64 ORACLE's head values: at least 10 % of the entries
    in each class saturation_shares names."""
    d, o64, o32 = _gaps(case)
    shares = EC.saturation_shares(case, o64)
    print(case['id'], {k: round(v, 3) for k, v in shares.items()})
    assert shares and all(v >= 0.10 for v in shares.values()), shares
    _check(case, d, o64, o32)


@pytest.mark.parametrize('case', EC.OVERFLOW_CASES, ids=EC.ids(EC.OVERFLOW_CASES))
def test_overflow_case_is_well_conditioned_on_the_steps_it_keeps(case):
    """As tests/test_fast_envelope_cases.py: the drifting dimension is decoupled from everything the bars are applied to,
    so the conditioning of the kept steps (6 in exact fp32, 1 on split operands) is that of the problem without the drift;
    in fp32 the dimension is finite through x_6 and not at x_7."""
    for n in sorted(set(EC.OVERFLOW_STEPS.values())):
        d, o64, o32 = _gaps(case, n, drift=0.0)
        _check(case, d, EC.split_drift(o64), EC.split_drift(o32), o64)
    if not case['cfg']['mm']:
        x = EC.oracle(EC.problem(case), torch.float32, n_steps=8)['states'][..., EC.DRIFT_DIM]
        assert np.all(np.isfinite(x[:7])) and not np.any(np.isfinite(x[7]))


def test_ids_are_unique_and_half_the_seeds_are_not_zero():
    assert len({c['id'] for c in EC.ALL_CASES}) == len(EC.ALL_CASES)
    assert 2 * sum(c['seed'] != 0 for c in EC.ALL_CASES) >= len(EC.ALL_CASES)
    for cid in EC.TWICE_CASES + (EC.RANGE_CASE,):
        assert EC.by_id(cid)['inside']
    assert EC.by_id(EC.RANGE_CASE)['cfg']['H'] == 5


def test_no_case_is_another_family_s():
    """plan_layout: what keeps a shape off the latency-optimised family (pm_fast_net_ok and the flags), unless the case
    asks for this family; the register-resident family serves a subset of the latency-optimised one's shapes"""
    for c in EC.ALL_CASES:
        cfg, x = c['cfg'], c['extra']
        D, U = cfg['D'], cfg['U']
        takes = lambda hid, n_in, n_out: len(hid) >= 1 and n_in <= 16 and n_out <= 16 and max(hid) <= 256      # noqa: E731
        fast = takes(cfg['pol_hid'], D, 2 * U) and takes(cfg['dyn_hid'], D + U, 2 * D) and not any(
            x.get(k) for k in ('pol_ang', 'dyn_ang', 'pol_step_masks', 'dyn_step_masks', 'infer_ns', 'pol_act', 'dyn_act'))
        assert c['generic'] or not fast, c['id']


def test_the_expectations_name_every_instance():
    seen = {e['_inst'] for c in EC.INSIDE + EC.OVERFLOW_CASES for e in c['expect'].values()}
    assert seen == set(EC.INSTANCES), (sorted(set(EC.INSTANCES) - seen), sorted(seen - set(EC.INSTANCES)))
    assert len(set(EC.INSTANCES)) == len(EC.INSTANCES) == 3 + 6 + 6
    # ... the lists are those of csrc/pmbrl_instances.h: three rows by row tiles; those, and the three 64-row in-place
    # forms; two sets of three by piece planes
    src = open(os.path.join(ROOT, 'prob_mbrl_amd', 'csrc', 'pmbrl_instances.h')).read()
    flat = re.sub(r'\\\n', ' ', src)
    assert re.search(r'#define PM_GENERAL_ROWS\(VAR\) PM_INST\(1, 0, 0, VAR,[ 0,]*\) PM_INST\(2, 0, 0, VAR,[ 0,]*\) '
                     r'PM_INST\(4, 0, 0, VAR,[ 0,]*\)', flat)
    assert re.search(r'#define PM_GENERAL_F32_INSTANCES PM_GENERAL_ROWS\(0\)\n', flat)
    assert re.search(r'#define PM_GENERAL_SPLIT_INSTANCES\s+PM_GENERAL_ROWS\(0\) PM_INST\(4, 0, 0, 1,[ 0,]*\) '
                     r'PM_INST\(4, 0, 0, 2,[ 0,]*\) PM_INST\(4, 0, 0, 3,[ 0,]*\)\n', flat)
    assert re.search(r'#define PM_GENERAL_ACT_INSTANCES PM_GENERAL_ROWS\(0\) PM_GENERAL_ROWS\(2\)\n', flat)


def test_an_expectation_holds_every_field_the_gpu_test_compares():
    fields = {'fast', 'reg', 'row_tiles', 'rows_per_wg', 'n_wg', 'LD', 'lds_bytes', 'inplace', 'mm_mode', 'precision', '_inst'}
    for c in EC.INSIDE + EC.OVERFLOW_CASES:
        assert set(c['expect']) == set(c['precision']), c['id']
        for prec in c['precision']:
            assert set(c['expect'][prec]) == fields


def test_the_table_covers_the_axes():
    inside = [c for c in EC.CASES if c['inside']]
    plain = [c for c in inside if not c['cfg']['mm']]
    equal = {c['cfg']['pol_hid'][0] for c in plain if c['cfg']['pol_hid'] == c['cfg']['dyn_hid'] and
             len(set(c['cfg']['pol_hid'])) == 1 and c['hint'] == 0}
    assert {257, 258, 384, 385, 400, 416, 432, 512, 513, 1248} <= equal
    lds16 = {(p, c['expect'][p]['LD']) for c in plain for p in c['precision'] if c['expect'][p]['row_tiles'] == 1}
    assert {('f32', 424), ('f32', 440), ('split_f16', 400), ('split_f16', 432)} <= lds16      # the aliasing boundary
    depths = {(len(c['cfg']['pol_hid']), len(c['cfg']['dyn_hid'])) for c in plain}
    assert {(0, 3), (2, 0), (0, 0), (1, 1), (3, 3), (7, 7), (1, 3), (3, 1)} <= depths
    assert {1, 16, 17, 24, 25, 32} <= {c['cfg']['D'] for c in plain} and {1, 8, 9, 16} <= {c['cfg']['U'] for c in plain}
    widths = {c['cfg']['D'] + c['cfg']['U'] + len(c['extra'].get('dyn_ang', ())) for c in plain}
    assert {48, 49, 56} <= widths
    rows = {(c['cfg']['P'] * c['cfg']['S'], c['hint']) for c in plain}
    assert {(r, h) for r in (1, 15, 16, 17, 77) for h in (0, 32, 64)} | {(16352, 0), (16353, 0)} <= rows
    assert {1, 2, 3, 5, 12} <= {c['cfg']['H'] for c in plain}
    assert {c['expect']['split_f16']['inplace'] for c in EC.IP_CASES} == {0, 1, 2}
    mm = {(c['cfg']['D'], c['cfg']['S'], c['expect']['f32']['mm_mode']) for c in inside if c['cfg']['mm']}
    assert {(1, 2, 1), (4, 16, 1), (4, 17, 1), (4, 32, 1), (6, 33, 1), (4, 64, 1), (21, 32, 1), (22, 32, 2), (7, 200, 2),
            (16, 80, 2), (32, 283, 2), (32, 284, 2), (4, 65, 2), (4, 200, 2), (6, 65, 2), (6, 200, 2)} <= mm
    assert {(-2, 'D <= 32'), (-2, 'U <= 16'), (-2, 'n_layers'), (-3, 'LDS')} == {c['refused'] for c in EC.REFUSED}


def _two_buffer(c, prec, rt):
    e = c['expect'][prec]
    return EC._lds(16 * rt, e['LD'], c['cfg']['D'], c['cfg']['U'], rt)


def test_the_row_tiles_written_down_are_the_ones_that_fit():
    """Every plan fits 160 KiB; a plan that took fewer row tiles than its hint asks for did so because the two-buffer map
    of twice as many does not fit; an in-place plan likewise; a moment-matching case sits in the first of 16 / 32 / 64 rows
    that holds its group and fits with the scratch, or per step if none does."""
    for c in EC.INSIDE + EC.OVERFLOW_CASES:
        D, U, M = c['cfg']['D'], c['cfg']['U'], c['cfg']['S']
        for prec in c['precision']:
            e = c['expect'][prec]
            rt = e['row_tiles']
            assert e['lds_bytes'] <= EC.LDS_CAP, (c['id'], prec, e['lds_bytes'])
            if c['cfg']['mm']:
                first = next((t for t in (1, 2, 4) if M <= 16 * t and
                              EC._lds(16 * t, e['LD'], D, U, t, D) <= EC.LDS_CAP), None)
                assert (e['mm_mode'], rt) == ((1, first) if first else (2, 1)), (c['id'], prec, first)
                continue
            asked = 4 if c['hint'] >= 64 else 2 if c['hint'] >= 32 else rt
            if e['inplace']:
                assert rt == 4 and _two_buffer(c, prec, 4) > EC.LDS_CAP
            else:
                assert rt <= asked and _two_buffer(c, prec, rt) <= EC.LDS_CAP
                assert rt == asked or _two_buffer(c, prec, 2 * rt) > EC.LDS_CAP, (c['id'], prec)
    # ... and the refused width is the first that does not fit 16 rows
    assert EC._lds(16, EC._ld(78, 'f32'), 4, 1, 1) <= EC.LDS_CAP < EC._lds(16, EC._ld(79, 'f32'), 4, 1, 1)
    assert EC._lds(16, EC._ld(78, 'split_f16'), 4, 1, 1) <= EC.LDS_CAP < EC._lds(16, EC._ld(79, 'split_f16'), 4, 1, 1)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_lds_figures_are_the_map_s(tmp_path):
    plans = set()
    for c in EC.INSIDE + EC.OVERFLOW_CASES:
        for prec in c['precision']:
            e = c['expect'][prec]
            plans.add((16 * e['row_tiles'], e['LD'], c['cfg']['D'], c['cfg']['U'], e['row_tiles'],
                       c['cfg']['D'] if e['mm_mode'] == 1 else 0, int(e['inplace'] != 0), e['lds_bytes']))
    exe = str(tmp_path / 'general_lds_check')
    subprocess.check_call([HIPCC, '-x', 'c++', '-std=c++17', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'),
                           '-I' + os.path.join(ROOT, 'prob_mbrl_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'general_lds_check.cpp'), '-o', exe])
    text = ''.join('%d %d %d %d %d %d %d %d\n' % p for p in sorted(plans))
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert ('%d plans, 0 disagree' % len(plans)) in r.stdout, r.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_per_step_forms_are_the_ones_written_down(tmp_path):
    """MM_PER_STEP_WIDE names exactly the cases that run per step in some arithmetic, and pm_mmw_ok (csrc/pmbrl_mm_wide.h,
    host side only: tests/general_mmw_check.cpp) gives what is written there for each (M, D, infer_ns) -- both sides of its
    LDS bound at D = 32, both sides of D = 6 | 7, and infer_ns at D = 7."""
    per_step = {c['id'] for c in EC.PLAIN_INSIDE if any(e['mm_mode'] == 2 for e in c['expect'].values())}
    assert per_step == set(EC.MM_PER_STEP_WIDE), per_step ^ set(EC.MM_PER_STEP_WIDE)
    lines = []
    for cid, wide in sorted(EC.MM_PER_STEP_WIDE.items()):
        c = EC.by_id(cid)
        lines.append('%d %d %d %d\n' % (c['cfg']['S'], c['cfg']['D'], 4 if c['extra'].get('infer_ns') else 0, int(wide)))
    forms = {(c, w) for c, w in ((EC.by_id(k)['cfg']['D'], v) for k, v in EC.MM_PER_STEP_WIDE.items())}
    assert {(6, False), (7, True), (32, True), (32, False), (4, False), (16, True)} <= forms
    assert [EC.MM_PER_STEP_WIDE[c] for c in EC.TWICE_CASES[-2:]] == [False, True]
    exe = str(tmp_path / 'general_mmw_check')
    subprocess.check_call([HIPCC, '-x', 'hip', '--offload-host-only', '-std=c++17', '-Wall', '-Werror', '-Wno-unused-function', '-Wno-unused-variable',
                           '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'prob_mbrl_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'general_mmw_check.cpp'), '-o', exe])
    r = subprocess.run([exe], input=''.join(lines), stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert ('%d groups, 0 disagree' % len(lines)) in r.stdout, r.stdout
