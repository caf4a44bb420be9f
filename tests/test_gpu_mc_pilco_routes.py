"""GPU (-m gpu): which calls an mc_pilco iteration makes on each of its three paths -- pipelined (forward, then one
backward call that ends in clip + Adam on the device), separate calls (forward, horizon read, loss, backward, clip +
Adam) and autograd (rollout()'s node, torch's optimiser) -- and how a failed rollout walks them.  Engine.forward,
Engine.backward (with or without adam=), Engine.valid_steps, Engine.weighted_sum, engine.clip_adam and the optimiser's
step are wrapped by counting shims; each form runs three iterations of a 32-unit fixture with H = 12, 40 rows.

The expected call sequences, optimiser-step counts and resampling counts were recorded by running THIS file against the
commit before mc_pilco was split into a driver and three iteration functions (it passes there unchanged): they pin the
routing, not the new code's own behaviour.  For the pipelined form they are also derivable: one forward, one backward
with adam=, none of the rest per iteration."""
import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_IT = 3

FWD, BWD, BWD_ADAM, STEPS, WSUM, CLIP_ADAM, OPT_STEP = 'forward', 'backward', 'backward+adam', 'valid_steps', \
    'weighted_sum', 'clip_adam', 'opt.step'
PIPELINED = [FWD, BWD_ADAM]
SEPARATE = [FWD, STEPS, WSUM, BWD, CLIP_ADAM]
SEPARATE_RETRIED = [FWD, STEPS, FWD, STEPS, WSUM, BWD, CLIP_ADAM]       # the forward sweep again, on the safe arithmetic
AUTOGRAD = [FWD, STEPS, BWD, OPT_STEP]


def _shims(monkeypatch, opt, pol):
    """the call log of one mc_pilco run, and the number of policy.resample() calls"""
    from prob_mbrl_amd import engine as E
    log, n_resample = [], [0]

    def wrap(owner, attr, name):
        real = getattr(owner, attr)

        def shim(*a, **kw):
            log.append((name(kw) if callable(name) else name))
            return real(*a, **kw)
        monkeypatch.setattr(owner, attr, shim)

    wrap(E.Engine, 'forward', FWD)
    wrap(E.Engine, 'backward', lambda kw: BWD_ADAM if kw.get('adam') is not None else BWD)
    wrap(E.Engine, 'valid_steps', STEPS)
    wrap(E.Engine, 'weighted_sum', WSUM)
    wrap(E, 'clip_adam', CLIP_ADAM)
    wrap(opt, 'step', OPT_STEP)
    real_resample = pol.resample

    def resample(*a, **kw):
        n_resample[0] += 1
        return real_resample(*a, **kw)
    monkeypatch.setattr(pol, 'resample', resample)
    return log, n_resample


def _run(monkeypatch, capsys, d, name, frozen=False, **kw):
    import prob_mbrl_amd as pm
    torch.manual_seed(11)
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    opt = torch.optim.Adam(pol.parameters(), 1e-4)
    log, n_resample = _shims(monkeypatch, opt, pol)
    x0 = torch.tensor(d['x0'], device=DEV)
    H = int(d['H'])
    assert H <= 12
    if frozen:
        kw['frozen_noise'] = dict(z_mm=torch.zeros(H + x0.shape[0], 4), z_rr=torch.zeros(H + x0.shape[0], 1))
    before = pm.algorithms.policy_update_counter[pol]
    pm.algorithms.mc_pilco(x0, dyn, pol, H, opt, None, N_IT, **kw)
    monkeypatch.undo()
    st = opt.state.get(next(iter(pol.parameters())), {})
    res = dict(log=log, opt_steps=pm.algorithms.policy_update_counter[pol] - before,
               adam_step=int(st['step']) if 'step' in st else 0, resamples=n_resample[0], out=capsys.readouterr().out)
    print({k: v for k, v in res.items()})
    return res


def _flat(iterations):
    return [c for it in iterations for c in it]


def test_defaults_take_the_pipelined_path(monkeypatch, capsys):
    r = _run(monkeypatch, capsys, common.load('nomm_d4'), 'nomm_d4')
    assert r['log'] == _flat([PIPELINED] * N_IT)
    assert r['opt_steps'] == N_IT and r['adam_step'] == N_IT and r['resamples'] == 2
    assert 'RuntimeError' not in r['out']


def test_an_on_rollout_hook_takes_the_separate_calls(monkeypatch, capsys):
    seen = []
    r = _run(monkeypatch, capsys, common.load('nomm_d4'), 'nomm_d4',
             on_rollout=lambda i, s, a, rw, disc: seen.append((i, len(s), len(a), len(rw))))
    assert r['log'] == _flat([SEPARATE] * N_IT)
    assert seen == [(i, 13, 12, 12) for i in range(N_IT)]
    assert r['opt_steps'] == N_IT and r['adam_step'] == N_IT and r['resamples'] == 2


def test_cvar_and_regulariser_take_the_autograd_path(monkeypatch, capsys):
    r = _run(monkeypatch, capsys, common.load('nomm_d4'), 'nomm_d4', cvar_eps=0.3, reg_weight=1e-3)
    assert r['log'] == _flat([AUTOGRAD] * N_IT)
    assert r['opt_steps'] == N_IT and r['adam_step'] == N_IT and r['resamples'] == 2


def test_scaled_parameter_copies_take_the_autograd_path(monkeypatch, capsys):
    """per-unit dropout rates: the kernels run on scaled copies of the parameters, which the device-side Adam step must
    not update"""
    r = _run(monkeypatch, capsys, common.load('unit_rates_d4'), 'unit_rates_d4')
    assert r['log'] == _flat([AUTOGRAD] * N_IT)
    assert r['opt_steps'] == N_IT and r['adam_step'] == N_IT and r['resamples'] == 2


def _out_of_fp16_range():
    """tests/test_gpu_api.py::test_fp16_range_failure_is_retried_on_bf16_pieces: the same policy in exact arithmetic,
    its first hidden layer 2^20 times larger"""
    from prob_mbrl_amd import engine as E
    assert E.get_precision() == 'split_f16'
    d = dict(common.load('nomm_d4'))
    d['pol_W0'] = d['pol_W0'] * np.float32(2.0**20)
    d['pol_b0'] = d['pol_b0'] * np.float32(2.0**20)
    d['pol_W1'] = d['pol_W1'] * np.float32(2.0**-20)
    return d


def test_fp16_range_failure_switches_arithmetic_when_the_pipelined_iteration_settles(monkeypatch, capsys):
    """the device skipped the step of iteration 0 on its own; the host learns of it one iteration late, switches the
    arithmetic and neither reports a failed rollout nor draws new random numbers for it"""
    r = _run(monkeypatch, capsys, _out_of_fp16_range(), 'nomm_d4', frozen=True)
    assert r['log'] == _flat([PIPELINED] * N_IT)
    assert r['out'].count('continuing with split') == 1 and '(iteration 0)' in r['out']
    assert 'RuntimeError' not in r['out']
    # (iteration 0 is settled before iteration 1 is built: only its own step is lost)
    assert r['opt_steps'] == N_IT - 1 and r['adam_step'] == N_IT - 1


def test_fp16_range_failure_is_retried_inside_the_iteration_on_the_separate_calls(monkeypatch, capsys):
    r = _run(monkeypatch, capsys, _out_of_fp16_range(), 'nomm_d4', frozen=True, on_rollout=lambda *a: None)
    assert r['log'] == _flat([SEPARATE_RETRIED] + [SEPARATE] * (N_IT - 1))
    assert 'RuntimeError' not in r['out']
    assert r['opt_steps'] == N_IT and r['adam_step'] == N_IT


def test_failed_rollouts_are_reported_resampled_and_skipped(monkeypatch, capsys):
    """twenty moment-matching groups of two rows: a rank-one covariance in four dimensions, the Cholesky factorisation
    fails in the first step of every iteration.  The first failure may be the fp16 range (arithmetic switched, no
    report); every later one is reported and followed by new random numbers; no optimiser step is taken."""
    r = _run(monkeypatch, capsys, common.load('mmg_d4'), 'mmg_d4', mm_states=True, mm_rewards=True, mm_groups=20)
    assert r['log'] == _flat([PIPELINED] * N_IT)
    assert r['opt_steps'] == 0 and r['adam_step'] == 0
    assert r['out'].count('continuing with') == 1
    assert r['out'].count('RuntimeError: rollout failed at step') == N_IT - 1
    # the call's first draw, one at the top of every iteration (no optimiser step was counted), one per reported failure
    assert r['resamples'] == 1 + N_IT + (N_IT - 1)
