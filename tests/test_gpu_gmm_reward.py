"""GPU (-m gpu): a learned reward head on a Gaussian-mixture dynamics model (reward_func=None with
GaussianMixtureDensity(D + 1, n), PMBRL_REWARD_LEARNED with dyn_components > 1) through the general kernel family, the
stand-alone calls, utils.rollout, mc_pilco, train_regressor and the example -- against the reference's fixtures
(tests/golden/gmm_reward, tools/make_golden_gmm_reward.py) and the fp64 restatement (tests/gmm_reward_ref.py).

The bars are those of the mixture cases of tests/test_gpu_kernels.py (TOL_TRAJ, TOL_GRAD: what
tests/test_gpu_learned_reward.py holds too), tests/grad_bars.py for parameter gradients and, for the fit, those of
tests/test_gpu_kernels.py::test_bnn_training_matches_reference.  Every plan-creating test fails on a build that
refuses the combination (pmbrl_plan_create: -2)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import common, grad_bars
from tests import gmm_reward_ref as GR
from tests.common import flat_grad, loss_of
from tests.test_gpu_kernels import TOL_GRAD, TOL_TRAJ

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def engine(d, precision='f32', **kw):
    from prob_mbrl_amd import engine as E
    from prob_mbrl_amd.problem import engine_from_problem
    eng, args, rows = engine_from_problem(d, DEV, precision=precision, reward_spec=E.LEARNED_REWARD, **kw)
    assert eng.learned and eng.n_comp == int(d['dyn_gmm_n']) and eng.info['fast'] == 0 and eng.info['reg'] == 0
    assert eng.info['precision'] == precision
    return eng, args, rows


def run(d, precision='f32', Bg=None, **kw):
    """Forward, mc_pilco's loss weights, adjoint: (engine, states, rewards, loss, gradient) as numpy / float."""
    eng, args, (lo, hi) = engine(d, precision, **kw)
    S, A, Rw = eng.forward(**args)
    gw = torch.tensor(common.loss_weights(d, Bg or d['x0'].shape[0])[:, lo:hi].copy(), device=DEV)
    loss = float(eng.weighted_sum(Rw, gw))
    g, _, _ = eng.backward(gw)
    torch.cuda.synchronize()
    assert eng.reg_calls() == (0, 0)
    return eng, S.cpu().numpy(), Rw.cpu().numpy(), loss, g.cpu().numpy().copy()


def hold(what, S, Rw, loss, g, S_ref, R_ref, loss_ref, g_ref):
    """Print every figure, then hold states, rewards and loss to TOL_TRAJ and the gradient to TOL_GRAD."""
    e = (common.rel(S, S_ref), common.rel(np.asarray(Rw).reshape(np.shape(R_ref)), R_ref),
         abs(loss - float(loss_ref)) / abs(float(loss_ref)), common.rel(g, g_ref))
    print('%s: states %.2e, rewards %.2e, loss %.2e, gradient %.2e' % ((what,) + e))
    assert e[0] < TOL_TRAJ and e[1] < TOL_TRAJ and e[2] <= TOL_TRAJ and e[3] < TOL_GRAD, (what, e)


def mm_kw(d):
    if not bool(d['mm_states']):
        return {}
    G = int(d['mm_groups'])
    return dict(mm_states=True, mm_rewards=True, mm_groups=G if G > 0 else None,
                z_mm=torch.tensor(d['z_mm'], device=DEV), z_rr=torch.tensor(d['z_rr'], device=DEV))


@pytest.mark.parametrize('precision', ['f32', 'split_f16'])
@pytest.mark.parametrize('name', GR.ROLLOUTS)
def test_sweeps_match_reference_and_restatement(name, precision):
    """gr_d4: a head of two 16-column tiles, padded hidden widths, a partial row tile; gr_d4_mmg: moment-matched states
    and rewards in two groups; gr_8comp: PMBRL_MAX_COMP components and an angle dimension; gr_step: fresh masks at every
    step."""
    d = GR.load(name)
    eng, S, Rw, loss, g = run(d, precision)
    assert eng.valid_steps() == int(d['H'])
    hold(name + ' / fixture', S, Rw, loss, g, d['ref64_states'], d['ref64_rewards'], d['ref64_loss'], d['ref64_grad'])
    lo, go, So, Ro = GR.reference(name)
    hold(name + ' / restatement', S, Rw, loss, g, So, Ro, lo, go)


@pytest.mark.parametrize('name', ['gr_d4', 'gr_d4_mmg', 'gr_8comp'])
def test_rollout_autograd_matches_reference(name):
    """utils.rollout + loss.backward() on the reference-shaped modules (rollout.Bundle accepts the head)."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    d = GR.load(name)
    dyn, pol = GR.modules(d, DEV)
    x0 = torch.tensor(d['x0'], device=DEV)
    H = int(d['H'])
    RO._ENGINES.clear()
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, resample_state_noise=False, resample_action_noise=False,
                                                precision='f32', **mm_kw(d))
    assert len(states) == H + 1 and rewards[0].shape == (x0.shape[0], 1) and states[0].shape == x0.shape
    loss = loss_of(rewards, d)
    pol.zero_grad()
    loss.backward()
    hold(name, torch.stack(states).detach().cpu().numpy(), torch.stack(rewards).detach().cpu().numpy(), float(loss),
         flat_grad(pol), d['ref64_states'], d['ref64_rewards'], d['ref64_loss'], d['ref64_grad'])
    engs = list(RO._ENGINES.values())
    assert len(engs) == 1 and engs[0].learned and engs[0].n_comp == int(d['dyn_gmm_n'])
    assert engs[0].info['fast'] == 0 and engs[0].reg_calls() == (0, 0) and engs[0].valid_steps() == H
    assert dyn.output_density.z_normal.shape[-1] == x0.shape[1] + 1


def test_both_noise_gradient_conventions():
    """The last draw (the reference's autograd: the fixture's gradient) and, under PMBRL_FLAG_GMM_EXACT_NOISE_GRAD, each
    step's own draw (the restatement in that mode) -- for all D + 1 dimensions."""
    import prob_mbrl_amd as pm
    d = GR.load('gr_d4')
    x0 = torch.tensor(d['x0'], device=DEV)
    H = int(d['H'])
    lo_e, g_e, _ = GR.iteration(d, dyn_update=dict(exact_noise_grad=True))
    assert common.rel(g_e.numpy(), d['ref64_grad']) > 1e-2           # (it IS a different gradient)
    for exact, g_ref in ((False, d['ref64_grad']), (True, g_e.numpy())):
        dyn, pol = GR.modules(d, DEV)
        dyn.output_density.exact_noise_grad = exact
        states, _, rewards = pm.utils.rollout(x0, dyn, pol, H, resample_state_noise=False, resample_action_noise=False,
                                              precision='f32')
        loss = loss_of(rewards, d)
        pol.zero_grad()
        loss.backward()
        hold('gr_d4 exact=%s' % exact, torch.stack(states).detach().cpu().numpy(), torch.stack(rewards).detach().cpu().numpy(),
             float(loss), flat_grad(pol), d['ref64_states'], d['ref64_rewards'], d['ref64_loss'], g_ref)


def test_truncated_horizon_and_mc_pilco_skips():
    """The reward's noise is inf at step 2 of one row: status says 2, the adjoint covers the two steps the sweep
    completed (the restatement truncated there), and mc_pilco -- two steps are too few to optimise on -- skips the
    iteration."""
    import prob_mbrl_amd as pm
    d = dict(GR.load('gr_d4'))
    D = d['x0'].shape[1]
    z = np.array(d['dyn_z'], dtype=np.float32)
    z[2, 3, D] = np.inf
    d['dyn_z'] = z
    eng, S, Rw, loss, g = run(d)
    assert eng.valid_steps() == 2 and int(eng.status[0].item()) == 2
    assert not np.isfinite(Rw[2, 3]) and np.isfinite(S).all()
    lo, go, (So, _, Ro) = GR.iteration(d, dyn_update=dict(z=torch.tensor(z, dtype=torch.float64)), n_steps=2)
    hold('gr_d4 truncated', S[:3], Rw[:2], loss, g, torch.stack(So).detach().numpy(), torch.stack(Ro).detach().numpy(),
         float(lo), go.numpy())
    dyn, pol = GR.modules(d, DEV)
    before = flat_grad_free_params(pol)
    seen = []
    pm.algorithms.mc_pilco(torch.tensor(d['x0'], device=DEV), dyn, pol, int(d['H']), torch.optim.Adam(pol.parameters(), 1e-3),
                           None, 1, maximize=True, on_iteration=lambda i, loss, *a: seen.append(float(loss)))
    assert not seen and np.array_equal(flat_grad_free_params(pol), before)


def flat_grad_free_params(pol):
    lins = [m for m in pol.model._modules.values() if isinstance(m, torch.nn.Linear)]
    return torch.cat([t.detach().reshape(-1) for l in lins for t in (l.weight, l.bias)]).cpu().numpy()


def test_replay_gives_the_eager_bits():
    """Two iterations with every call replayed as a hipGraph (set_replay(2)) and with none (set_replay(0))."""
    from prob_mbrl_amd import rollout as RO
    d = GR.load('gr_d4_mmg')
    dyn, pol = GR.modules(d, DEV)
    x0 = torch.tensor(d['x0'], device=DEV)
    H, kw = int(d['H']), mm_kw(d)
    out = {}
    for mode in (0, 2):
        b = RO.Bundle(dyn, pol, x0.shape[0], H, False, False, True, True, kw['mm_groups'], kw['z_mm'], kw['z_rr'],
                      precision='f32')
        b.engine.set_replay(mode)
        res = []
        for _ in range(2):
            S, A, R = RO.RolloutFunction.apply(b, x0, *b.pol_params)
            loss = loss_of(list(R.unbind(0)), d)
            pol.zero_grad()
            loss.backward()
            res.append((S.detach().cpu().numpy(), R.detach().cpu().numpy(), float(loss), flat_grad(pol)))
        b.engine.set_replay(1)
        out[mode] = res
    for a, b in zip(out[0], out[2]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert np.array_equal(a[3], b[3])
    assert np.isfinite(out[0][0][1]).all()


def _first_step_draws(d):
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)  # noqa: E731
    return (T(d['dyn_z'][0]), T(d['dyn_z'][-1]), T(d['dyn_ucat'][0]))


def test_standalone_call_and_its_parameter_gradient():
    """DynamicsModel((x, u), return_samples=True, separate_outputs=True) returns (states, rewards): the rollout's first
    transition, the restatement's, the same values inside models.param_grad(), and there the gradient of a linear
    functional in the network's own parameters against fp64 autograd over the restatement's step."""
    import prob_mbrl_amd as pm
    from oracle import ref_torch as R
    d = GR.load('gr_d4')
    dyn, pol = GR.modules(d, DEV)
    x0 = torch.tensor(d['x0'], device=DEV)
    B, D = x0.shape
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, int(d['H']), resample_state_noise=False,
                                                resample_action_noise=False, precision='f32')
    u = actions[0].detach()
    kw = dict(return_samples=True, resample=False, resample_noise=False, gmm_draws=_first_step_draws(d))
    x1, r0 = dyn((x0, u), separate_outputs=True, deltas=False, **kw)
    assert x1.shape == x0.shape and r0.shape == (B, 1) and not x1.requires_grad
    assert common.rel(x1.cpu().numpy(), states[1].detach().cpu().numpy()) < 2e-6
    assert common.rel(r0.cpu().numpy(), rewards[0].detach().cpu().numpy()) < 2e-6
    dx, _ = dyn((x0, u), separate_outputs=True, deltas=True, **kw)
    assert common.rel(dx.cpu().numpy(), (x1 - x0).cpu().numpy()) < 1e-5
    cat = dyn(torch.cat([x0, u], -1), separate_outputs=False, deltas=False, **kw)
    assert cat.shape == (B, D + 1) and common.rel(cat.cpu().numpy(), torch.cat([x1, r0], -1).cpu().numpy()) < 2e-6
    # the restatement's one transition in fp64, its parameters as leaves
    x64, _, dyn64, _, _, _, _, _ = R.problem_from_npz(d, torch.float64)
    dyn64['weights'] = [(W.requires_grad_(True), b.requires_grad_(True)) for W, b in dyn64['weights']]
    u64 = torch.tensor(u.cpu().numpy(), dtype=torch.float64)
    s64 = R.gmm_sample(GR._dyn_net((torch.cat([x64, u64], -1) - dyn64['mx']) * dyn64['iSx'], dyn64, 0), dyn64, D + 1, 0)
    n64, r64 = x64 + s64[:, :D], s64[:, D:]
    assert common.rel(x1.cpu().numpy(), n64.detach().numpy()) < TOL_TRAJ
    assert common.rel(r0.cpu().numpy(), r64.detach().numpy()) < TOL_TRAJ
    g = torch.Generator().manual_seed(3)
    ws, wr = torch.randn(B, D, generator=g), torch.randn(B, 1, generator=g)
    lins = [m for m in dyn.model._modules.values() if isinstance(m, torch.nn.Linear)]
    params = [t for lin in lins for t in (lin.weight, lin.bias)]
    for t in params:
        t.grad = None
    with pm.models.param_grad():
        x1g, r0g = dyn((x0, u), separate_outputs=True, deltas=False, **kw)
    assert x1g.requires_grad and r0g.requires_grad
    assert torch.equal(x1g.detach(), x1) and torch.equal(r0g.detach(), r0)
    ((x1g * ws.to(DEV)).sum() + (r0g * wr.to(DEV)).sum()).backward()
    ref = torch.autograd.grad((n64 * ws.double()).sum() + (r64 * wr.double()).sum(), [t for p in dyn64['weights'] for t in p])
    grad_bars.hold('gr_d4 stand-alone samples', grad_bars.errors([t.grad.cpu().numpy() for t in params],
                                                               [t.numpy() for t in ref]))


@pytest.mark.parametrize('name', ['gr_d4', 'gr_d4_mmg'])
def test_stepwise_rollout_with_a_hook_equals_the_fused_rollout(name):
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    d = GR.load(name)
    dyn, pol = GR.modules(d, DEV)
    x0 = torch.tensor(d['x0'], device=DEV)
    H = int(d['H'])
    kw = dict(resample_state_noise=False, resample_action_noise=False, **mm_kw(d))
    seen = []

    def hook(i, states, actions):
        seen.append(i)
        return states, actions

    RO._ENGINES.clear()
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, on_pol_eval=hook, **kw)
    assert not RO._ENGINES and seen == list(range(H))            # no fused rollout was built for it
    loss = loss_of(rewards, d)
    pol.zero_grad()
    loss.backward()
    S, Rw, g = torch.stack(states).detach().cpu().numpy(), torch.stack(rewards).detach().cpu().numpy(), flat_grad(pol)
    hold(name + ' stepwise / fixture', S, Rw, float(loss), g, d['ref64_states'], d['ref64_rewards'], d['ref64_loss'],
         d['ref64_grad'])
    fs, _, fr = pm.utils.rollout(x0, dyn, pol, H, precision='f32', **kw)
    floss = loss_of(fr, d)
    pol.zero_grad()
    floss.backward()
    hold(name + ' stepwise / fused', S, Rw, float(loss), g, torch.stack(fs).detach().cpu().numpy(),
         torch.stack(fr).detach().cpu().numpy(), float(floss), flat_grad(pol))


@pytest.mark.parametrize('precision', ['f32', 'split_f16'])
def test_act_instance_with_one_tanh_layer(precision):
    """The dynamics model's first hidden layer Tanh, everything else ReLU: the ACT instances of the general family.  It is
    another network than the one the fixture's components were recorded with (some of them have no probability under
    it), so the uniforms are seeded ones and the restatement takes the components they draw under THIS network."""
    from prob_mbrl_amd import activations as ACT
    d = dict(GR.load('gr_d4'))
    acts = [ACT.TANH, ACT.RELU]
    d['dyn_acts'] = np.asarray(acts)
    u = np.random.RandomState(7).uniform(0.02, 0.98, size=d['dyn_kidx'].shape).astype(np.float32)
    d['dyn_kidx'], margin = GR.indices_from_uniforms(d, u, dict(acts=acts))
    d['dyn_ucat'] = u
    assert margin >= GR.MIN_INTERVAL and len(np.unique(d['dyn_kidx'])) == 2, (margin, d['dyn_kidx'])
    eng, S, Rw, loss, g = run(d, precision)
    assert eng.valid_steps() == int(d['H'])
    fwd, bwd = eng.sweep_kernels()['lean']
    assert 'pm_rollout_fwd' in fwd and 'pm_rollout_bwd' in bwd and 'Lb1E' in fwd and 'Lb1E' in bwd, (fwd, bwd)      # ACT = true
    lo, go, (So, _, Ro) = GR.iteration(d, dyn_update=dict(acts=acts))
    assert common.rel(torch.stack(So).detach().numpy(), d['ref64_states']) > 1e-3      # (it IS another network)
    hold('gr_d4 tanh layer', S, Rw, loss, g, torch.stack(So).detach().numpy(), torch.stack(Ro).detach().numpy(), float(lo),
         go.numpy())


def _hundred_rows_one_group(seed=11):
    """gr_d4_mmg's networks on 100 rows (its 20 rows' start states, masks and frozen noise five times over, the start states
    jittered; fresh per-step noise and moment-matching noise) in ONE moment-matching group, with seeded uniforms and the
    components they draw under the restatement."""
    d = dict(GR.load('gr_d4_mmg'))
    rng = np.random.RandomState(seed)
    B, D = d['x0'].shape
    H, k = int(d['H']), 5
    for key in list(d):
        v = np.asarray(d[key])
        if key in ('x0', 'pol_z', 'dyn_zpi') or ('_mask' in key and v.ndim == 2 and v.shape[0] == B):
            d[key] = np.tile(v, (k, 1))
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    d['x0'] = f32(d['x0'] + 0.05 * rng.standard_normal(d['x0'].shape))
    d['dyn_z'] = f32(rng.standard_normal((H, k * B, D + 1)))
    d['z_mm'], d['z_rr'] = f32(rng.standard_normal((H + k * B, D))), f32(rng.standard_normal((H + k * B, 1)))
    d['mm_groups'] = np.int64(0)
    u = f32(rng.uniform(0.02, 0.98, size=(H, k * B)))
    d['dyn_kidx'] = np.zeros((H, k * B), dtype=np.int64)
    d['dyn_kidx'], margin = GR.indices_from_uniforms(d, u)
    d['dyn_ucat'] = u
    return d, margin


@pytest.mark.parametrize('precision', ['f32', 'split_f16'])
def test_one_group_spanning_workgroups(precision):
    """One moment-matching group of 100 rows: more than a workgroup holds, so the moment matching runs in launches of its
    own behind every step (mm_mode 2) and the sweep writes r~ ahead of it -- the form the examples take by default
    (mm_groups=None).  Held against the restatement."""
    d, margin = _hundred_rows_one_group()
    assert margin >= GR.MIN_INTERVAL, margin
    eng, S, Rw, loss, g = run(d, precision)
    assert eng.info['mm_mode'] == 2 and eng.info['n_wg'] > 1 and eng.valid_steps() == int(d['H']), eng.info
    lo, go, (So, _, Ro) = GR.iteration(d)
    hold('100 rows, one group', S, Rw, loss, g, torch.stack(So).detach().numpy(), torch.stack(Ro).detach().numpy(), float(lo),
         go.numpy())


def test_fit_on_d_plus_one_targets():
    """gr_fit: the reference's train_regressor iterations with the mixture log-likelihood on D + 1 = 5 targets, replayed
    (recorded minibatches and dropout draws) through pmbrl_bnn_loss_grad + pmbrl_clip_adam at the bars of
    tests/test_gpu_kernels.py::test_bnn_training_matches_reference; then utils.train_regressor itself on a
    reward_func=None model with GaussianMixtureDensity(D + 1, n) and losses.gaussian_mixture_log_likelihood."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import engine as E
    d = np.load(os.path.join(GR.DIR, GR.FIT + '.npz'))
    nl = int(d['n_layers'])
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)  # noqa: E731
    parts, keys = [], []
    for l in range(nl):
        parts += [T(d['W%d_init' % l]).reshape(-1), T(d['b%d_init' % l]).reshape(-1)]
        keys += ['W%d' % l, 'b%d' % l]
        if l < nl - 1:
            parts.append(T(d['logit_p%d_init' % l]).reshape(-1))
            keys.append('logit_p%d' % l)
    flat = torch.cat(parts).contiguous()
    sizes = [p.numel() for p in parts]
    dims = [d['W0_init'].shape[1]] + [d['W%d_init' % l].shape[0] for l in range(nl)]
    n_comp = int(d['n_components'])
    assert dims[-1] == (2 * 5 + 1) * n_comp + 1 and d['Yn'].shape[1] == 5
    step = E.BnnStep(dims, [float(d['temp%d' % l]) for l in range(nl - 1)], [float(d['reg_scale%d' % l]) for l in range(nl - 1)],
                     [float(d['drop_reg%d' % l]) for l in range(nl - 1)], int(d['M']), int(d['N']), float(d['reg_weight']),
                     max_log_std=float(d['max_log_std']), device=torch.device(DEV), loss_kind='gmm', n_components=n_comp)
    Xn, Yn = T(d['Xn']), T(d['Yn'])
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    for it in range(int(d['iters'])):
        idx = torch.tensor(d['idx_it%d' % it].astype(np.int32), device=DEV)
        u = torch.cat([T(d['u%d_it%d' % (l, it)]).reshape(-1) for l in range(nl - 1)])
        bvar = 1.0 - torch.cat([T(d['hard%d_it%d' % (l, it)]).reshape(-1) for l in range(nl - 1)])
        grad, loss = step.loss_grad(Xn, Yn, idx, flat, u.contiguous(), bvar.contiguous())
        assert np.allclose(loss.cpu().numpy(), d['losses'][it], rtol=3e-5, atol=2e-6), (it, loss, d['losses'][it])
        if it == 0:
            off = 0
            for key, n in zip(keys, sizes):
                assert common.rel(grad[off:off + n].cpu().numpy(), d['g%s_it0' % key].reshape(-1)) < 5e-5, key
                off += n
        E.clip_adam(flat, grad, m, v, it + 1, float(d['lr']), max_norm=None)
    off = 0
    for key, n in zip(keys, sizes):
        assert np.allclose(flat[off:off + n].cpu().numpy(), d[key + '_final'].reshape(-1), rtol=2e-5, atol=5e-7), key
        off += n
    # train_regressor on a data set with the reward as its last target column
    D, U, n = 4, 2, 3
    torch.manual_seed(0)
    dyn = pm.models.DynamicsModel(
        pm.models.mlp(D + U, (2 * (D + 1) + 1) * n + 1, [24, 25],
                      dropout_layers=[pm.models.CDropout(0.1 * np.ones(h)) for h in (24, 25)], nonlin=torch.nn.ReLU),
        reward_func=None, output_density=pm.models.GaussianMixtureDensity(D + 1, n)).float().to(DEV)
    X = torch.randn(120, D + U, device=DEV)
    Y = torch.cat([0.3 * torch.randn(120, D, device=DEV) + 0.5 * X[:, :D] * X[:, D:D + 1], X[:, :1] ** 2], -1)
    dyn.set_dataset(X, Y)
    opt = torch.optim.Adam(dyn.parameters(), 1e-3)
    ll = pm.losses.gaussian_mixture_log_likelihood
    first = pm.utils.train_regressor(dyn, 5, 32, True, opt, log_likelihood=ll)
    last = pm.utils.train_regressor(dyn, 300, 32, True, opt, log_likelihood=ll)
    assert np.isfinite(float(last[1])) and float(last[1]) < float(first[1]), (first, last)


def test_one_mc_pilco_iteration_on_the_fused_and_the_autograd_route():
    """The same first iteration by both routes (rollout_kwargs sends it through autograd): the restatement's loss, the
    same Adam step, the general family throughout."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    d = GR.load('gr_d4_mmg')
    lo, _, _, _ = GR.reference('gr_d4_mmg')
    x0 = torch.tensor(d['x0'], device=DEV)
    finals = {}
    for route, kw in (('fused', {}), ('autograd', dict(rollout_kwargs=dict(infer_noise_variables=False)))):
        dyn, pol = GR.modules(d, DEV)
        init = flat_grad_free_params(pol)
        losses = []
        RO._ENGINES.clear()
        pm.algorithms.mc_pilco(x0, dyn, pol, int(d['H']), torch.optim.Adam(pol.parameters(), 1e-3), None, 1,
                               mm_states=True, mm_rewards=True, mm_groups=int(d['mm_groups']), maximize=True, clip_grad=1.0,
                               on_iteration=lambda i, loss, *a: losses.append(float(loss)),
                               frozen_noise=dict(z_mm=torch.tensor(d['z_mm']), z_rr=torch.tensor(d['z_rr'])), **kw)
        engs = list(RO._ENGINES.values())
        assert engs and all(e.reg_calls() == (0, 0) and e.info['fast'] == 0 and e.learned and e.n_comp == 2 for e in engs)
        assert len(losses) == 1 and abs(losses[0] - lo) <= TOL_TRAJ * abs(lo), (route, losses, lo)
        finals[route] = flat_grad_free_params(pol)
        # Adam's first step is -lr g / (|g| + eps): -lr sign(g) to 1e-3 of lr wherever |g| > 1e3 eps = 1e-5; held on
        # the elements whose gradient is no rounding noise (an element with |g| ~ eps moves by up to lr on noise)
        g_ref = GR.reference('gr_d4_mmg')[1]
        big = np.abs(g_ref) > max(1e-5, 0.05 * np.abs(g_ref).max())
        assert big.sum() > 10
        assert np.allclose((finals[route] - init)[big], -1e-3 * np.sign(g_ref[big]), rtol=0, atol=2e-6), route
    assert np.allclose(finals['fused'][big], finals['autograd'][big], rtol=0, atol=2e-6)


def test_groups_spread_over_ranks_stay_refused():
    from prob_mbrl_amd import _lib
    from prob_mbrl_amd import engine as E
    D, U, n = 4, 1, 2
    with pytest.raises(_lib.PmbrlError, match='spread over ranks'):
        E.Engine(32, D, U, 4, [D, 16, 2 * U], [1.0], [D + U, 16, (2 * (D + 1) + 1) * n + 1], [1.0], E.LEARNED_REWARD,
                 mm_states=True, mm_rewards=True, mm_groups=1, device=DEV, B_global=64, mm_span=(64, 0, 2, 0),
                 dyn_components=n)
    # ... and a head as wide as the mixture of the states alone is told what is expected
    with pytest.raises(_lib.PmbrlError, match=r'\(2 \(D \+ 1\) \+ 1\) dyn_components \+ 1'):
        E.Engine(32, D, U, 4, [D, 16, 2 * U], [1.0], [D + U, 16, (2 * D + 1) * n + 1], [1.0], E.LEARNED_REWARD,
                 device=DEV, dyn_components=n)


def _shard_worker(rank, world, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        d = GR.load('gr_d4_mmg')
        B = d['x0'].shape[0]
        eng, S, Rw, loss, g = run(d, 'f32', Bg=B, shard=(rank, world))
        assert eng.B == B // world and eng.valid_steps() == int(d['H'])
        tot = torch.cat([torch.tensor([loss], dtype=torch.float64), torch.tensor(g, dtype=torch.float64)])
        dist.all_reduce(tot)
        out.put((rank, S, Rw, float(tot[0]), tot[1:].numpy()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_rank_local_groups():
    """Two processes on one device, 10 + 10 of the fixture's 20 rows, one whole moment-matching group each: the
    reference's single-process trajectory, and its loss and gradient as the sum over the ranks."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = common.free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = [out.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    d = GR.load('gr_d4_mmg')
    B = d['x0'].shape[0]
    S, Rw = np.zeros(d['ref64_states'].shape), np.zeros(d['ref64_rewards'].shape)
    for rank, s, r, loss, g in res:
        S[:, rank * B // 2:(rank + 1) * B // 2] = s
        Rw[:, rank * B // 2:(rank + 1) * B // 2] = r
    hold('gr_d4_mmg two ranks', S, Rw, res[0][3], res[0][4], d['ref64_states'], d['ref64_rewards'], d['ref64_loss'],
         d['ref64_grad'])


def test_deep_pilco_learn_reward_with_two_components_runs(tmp_path):
    """examples/deep_pilco.py --learn_reward --dyn_components 2 --ps_iters 1 at tiny sizes, in a fresh child process: runs
    to completion, writes its checkpoints and reports finite losses."""
    root = common.ROOT
    code = ('import sys; sys.path.insert(0, %r); import json; from examples import deep_pilco; '
            'folder, hist = deep_pilco.main(sys.argv[1:]); print("RESULT", json.dumps([folder, hist]))' % root)
    args = ['--learn_reward', '--dyn_components', '2', '--ps_iters', '1', '--pol_opt_iters', '3', '--dyn_opt_iters', '20',
            '--control_H', '20', '--pred_H', '8', '--pol_batch_size', '20', '--dyn_shape', '32,32', '--pol_shape', '32,32',
            '-o', str(tmp_path)]
    r = subprocess.run([sys.executable, '-c', code] + args, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    folder, hist = json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
    for f in ('experience.pth.tar', 'latest_dynamics.pth.tar', 'latest_policy.pth.tar'):
        assert os.path.exists(os.path.join(folder, f)), f
    assert len(hist) == 1 and np.isfinite(hist[0]['first_loss']) and np.isfinite(hist[0]['last_loss'])



def test_compat_example_runs_with_both_flags():
    """examples/deep_pilco_mm_compat.py --learn_reward --dyn_components 2 end to end through the prob_mbrl import surface
    (mm_groups=None: one moment-matching group over all rows), tiny sizes."""
    sys.path.insert(0, os.path.join(common.ROOT, 'examples'))
    import deep_pilco_mm_compat as ex
    dyn, pol, log = ex.main(['--learn_reward', '--dyn_components', '2', '--ps_iters', '1', '--dyn_opt_iters', '30',
                             '--pol_opt_iters', '5', '--pred_H', '8', '--pol_batch_size', '30', '--dyn_shape', '32,32',
                             '--pol_shape', '32,32'])
    assert dyn.reward_func is None and dyn.output_density.n_components == 2
    assert len(log) == 1 and len(log[0]['losses']) == 5 and all(np.isfinite(log[0]['losses']))
    assert all(torch.isfinite(p).all() for p in pol.parameters())
