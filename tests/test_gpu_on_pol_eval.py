"""`rollout(..., on_pol_eval=hook)`: the reference's loop (utils/rollout.py:93-163) step by step over the modules' own
differentiable stand-alone calls (models.param_grad), the hook between the policy and the dynamics half of a step.

An identity hook must give what the fused rollout gives: the fixture's own ref64_* at the bars of
test_gpu_api.test_rollout_autograd_matches_reference (states 2e-5, loss 2e-5, policy gradient 1e-4).  A hook that changes
the trajectory is held, at the same bars, to a test-side fp64 loop over the oracle's step functions with the same
hook."""
import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDENTITY = ['nomm_d4', 'mmg_d4', 'mm1_d5', 'mmg_infer_ns', 'angles_d4', 'act_silu_mmg_d4', 'gmm_d4', 'lr_nomm_d4',
            'unit_rates_d4']


def setup(name):
    d = common.load(name)
    dyn, pol = common.modules_from_fixture(d, name, DEV, learned=name.startswith('lr_'))
    x0 = torch.tensor(d['x0'], device=DEV)
    G = int(d['mm_groups'])
    kw = dict(resample_state_noise=False, resample_action_noise=False)
    if bool(d['mm_states']):
        kw.update(mm_states=True, mm_rewards=True, mm_groups=G if G > 0 else None,
                  z_mm=torch.tensor(d['z_mm'], device=DEV), z_rr=torch.tensor(d['z_rr'], device=DEV),
                  infer_noise_variables=bool(d['infer_ns']) if 'infer_ns' in d else False)
    return d, dyn, pol, x0, kw


def hold(name, d, pol, states, rewards, S_ref, loss_ref, g_ref):
    loss = common.loss_of(rewards, d)
    pol.zero_grad()
    loss.backward()
    e_s = common.rel(torch.stack(states).detach().cpu().numpy(), S_ref)
    e_l = abs(float(loss.detach()) - float(loss_ref)) / abs(float(loss_ref))
    e_g = common.rel(common.flat_grad(pol), g_ref)
    print('%s: states %.2e, loss %.2e, gradient %.2e' % (name, e_s, e_l, e_g))
    assert e_s < 2e-5 and e_l <= 2e-5 and e_g < 1e-4


@pytest.mark.parametrize('name', IDENTITY)
def test_identity_hook_matches_the_fixture(name):
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    d, dyn, pol, x0, kw = setup(name)
    H = int(d['H'])
    seen = []

    def hook(i, states, actions):
        seen.append((i, states.requires_grad, actions.requires_grad))
        return states, actions

    RO._ENGINES.clear()
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, on_pol_eval=hook, **kw)
    assert not RO._ENGINES                       # no fused rollout was built for it
    assert [s[0] for s in seen] == list(range(H))
    assert all(a for _, _, a in seen) and all(s for i, s, _ in seen if i > 0)
    assert len(states) == H + 1 and len(actions) == H and len(rewards) == H
    assert states[0].shape == x0.shape and rewards[0].shape == (x0.shape[0], 1)
    hold(name, d, pol, states, rewards, d['ref64_states'], d['ref64_loss'], d['ref64_grad'])


def perturb_actions(i, states, actions):
    """differentiable in the state: the hook's own term joins the chain"""
    return (states, actions + 0.05 * torch.sin(states[:, :1])) if i % 2 else (states, actions)


def zero_a_column(i, states, actions):
    keep = torch.ones(states.shape[1], dtype=states.dtype, device=states.device)
    keep[1] = 0.0
    return states * keep, actions


def oracle_loop(d, hook):
    """oracle.ref_torch.rollout with the hook between its two halves, fp64: (states, loss, flat policy gradient)."""
    from oracle import ref_torch as R
    x0, pol, dyn, spec, meta, z_mm, z_rr, gamma = R.problem_from_npz(d, torch.float64)
    for p in R.policy_params(pol):
        p.requires_grad_(True)
    B, D = x0.shape
    G = meta['mm_groups']
    j1, j2 = 1e-12 * torch.eye(D, dtype=x0.dtype), 1e-12 * torch.eye(1, dtype=x0.dtype)

    def mm(t, z, j):
        w = t.shape[-1]
        if G is not None:
            return R.mm_resample(t.view(G, -1, w), z.view(G, -1, w), j, meta['infer_ns']).view(-1, w)
        return R.mm_resample(t, z, j, meta['infer_ns'])

    states, S, Rw = x0, [], []
    for i in range(meta['H']):
        actions = R.policy_forward(states, pol, i)
        states, actions = hook(i, states, actions)
        nxt, rew = R.dynamics_forward(states, actions, dyn, spec, i)
        if meta['mm_states']:
            nxt = mm(nxt, R.get_z_rnd(z_mm, i, B), j1)
        if meta['mm_rewards']:
            rew = mm(rew, R.get_z_rnd(z_rr, i, B), j2)
        S.append(states)
        Rw.append(rew)
        states = nxt
    S.append(states)
    loss = R.mc_loss(Rw, gamma, meta['maximize'])
    loss.backward()
    return torch.stack(S).detach().numpy(), float(loss.detach()), R.flat_grad(pol).numpy()


@pytest.mark.parametrize('hook', [perturb_actions, zero_a_column])
@pytest.mark.parametrize('name', ['nomm_d4', 'mmg_d4'])
def test_hooks_that_change_the_trajectory(name, hook):
    import prob_mbrl_amd as pm
    d, dyn, pol, x0, kw = setup(name)
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, int(d['H']), on_pol_eval=hook, **kw)
    S_ref, loss_ref, g_ref = oracle_loop(d, hook)
    # the hook did something: a rollout that ignored it would miss the states' bar by a factor of ten or more
    assert common.rel(S_ref, d['ref64_states']) > 2e-4
    # the trajectory records what the hook returned
    if hook is zero_a_column:
        assert all(float(s[:, 1].abs().max()) == 0.0 for s in states[:-1])
    hold('%s %s' % (name, hook.__name__), d, pol, states, rewards, S_ref, loss_ref, g_ref)


def test_a_late_error_truncates_and_an_early_one_propagates():
    import prob_mbrl_amd as pm
    d, dyn, pol, x0, kw = setup('nomm_d4')
    H = int(d['H'])
    assert H == 12

    def fails_at(n):
        def hook(i, states, actions):
            if i == n:
                raise RuntimeError('hook failed at step %d' % i)
            return states, actions
        return hook

    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, on_pol_eval=fails_at(8), **kw)
    assert (len(states), len(actions), len(rewards)) == (9, 8, 8)
    assert common.rel(torch.stack(states).detach().cpu().numpy(), d['ref64_states'][:9]) < 2e-5
    with pytest.raises(RuntimeError, match='hook failed at step 3'):
        pm.utils.rollout(x0, dyn, pol, H, on_pol_eval=fails_at(3), **kw)


def test_sharded_rows_with_a_hook_are_refused():
    import prob_mbrl_amd as pm
    d, dyn, pol, x0, kw = setup('nomm_d4')
    with pytest.raises(NotImplementedError, match='B_global'):
        pm.utils.rollout(x0, dyn, pol, int(d['H']), on_pol_eval=lambda i, s, a: (s, a), B_global=2 * x0.shape[0], **kw)


@pytest.mark.parametrize('name', ['mcp_nomm', 'mcp_mm1'])
def test_mc_pilco_with_a_hook_matches_reference_iterations(name):
    """mc_pilco(rollout_kwargs=dict(on_pol_eval=identity)): the autograd iteration over the stepwise rollout."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    from prob_mbrl_amd.problem import flat_params
    d = common.load(name)
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    opt = torch.optim.Adam(pol.parameters(), float(d['mcp_lr']))
    x0 = torch.tensor(d['x0'], device=DEV)
    G = int(d['mm_groups'])
    gam = np.asarray(d['gamma'])
    disc = None if np.allclose(gam, gam[0]) else float(gam[1] / gam[0])
    losses, calls = [], []

    def identity(i, states, actions):
        calls.append(i)
        return states, actions

    RO._ENGINES.clear()
    pm.algorithms.mc_pilco(
        x0, dyn, pol, int(d['H']), opt, None, int(d['mcp_n_iters']), mm_states=bool(d['mm_states']),
        mm_rewards=bool(d['mm_rewards']), mm_groups=G if G > 0 else None, maximize=True,
        clip_grad=float(d['mcp_clip']), discount=disc,
        on_iteration=lambda i, loss, *a: losses.append(float(loss)),
        frozen_noise=dict(z_mm=torch.tensor(d['z_mm']), z_rr=torch.tensor(d['z_rr'])),
        rollout_kwargs=dict(on_pol_eval=identity))
    assert calls == list(range(int(d['H']))) * int(d['mcp_n_iters'])
    # (the driver builds the plan of the shape before it routes an iteration; no fused sweep ran on it)
    assert all(e.generation == 0 for e in RO._ENGINES.values())
    print('%s losses: %s against %s' % (name, losses, list(d['ref32_mcp_losses'])))
    assert np.allclose(losses, d['ref32_mcp_losses'], rtol=5e-5)
    lins = [m for m in pol.model._modules.values() if isinstance(m, torch.nn.Linear)]
    final = torch.cat([t.detach().reshape(-1) for l in lins for t in (l.weight, l.bias)]).cpu().numpy()
    common.assert_mcp_update(final, flat_params(d, 'pol'), d)
