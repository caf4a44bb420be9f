"""A policy with concrete dropout in train() mode -- how mc_pilco runs a policy (algorithms/mc_pilco.py:44) -- in
`rollout()` and `mc_pilco()`: the stepwise rollout over the modules' differentiable stand-alone calls, with the
reference's recorded draws replayed one per call (CDropout._forced_samples), against the fixtures of
tests/golden/concrete_policy.

Bars, as in test_gpu_on_pol_eval.py: states < 2e-5 and loss <= 2e-5 against the fp64 results, the flat gradient (the
Linear layers and the logits) < 1e-4, and each logit tensor < 1e-4 on its own.  mc_pilco: the losses at rtol 5e-5 against the
reference's fp32 losses, the final Linear parameters and, separately, the final logits through common.assert_mcp_update.
The example's --pol_dropout concrete runs end to end."""
from functools import partial

import numpy as np
import pytest
import torch

from tests import common
from tests import concrete_policy_ref as CP

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def modules(name):
    """(fixture, dynamics in eval(), policy in train() holding the fixture's parameters, noise and draws, x0, kwargs)"""
    import prob_mbrl_amd as pm
    d = CP.load(name)
    dyn, _ = common.modules_from_fixture(d, name, DEV)
    B, D = d['x0'].shape
    U = d['pol_z'].shape[1]
    n = int(d['pol_n_layers'])
    hid = [d['pol_W%d' % i].shape[0] for i in range(n - 1)]
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))  # noqa: E731
    drops = [pm.models.CDropout(0.1 * np.ones(h), temperature=float(d['pol_temp%d' % l])) for l, h in enumerate(hid)]
    maxU = np.asarray(d['pol_scale'], dtype=np.float32)
    pol = pm.models.Policy(pm.models.mlp(D, 2 * U, hid, dropout_layers=drops, nonlin=common.act_module(d['pol_act']),
                                         output_nonlin=partial(pm.models.DiagGaussianDensity, U)), maxU, -maxU).float()
    lins = [m for m in pol.model._modules.values() if isinstance(m, torch.nn.Linear)]
    resample = bool(d['resample_policy'])
    with torch.no_grad():
        for i, lin in enumerate(lins):
            lin.weight.copy_(T(d['pol_W%d' % i]))
            lin.bias.copy_(T(d['pol_b%d' % i]))
        for l, dr in enumerate(drops):
            dr.logit_p.copy_(T(d['pol_logit_p%d' % l]))
            hard, u = T(d['pol_hard%d' % l]), T(d['pol_u%d' % l])
            dr._forced_samples = [hard[it, t] for it in range(hard.shape[0]) for t in range(hard.shape[1])]
            if resample:      # new uniform noise at every call: replayed too
                dr._forced_noises = [u[t] for t in range(u.shape[0])]
            dr.noise.data = u[0] if resample else u
            dr.concrete_noise = torch.zeros(B, hid[l])
        pol.model.fc_nonlin.z.data = T(d['pol_z'])
    pol = pol.to(DEV)
    pol.train()
    x0 = torch.tensor(d['x0'], device=DEV)
    G = int(d['mm_groups'])
    kw = dict(resample_state_noise=False, resample_action_noise=False, resample_policy=resample)
    if bool(d['mm_states']):
        kw.update(mm_states=True, mm_rewards=True, mm_groups=G if G > 0 else None,
                  z_mm=torch.tensor(d['z_mm'], device=DEV), z_rr=torch.tensor(d['z_rr'], device=DEV))
    return d, dyn, pol, lins, drops, x0, kw


@pytest.mark.parametrize('name', CP.ITER)
def test_rollout_matches_the_reference(name):
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    d, dyn, pol, lins, drops, x0, kw = modules(name)
    H = int(d['H'])
    RO._ENGINES.clear()
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, **kw)
    assert not RO._ENGINES                       # no fused rollout was built for it
    assert all(not dr._forced_samples for dr in drops)      # one draw per call and layer
    assert len(states) == H + 1 and len(actions) == H and len(rewards) == H
    loss = common.loss_of(rewards, d)
    pol.zero_grad()
    loss.backward()
    e_s = common.rel(torch.stack(states).detach().cpu().numpy(), d['ref64_states'])
    e_l = abs(float(loss.detach()) - float(d['ref64_loss'])) / abs(float(d['ref64_loss']))
    gl = [dr.logit_p.grad.cpu().numpy() for dr in drops]
    rl = [d['ref64_glogit%d' % l] for l in range(len(drops))]
    e_g = common.rel(np.concatenate([common.flat_grad(pol)] + gl), np.concatenate([d['ref64_grad']] + rl))
    e_lin = common.rel(common.flat_grad(pol), d['ref64_grad'])
    e_logit = [common.rel(g, r) for g, r in zip(gl, rl)]
    print('%s: states %.2e, loss %.2e, gradient %.2e (Linear layers %.2e), logits %s' % (
        name, e_s, e_l, e_g, e_lin, ', '.join('%.2e' % e for e in e_logit)))
    assert e_s < 2e-5 and e_l <= 2e-5 and e_g < 1e-4 and e_lin < 1e-4
    assert all(e < 1e-4 for e in e_logit)


@pytest.mark.parametrize('name', CP.MCP)
def test_mc_pilco_learns_the_rates_like_the_reference(name):
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    from prob_mbrl_amd.problem import flat_params
    d, dyn, pol, lins, drops, x0, kw = modules(name)
    opt = torch.optim.Adam(pol.parameters(), float(d['mcp_lr']))
    assert any(p is drops[0].logit_p for g in opt.param_groups for p in g['params'])
    losses = []
    RO._ENGINES.clear()
    pm.algorithms.mc_pilco(x0, dyn, pol, int(d['H']), opt, None, int(d['mcp_n_iters']), maximize=True,
                           clip_grad=float(d['mcp_clip']), reg_weight=float(d['mcp_reg_weight']),
                           on_iteration=lambda i, loss, *a: losses.append(float(loss)),
                           frozen_noise=dict(z_mm=torch.tensor(d['z_mm']), z_rr=torch.tensor(d['z_rr'])))
    assert not RO._ENGINES                       # the fused and pipelined paths never saw this policy
    assert all(not dr._forced_samples for dr in drops)
    print('%s losses: %s against %s' % (name, losses, list(d['ref32_mcp_losses'])))
    assert np.allclose(losses, d['ref32_mcp_losses'], rtol=5e-5)
    final = torch.cat([t.detach().reshape(-1) for l in lins for t in (l.weight, l.bias)]).cpu().numpy()
    err, _, cos = common.assert_mcp_update(final, flat_params(d, 'pol'), d)
    print('%s Linear layers: max error %.2e, 1 - cos %.2e' % (name, err.max(), 1 - cos))
    # the logits on their own, by the same rule (Adam's normalisation of each element's gradient)
    init = np.concatenate([np.asarray(d['pol_logit_p%d' % l], np.float64) for l in range(len(drops))])
    dl = dict(ref32_mcp_final=np.concatenate([d['ref32_mcp_logit_final%d' % l] for l in range(len(drops))]),
              ref32_mcp_exp_avg_sq=np.concatenate([d['ref32_mcp_logit_exp_avg_sq%d' % l] for l in range(len(drops))]),
              mcp_n_iters=d['mcp_n_iters'], mcp_lr=d['mcp_lr'])
    got = torch.cat([dr.logit_p.detach().reshape(-1) for dr in drops]).cpu().numpy()
    assert np.abs(got - init).max() > float(d['mcp_lr'])      # they moved: up to lr per step
    err, _, cos = common.assert_mcp_update(got, init, dl)
    print('%s logits: moved by %.2e, max error %.2e, 1 - cos %.2e' % (name, np.abs(got - init).max(), err.max(), 1 - cos))
    assert not pol.training and not dyn.training      # mc_pilco leaves both in eval(), like the reference


def test_combinations_the_stepwise_rollout_does_not_serve_are_refused():
    import prob_mbrl_amd as pm
    d, dyn, pol, lins, drops, x0, kw = modules('cp_iter_tanh')
    H = int(d['H'])
    with pytest.raises(NotImplementedError, match='B_global'):
        pm.utils.rollout(x0, dyn, pol, H, B_global=2 * x0.shape[0], **kw)
    with pytest.raises(NotImplementedError, match='prioritized replay'):
        pm.utils.rollout(x0, dyn, pol, H, action_grad_norms_out=[], **kw)
    # a DYNAMICS model in train() mode stays refused, with either kind of policy
    dyn.train()
    with pytest.raises(NotImplementedError, match='dynamics.eval'):
        pm.utils.rollout(x0, dyn, pol, H, **kw)
    pol.eval()
    with pytest.raises(NotImplementedError, match='dynamics.eval'):
        pm.utils.rollout(x0, dyn, pol, H, **kw)


def test_deep_pilco_with_a_concrete_policy_runs(tmp_path):
    """examples/deep_pilco.py --pol_dropout concrete at tiny sizes, in a fresh child process: the policy search runs (with
    moment matching, the example's default) and moves the policy's dropout logits off their initial value."""
    import json
    import math
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import sys; sys.path.insert(0, %r); import json; from examples import deep_pilco; '
            'folder, hist = deep_pilco.main(sys.argv[1:]); print("RESULT", json.dumps([folder, hist]))' % root)
    args = ['--pol_dropout', 'concrete', '--ps_iters', '1', '--pol_opt_iters', '3', '--dyn_opt_iters', '20', '--control_H', '20',
            '--pred_H', '6', '--pol_batch_size', '20', '--dyn_shape', '32,32', '--pol_shape', '32,32', '-o', str(tmp_path)]
    r = subprocess.run([sys.executable, '-c', code] + args, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    folder, hist = json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
    assert len(hist) == 1 and all(np.isfinite(h['first_loss']) and np.isfinite(h['last_loss']) for h in hist)
    sd = torch.load(os.path.join(folder, 'latest_policy.pth.tar'), map_location='cpu')
    for k in ('model.drop0.logit_p', 'model.drop1.logit_p'):
        moved = (sd[k] - math.log(9.0)).abs()      # CDropout(0.1): logit_p = log(0.9 / 0.1)
        assert bool(torch.isfinite(sd[k]).all()) and float(moved.max()) > 1e-3, k
