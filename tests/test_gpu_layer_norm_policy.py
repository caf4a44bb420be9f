"""Layer-normalised networks (mlp(layer_norm=True)) in `rollout()` and `mc_pilco()`: the stepwise rollout over the
modules' differentiable stand-alone calls, against the fixtures of tests/golden/layer_norm (the reference's own rollout and
mc_pilco with such a policy, or such a dynamics model).

Bars, as in test_gpu_concrete_policy.py: states < 2e-5 and loss <= 2e-5 against the fp64 results, the flat gradient (all
policy parameters) < 1e-4, and each ln* tensor < 1e-4 on its own.  mc_pilco: the losses at rtol 5e-5 against the
reference's fp32 losses, the final parameters -- ln* among them -- through common.assert_mcp_update.  A network without
layer norm stays on the fused path.  The example's --pol_layer_norm runs end to end."""
from functools import partial

import numpy as np
import pytest
import torch

from tests import common
from tests import layer_norm_ref as LN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def modules(name):
    """(fixture, dynamics in eval(), policy holding the fixture's parameters, masks and noise, x0, rollout kwargs)"""
    import prob_mbrl_amd as pm
    d = LN.load(name)
    B, D = d['x0'].shape
    U = d['pol_z'].shape[1]
    hid = lambda pre: [d['%s_W%d' % (pre, i)].shape[0] for i in range(int(d[pre + '_n_layers']) - 1)]  # noqa: E731
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))  # noqa: E731
    dyn = pm.models.DynamicsModel(
        pm.models.mlp(D + U, 2 * D, hid('dyn'), dropout_layers=[pm.models.CDropout(0.1 * np.ones(h)) for h in hid('dyn')],
                      nonlin=common.act_module(d['dyn_act']), layer_norm='dyn_ln_g0' in d),
        reward_func=pm.rewards.CartpoleReward(pole_length=torch.tensor(0.5)), output_density=pm.models.DiagGaussianDensity(D)).float()
    maxU = np.asarray(d['pol_scale'], dtype=np.float32)
    pol = pm.models.Policy(
        pm.models.mlp(D, 2 * U, hid('pol'), dropout_layers=[pm.models.BDropout(0.1) for _ in hid('pol')],
                      nonlin=common.act_module(d['pol_act']), output_nonlin=partial(pm.models.DiagGaussianDensity, U),
                      layer_norm='pol_ln_g0' in d), maxU, -maxU).float()
    common.fill_modules(dyn, pol, d)
    with torch.no_grad():
        for pre, net in (('pol', pol.model), ('dyn', dyn.model)):
            for l, ln in enumerate(net.layer_norms()):
                if ln is not None:
                    ln.weight.copy_(T(d['%s_ln_g%d' % (pre, l)]))
                    ln.bias.copy_(T(d['%s_ln_b%d' % (pre, l)]))
                    assert ln.eps == float(d['%s_ln_eps%d' % (pre, l)])
    dyn, pol = dyn.to(DEV), pol.to(DEV)
    dyn.eval()
    x0 = torch.tensor(d['x0'], device=DEV)
    G = int(d['mm_groups'])
    kw = dict(resample_state_noise=False, resample_action_noise=False)
    if bool(d['mm_states']):
        kw.update(mm_states=True, mm_rewards=True, mm_groups=G if G > 0 else None,
                  z_mm=torch.tensor(d['z_mm'], device=DEV), z_rr=torch.tensor(d['z_rr'], device=DEV))
    return d, dyn, pol, x0, kw


def flat(pol, what):
    return torch.cat([getattr(p, what).detach().reshape(-1) if what == 'grad' else p.detach().reshape(-1)
                      for p in pol.parameters()]).cpu().numpy()


@pytest.mark.parametrize('name', LN.ITER)
def test_rollout_matches_the_reference(name):
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    d, dyn, pol, x0, kw = modules(name)
    H = int(d['H'])
    RO._ENGINES.clear()
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, **kw)
    assert not RO._ENGINES                       # the stepwise route: no fused rollout was built for it
    assert len(states) == H + 1 and len(actions) == H and len(rewards) == H
    loss = common.loss_of(rewards, d)
    pol.zero_grad()
    loss.backward()
    e_s = common.rel(torch.stack(states).detach().cpu().numpy(), d['ref64_states'])
    e_l = abs(float(loss.detach()) - float(d['ref64_loss'])) / abs(float(d['ref64_loss']))
    e_g = common.rel(flat(pol, 'grad'), d['ref64_grad'])
    P = LN.Problem(d)
    assert P.names() == [n for n, _ in pol.model.named_parameters()]
    got, ref = P.split(flat(pol, 'grad')), P.split(d['ref64_grad'])
    e_ln = {k: common.rel(got[k], ref[k]) for k in got if k.startswith('ln')}
    print('%s: states %.2e, loss %.2e, gradient %.2e, %s' % (name, e_s, e_l, e_g, ', '.join('%s %.2e' % kv for kv in e_ln.items())))
    assert e_s < 2e-5 and e_l <= 2e-5 and e_g < 1e-4
    assert all(e < 1e-4 for e in e_ln.values())
    assert bool(e_ln) == (name != 'ln_iter_dyn')


@pytest.mark.parametrize('name', LN.MCP)
def test_mc_pilco_trains_the_layer_norms_like_the_reference(name):
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    d, dyn, pol, x0, kw = modules(name)
    opt = torch.optim.Adam(pol.parameters(), float(d['mcp_lr']))
    assert any(p is pol.model.ln0.weight for g in opt.param_groups for p in g['params'])
    init = flat(pol, 'data')
    losses = []
    RO._ENGINES.clear()
    pm.algorithms.mc_pilco(x0, dyn, pol, int(d['H']), opt, None, int(d['mcp_n_iters']), maximize=True,
                           clip_grad=float(d['mcp_clip']), on_iteration=lambda i, loss, *a: losses.append(float(loss)),
                           frozen_noise=dict(z_mm=torch.tensor(d['z_mm']), z_rr=torch.tensor(d['z_rr'])))
    assert not RO._ENGINES                       # the fused and pipelined paths never saw this policy
    print('%s losses: %s against %s' % (name, losses, list(d['ref32_mcp_losses'])))
    assert np.allclose(losses, d['ref32_mcp_losses'], rtol=5e-5)
    final = flat(pol, 'data')
    err, _, cos = common.assert_mcp_update(final, init, d)
    print('%s all parameters: max error %.2e, 1 - cos %.2e' % (name, err.max(), 1 - cos))
    # the LayerNorm tensors on their own: they moved, and as the reference's did
    P = LN.Problem(d)
    got, ref, start = P.split(final), P.split(d['ref32_mcp_final']), P.split(init)
    for k in ('ln0.weight', 'ln0.bias', 'ln1.weight', 'ln1.bias'):
        assert np.abs(got[k] - start[k]).max() > float(d['mcp_lr']), k
        upd, upd_ref = (got[k] - start[k]).ravel(), (ref[k] - start[k]).ravel()
        assert float(upd @ upd_ref / (np.linalg.norm(upd) * np.linalg.norm(upd_ref))) > 1 - 1e-6, k
    assert not pol.training and not dyn.training      # mc_pilco leaves both in eval(), like the reference


def test_a_network_without_layer_norm_stays_on_the_fused_path():
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    d = common.load('nomm_d4')
    dyn, pol = common.modules_from_fixture(d, 'nomm_d4', DEV)
    assert RO.stepwise_networks(dyn, pol) is None
    RO._ENGINES.clear()
    pm.utils.rollout(torch.tensor(d['x0'], device=DEV), dyn, pol, int(d['H']), resample_state_noise=False,
                     resample_action_noise=False)
    assert len(RO._ENGINES) == 1
    for name in ('ln_iter_tanh', 'ln_iter_dyn'):
        _, dyn, pol, _, _ = modules(name)
        assert RO.stepwise_networks(dyn, pol) == 'a network with layer norm'


def test_combinations_the_stepwise_rollout_does_not_serve_are_refused():
    import prob_mbrl_amd as pm
    d, dyn, pol, x0, kw = modules('ln_iter_tanh')
    H = int(d['H'])
    with pytest.raises(NotImplementedError, match='layer norm.*B_global'):
        pm.utils.rollout(x0, dyn, pol, H, B_global=2 * x0.shape[0], **kw)
    with pytest.raises(NotImplementedError, match='layer norm.*prioritized replay'):
        pm.utils.rollout(x0, dyn, pol, H, action_grad_norms_out=[], **kw)


def test_checkpoint_round_trip(tmp_path):
    import prob_mbrl_amd as pm
    d, dyn, pol, x0, kw = modules('ln_iter_tanh')
    path = str(tmp_path / 'policy.pth.tar')
    torch.save(pol.state_dict(), path)
    sd = torch.load(path, map_location='cpu')
    assert all(k in sd for k in ('model.ln0.weight', 'model.ln0.bias', 'model.ln1.weight', 'model.ln1.bias'))
    _, _, other, _, _ = modules('ln_mcp')
    want = pol(x0, resample=False, resample_noise=False)
    assert not torch.equal(other(x0, resample=False, resample_noise=False), want)
    other.load(sd)
    assert torch.equal(other.model.ln1.weight, pol.model.ln1.weight)
    assert torch.equal(other(x0, resample=False, resample_noise=False), want)


def test_deep_pilco_with_a_layer_norm_policy_runs(tmp_path):
    """examples/deep_pilco.py --pol_layer_norm at tiny sizes, in a fresh child process: the policy search runs and trains
    the policy's LayerNorm weights off their initial ones."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import sys; sys.path.insert(0, %r); import json; from examples import deep_pilco; '
            'folder, hist = deep_pilco.main(sys.argv[1:]); print("RESULT", json.dumps([folder, hist]))' % root)
    args = ['--pol_layer_norm', '--ps_iters', '1', '--pol_opt_iters', '3', '--dyn_opt_iters', '20', '--control_H', '20',
            '--pred_H', '6', '--pol_batch_size', '20', '--dyn_shape', '32,32', '--pol_shape', '32,32', '-o', str(tmp_path)]
    r = subprocess.run([sys.executable, '-c', code] + args, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    folder, hist = json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
    assert len(hist) == 1 and all(np.isfinite(h['first_loss']) and np.isfinite(h['last_loss']) for h in hist)
    sd = torch.load(os.path.join(folder, 'latest_policy.pth.tar'), map_location='cpu')
    for k in ('model.ln0.weight', 'model.ln1.weight'):
        assert bool(torch.isfinite(sd[k]).all()) and float((sd[k] - 1).abs().max()) > 1e-4, k
