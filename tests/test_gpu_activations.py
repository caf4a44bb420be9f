"""GPU (-m gpu): Tanh / SiLU hidden layers through the rollout plans (general kernel family, F32 and SPLIT_F16), the
stand-alone network calls, the BNN fit, mc_pilco and the example, against the reference's fixtures
(tests/golden/activations, tools/make_golden_activations.py) and the fp64 oracle (oracle/ref_torch.py, the networks'
activations in its dicts).
Bars: those of tests/test_gpu_kernels.py (TOL_TRAJ 2e-5, TOL_GRAD 1e-4, the BNN bars) and, for mc_pilco's parameter
update, tests/common.py::assert_mcp_update."""
import os
import subprocess
import sys
import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from prob_mbrl_amd import activations as ACT
from tests import common

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL_TRAJ, TOL_GRAD = 2e-5, 1e-4


def run_engine(d, precision, replay=None, n_calls=1):
    eng, args, _ = common.engine_from_fixture(d, DEV, precision=precision)
    if replay is not None:
        eng.set_replay(replay)
    B = d['x0'].shape[0]
    gw = torch.tensor(common.loss_weights(d, B), device=DEV)
    out = []
    for _ in range(n_calls):
        S, A, R = eng.forward(**args)
        loss = float(eng.weighted_sum(R, gw))
        g, _, _ = eng.backward(gw)
        torch.cuda.synchronize()
        out.append((S.cpu().numpy().copy(), A.cpu().numpy().copy(), R.cpu().numpy().copy(), loss, g.cpu().numpy().copy()))
    return eng, out


@pytest.mark.parametrize('precision', ['f32', 'split_f16'])
@pytest.mark.parametrize('name', common.ACT_ITER)
def test_rollout_matches_reference(name, precision):
    """One rollout and its policy gradient on every rollout fixture, in both arithmetics of the general family."""
    d = common.load(name)
    eng, out = run_engine(d, precision)
    S, A, R, loss, g = out[0]
    # the general family served it, on the arithmetic asked for; the families that are ReLU-only did not
    assert eng.info['fast'] == 0 and eng.info['reg'] == 0 and eng.info['inplace'] == 0 and eng.reg_calls() == (0, 0)
    assert eng.info['precision'] == precision and eng.valid_steps() == int(d['H'])
    floor = common.rel(d['ref32_grad'], d['ref64_grad'])
    print('%s %s: states %.2e actions %.2e rewards %.2e loss %.2e grad vs fp64 %.2e (reference fp32 vs fp64: %.2e)' % (
        name, precision, common.rel(S, d['ref32_states']), common.rel(A, d['ref32_actions']),
        common.rel(R.reshape(d['ref32_rewards'].shape), d['ref32_rewards']),
        abs(loss - float(d['ref64_loss'])) / abs(float(d['ref64_loss'])), common.rel(g, d['ref64_grad']), floor))
    assert np.isfinite(S).all() and np.isfinite(g).all()
    assert common.rel(S, d['ref32_states']) < TOL_TRAJ
    assert common.rel(A, d['ref32_actions']) < TOL_TRAJ
    assert common.rel(R.reshape(d['ref32_rewards'].shape), d['ref32_rewards']) < TOL_TRAJ
    assert abs(loss - float(d['ref64_loss'])) <= TOL_TRAJ * abs(float(d['ref64_loss']))
    assert common.rel(g, d['ref64_grad']) < TOL_GRAD
    assert common.rel(g, d['ref32_grad']) < TOL_GRAD + floor


@pytest.mark.parametrize('name', ['act_mcp_tanh', 'act_mcp_silu_mmg', 'act_critic_tanh'])
def test_mc_pilco_matches_reference_iterations(name):
    """The real mc_pilco's iterations (pipelined iteration, clip + Adam): losses per iteration and the parameter update,
    at the bars of common.assert_mcp_update.  act_critic_tanh: a Tanh critic
    as value_func -- the value bootstrap's dV/ds_H comes from pmbrl_mlp_grad_input."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import rollout as RO
    from prob_mbrl_amd.problem import flat_params
    d = common.load(name)
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    opt = torch.optim.Adam(pol.parameters(), float(d['mcp_lr']))
    x0 = torch.tensor(d['x0'], device=DEV)
    G = int(d['mm_groups'])
    losses, kw = [], {}
    if 'val_n_layers' in d:
        kw['value_func'] = common.value_from_fixture(d, DEV)
    RO._ENGINES.clear()
    pm.algorithms.mc_pilco(x0, dyn, pol, int(d['H']), opt, None, int(d['mcp_n_iters']), mm_states=bool(d['mm_states']),
                           mm_rewards=bool(d['mm_rewards']), mm_groups=G if G > 0 else None, maximize=True,
                           clip_grad=float(d['mcp_clip']), cvar_eps=float(d['mcp_cvar_eps']),
                           reg_weight=float(d['mcp_reg_weight']),
                           on_iteration=lambda i, loss, *a: losses.append(float(loss)),
                           frozen_noise=dict(z_mm=torch.tensor(d['z_mm']), z_rr=torch.tensor(d['z_rr'])), **kw)
    engs = list(RO._ENGINES.values())
    assert engs and all(e.reg_calls() == (0, 0) and e.info['fast'] == 0 for e in engs)      # the general family served it
    assert np.allclose(losses, d['ref32_mcp_losses'], rtol=5e-5), (losses, d['ref32_mcp_losses'])
    lins = [m for m in pol.model._modules.values() if isinstance(m, torch.nn.Linear)]
    final = torch.cat([t.detach().reshape(-1) for l in lins for t in (l.weight, l.bias)]).cpu().numpy()
    common.assert_mcp_update(final, flat_params(d, 'pol'), d)


def test_critic_value_and_input_gradient():
    """pmbrl_mlp_forward / pmbrl_mlp_grad_input through a Tanh critic against the fp64 oracle."""
    d = common.load('act_critic_tanh')
    V = common.value_from_fixture(d, DEV)
    val = R.value_from_npz(d, torch.float64)
    xr = torch.tensor(d['x0'], dtype=torch.float64, requires_grad=True)
    vr = R.value_forward(xr, val)
    vr.sum().backward()
    xd = torch.tensor(d['x0'], device=DEV).requires_grad_(True)
    vd = V(xd, resample=False, return_samples=True)
    vd.sum().backward()
    assert common.rel(vd.detach().cpu().numpy(), vr.detach().numpy()) < 2e-6
    assert common.rel(xd.grad.cpu().numpy(), xr.grad.numpy()) < 1e-5


@pytest.mark.parametrize('name', ['act_tanh_d4', 'act_silu_d4', 'act_mixed_nets_d4'])
def test_standalone_forward_and_grad_input(name):
    """The stand-alone policy and dynamics evaluations (raw head rows and their input gradients) on the d4 fixtures
    against the fp64 oracle: pmbrl_mlp_forward, pmbrl_mlp_grad_input."""
    from prob_mbrl_amd import engine as E
    from prob_mbrl_amd.problem import flat_params, layer_dims
    d = common.load(name)
    x0, pol, dyn, spec, meta, z_mm, z_rr, gamma = R.problem_from_npz(d, torch.float64)
    B, D = d['x0'].shape
    g = torch.Generator().manual_seed(11)
    for pre, net, width in (('pol', pol, D), ('dyn', dyn, D + 1)):
        x = torch.randn(B, width, generator=g, dtype=torch.float64)
        xr = x.clone().requires_grad_(True)
        o = R.mlp_forward(xr, net['weights'], net['masks'], net['keep'], act=net['act'])
        n = o.shape[1] // 2
        w = torch.randn(B, n, generator=g, dtype=torch.float64)
        (o[:, :n] * w).sum().backward()
        bits = [E.pack_mask(torch.tensor(np.asarray(d['%s_mask%d' % (pre, i)], np.float32), device=DEV))
                for i in range(int(d[pre + '_n_layers']) - 1)]
        xd = x.float().to(DEV).requires_grad_(True)
        out = E.mlp_forward(xd, torch.tensor(flat_params(d, pre), device=DEV), layer_dims(d, pre),
                            list(np.asarray(d[pre + '_keep'])), bits, want=('mean',), max_log_std=100.0,
                            act=int(d[pre + '_act']))
        (out['mean'] * w.float().to(DEV)).sum().backward()
        assert common.rel(out['mean'].detach().cpu().numpy(), o[:, :n].detach().numpy()) < 2e-6, pre
        assert common.rel(xd.grad.cpu().numpy(), xr.grad.numpy()) < 1e-5, pre


def _bnn_setup(d):
    from prob_mbrl_amd import engine as E
    nl = int(d['n_layers'])
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)  # noqa: E731
    parts, keys = [], []
    for l in range(nl):
        parts += [T(d['W%d_init' % l]).reshape(-1), T(d['b%d_init' % l]).reshape(-1)]
        keys += ['W%d' % l, 'b%d' % l]
        if l < nl - 1:
            parts.append(T(d['logit_p%d_init' % l]).reshape(-1))
            keys.append('logit_p%d' % l)
    dims = [d['W0_init'].shape[1]] + [d['W%d_init' % l].shape[0] for l in range(nl)]
    n_comp = int(d['n_components']) if 'n_components' in d else 0
    step = E.BnnStep(dims, [float(d['temp%d' % l]) for l in range(nl - 1)], [float(d['reg_scale%d' % l]) for l in range(nl - 1)],
                     [float(d['drop_reg%d' % l]) for l in range(nl - 1)], int(d['M']), int(d['N']), float(d['reg_weight']),
                     max_log_std=float(d['max_log_std']), device=torch.device(DEV), loss_kind='gmm' if n_comp > 1 else 'nll',
                     n_components=n_comp, act=int(d['act']))
    draws = lambda it: (torch.cat([T(d['u%d_it%d' % (l, it)]).reshape(-1) for l in range(nl - 1)]).contiguous(),  # noqa: E731
                        torch.cat([1.0 - T(d['hard%d_it%d' % (l, it)]).reshape(-1) for l in range(nl - 1)]).contiguous())
    return step, torch.cat(parts).contiguous(), keys, [p.numel() for p in parts], T, draws


@pytest.mark.parametrize('name', common.ACT_BNN)
def test_bnn_loss_grad_matches_reference(name):
    """pmbrl_bnn_loss_grad + pmbrl_clip_adam replaying the reference's iterations (act_bnn_silu: the mixture head), at the
    bars of test_gpu_kernels.py::test_bnn_training_matches_reference."""
    from prob_mbrl_amd import engine as E
    d = common.load(name)
    step, flat, keys, sizes, T, draws = _bnn_setup(d)
    Xn, Yn = T(d['Xn']), T(d['Yn'])
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    for it in range(int(d['iters'])):
        idx = torch.tensor(d['idx_it%d' % it].astype(np.int32), device=DEV)
        u, bvar = draws(it)
        grad, loss = step.loss_grad(Xn, Yn, idx, flat, u, bvar)
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


def test_bnn_train_steps_matches_reference():
    """pmbrl_bnn_train_steps on the Tanh fixture, one iteration per call with the recorded draws replayed (the fused
    steps serve the Gaussian likelihood, as for ReLU), at the bars of test_bnn_fused_training_matches_reference."""
    d = common.load('act_bnn_tanh')
    step, flat, keys, sizes, T, draws = _bnn_setup(d)
    Xn, Yn = T(d['Xn']), T(d['Yn'])
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    stepc = torch.zeros(1, dtype=torch.int64, device=DEV)
    iters = int(d['iters'])
    for it in range(iters):
        idx = torch.tensor(d['idx_it%d' % it].astype(np.int32), device=DEV).reshape(1, -1).contiguous()
        u, bvar = draws(it)
        loss = step.train_steps(Xn, Yn, idx, flat, m, v, stepc, float(d['lr']), u=u, bvar=bvar)
        assert np.allclose(loss.cpu().numpy(), d['losses'][it], rtol=3e-5, atol=2e-6), (it, loss, d['losses'][it])
    assert int(stepc.item()) == iters
    off = 0
    for key, n in zip(keys, sizes):
        got, want = flat[off:off + n].cpu().numpy(), d[key + '_final'].reshape(-1)
        assert np.allclose(got, want, rtol=1e-4, atol=2e-6), (key, np.abs(got - want).max())
        off += n


def test_truncated_horizon_matches_oracle():
    """A SiLU plan whose forward sweep is declared failed at step 7: loss and gradient are the oracle's truncated there."""
    d = common.load('act_silu_d4')
    eng, args, _ = common.engine_from_fixture(d, DEV, precision='f32')
    S, A, R = eng.forward(**args)
    n = 7
    eng.status[0] = n
    gw = torch.tensor(common.loss_weights(d, d['x0'].shape[0]), device=DEV)
    loss = float(eng.weighted_sum(R, gw))
    g, _, _ = eng.backward(gw)
    lo, go, _ = common.oracle_iteration(d, n_steps=n)
    assert abs(loss - float(lo)) <= TOL_TRAJ * abs(float(lo))
    assert common.rel(g.cpu().numpy(), go.numpy()) < TOL_GRAD


def test_graph_replay_gives_the_eager_bits():
    """set_replay(2) on a Tanh plan: the replayed calls give the eager calls' bits."""
    d = common.load('act_tanh_d4')
    eng0, eager = run_engine(d, 'split_f16', replay=0, n_calls=3)
    eng2, replayed = run_engine(d, 'split_f16', replay=2, n_calls=3)
    assert eng0.replay_count() == (0, 0) and min(eng2.replay_count()) >= 1
    for a, b in zip(eager, replayed):
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y))


def test_learned_reward_head_with_tanh_dynamics():
    """A Tanh dynamics model that predicts the reward (2 (D + 1) head), through utils.rollout and autograd, against the
    oracle with a learned reward and both activations Tanh."""
    import prob_mbrl_amd as pm
    d = dict(common.load('lr_nomm_d4'))
    d['pol_act'], d['dyn_act'] = ACT.TANH, ACT.TANH
    dyn, pol = common.modules_from_fixture(d, 'lr_nomm_d4', DEV, learned=True)
    x0 = torch.tensor(d['x0'], device=DEV)
    H = int(d['H'])
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, resample_state_noise=False, resample_action_noise=False,
                                                precision='f32')
    loss = common.loss_of(rewards, d)
    pol.zero_grad()
    loss.backward()
    lo, go, (So, _, Ro) = common.oracle_iteration(d)
    assert common.rel(torch.stack(states).detach().cpu().numpy(), torch.stack(So).detach().numpy()) < TOL_TRAJ
    assert common.rel(torch.stack(rewards).detach().cpu().numpy(), torch.stack(Ro).detach().numpy()) < TOL_TRAJ
    assert common.rel(common.flat_grad(pol), go.numpy()) < TOL_GRAD


def test_mixture_head_with_silu_dynamics():
    """A SiLU dynamics model with a 2-component mixture head, the recorded component draws replayed through
    _forced_draws, against the oracle with both activations SiLU."""
    import prob_mbrl_amd as pm
    d = dict(common.load('gmm_d6_mmg'))
    d['pol_act'], d['dyn_act'] = ACT.SILU, ACT.SILU
    # the uniforms that reproduce the recorded component indices under THIS activation's softmax (common.gmm_uniforms)
    d['dyn_ucat'] = common.gmm_uniforms(d)
    dyn, pol = common.modules_from_fixture(d, 'gmm_d6_mmg', DEV)
    assert dyn.output_density.n_components == 2
    assert not any(isinstance(m, torch.nn.ReLU) for net in (dyn.model, pol.model) for m in net.modules())
    G = int(d['mm_groups'])
    kw = dict(mm_states=True, mm_rewards=True, mm_groups=G if G > 0 else None, z_mm=torch.tensor(d['z_mm'], device=DEV),
              z_rr=torch.tensor(d['z_rr'], device=DEV)) if bool(d['mm_states']) else {}
    x0 = torch.tensor(d['x0'], device=DEV)
    H = int(d['H'])
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, resample_state_noise=False, resample_action_noise=False,
                                                precision='f32', **kw)
    loss = common.loss_of(rewards, d)
    pol.zero_grad()
    loss.backward()
    lo, go, (So, _, _) = common.oracle_iteration(d)
    assert common.rel(torch.stack(states).detach().cpu().numpy(), torch.stack(So).detach().numpy()) < TOL_TRAJ
    assert abs(float(loss) - float(lo)) <= TOL_TRAJ * abs(float(lo))
    assert common.rel(common.flat_grad(pol), go.numpy()) < TOL_GRAD


def test_unknown_activation_fails_plan_creation():
    from prob_mbrl_amd import _lib
    from prob_mbrl_amd import engine as E
    D, U = 4, 1
    spec = dict(kind='exp', expand=False, angle_dims=[], C=np.eye(2, D), tip_target=np.zeros(2), norm=1.0, w=1.0,
                Q=np.eye(2), R=np.eye(U))
    with pytest.raises(_lib.PmbrlError, match=r'\(-2\).*unknown activation'):
        E.Engine(32, D, U, 4, [D, 16, 2 * U], [1.0], [D + U, 16, 2 * D], [1.0], spec, device=DEV, dyn_act=7)
    with pytest.raises(_lib.PmbrlError, match=r'\(-2\).*unknown activation'):
        E.BnnStep([5, 16, 8], [0.1], [0.5], [1.0], 8, 16, device=DEV, act=3)
    with pytest.raises(ValueError, match='unknown activation'):
        E.mlp_forward(torch.zeros(4, 5, device=DEV), torch.zeros(5 * 16 + 16 + 16 * 8 + 8, device=DEV), [5, 16, 8], [1.0], act=9)
    # a plan that is not ReLU is the general family's, whatever else would have made it fast
    eng = E.Engine(32, D, U, 4, [D, 16, 2 * U], [1.0], [D + U, 16, 2 * D], [1.0], spec, device=DEV, pol_act=1)
    assert eng.info['fast'] == 0 and eng.info['reg'] == 0 and eng.info['inplace'] == 0


def test_deep_pilco_nonlin_silu_runs(tmp_path):
    """examples/deep_pilco.py --nonlin silu at tiny sizes: two policy-search iterations end with finite losses and the
    checkpoints on disk (a SiLU dynamics model fitted by train_regressor, a SiLU policy optimised by mc_pilco)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import sys; sys.path.insert(0, %r); import json; from examples import deep_pilco; '
            'folder, hist = deep_pilco.main(sys.argv[1:]); print("RESULT", json.dumps([folder, hist]))' % root)
    args = ['--nonlin', 'silu', '--ps_iters', '2', '--pol_opt_iters', '3', '--dyn_opt_iters', '20', '--control_H', '20',
            '--pred_H', '8', '--pol_batch_size', '20', '--dyn_shape', '32,32', '--pol_shape', '32,32', '-o', str(tmp_path)]
    r = subprocess.run([sys.executable, '-c', code] + args, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import json
    folder, hist = json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
    for f in ('experience.pth.tar', 'latest_dynamics.pth.tar', 'latest_policy.pth.tar'):
        assert os.path.exists(os.path.join(folder, f)), f
    assert len(hist) == 2 and all(np.isfinite(h['first_loss']) and np.isfinite(h['last_loss']) for h in hist)
