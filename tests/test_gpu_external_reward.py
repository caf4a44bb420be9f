"""GPU (-m gpu): any torch callable as DynamicsModel.reward_func on the fused rollout and mc_pilco's fused routes
(PMBRL_REWARD_EXTERNAL: the host evaluates the reward and its Jacobians between pmbrl_rollout_fwd and
pmbrl_rollout_rewards).  The reference's recorded numbers through a callable, a reward no spec expresses against the
fp64 oracle, a horizon truncated by the callable's own NaN, forward-only rollouts, mc_pilco, rows sharded over two
processes, the shape check and the example."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# every reward kind, the general, the latency-optimised and the register-resident family, U = 4
FIXTURES = ['nomm_d4', 'nomm_h1', 'mmg_d4', 'mm1_d5', 'mmg_infer_ns', 'pend_d2', 'rdv_d8_u4_3layer', 'dcp_d6_mmg',
            'angles_d4', 'gmm_d4', 'full200_nomm', 'full200_mmg']


def shaped_reward(x, u):
    """A reward no spec of prob_mbrl_amd.rewards expresses: -log(1 + x0^2) - (1 - cos x2) - 0.1 sum tanh(u)^2."""
    return (-torch.log1p(x[:, 0:1] ** 2) - (1.0 - torch.cos(x[:, 2:3])) - 0.1 * (torch.tanh(u) ** 2).sum(-1, keepdim=True))


def _set_reward(dyn, fn):
    """dyn.reward_func = fn, for a model built around a reward MODULE (torch registers that one as a child module, and
    a child module is not replaced by a plain function through assignment alone)."""
    if 'reward_func' in dyn._modules:
        del dyn._modules['reward_func']
    dyn.reward_func = fn


def _mm_kwargs(d):
    if not bool(d['mm_states']):
        return {}
    G = int(d['mm_groups'])
    return dict(mm_states=True, mm_rewards=True, mm_groups=G if G > 0 else None,
                z_mm=torch.tensor(d['z_mm'], device=DEV), z_rr=torch.tensor(d['z_rr'], device=DEV),
                infer_noise_variables=bool(d['infer_ns']) if 'infer_ns' in d else False)


def _spy_engines(monkeypatch):
    """The engines rollout.Bundle asks for from now on, in order."""
    from prob_mbrl_amd import rollout as RO
    seen, real = [], RO.get_engine

    def spy(*a, **kw):
        seen.append(real(*a, **kw))
        return seen[-1]

    monkeypatch.setattr(RO, 'get_engine', spy)
    return seen


def _rollout_loss_grad(d, dyn, pol, **extra):
    """rollout + the reference's loss + backward, as test_rollout_autograd_matches_reference does."""
    import prob_mbrl_amd as pm
    x0 = torch.tensor(d['x0'], device=DEV)
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, int(d['H']), resample_state_noise=False,
                                                resample_action_noise=False, **_mm_kwargs(d), **extra)
    loss = common.loss_of(rewards, d)
    pol.zero_grad()
    loss.backward()
    return (torch.stack(states).detach(), torch.stack(actions).detach(), torch.stack(rewards).detach(), float(loss.detach()),
            common.flat_grad(pol))


def _assert_bars(tag, S, loss, g, ref_S, ref_loss, ref_g):
    """The bars of the parity tests: states < 2e-5, loss <= 2e-5, flat gradient < 1e-4 (each figure printed first)."""
    es, el, eg = common.rel(S, ref_S), abs(loss - ref_loss) / abs(ref_loss), common.rel(g, ref_g)
    print('%s: states %.2e  loss %.2e  gradient %.2e' % (tag, es, el, eg))
    assert es < 2e-5, es
    assert el <= 2e-5, el
    assert eg < 1e-4, eg


@pytest.mark.parametrize('name', FIXTURES)
def test_reference_numbers_through_a_callable(name, monkeypatch):
    """The fixture's own reward handed over as a plain function (the module's torch forward, no .spec): the
    reference-recorded fp64 states, loss and gradient at the existing bars; against the analytic module on the same plan
    shape the trajectory is the same bit for bit and the same kernel family served."""
    d = common.load(name)
    seen = _spy_engines(monkeypatch)
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    from prob_mbrl_amd import rollout as RO
    analytic = dyn.reward_func
    assert analytic is not None

    def counted(run):
        """run()'s results, the engine it ran on and the sweeps the register-resident family served for it (engines are
        shared between tests by shape: the counters are differences)."""
        base = {id(e): e.reg_calls() for e in RO._ENGINES.values()}
        out = run()
        eng = seen[-1]
        return out, eng, tuple(a - b for a, b in zip(eng.reg_calls(), base.get(id(eng), (0, 0))))

    (S_a, A_a, R_a, loss_a, g_a), eng_a, served_a = counted(lambda: _rollout_loss_grad(d, dyn, pol))
    _set_reward(dyn, lambda x, u: analytic(x, u))
    assert not hasattr(dyn.reward_func, 'spec') and not isinstance(dyn.reward_func, torch.nn.Module)
    n0 = len(seen)
    (S, A, R, loss, g), eng, served = counted(lambda: _rollout_loss_grad(d, dyn, pol))
    assert len(seen) == n0 + 1 and eng.external and not eng_a.external
    _assert_bars(name, S.cpu().numpy(), loss, g, d['ref64_states'], float(d['ref64_loss']), d['ref64_grad'])
    assert torch.equal(S, S_a) and torch.equal(A, A_a)
    assert eng.sweep_kernels() == eng_a.sweep_kernels()
    for k in ('fast', 'reg', 'mm_mode', 'mm_parts', 'row_tiles', 'rows_per_wg', 'n_wg', 'precision', 'lds_bytes', 'stages'):
        assert eng.info[k] == eng_a.info[k], k
    assert served == served_a, (served, served_a)
    print('%s: rewards, callable against the analytic launch: %.2e (relative); register-resident sweeps %s' %
          (name, common.rel(R.cpu().numpy(), R_a.cpu().numpy()), served))


@pytest.mark.parametrize('name', ['nomm_d4', 'mmg_d4', 'full200_mmg'])
def test_a_reward_no_spec_expresses(name, monkeypatch):
    """shaped_reward against oracle.ref_torch.iteration with the oracle's reward replaced by the same formula in fp64."""
    from oracle import ref_torch
    d = common.load(name)
    monkeypatch.setattr(ref_torch, 'reward_forward', lambda x, u, spec: shaped_reward(x, u))
    ref_loss, ref_g, (ref_S, _, _) = common.oracle_iteration(d)
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    _set_reward(dyn, shaped_reward)
    S, A, R, loss, g = _rollout_loss_grad(d, dyn, pol)
    _assert_bars(name + ' (shaped)', S.cpu().numpy(), loss, g, torch.stack(ref_S).detach().numpy(), float(ref_loss),
                 ref_g.numpy())


def test_truncated_horizon_from_the_callables_own_nan(monkeypatch):
    """The callable returns NaN where x[:, 1] lies beyond a threshold that a clean run first crosses at a known step t0
    (5 < t0 < H): the rollout stops there, and trajectory and gradient are the oracle's n_steps = t0 rollout's."""
    name = 'nomm_d4'
    d = common.load(name)
    H = int(d['H'])
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    analytic = dyn.reward_func
    S_clean = _rollout_loss_grad(d, dyn, pol)[0]
    # row-step t of the callable's input is the state sampled by step t: S[t + 1] (no moment matching here)
    v = S_clean[1:, :, 1]
    t0 = sign = thr = None
    for sg in (1.0, -1.0):
        m = (sg * v).max(1).values.cpu().numpy()
        for t in range(6, H):
            if m[t] > m[:t].max():
                t0, sign, thr = t, sg, 0.5 * (float(m[t]) + float(m[:t].max()))
                break
        if t0 is not None:
            break
    assert t0 is not None and 5 < t0 < H, 'the fixture never reaches a new extreme of x[:, 1] at a step in 6 .. H - 1'

    def failing(x, u):
        r = analytic(x, u)
        return torch.where(sign * x[:, 1:2] > thr, torch.full_like(r, float('nan')), r)

    seen = _spy_engines(monkeypatch)
    _set_reward(dyn, failing)
    import prob_mbrl_amd as pm
    x0 = torch.tensor(d['x0'], device=DEV)
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, resample_state_noise=False, resample_action_noise=False)
    assert seen[-1].valid_steps() == t0
    assert len(states) == t0 + 1 and len(actions) == t0 and len(rewards) == t0
    loss = common.loss_of(rewards, d)
    pol.zero_grad()
    loss.backward()
    g = common.flat_grad(pol)
    for t in (torch.stack(states), torch.stack(actions), torch.stack(rewards), torch.tensor(g)):
        assert bool(torch.isfinite(t).all())
    assert np.isfinite(float(loss.detach()))
    ref_loss, ref_g, (ref_S, _, _) = common.oracle_iteration(d, n_steps=t0)
    _assert_bars('%s truncated at %d' % (name, t0), torch.stack(states).detach().cpu().numpy(), float(loss.detach()), g,
                 torch.stack(ref_S).detach().numpy(), float(ref_loss), ref_g.numpy())


@pytest.mark.parametrize('name', ['nomm_d4', 'mmg_d4'])
def test_forward_only_rollout_forms_no_jacobian(name, monkeypatch):
    """Under torch.no_grad(): one call with H * B rows, no autograd graph, and an adjoint call afterwards is refused."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd._lib import PmbrlError
    d = common.load(name)
    H, B = int(d['H']), d['x0'].shape[0]
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    analytic = dyn.reward_func
    calls = []

    def fn(x, u):
        calls.append((tuple(x.shape), tuple(u.shape), torch.is_grad_enabled(), x.requires_grad, u.requires_grad))
        r = analytic(x, u)
        calls.append(r.requires_grad)
        return r

    seen = _spy_engines(monkeypatch)
    _set_reward(dyn, fn)
    x0 = torch.tensor(d['x0'], device=DEV)
    with torch.no_grad():
        states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, resample_state_noise=False,
                                                    resample_action_noise=False, **_mm_kwargs(d))
    D, U = x0.shape[1], actions[0].shape[1]
    assert calls == [((H * B, D), (H * B, U), False, False, False), False], calls
    assert len(rewards) == H and not rewards[0].requires_grad
    assert common.rel(torch.stack(states).cpu().numpy(), d['ref64_states']) < 2e-5
    assert abs(float(common.loss_of(rewards, d)) - float(d['ref64_loss'])) <= 2e-5 * abs(float(d['ref64_loss']))
    eng = seen[-1]
    gw = torch.tensor(common.loss_weights(d, B), device=DEV)
    with pytest.raises(PmbrlError, match='no Jacobians'):
        eng.backward(gw)
    # ... and with gradients wanted the same callable is again called once, on leaves that require them
    del calls[:]
    states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, resample_state_noise=False,
                                                resample_action_noise=False, **_mm_kwargs(d))
    assert calls == [((H * B, D), (H * B, U), True, True, True), True], calls


@pytest.mark.parametrize('name', ['mcp_nomm', 'mcp_mm1', 'mcp_full200'])
def test_mc_pilco_serves_a_callable_on_the_pipelined_route(name, monkeypatch):
    """Fixtures from the real algorithms.mc_pilco, the reward handed over as a plain function: the reference's losses and
    final parameters, every iteration on the pipelined route."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import algorithms as ALG
    from prob_mbrl_amd.problem import flat_params
    d = common.load(name)
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    analytic = dyn.reward_func
    _set_reward(dyn, lambda x, u: analytic(x, u))
    opt = torch.optim.Adam(pol.parameters(), float(d['mcp_lr']))
    x0 = torch.tensor(d['x0'], device=DEV)
    G = int(d['mm_groups'])
    gam = np.asarray(d['gamma'])
    disc = None if np.allclose(gam, gam[0]) else float(gam[1] / gam[0])
    routes, real = [], ALG._iterate_pipelined

    def spy(run, bundle, *a, **kw):
        routes.append(bundle.engine.external)
        return real(run, bundle, *a, **kw)

    monkeypatch.setattr(ALG, '_iterate_pipelined', spy)
    losses = []
    pm.algorithms.mc_pilco(
        x0, dyn, pol, int(d['H']), opt, None, int(d['mcp_n_iters']), mm_states=bool(d['mm_states']),
        mm_rewards=bool(d['mm_rewards']), mm_groups=G if G > 0 else None, maximize=True,
        clip_grad=float(d['mcp_clip']), discount=disc, on_iteration=lambda i, loss, *a: losses.append(float(loss)),
        frozen_noise=dict(z_mm=torch.tensor(d['z_mm']), z_rr=torch.tensor(d['z_rr'])))
    assert routes == [True] * int(d['mcp_n_iters']), routes
    print('%s: losses %s against %s' % (name, losses, list(d['ref32_mcp_losses'])))
    assert np.allclose(losses, d['ref32_mcp_losses'], rtol=5e-5)
    lins = [m for m in pol.model._modules.values() if isinstance(m, torch.nn.Linear)]
    final = torch.cat([t.detach().reshape(-1) for l in lins for t in (l.weight, l.bias)]).cpu().numpy()
    err, _, cos = common.assert_mcp_update(final, flat_params(d, 'pol'), d)
    print('%s: worst parameter error %.2e, cosine of the total update 1 - %.2e' % (name, float(err.max()), 1.0 - cos))


def _sharded_worker(rank, world, port, name, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import prob_mbrl_amd as pm
        d = dict(common.load(name))
        B, H = d['x0'].shape[0], int(d['H'])
        lo, hi = rank * B // world, (rank + 1) * B // world
        for k in list(d):
            if k in ('x0', 'pol_z', 'dyn_z') or ('_mask' in k and not k.endswith(('_shape', '_bits'))):
                d[k] = d[k][lo:hi]
        dyn, pol = common.modules_from_fixture(d, name, DEV)
        _set_reward(dyn, shaped_reward)
        S, A, R = pm.utils.rollout(torch.tensor(d['x0'], device=DEV), dyn, pol, H, resample_state_noise=False,
                                   resample_action_noise=False, B_global=B, row_offset=lo)
        gamma = [float(g) for g in d['gamma']]
        loss = (-torch.stack([r * gamma[i] for i, r in enumerate(R)]).sum(0)).sum() / B
        pol.zero_grad()
        loss.backward()
        tot = torch.cat([loss.detach().double().cpu().reshape(1), torch.tensor(common.flat_grad(pol)).double()])
        dist.all_reduce(tot)
        out.put((rank, float(tot[0]), tot[1:].numpy()))
    finally:
        dist.destroy_process_group()


def test_rows_sharded_over_two_processes_on_one_device():
    """nomm_d4 sharded in two (as tests/test_gpu_two_ranks.py shards): the callable's loss and gradient, summed over the
    ranks, against the one-process run at the bars of the existing sharded rollout test (loss 2e-5, gradient 1e-4)."""
    import torch.multiprocessing as mp
    name = 'nomm_d4'
    d = common.load(name)
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    _set_reward(dyn, shaped_reward)
    _, _, _, loss1, g1 = _rollout_loss_grad(d, dyn, pol)
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = common.free_port()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, name, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = [out.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, loss, g in res:
        print('rank %d: loss %.2e  gradient %.2e against one process' % (rank, abs(loss - loss1) / abs(loss1), common.rel(g, g1)))
        assert abs(loss - loss1) <= 2e-5 * abs(loss1)
        assert common.rel(g, g1) < 1e-4


def _span_worker(rank, world, port, name, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import prob_mbrl_amd as pm
        d = dict(common.load(name))
        B, H = d['x0'].shape[0], int(d['H'])
        lo, hi = rank * B // world, (rank + 1) * B // world
        for k in list(d):
            if k in ('x0', 'pol_z', 'dyn_z') or ('_mask' in k and not k.endswith(('_shape', '_bits'))):
                d[k] = d[k][lo:hi]
        dyn, pol = common.modules_from_fixture(d, name, DEV)
        analytic = dyn.reward_func
        _set_reward(dyn, lambda x, u: analytic(x, u))
        S, A, R = pm.utils.rollout(
            torch.tensor(d['x0'], device=DEV), dyn, pol, H, resample_state_noise=False, resample_action_noise=False,
            mm_states=True, mm_rewards=True, z_mm=torch.tensor(d['z_mm'], device=DEV), z_rr=torch.tensor(d['z_rr'], device=DEV),
            B_global=B, mm_span=(B, lo, world, rank), process_group=dist.group.WORLD)
        gamma = [float(g) for g in d['gamma']]
        loss = (-torch.stack([r * gamma[i] for i, r in enumerate(R)]).sum(0)).sum() / B
        pol.zero_grad()
        loss.backward()
        tot = torch.cat([loss.detach().double().cpu().reshape(1), torch.tensor(common.flat_grad(pol)).double()])
        dist.all_reduce(tot)
        out.put((rank, lo, hi, torch.stack(S).detach().cpu().numpy(), float(tot[0]), tot[1:].numpy()))
    finally:
        dist.destroy_process_group()


def test_one_moment_matching_group_spread_over_two_processes():
    """Groups spread over ranks (mm_span_rows > 0) stay served: one group of 100 rows over two processes at H = 40, the
    rewards' statistics exchanged by the rewards call -- the reference's fp64 trajectory, loss and gradient, as
    tests/test_gpu_two_ranks.py asserts them for the analytic module."""
    import torch.multiprocessing as mp
    name = 'mm1_b100_h40'
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = common.free_port()
    procs = [ctx.Process(target=_span_worker, args=(r, 2, port, name, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = [out.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    d = common.load(name)
    S = np.zeros(d['ref64_states'].shape)
    for rank, lo, hi, s, loss, g in res:
        S[:, lo:hi] = s
        print('rank %d: loss %.2e  gradient %.2e' % (rank, abs(loss - float(d['ref64_loss'])) / abs(float(d['ref64_loss'])),
                                                   common.rel(g, d['ref64_grad'])))
        assert abs(loss - float(d['ref64_loss'])) <= 2e-5 * abs(float(d['ref64_loss']))
        assert common.rel(g, d['ref64_grad']) < 1e-4
    assert common.rel(S, d['ref64_states']) < 2e-5


def test_replayed_forward_calls_match_eager_calls(monkeypatch):
    """pmbrl_plan_set_replay on an external plan: a per-step-launch form (one moment-matching group over 100 rows) records
    and replays its forward call -- pack and sweeps only -- and its adjoint call; the rewards call between them always
    runs eagerly.  The parameters after 6 iterations are the eager calls' bit for bit."""
    from prob_mbrl_amd import engine as E
    name = 'mmg_h40'
    d = dict(common.load(name))
    d['mm_groups'] = np.asarray(0)
    monkeypatch.setenv('PMBRL_MM_PERSTEP', '1')
    monkeypatch.setenv('PMBRL_MM_PARTS', '1')
    H, B = int(d['H']), d['x0'].shape[0]
    dyn, _ = common.modules_from_fixture(common.load('nomm_d4'), 'nomm_d4', DEV)
    analytic = dyn.reward_func      # (the cart-pole reward: mmg_h40 is a cart-pole fixture)

    def run(replay):
        eng, args, _ = common.engine_from_fixture(d, torch.device(DEV), reward_spec=E.EXTERNAL_REWARD)
        eng.set_replay(replay)
        gw = torch.tensor(common.loss_weights(d, B), device=DEV)
        params = args['pol_flat'].clone()
        args['pol_flat'] = params
        m, v = torch.zeros_like(params), torch.zeros_like(params)
        step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
        loss = torch.zeros(1, device=DEV)
        adam = dict(params=params, exp_avg=m, exp_avg_sq=v, step=step_dev, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                    max_norm=1.0, loss_out=loss)
        losses = []
        for _ in range(6):
            eng.forward(**args, reward_fn=lambda x, u: analytic(x, u))
            eng.backward(gw, adam=adam)
            losses.append(float(loss))
        torch.cuda.synchronize()
        assert eng.valid_steps() == H and eng.info['mm_mode'] in (2, 3)
        return params.clone(), int(step_dev.item()), losses, eng.replay_count()

    p_e, s_e, l_e, n_e = run(0)
    p_r, s_r, l_r, n_r = run(1)
    assert n_e == (0, 0) and n_r[0] >= 3 and n_r[1] >= 3, (n_e, n_r)
    assert s_e == 6 and s_r == 6 and l_e == l_r
    assert torch.equal(p_e, p_r)


def test_wrong_shape_is_a_value_error():
    import prob_mbrl_amd as pm
    d = common.load('nomm_d4')
    dyn, pol = common.modules_from_fixture(d, 'nomm_d4', DEV)
    analytic = dyn.reward_func
    x0 = torch.tensor(d['x0'], device=DEV)
    for bad in (lambda x, u: analytic(x, u).expand(-1, 2), lambda x, u: analytic(x, u).double(),
                lambda x, u: analytic(x, u)[:-1]):
        _set_reward(dyn, bad)
        with pytest.raises(ValueError, match='reward_func'):
            pm.utils.rollout(x0, dyn, pol, int(d['H']), resample_state_noise=False, resample_action_noise=False)
    _set_reward(dyn, 3.0)      # not callable: today's refusal
    with pytest.raises(NotImplementedError, match='must be a prob_mbrl_amd.rewards module'):
        pm.utils.rollout(x0, dyn, pol, int(d['H']), resample_state_noise=False, resample_action_noise=False)


def test_deep_pilco_with_a_callable_reward_runs(tmp_path):
    """examples/deep_pilco.py --reward callable at the tiny sizes of the other example tests, in a fresh child process."""
    root = common.ROOT
    code = ('import sys; sys.path.insert(0, %r); import json; from examples import deep_pilco; '
            'folder, hist = deep_pilco.main(sys.argv[1:]); print("RESULT", json.dumps([folder, hist]))' % root)
    args = ['--reward', 'callable', '--ps_iters', '2', '--pol_opt_iters', '3', '--dyn_opt_iters', '20', '--control_H', '20',
            '--pred_H', '8', '--pol_batch_size', '20', '--dyn_shape', '32,32', '--pol_shape', '32,32', '-o', str(tmp_path)]
    r = subprocess.run([sys.executable, '-c', code] + args, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    folder, hist = json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
    for f in ('experience.pth.tar', 'latest_dynamics.pth.tar', 'latest_policy.pth.tar'):
        assert os.path.exists(os.path.join(folder, f)), f
    assert len(hist) == 2 and all(np.isfinite(h['first_loss']) and np.isfinite(h['last_loss']) for h in hist)
