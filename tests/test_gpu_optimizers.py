"""GPU (-m gpu): optimiser rules on the device -- any torch.optim.Adam / AdamW configuration (parameter groups, L2 and
decoupled weight decay, amsgrad, maximize) through pmbrl_clip_adam_rule(_guarded), pmbrl_plan_set_optimizer (the fused
iteration tail, its replay and the sharded tail), pmbrl_bnn_plan_set_optimizer (pmbrl_bnn_train_steps), mc_pilco,
train_regressor, the critic fit and the example.  References: torch's own optimisers stepping CPU fp32 copies, and the
real reference's runs with these optimisers (tests/golden/optimizers, tools/make_golden_optimizers.py).
Bars: those of tests/test_gpu_kernels.py::test_clip_adam_matches_torch for the kernel, tests/common.py::assert_mcp_update
for mc_pilco's parameter update, those of tests/test_gpu_activations.py's BNN tests and of
tests/test_gpu_api.py::test_critic_fit_matches_reference for the fits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OPT_DIR = os.path.join(common.GOLDEN, 'optimizers')
DEC, AMS, MAX = 1, 2, 4
# parameters, exp_avg, exp_avg_sq / max_exp_avg_sq, stored gradient: (rtol, atol) of test_clip_adam_matches_torch
BAR_P, BAR_M, BAR_V, BAR_G = (1e-5, 1e-6), (1e-5, 1e-7), (1e-5, 1e-12), (1e-5, 1e-8)


def load(name):
    from oracle import ref_torch
    return ref_torch.load_fixture(os.path.join(OPT_DIR, name + '.npz'))


def G(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, flags=0):
    return dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, flags=flags)


def _cut(sizes, n):
    """segment ends of runs of these sizes and the rest, within n elements (empty runs dropped)"""
    ends, off = [], 0
    for s in sizes:
        off = min(n, off + s)
        if not ends or off > ends[-1]:
            ends.append(off)
    if ends[-1] < n:
        ends.append(n)
    return ends


def rule_cases(n):
    """name -> (groups, segments [(end, group)])"""
    two = _cut([5, 64, 1, 257], n)
    many = _cut([max(1, n // 40)] * 31, n)
    eight = [G(lr=1e-3 * (1 + k), betas=(0.9 - 0.05 * k, 0.999 - 0.01 * k), eps=1e-8 * (1 + k), weight_decay=1e-2 * (k % 3),
               flags=(DEC if k % 4 else 0) | (AMS if k % 2 else 0) | (MAX if k == 5 else 0)) for k in range(8)]
    return {
        'adam_l2': ([G(weight_decay=1e-2)], [(n, 0)]),
        'adam_amsgrad': ([G(flags=AMS)], [(n, 0)]),
        'adam_l2_amsgrad_maximize': ([G(weight_decay=1e-2, flags=AMS | MAX)], [(n, 0)]),
        'adamw': ([G(weight_decay=1e-2, flags=DEC)], [(n, 0)]),
        'adamw_amsgrad': ([G(weight_decay=1e-2, flags=DEC | AMS)], [(n, 0)]),
        'adamw_two_groups': ([G(weight_decay=1e-2, flags=DEC), G(lr=3e-3, betas=(0.8, 0.99), flags=DEC)],
                             [(e, q % 2) for q, e in enumerate(two)]),
        'eight_groups_32_segments': (eight, [(e, (3 * q) % 8) for q, e in enumerate(many)]),
    }


def torch_twin(p0, groups, segments):
    """torch's optimiser over CPU fp32 copies of the segments of p0: (optimiser, parameters in flat order)"""
    params, lo = [], 0
    for end, _ in segments:
        params.append(torch.nn.Parameter(p0[lo:end].clone()))
        lo = end
    spec = []
    for k, g in enumerate(groups):
        mine = [p for p, (_, q) in zip(params, segments) if q == k]
        if mine:
            spec.append(dict(params=mine, lr=g['lr'], betas=g['betas'], eps=g['eps'], weight_decay=g['weight_decay'],
                             amsgrad=bool(g['flags'] & AMS), maximize=bool(g['flags'] & MAX),
                             decoupled_weight_decay=bool(g['flags'] & DEC)))
    return torch.optim.Adam(spec), params


def flat_state(opt, params, key):
    return torch.cat([(opt.state[p][key] if key in opt.state[p] else torch.zeros_like(p)).reshape(-1) for p in params])


def close(a, b, bar):
    return torch.allclose(a.cpu(), b.cpu(), rtol=bar[0], atol=bar[1])


def assert_state_matches(p, m, v, vmax, opt, params, groups, segments):
    assert close(p, torch.cat([q.detach().reshape(-1) for q in params]), BAR_P)
    assert close(m, flat_state(opt, params, 'exp_avg'), BAR_M)
    assert close(v, flat_state(opt, params, 'exp_avg_sq'), BAR_V)
    if vmax is not None:
        lo = 0
        for (end, k), q in zip(segments, params):       # (the buffer of a group without amsgrad is never written)
            want = opt.state[q]['max_exp_avg_sq'].reshape(-1) if groups[k]['flags'] & AMS else torch.zeros(end - lo)
            assert close(vmax[lo:end], want, BAR_V), (lo, end, k)
            lo = end


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against torch
# (131077 = PM_RED_MAXB x 256 x 4 + 5: the smallest size at which the kernel's loop takes a second trip)
@pytest.mark.parametrize('clip', [None, 1.0])
@pytest.mark.parametrize('n', [1, 3, 1023, 1025, 131077])
@pytest.mark.parametrize('case', list(rule_cases(1000)))
def test_clip_adam_rule_matches_torch(case, n, clip):
    from prob_mbrl_amd import engine as E
    from prob_mbrl_amd import optim
    groups, segments = rule_cases(n)[case]
    torch.manual_seed(n)
    p0 = torch.randn(n)
    opt, params = torch_twin(p0, groups, segments)
    p = p0.to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    vmax = torch.zeros_like(p) if any(g['flags'] & AMS for g in groups) else None
    rule = optim.Rule(groups, segments, vmax)
    for step in range(1, 5):
        g = torch.randn(n) * (10.0 if step == 2 else 0.1)
        lo = 0
        for q, (end, _) in zip(params, segments):
            q.grad = g[lo:end].clone()
            lo = end
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(params, clip)
        opt.step()
        gg = g.to(DEV)
        norm = torch.empty(1, device=DEV)
        E.clip_adam(p, gg, m, v, step, max_norm=clip, norm_out=norm, rule=rule)
        assert abs(float(norm) - float(g.double().norm())) <= 1e-5 * float(g.double().norm())
        assert close(gg, torch.cat([q.grad.reshape(-1) for q in params]), BAR_G)       # torch's clipped .grad: no decay term
        assert close(p, torch.cat([q.detach().reshape(-1) for q in params]), BAR_P), step
    assert_state_matches(p, m, v, vmax, opt, params, groups, segments)


# 2. a rule that describes plain Adam gives the bits of the call without a rule
@pytest.mark.parametrize('clip', [None, 1.0])
@pytest.mark.parametrize('n', [1025, 131077])
def test_plain_rule_gives_the_plain_kernels_bits(n, clip):
    from prob_mbrl_amd import engine as E
    from prob_mbrl_amd import optim
    torch.manual_seed(n + 1)
    p0 = torch.randn(n, device=DEV)
    runs = []
    for rule in (None, optim.Rule([G(lr=2e-3, betas=(0.85, 0.995), eps=1e-7)], [(n, 0)])):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        gen = torch.Generator(device=DEV).manual_seed(5)
        norm = torch.zeros(1, device=DEV)
        for step in range(1, 4):
            g = torch.randn(n, device=DEV, generator=gen) * (10.0 if step == 2 else 0.1)
            E.clip_adam(p, g, m, v, step, 2e-3, (0.85, 0.995), 1e-7, max_norm=clip, norm_out=norm, rule=rule)
        runs.append([t.cpu() for t in (p, m, v, g, norm)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], p0.cpu())
    # the guarded form too: the bias corrections of the device-side counter
    runs = []
    status = torch.tensor([8, 0], dtype=torch.int32, device=DEV)
    for rule in (None, optim.Rule([G(lr=2e-3, betas=(0.85, 0.995), eps=1e-7)], [(n, 0)])):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        gen = torch.Generator(device=DEV).manual_seed(5)
        cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
        for step in range(1, 4):
            g = torch.randn(n, device=DEV, generator=gen) * (10.0 if step == 2 else 0.1)
            E.clip_adam_guarded(p, g, m, v, cnt, 2e-3, status, 8, (0.85, 0.995), 1e-7, max_norm=clip, rule=rule)
        runs.append([t.cpu() for t in (p, m, v, g, cnt)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert int(runs[0][4]) == 3


# 3. the guarded form
@pytest.mark.parametrize('case', ['adam_l2_amsgrad_maximize', 'adamw_two_groups', 'eight_groups_32_segments'])
def test_guarded_rule_step(case):
    from prob_mbrl_amd import engine as E
    from prob_mbrl_amd import optim
    n = 1025
    groups, segments = rule_cases(n)[case]
    torch.manual_seed(9)
    p0 = torch.randn(n)
    opt, params = torch_twin(p0, groups, segments)
    p = p0.to(DEV)
    m, v = torch.rand(n, device=DEV) * 0.01, torch.rand(n, device=DEV) * 0.01
    vmax = torch.rand(n, device=DEV) * 0.01
    rule = optim.Rule(groups, segments, vmax if any(g['flags'] & AMS for g in groups) else None)
    cnt = torch.tensor([7], dtype=torch.int64, device=DEV)
    before = [t.clone() for t in (p, m, v, vmax, cnt)]
    # the rollout did not complete: nothing moves (the stored gradient is left as it came, too)
    g = torch.randn(n, device=DEV)
    g0 = g.clone()
    E.clip_adam_guarded(p, g, m, v, cnt, None, torch.tensor([5, 0], dtype=torch.int32, device=DEV), 6, max_norm=1.0, rule=rule)
    E.clip_adam_guarded(p, g, m, v, cnt, None, torch.tensor([6, 1], dtype=torch.int32, device=DEV), 6, max_norm=1.0, rule=rule)
    for a, b in zip(before + [g0], (p, m, v, vmax, cnt, g)):
        assert torch.equal(a, b)
    # ... it did: five steps on the device-side counter
    m.zero_(); v.zero_(); vmax.zero_(); cnt.zero_()
    status = torch.tensor([6, 0], dtype=torch.int32, device=DEV)
    for step in range(1, 6):
        gh = torch.randn(n) * (10.0 if step == 2 else 0.1)
        lo = 0
        for q, (end, _) in zip(params, segments):
            q.grad = gh[lo:end].clone()
            lo = end
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        gg = gh.to(DEV)
        E.clip_adam_guarded(p, gg, m, v, cnt, None, status, 6, max_norm=1.0, rule=rule)
        assert close(gg, torch.cat([q.grad.reshape(-1) for q in params]), BAR_G)
        assert close(p, torch.cat([q.detach().reshape(-1) for q in params]), BAR_P), step
    assert int(cnt) == 5
    assert_state_matches(p, m, v, rule.vmax, opt, params, groups, segments)


# ---------------------------------------------------------------------------------------------------------------------
def opt_from_fixture(d, params, device_params=None):
    """The optimiser a fixture records (class, groups, segments) over `params`, which are in flat order."""
    ends, segg = [int(e) for e in d['opt_seg_end']], [int(g) for g in d['opt_seg_group']]
    owner, off, q = [], 0, 0
    for p in params:
        while off >= ends[q]:
            q += 1
        owner.append(segg[q])
        off += p.numel()
        assert off <= ends[q]
    ng = int(d['opt_n_groups'])
    spec = []
    for k in range(ng):
        f = int(d['opt_group_flags'][k])
        spec.append(dict(params=[p for p, o in zip(params, owner) if o == k], lr=float(d['opt_group_lr'][k]),
                         betas=tuple(float(b) for b in d['opt_group_betas'][k]), eps=float(d['opt_group_eps'][k]),
                         weight_decay=float(d['opt_group_weight_decay'][k]), amsgrad=bool(f & AMS), maximize=bool(f & MAX)))
    return (torch.optim.AdamW if int(d['opt_class']) == 1 else torch.optim.Adam)(spec)


def rule_from_fixture(d, vmax=None):
    from prob_mbrl_amd import optim
    groups = [G(float(d['opt_group_lr'][k]), tuple(float(b) for b in d['opt_group_betas'][k]), float(d['opt_group_eps'][k]),
                float(d['opt_group_weight_decay'][k]), int(d['opt_group_flags'][k])) for k in range(int(d['opt_n_groups']))]
    return optim.Rule(groups, [(int(e), int(g)) for e, g in zip(d['opt_seg_end'], d['opt_seg_group'])], vmax)


# 4. replay
def test_replayed_backward_with_a_rule_gives_the_eager_bits_and_never_a_stale_lr():
    """opt_mcp_adamw_mmg (moment-matching groups: the form that replays), set_replay(2): five iterations, the rule's
    learning rates changed before the fourth -- the calls whose arguments repeat go out as graphs, the changed rule is
    part of the key, and every parameter bit is the eager run's."""
    d = load('opt_mcp_adamw_mmg')
    B = d['x0'].shape[0]
    out = {}
    for replay in (0, 2):
        eng, args, _ = common.engine_from_fixture(d, DEV)
        eng.set_replay(replay)
        gw = torch.tensor(common.loss_weights(d, B), device=DEV)
        p = args['pol_flat']
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
        loss = torch.zeros(1, device=DEV)
        rule = rule_from_fixture(d)
        hist = []
        for it in range(5):
            if it == 3:
                for g in rule.groups:
                    g['lr'] = 10.0 * g['lr']
            eng.forward(**args)
            eng.backward(gw, adam=dict(params=p, exp_avg=m, exp_avg_sq=v, step=cnt, lr=0.0, betas=(0.0, 0.0), eps=0.0,
                                       max_norm=float(d['mcp_clip']), expect=int(d['H']), loss_out=loss, rule=rule))
            torch.cuda.synchronize()
            hist.append(p.cpu().clone())
        assert int(cnt) == 5
        out[replay] = (hist, eng.replay_count())
    assert out[0][1] == (0, 0) and out[2][1][1] >= 1, (out[0][1], out[2][1])
    for a, b in zip(out[0][0], out[2][0]):
        assert torch.equal(a, b)
    moved = [float((out[0][0][i + 1] - out[0][0][i]).abs().max()) for i in range(4)]      # by iterations 1 .. 4
    assert moved[2] > 3.0 * moved[1], moved          # the ten times larger learning rate was the one applied


# 5. mc_pilco
@pytest.mark.parametrize('name', ['opt_mcp_adamw_groups', 'opt_mcp_adam_l2_amsgrad', 'opt_mcp_adamw_mmg'])
def test_mc_pilco_matches_the_reference_with_its_optimiser(name, monkeypatch):
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import engine as E
    from prob_mbrl_amd.problem import flat_params
    d = load(name)
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    params = [p for p in pol.parameters() if p.requires_grad]
    opt = opt_from_fixture(d, params)
    log = []
    real_bwd, real_step = E.Engine.backward, opt.step
    monkeypatch.setattr(E.Engine, 'backward', lambda self, *a, **kw: (
        log.append('backward+adam+rule' if kw.get('adam') is not None and kw['adam'].get('rule') is not None else 'backward'),
        real_bwd(self, *a, **kw))[1])
    monkeypatch.setattr(opt, 'step', lambda *a, **kw: (log.append('opt.step'), real_step(*a, **kw))[1])
    x0 = torch.tensor(d['x0'], device=DEV)
    Gm = int(d['mm_groups'])
    n_it = int(d['mcp_n_iters'])
    losses = []
    pm.algorithms.mc_pilco(x0, dyn, pol, int(d['H']), opt, None, n_it, mm_states=bool(d['mm_states']),
                           mm_rewards=bool(d['mm_rewards']), mm_groups=Gm if Gm > 0 else None, maximize=True,
                           clip_grad=float(d['mcp_clip']), on_iteration=lambda i, loss, *a: losses.append(float(loss)),
                           frozen_noise=dict(z_mm=torch.tensor(d['z_mm']), z_rr=torch.tensor(d['z_rr'])))
    monkeypatch.undo()
    assert log == ['backward+adam+rule'] * n_it, log           # the pipelined route served it; torch's step never ran
    assert np.allclose(losses, d['ref32_mcp_losses'], rtol=5e-5), (losses, d['ref32_mcp_losses'])
    final = torch.cat([p.detach().reshape(-1) for p in params]).cpu().numpy()
    common.assert_mcp_update(final, flat_params(d, 'pol'), d)
    # the optimiser's state, exposed again
    sd = opt.state_dict()['state']
    assert len(sd) == len(params) and all(float(s['step']) == n_it for s in sd.values())
    keys = [('exp_avg', BAR_M), ('exp_avg_sq', BAR_V)] + ([('max_exp_avg_sq', BAR_V)] if 'opt_max_exp_avg_sq' in d else [])
    for key, bar in keys:
        got = flat_state(opt, params, key).cpu().numpy()
        want = np.asarray(d['opt_' + key])
        print('%s %s: rel %.3e, max abs %.3e' % (name, key, common.rel(got, want), np.abs(got - want).max()))
    for key, bar in keys:
        assert np.allclose(flat_state(opt, params, key).cpu().numpy(), d['opt_' + key], rtol=bar[0], atol=bar[1]), key
    # torch continues where the device left off: one more step of torch's on a fixed gradient, against the same step on a
    # CPU copy of the state
    twins = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    twin_opt = opt_from_fixture(d, twins)
    for p, t in zip(params, twins):
        twin_opt.state[t] = {k: (s.detach().cpu().clone() if torch.is_tensor(s) else s) for k, s in opt.state[p].items()}
        p.grad = torch.full_like(p, 0.05)
        t.grad = torch.full_like(t, 0.05)
    opt.step()
    twin_opt.step()
    for p, t in zip(params, twins):
        assert torch.allclose(p.detach().cpu(), t.detach(), rtol=0, atol=1e-6)
        assert float(opt.state[p]['step']) == n_it + 1


# ---------------------------------------------------------------------------------------------------------------------
# 6. the network fit
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
    step = E.BnnStep(dims, [float(d['temp%d' % l]) for l in range(nl - 1)], [float(d['reg_scale%d' % l]) for l in range(nl - 1)],
                     [float(d['drop_reg%d' % l]) for l in range(nl - 1)], int(d['M']), int(d['N']), float(d['reg_weight']),
                     max_log_std=float(d['max_log_std']), device=torch.device(DEV))
    draws = lambda it: (torch.cat([T(d['u%d_it%d' % (l, it)]).reshape(-1) for l in range(nl - 1)]).contiguous(),  # noqa: E731
                        torch.cat([1.0 - T(d['hard%d_it%d' % (l, it)]).reshape(-1) for l in range(nl - 1)]).contiguous())
    return step, torch.cat(parts).contiguous(), keys, [p.numel() for p in parts], T, draws


@pytest.mark.parametrize('name', ['opt_bnn_adamw_logit_lr', 'opt_bnn_adam_amsgrad'])
def test_bnn_train_steps_with_a_rule_matches_reference(name):
    """pmbrl_bnn_train_steps with the fixture's rule attached (pmbrl_bnn_plan_set_optimizer), one iteration per call with
    the recorded draws, at the bars of test_bnn_train_steps_matches_reference."""
    d = load(name)
    step, flat, keys, sizes, T, draws = _bnn_setup(d)
    assert flat.numel() == int(d['opt_seg_end'][-1])
    Xn, Yn = T(d['Xn']), T(d['Yn'])
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    vmax = torch.zeros_like(flat) if 'opt_max_exp_avg_sq' in d else None
    rule = rule_from_fixture(d, vmax)
    stepc = torch.zeros(1, dtype=torch.int64, device=DEV)
    iters = int(d['iters'])
    for it in range(iters):
        idx = torch.tensor(d['idx_it%d' % it].astype(np.int32), device=DEV).reshape(1, -1).contiguous()
        u, bvar = draws(it)
        loss = step.train_steps(Xn, Yn, idx, flat, m, v, stepc, 0.0, (0.0, 0.0), 0.0, u=u, bvar=bvar, rule=rule)
        assert np.allclose(loss.cpu().numpy(), d['losses'][it], rtol=3e-5, atol=2e-6), (it, loss, d['losses'][it])
    assert int(stepc.item()) == iters
    off = 0
    for key, n in zip(keys, sizes):
        got, want = flat[off:off + n].cpu().numpy(), d[key + '_final'].reshape(-1)
        assert np.allclose(got, want, rtol=1e-4, atol=2e-6), (key, np.abs(got - want).max())
        off += n
    for got, key in ((m, 'opt_exp_avg'), (v, 'opt_exp_avg_sq'), (vmax, 'opt_max_exp_avg_sq')):       # (reported, not a bar)
        if got is not None:
            print('%s %s: rel %.3e' % (name, key, common.rel(got.cpu().numpy(), d[key])))


@pytest.mark.parametrize('name', ['opt_bnn_adamw_logit_lr', 'opt_bnn_adam_amsgrad'])
def test_bnn_loss_grad_and_clip_adam_rule_match_reference(name):
    """The non-fused path: pmbrl_bnn_loss_grad + pmbrl_clip_adam_rule replaying the reference's iterations, at the bars
    of test_bnn_loss_grad_matches_reference."""
    from prob_mbrl_amd import engine as E
    d = load(name)
    step, flat, keys, sizes, T, draws = _bnn_setup(d)
    Xn, Yn = T(d['Xn']), T(d['Yn'])
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    rule = rule_from_fixture(d, torch.zeros_like(flat) if 'opt_max_exp_avg_sq' in d else None)
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
        E.clip_adam(flat, grad, m, v, it + 1, max_norm=None, rule=rule)
    off = 0
    for key, n in zip(keys, sizes):
        assert np.allclose(flat[off:off + n].cpu().numpy(), d[key + '_final'].reshape(-1), rtol=2e-5, atol=5e-7), key
        off += n


def _small_dynamics(seed=0):
    import prob_mbrl_amd as pm
    torch.manual_seed(seed)
    np.random.seed(seed)
    D, U, N = 3, 1, 128
    dyn = pm.models.DynamicsModel(
        pm.models.mlp(D + U, 2 * D, [32, 32], dropout_layers=[pm.models.CDropout(0.1 * np.ones(32)) for _ in range(2)],
                      nonlin=torch.nn.ReLU), reward_func=None, output_density=pm.models.DiagGaussianDensity(D)).float().to(DEV)
    X = torch.randn(N, D + U, device=DEV)
    dyn.set_dataset(X, torch.tanh(X[:, :D] + 0.5 * X[:, D:D + 1]) + 0.05 * torch.randn(N, D, device=DEV))
    return dyn


@pytest.mark.parametrize('mode', ['fused', 'non_fused', 'decoupled_reg', 'prioritized_sampling'])
def test_train_regressor_accepts_adamw_with_groups(mode, monkeypatch):
    """utils.train_regressor with an AdamW over three groups (weights decayed, biases, logits at 10 x lr) on every path
    that takes an optimiser; the state it leaves is torch's to continue with.  A torch.optim.SGD is still refused, by a
    message that names what is offered."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import engine as E
    dyn = _small_dynamics()
    named = [(n, p) for n, p in dyn.named_parameters() if p.requires_grad]
    logits = [p for n, p in named if n.endswith('logit_p')]
    W = [p for n, p in named if p.dim() > 1]
    b = [p for n, p in named if p.dim() <= 1 and not n.endswith('logit_p')]
    assert len(logits) == 2 and len(W) == 3 and len(b) == 3
    opt = torch.optim.AdamW([dict(params=W, weight_decay=1e-2), dict(params=b, weight_decay=0.0),
                             dict(params=logits, weight_decay=0.0, lr=2e-2)], lr=2e-3, amsgrad=True)
    calls = []
    real = E.BnnStep.train_steps
    monkeypatch.setattr(E.BnnStep, 'train_steps', lambda self, *a, **kw: (calls.append(kw.get('rule')), real(self, *a, **kw))[1])
    if mode == 'non_fused':
        monkeypatch.setenv('PMBRL_BNN_FUSED', '0')
    kw = {'decoupled_reg': dict(decoupled_reg=True), 'prioritized_sampling': dict(prioritized_sampling=True)}.get(mode, {})
    before = [p.detach().clone() for n, p in named]
    l0 = pm.utils.train_regressor(dyn, iters=3, batchsize=32, optimizer=opt, **kw).clone()
    l1 = pm.utils.train_regressor(dyn, iters=120, batchsize=32, optimizer=opt, **kw).clone()
    assert bool(calls) == (mode == 'fused') and all(r is not None and len(r.groups) == 3 for r in calls)
    assert bool(torch.isfinite(l1).all())
    if mode in ('fused', 'non_fused'):
        assert float(l1[1]) < float(l0[1]), (l0, l1)          # E[-lml] went down
    assert all(not torch.equal(a, p.detach()) for a, (n, p) in zip(before, named))
    for n, p in named:
        st = opt.state[p]
        assert int(st['step']) == 4 + 121 and st['exp_avg'].shape == p.shape and st['max_exp_avg_sq'].shape == p.shape
        assert bool((st['max_exp_avg_sq'] >= st['exp_avg_sq']).all())
        p.grad = torch.zeros_like(p)
    opt.step()          # torch's own step continues from the device's state
    assert int(opt.state[W[0]]['step']) == 4 + 121 + 1
    with pytest.raises(NotImplementedError, match='Adam.*AdamW'):
        pm.utils.train_regressor(dyn, iters=1, batchsize=32, optimizer=torch.optim.SGD(dyn.parameters(), 1e-3))


# 7. the critic fit
def test_critic_fit_with_adamw_matches_reference():
    """critic.update_value_function with the fixture's AdamW against the reference example's own function, at the bars
    of tests/test_gpu_api.py::test_critic_fit_matches_reference."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd.critic import update_value_function
    d = load('opt_critic_adamw')
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))  # noqa: E731
    n = int(d['n_layers'])
    hid = [d['W%d_init' % i].shape[0] for i in range(n - 1)]
    D = d['W0_init'].shape[1]
    V = pm.models.Regressor(pm.models.mlp(
        D, 1, hid, dropout_layers=[pm.models.CDropout(0.2 * np.ones(h)) for h in hid], nonlin=torch.nn.ReLU)).float()
    with torch.no_grad():
        lins = [m for m in V.model._modules.values() if isinstance(m, torch.nn.Linear)]
        for i, lin in enumerate(lins):
            lin.weight.copy_(T(d['W%d_init' % i]))
            lin.bias.copy_(T(d['b%d_init' % i]))
        for i in range(n - 1):
            dr = getattr(V.model, 'drop%d' % i)
            dr.logit_p.copy_(T(d['logit_p%d_init' % i]))
            dr.noise.data = T(d['u%d' % i])
            dr.concrete_noise = torch.ones_like(dr.noise)
        for k in ('mx', 'iSx', 'my', 'Sy'):
            getattr(V, k).data = T(d[k]).reshape(1, -1)
    V = V.to(DEV)
    params = [p for p in V.parameters() if p.requires_grad]
    opt = opt_from_fixture(d, params)
    assert type(opt) is torch.optim.AdamW and opt.param_groups[0]['weight_decay'] == 0.5
    H, gam = int(d['H']), float(d['gamma'])
    states = [None] * (H + 1)
    states[0], states[H] = T(d['states0']).to(DEV), T(d['statesH']).to(DEV)
    rewards = [T(r).to(DEV) for r in d['rewards']]
    for it in range(int(d['n_updates'])):
        draws = [d['hard%d_it%d' % (k, it)] for k in range(2 * (n - 1))]
        update_value_function(V, opt, H, it, states, None, rewards, lambda i: gam**i,
                              reg_weight=float(d['reg_weight']), _bernoulli=draws)
        for i, lin in enumerate(lins):
            assert np.allclose(lin.weight.detach().cpu().numpy(), d['W%d_it%d' % (i, it)], rtol=5e-4, atol=5e-6), (it, i)
            assert np.allclose(lin.bias.detach().cpu().numpy(), d['b%d_it%d' % (i, it)], rtol=5e-4, atol=5e-6)
        for i in range(n - 1):
            assert np.allclose(getattr(V.model, 'drop%d' % i).logit_p.detach().cpu().numpy(),
                               d['logit_p%d_it%d' % (i, it)], rtol=5e-4, atol=5e-6)
    with pytest.raises(NotImplementedError, match='Adam.*AdamW'):
        update_value_function(V, torch.optim.SGD(V.parameters(), 1e-3), H, 0, states, None, rewards, lambda i: gam**i)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the sharded tail: two processes on one device, the peer-to-peer transport
def _mcp_worker(rank, world, port, case, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['PMBRL_P2P'] = '1'
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import prob_mbrl_amd as pm
        from prob_mbrl_amd import distributed as D
        from prob_mbrl_amd import rollout as RO
        name = case['name']
        d = dict(load(name))
        B = d['x0'].shape[0]
        lo, hi = D.shard_bounds(B, None, world, rank)
        for k in list(d):
            if k == 'x0' or k in ('pol_z', 'dyn_z') or '_mask' in k:
                d[k] = d[k][lo:hi]
        dyn, pol = common.modules_from_fixture(d, name, 'cuda:0')
        params = [p for p in pol.parameters() if p.requires_grad]
        opt = opt_from_fixture(d, params)
        losses = []
        pm.algorithms.mc_pilco(
            torch.tensor(d['x0'], device='cuda:0'), dyn, pol, int(d['H']), opt, None,
            int(d['mcp_n_iters']), maximize=True, clip_grad=float(d['mcp_clip']),
            on_iteration=lambda i, loss, *a: losses.append(float(loss)),
            frozen_noise=dict(z_mm=torch.zeros(1, 4), z_rr=torch.zeros(1, 1)),
            mm_states=bool(d['mm_states']), mm_rewards=bool(d['mm_rewards']), process_group=dist.group.WORLD)
        final = torch.cat([p.detach().reshape(-1) for p in params])
        out.put(dict(rank=rank, losses=losses, final=final.cpu().numpy(), n_iters=int(d['mcp_n_iters']),
                     tail_calls=sum(e.tail_calls() for e in RO._ENGINES.values()),
                     opt_steps=int(pm.algorithms.policy_update_counter[pol]),
                     adam_step=int(opt.state[params[0]]['step']),
                     exp_avg_sq=flat_state(opt, params, 'exp_avg_sq').cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_mc_pilco_two_ranks_through_the_sharded_tail_with_adamw_groups():
    """opt_mcp_adamw_groups, its rows split over two ranks: every iteration is served by the backward call with the
    exchange inside and the rule's optimiser launch behind it; the replicas hold the same bits and the reference's
    update."""
    import queue
    import time

    import torch.multiprocessing as mp
    from prob_mbrl_amd.problem import flat_params
    name = 'opt_mcp_adamw_groups'
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = common.free_port()
    procs = [ctx.Process(target=_mcp_worker, args=(r, 2, port, dict(name=name), out)) for r in range(2)]
    for p in procs:
        p.start()
    res, deadline = [], time.monotonic() + 180
    try:
        while len(res) < 2:
            try:
                res.append(out.get(timeout=0.5))
            except queue.Empty:
                # a dead or late worker fails the test: no retry, and no waiting for the other once one is gone
                assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
                assert time.monotonic() < deadline, 'a worker did not answer in time'
        res.sort(key=lambda r: r['rank'])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    d = load(name)
    for r in res:
        assert r['tail_calls'] == r['n_iters'] > 0
        assert r['opt_steps'] == r['n_iters'] and r['adam_step'] == r['n_iters']
        assert np.allclose(r['losses'], d['ref32_mcp_losses'], rtol=5e-5)
        common.assert_mcp_update(r['final'], flat_params(d, 'pol'), d)
    assert np.array_equal(res[0]['final'], res[1]['final'])      # replicas stay bit-identical
    assert np.array_equal(res[0]['exp_avg_sq'], res[1]['exp_avg_sq']) and res[0]['losses'] == res[1]['losses']


# ---------------------------------------------------------------------------------------------------------------------
# 9. the example
def test_deep_pilco_with_adamw_groups_runs(tmp_path):
    """examples/deep_pilco.py --pol_opt adamw --pol_weight_decay 1e-2 --dyn_logit_lr 1e-3 at the tiny sizes of
    test_deep_pilco_nonlin_silu_runs: finite losses, checkpoints on disk."""
    root = common.ROOT
    code = ('import sys; sys.path.insert(0, %r); import json; from examples import deep_pilco; '
            'folder, hist = deep_pilco.main(sys.argv[1:]); print("RESULT", json.dumps([folder, hist]))' % root)
    args = ['--pol_opt', 'adamw', '--pol_weight_decay', '1e-2', '--dyn_logit_lr', '1e-3', '--ps_iters', '2',
            '--pol_opt_iters', '3', '--dyn_opt_iters', '20', '--control_H', '20', '--pred_H', '8', '--pol_batch_size', '20',
            '--dyn_shape', '32,32', '--pol_shape', '32,32', '-o', str(tmp_path)]
    r = subprocess.run([sys.executable, '-c', code] + args, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import json
    folder, hist = json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
    for f in ('experience.pth.tar', 'latest_dynamics.pth.tar', 'latest_policy.pth.tar'):
        assert os.path.exists(os.path.join(folder, f)), f
    assert len(hist) == 2 and all(np.isfinite(h['first_loss']) and np.isfinite(h['last_loss']) for h in hist)
