#!/usr/bin/env python
"""Generate the fixtures tests/golden/concrete_policy/cp_*.npz: the REAL reference's utils.rollout and
algorithms.mc_pilco with a policy whose hidden layers are followed by concrete dropout (models.modules.CDropout) in
train() mode, which is how mc_pilco runs a policy (algorithms/mc_pilco.py:44): every policy call draws a hard Bernoulli
sample of the relaxed probabilities and the backward goes through those probabilities (models/modules.py:102-118,
151-153), so logit_p has a gradient.  Runs through tools/make_golden.py's import shims; no existing fixture is touched.

The fp32 run records every draw (torch.bernoulli: one per policy layer and step; torch.rand_like: the uniform noise of a
call with resample_policy=True).  The same modules switched to .double() then replay the recorded draws, so that the
ref64_* results belong to the same masks.  For the mc_pilco cases the fp64 run is the loop body of
algorithms/mc_pilco.py:86-216 over the reference's own rollout, modules, clip and Adam (one resampling period: nothing
is redrawn between the iterations but the hard samples).

Keys, beside those of tools/make_golden.py's rollout fixtures (capture_inputs):  pol_act;  pol_logit_p{l}, pol_temp{l},
pol_reg_scale{l}, pol_drop_reg{l};  pol_u{l} [B, h] (the stored noise) or [H, B, h] (resample_policy=True: one per call);
pol_hard{l} [iterations, H, B, h] uint8;  ref32_* / ref64_*: states, loss, grad (the Linear layers, flat), glogit{l};
mc_pilco cases: mcp_* and ref32_mcp_* / ref64_mcp_* losses, final (Linear layers), exp_avg_sq, logit_final{l},
logit_exp_avg_sq{l}.

Usage:  python tools/make_golden_concrete_policy.py [--out tests/golden/concrete_policy] [--only name]
"""
import copy
import os
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (import shims, the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from prob_mbrl import algorithms, models, utils  # noqa: E402
from prob_mbrl.models.activations import Swish  # noqa: E402
from prob_mbrl.models.modules import CDropout  # noqa: E402

RELU, TANH, SILU = 0, 1, 2
MODULES = {RELU: torch.nn.ReLU, TANH: torch.nn.Tanh, SILU: Swish}
f = lambda t: t.detach().double().cpu().numpy().copy()  # noqa: E731


class _Draws:
    """torch.bernoulli / torch.rand_like recorded in call order (replay=None), or answered from a recording."""

    def __init__(self, replay=None):
        self.b, self.u = [], []
        self.replay = replay

    def __enter__(self):
        self.orig = torch.bernoulli, torch.rand_like
        rec = self

        def bern(p, *a, **k):
            if rec.replay is not None:
                out = rec.replay.b[len(rec.b)].to(p.dtype)
                assert out.shape == p.shape
            else:
                out = rec.orig[0](p, *a, **k)
            rec.b.append(out.detach().clone())
            return out

        def rand_like(x, *a, **k):
            if rec.replay is not None:
                out = rec.replay.u[len(rec.u)].to(x.dtype)
                assert out.shape == x.shape
            else:
                out = rec.orig[1](x, *a, **k)
            rec.u.append(out.detach().clone())
            return out

        torch.bernoulli, torch.rand_like = bern, rand_like
        return self

    def __exit__(self, *exc):
        torch.bernoulli, torch.rand_like = self.orig


def build(D, U, hid, act, rew, maxU, seed, B):
    """examples/deep_pilco_mm.py:117-151 with --pol_dropout concrete: CDropout on both policy layers."""
    dyn, _ = mg.build(D, U, hid, hid, rew, maxU, seed)
    torch.manual_seed(seed + 3)
    pol_model = models.mlp(D, 2 * U, hid, dropout_layers=[CDropout(0.1 * np.ones(h)) for h in hid], nonlin=MODULES[act],
                           output_nonlin=partial(models.DiagGaussianDensity, U))
    maxU_t = np.asarray(maxU, dtype=np.float32).reshape(-1)
    pol = models.Policy(pol_model, maxU_t, -maxU_t).float()
    with torch.no_grad():      # rates that differ per unit
        for m in pol.modules():
            if isinstance(m, CDropout):
                m.logit_p.add_(0.3 * torch.randn_like(m.logit_p))
    dyn.eval()
    pol.train()
    torch.manual_seed(seed + 1000)
    x0 = 0.1 * torch.randn(B, D)
    with torch.no_grad():      # sizes the [B, h] / [B, D] buffers
        utils.rollout(x0, dyn, pol, 1, resample_state_noise=False, resample_action_noise=False)
    return dyn, pol, x0


def pol_layers(pol):
    lins = [m for m in pol.model._modules.values() if isinstance(m, torch.nn.Linear)]
    drops = [m for m in pol.model._modules.values() if isinstance(m, CDropout)]
    return lins, drops


def detach_state(*mods):
    """p and concrete_noise of a CDropout carry the last forward's graph: drop it (both are recomputed by the next
    train-mode forward; an eval-mode model applies concrete_noise detached anyway)."""
    for mod in mods:
        for m in mod.modules():
            if isinstance(m, CDropout):
                m.concrete_noise = m.concrete_noise.detach()
                m._buffers['p'] = m._buffers['p'].detach() if 'p' in m._buffers else m.p.detach()


def describe_policy(d, pol, act):
    lins, drops = pol_layers(pol)
    d['pol_act'] = act
    for l, m in enumerate(drops):
        d['pol_logit_p%d' % l] = f(m.logit_p)
        d['pol_temp%d' % l] = float(m.temp)
        d['pol_reg_scale%d' % l] = float(m.regularizer_scale)
        d['pol_drop_reg%d' % l] = float(m.dropout_regularizer)
        d['pol_u%d' % l] = f(m.noise)
        d['pol_mask%d' % l] = np.round(d['pol_mask%d' % l])      # (the last hard sample, up to rounding; unused)


def one_iteration(dyn, pol, x0, H, gamma, kw, reg_weight=0.0):
    pol.zero_grad()
    dyn.zero_grad()
    states, actions, rewards = utils.rollout(x0, dyn, pol, H, resample_state_noise=False, resample_action_noise=False, **kw)
    disc = torch.stack([r * gamma[i] for i, r in enumerate(rewards)])
    loss = (-disc.sum(0)).mean()
    if reg_weight > 0:
        loss = loss + reg_weight * pol.regularization_loss()
    loss.backward()
    lins, drops = pol_layers(pol)
    out = dict(states=torch.stack(states).detach().numpy().copy(), loss=float(loss),
               grad=torch.cat([t.grad.reshape(-1) for m in lins for t in (m.weight, m.bias)]).numpy().copy())
    for l, m in enumerate(drops):
        out['glogit%d' % l] = m.logit_p.grad.numpy().copy()
    return out


def hard_of(rec, n_it, H, n_drop):
    """[iterations, H, B, h] per policy layer from the call-ordered recording (step-major, layer-minor)."""
    assert len(rec.b) == n_it * H * n_drop, (len(rec.b), n_it, H, n_drop)
    return [np.stack([np.stack([f(rec.b[(it * H + t) * n_drop + l]) for t in range(H)]) for it in range(n_it)]).astype(np.uint8)
            for l in range(n_drop)]


def make_iter_case(name, act, B, H, seed, mm_groups=None, resample_policy=False, D=4, U=1, hid=(32, 32)):
    print('[concrete policy] %s' % name)
    rew = mg._cartpole()
    dyn, pol, x0 = build(D, U, list(hid), act, rew, 10.0, seed, B)
    seed_t = torch.tensor([seed + 77])
    dyn.resample(seed=seed_t)
    pol.resample(seed=seed_t)
    torch.manual_seed(seed + 5)
    pol.model.fc_nonlin.z.data = torch.randn_like(pol.model.fc_nonlin.z)
    z_mm, z_rr = torch.randn(H + B, D), torch.randn(H + B, 1)
    gamma = [1.0 / H] * H
    mm = mm_groups is not None
    d = mg.capture_inputs(dyn, pol, x0, H, gamma, mm, mm, mm_groups, z_mm, z_rr, True, False, rew)
    describe_policy(d, pol, act)
    detach_state(dyn, pol)
    dyn64, pol64, rew64 = copy.deepcopy(dyn).double(), copy.deepcopy(pol).double(), copy.deepcopy(rew).double()
    dyn64.reward_func = rew64
    kw = dict(mm_states=mm, mm_rewards=mm, mm_groups=mm_groups, z_mm=z_mm, z_rr=z_rr, resample_policy=resample_policy)
    with _Draws() as rec:
        r32 = one_iteration(dyn, pol, x0, H, gamma, kw)
    with _Draws(replay=rec) as rec64:
        r64 = one_iteration(dyn64, pol64, x0.double(), H, gamma, dict(kw, z_mm=z_mm.double(), z_rr=z_rr.double()))
    assert len(rec64.b) == len(rec.b) and len(rec64.u) == len(rec.u)
    n_drop = len(hid)
    for l, h in enumerate(hard_of(rec, 1, H, n_drop)):
        d['pol_hard%d' % l] = h
    if resample_policy:
        assert len(rec.u) == H * n_drop
        for l in range(n_drop):
            d['pol_u%d' % l] = np.stack([f(rec.u[t * n_drop + l]) for t in range(H)])
    else:
        assert not rec.u
    d['resample_policy'] = int(resample_policy)
    for k, v in r32.items():
        d['ref32_' + k] = np.asarray(v, dtype=np.float32)
    for k, v in r64.items():
        d['ref64_' + k] = np.asarray(v, dtype=np.float64)
    for k in ['grad'] + ['glogit%d' % l for l in range(n_drop)]:
        print('   %-8s |g32 - g64| / |g64| = %.2e, |g64| = %.2e' % (
            k, np.linalg.norm(r32[k] - r64[k]) / np.linalg.norm(r64[k]), np.linalg.norm(r64[k])))
    return d


def make_mcp_case(name, act, B, H, n_iters, seed, reg_weight, lr=1e-3, clip=1.0, D=4, U=1, hid=(32, 32)):
    """The real algorithms.mc_pilco for n_iters iterations (fp32), the frozen randomness captured at its first rollout."""
    print('[concrete policy mc_pilco] %s' % name)
    rew = mg._cartpole()
    dyn, pol, x0 = build(D, U, list(hid), act, rew, 10.0, seed, B)
    opt = torch.optim.Adam(pol.parameters(), lr)
    cap, losses = {}, []
    orig_rollout = utils.rollout
    n_drop = len(hid)

    def wrapped(states, dynamics, policy, steps, **kw):
        if 'd' not in cap:
            gamma = [1.0 / steps] * steps
            detach_state(dynamics, policy)
            cap['d'] = mg.capture_inputs(dynamics, policy, states, steps, gamma, kw['mm_states'], kw['mm_rewards'],
                                         kw['mm_groups'], kw['z_mm'], kw['z_rr'], True, False, rew)
            describe_policy(cap['d'], policy, act)
            cap['m64'] = (copy.deepcopy(dynamics).double(), copy.deepcopy(policy).double(), copy.deepcopy(rew).double())
            cap['z'] = (kw['z_mm'].clone(), kw['z_rr'].clone())
            cap['n_before'] = len(rec.b)
        return orig_rollout(states, dynamics, policy, steps, **kw)

    utils.rollout = wrapped
    torch.manual_seed(seed + 5)
    try:
        with _Draws() as rec:
            algorithms.mc_pilco(x0, dyn, pol, H, opt, None, n_iters, maximize=True, clip_grad=clip, reg_weight=reg_weight,
                                on_iteration=lambda i, loss, *a: losses.append(float(loss)), resampling_period=99)
    finally:
        utils.rollout = orig_rollout
    d = cap['d']
    rec.b = rec.b[cap['n_before']:]        # (the draws of dynamics.resample() come first: eval-mode concrete dropout)
    for l, h in enumerate(hard_of(rec, n_iters, H, n_drop)):
        d['pol_hard%d' % l] = h
    d['resample_policy'] = 0
    lins, drops = pol_layers(pol)

    def results(pre, pol_, opt_, losses_, dtype):
        lins_, drops_ = pol_layers(pol_)
        lp = [t for m in lins_ for t in (m.weight, m.bias)]
        d[pre + 'mcp_losses'] = np.asarray(losses_, dtype=dtype)
        d[pre + 'mcp_final'] = torch.cat([p.detach().reshape(-1) for p in lp]).numpy().astype(dtype)
        d[pre + 'mcp_exp_avg_sq'] = torch.cat([opt_.state[p]['exp_avg_sq'].reshape(-1) for p in lp]).numpy().astype(dtype)
        for l, m in enumerate(drops_):
            d[pre + 'mcp_logit_final%d' % l] = m.logit_p.detach().numpy().astype(dtype)
            d[pre + 'mcp_logit_exp_avg_sq%d' % l] = opt_.state[m.logit_p]['exp_avg_sq'].numpy().astype(dtype)

    results('ref32_', pol, opt, losses, np.float32)
    # fp64: the loop body of algorithms/mc_pilco.py:86-216 on the captured modules, replaying the hard samples
    dyn64, pol64, rew64 = cap['m64']
    dyn64.reward_func = rew64
    dyn64.eval()
    pol64.train()
    opt64 = torch.optim.Adam(pol64.parameters(), lr)
    kw = dict(mm_states=False, mm_rewards=False, mm_groups=None, z_mm=cap['z'][0].double(), z_rr=cap['z'][1].double())
    losses64 = []
    with _Draws(replay=rec):
        for it in range(n_iters):
            opt64.zero_grad()
            r = one_iteration(dyn64, pol64, x0.double(), H, [1.0 / H] * H, kw, reg_weight)
            if it == 0:
                for k, v in r.items():
                    d['ref64_' + k] = np.asarray(v, dtype=np.float64)
            torch.nn.utils.clip_grad_norm_(pol64.parameters(), clip)
            opt64.step()
            losses64.append(r['loss'])
    results('ref64_', pol64, opt64, losses64, np.float64)
    d.update(mcp_lr=lr, mcp_reg_weight=reg_weight, mcp_clip=clip, mcp_n_iters=n_iters)
    print('   losses32 %s\n   losses64 %s' % (losses, losses64))
    for l in range(n_drop):
        print('   logit_p%d moved by %.2e' % (l, np.abs(d['ref64_mcp_logit_final%d' % l] - d['pol_logit_p%d' % l]).max()))
    return d


CASES = {
    'cp_iter_tanh': lambda: make_iter_case('cp_iter_tanh', TANH, 21, 4, seed=401),
    'cp_iter_relu_mmg': lambda: make_iter_case('cp_iter_relu_mmg', RELU, 24, 4, seed=402, mm_groups=2),
    'cp_iter_resample': lambda: make_iter_case('cp_iter_resample', SILU, 21, 4, seed=403, resample_policy=True),
    'cp_mcp_noreg': lambda: make_mcp_case('cp_mcp_noreg', TANH, 21, 4, 3, seed=404, reg_weight=0.0),
    'cp_mcp_reg': lambda: make_mcp_case('cp_mcp_reg', TANH, 21, 4, 3, seed=405, reg_weight=1e-3),
}


if __name__ == '__main__':
    mg.CASES = CASES
    if '--out' not in sys.argv:
        sys.argv += ['--out', os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'concrete_policy')]
    mg.main()
