#!/usr/bin/env python
"""Generate the fixtures tests/golden/layer_norm/ln_*.npz: the REAL reference's utils.rollout and algorithms.mc_pilco
with networks built by models.mlp(layer_norm=True) (models/core.py:56-58: a torch.nn.LayerNorm between every hidden Linear
and its activation; ln*.weight at ones, ln*.bias drawn by biases_initializer).  Runs through tools/make_golden.py's import
shims; no existing fixture is touched.

The policy's dropout is the reference's default fixed-rate BDropout, the dynamics model's is eval-mode concrete dropout, as
in tools/make_golden.py's rollout cases: nothing is drawn inside a rollout, so the same modules switched to .double() give
the ref64_* results on the same masks.  gamma is moved off its initial ones (a gamma of exactly one would hide a missing
factor).

Keys, beside those of tools/make_golden.py's rollout fixtures (capture_inputs):  pol_act, dyn_act;  pol_ln_g{l}, pol_ln_b{l},
pol_ln_eps{l} and dyn_ln_* for every layer-normalised hidden layer;  ref32_* / ref64_*: states, loss, grad (ALL policy
parameters, flat, in the order of policy.parameters(): fc0.weight, fc0.bias, ln0.weight, ln0.bias, fc1.weight, ...);  the
mc_pilco case: mcp_* and ref32_mcp_* / ref64_mcp_* losses, final, exp_avg_sq (the same order).

Usage:  python tools/make_golden_layer_norm.py [--out tests/golden/layer_norm] [--only name]
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

RELU, TANH = 0, 1
MODULES = {RELU: torch.nn.ReLU, TANH: torch.nn.Tanh}
f = lambda t: t.detach().double().cpu().numpy().copy()  # noqa: E731


def build(D, U, hid, rew, maxU, seed, B, pol_act, pol_ln, dyn_ln, n_data=300, y_scale=0.01):
    """tools/make_golden.py's build() with layer_norm on the policy and / or the dynamics model."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    dyn_model = models.mlp(D + U, 2 * D, hid, dropout_layers=[models.modules.CDropout(0.1 * np.ones(h)) for h in hid],
                           nonlin=torch.nn.ReLU, layer_norm=dyn_ln)
    dyn = models.DynamicsModel(dyn_model, reward_func=rew, output_density=models.DiagGaussianDensity(D)).float()
    pol_model = models.mlp(D, 2 * U, hid, dropout_layers=[models.modules.BDropout(0.1) for _ in hid], nonlin=MODULES[pol_act],
                           output_nonlin=partial(models.DiagGaussianDensity, U), layer_norm=pol_ln)
    maxU_t = np.asarray(maxU, dtype=np.float32).reshape(-1)
    pol = models.Policy(pol_model, maxU_t, -maxU_t).float()
    dyn.set_dataset(torch.randn(n_data, D + U), y_scale * torch.randn(n_data, D))
    with torch.no_grad():
        for net in (pol, dyn):
            for m in net.modules():
                if isinstance(m, torch.nn.LayerNorm):
                    m.weight.add_(0.3 * torch.randn_like(m.weight))
    dyn.eval()
    pol.train()
    torch.manual_seed(seed + 1000)
    x0 = 0.1 * torch.randn(B, D)
    with torch.no_grad():      # sizes the [B, h] / [B, D] buffers
        utils.rollout(x0, dyn, pol, 1, resample_state_noise=False, resample_action_noise=False)
    return dyn, pol, x0


def detach_state(*mods):
    """p and concrete_noise of a CDropout carry the graph of the last resample(): drop it before a deepcopy (an eval-mode
    model applies concrete_noise detached anyway)."""
    for mod in mods:
        for m in mod.modules():
            if isinstance(m, models.modules.CDropout):
                m.concrete_noise = m.concrete_noise.detach()
                m._buffers['p'] = m._buffers['p'].detach() if 'p' in m._buffers else m.p.detach()


def describe_norms(d, pol, dyn, pol_act):
    d['pol_act'], d['dyn_act'] = pol_act, RELU
    for pre, net in (('pol', pol), ('dyn', dyn)):
        for name, m in net.model._modules.items():
            if isinstance(m, torch.nn.LayerNorm):
                l = int(name[2:])
                d['%s_ln_g%d' % (pre, l)], d['%s_ln_b%d' % (pre, l)], d['%s_ln_eps%d' % (pre, l)] = f(m.weight), f(m.bias), m.eps


def one_iteration(dyn, pol, x0, H, gamma, kw):
    pol.zero_grad()
    dyn.zero_grad()
    states, actions, rewards = utils.rollout(x0, dyn, pol, H, resample_state_noise=False, resample_action_noise=False, **kw)
    disc = torch.stack([r * gamma[i] for i, r in enumerate(rewards)])
    loss = (-disc.sum(0)).mean()
    loss.backward()
    return dict(states=torch.stack(states).detach().numpy().copy(), loss=float(loss),
                grad=torch.cat([p.grad.reshape(-1) for p in pol.parameters()]).numpy().copy())


def make_iter_case(name, pol_act, B, H, seed, pol_ln=True, dyn_ln=False, mm_groups=None, D=4, U=1, hid=(24, 40)):
    print('[layer norm] %s' % name)
    rew = mg._cartpole()
    dyn, pol, x0 = build(D, U, list(hid), rew, 10.0, seed, B, pol_act, pol_ln, dyn_ln)
    seed_t = torch.tensor([seed + 77])
    dyn.resample(seed=seed_t)
    pol.resample(seed=seed_t)
    torch.manual_seed(seed + 5)
    pol.model.fc_nonlin.z.data = torch.randn_like(pol.model.fc_nonlin.z)
    z_mm, z_rr = torch.randn(H + B, D), torch.randn(H + B, 1)
    gamma = [1.0 / H] * H
    mm = mm_groups is not None
    d = mg.capture_inputs(dyn, pol, x0, H, gamma, mm, mm, mm_groups, z_mm, z_rr, True, False, rew)
    describe_norms(d, pol, dyn, pol_act)
    detach_state(dyn, pol)
    dyn64, pol64, rew64 = copy.deepcopy(dyn).double(), copy.deepcopy(pol).double(), copy.deepcopy(rew).double()
    dyn64.reward_func = rew64
    kw = dict(mm_states=mm, mm_rewards=mm, mm_groups=mm_groups, z_mm=z_mm, z_rr=z_rr)
    r32 = one_iteration(dyn, pol, x0, H, gamma, kw)
    r64 = one_iteration(dyn64, pol64, x0.double(), H, gamma, dict(kw, z_mm=z_mm.double(), z_rr=z_rr.double()))
    for k, v in r32.items():
        d['ref32_' + k] = np.asarray(v, dtype=np.float32)
    for k, v in r64.items():
        d['ref64_' + k] = np.asarray(v, dtype=np.float64)
    print('   names %s' % [n for n, _ in pol.model.named_parameters()])
    print('   grad |g32 - g64| / |g64| = %.2e, |g64| = %.2e' % (
        np.linalg.norm(r32['grad'] - r64['grad']) / np.linalg.norm(r64['grad']), np.linalg.norm(r64['grad'])))
    return d


def make_mcp_case(name, pol_act, B, H, n_iters, seed, lr=1e-3, clip=1.0, D=4, U=1, hid=(24, 40)):
    """The real algorithms.mc_pilco for n_iters iterations (fp32), the frozen randomness captured at its first rollout."""
    print('[layer norm mc_pilco] %s' % name)
    rew = mg._cartpole()
    dyn, pol, x0 = build(D, U, list(hid), rew, 10.0, seed, B, pol_act, True, False)
    opt = torch.optim.Adam(pol.parameters(), lr)
    cap, losses = {}, []
    orig_rollout = utils.rollout

    def wrapped(states, dynamics, policy, steps, **kw):
        if 'd' not in cap:
            gamma = [1.0 / steps] * steps
            cap['d'] = mg.capture_inputs(dynamics, policy, states, steps, gamma, kw['mm_states'], kw['mm_rewards'],
                                         kw['mm_groups'], kw['z_mm'], kw['z_rr'], True, False, rew)
            describe_norms(cap['d'], policy, dynamics, pol_act)
            detach_state(dynamics, policy)
            cap['m64'] = (copy.deepcopy(dynamics).double(), copy.deepcopy(policy).double(), copy.deepcopy(rew).double())
            cap['z'] = (kw['z_mm'].clone(), kw['z_rr'].clone())
        return orig_rollout(states, dynamics, policy, steps, **kw)

    utils.rollout = wrapped
    torch.manual_seed(seed + 5)
    try:
        algorithms.mc_pilco(x0, dyn, pol, H, opt, None, n_iters, maximize=True, clip_grad=clip,
                            on_iteration=lambda i, loss, *a: losses.append(float(loss)), resampling_period=99)
    finally:
        utils.rollout = orig_rollout
    d = cap['d']

    def results(pre, pol_, opt_, losses_, dtype):
        ps = list(pol_.parameters())
        d[pre + 'mcp_losses'] = np.asarray(losses_, dtype=dtype)
        d[pre + 'mcp_final'] = torch.cat([p.detach().reshape(-1) for p in ps]).numpy().astype(dtype)
        d[pre + 'mcp_exp_avg_sq'] = torch.cat([opt_.state[p]['exp_avg_sq'].reshape(-1) for p in ps]).numpy().astype(dtype)

    results('ref32_', pol, opt, losses, np.float32)
    # fp64: the loop body of algorithms/mc_pilco.py:86-216 on the captured modules
    dyn64, pol64, rew64 = cap['m64']
    dyn64.reward_func = rew64
    dyn64.eval()
    pol64.train()
    opt64 = torch.optim.Adam(pol64.parameters(), lr)
    kw = dict(mm_states=False, mm_rewards=False, mm_groups=None, z_mm=cap['z'][0].double(), z_rr=cap['z'][1].double())
    losses64 = []
    for it in range(n_iters):
        opt64.zero_grad()
        r = one_iteration(dyn64, pol64, x0.double(), H, [1.0 / H] * H, kw)
        if it == 0:
            for k, v in r.items():
                d['ref64_' + k] = np.asarray(v, dtype=np.float64)
        torch.nn.utils.clip_grad_norm_(pol64.parameters(), clip)
        opt64.step()
        losses64.append(r['loss'])
    results('ref64_', pol64, opt64, losses64, np.float64)
    d.update(mcp_lr=lr, mcp_clip=clip, mcp_n_iters=n_iters)
    print('   losses32 %s\n   losses64 %s' % (losses, losses64))
    return d


# the seeds keep every ReLU unit of the fp64 run -- the dynamics model's too -- more than 1e-4 from the kink
# (tests/test_layer_norm_oracle.py holds the fixtures to it)
CASES = {
    'ln_iter_tanh': lambda: make_iter_case('ln_iter_tanh', TANH, 21, 4, seed=515),
    'ln_iter_relu_mmg': lambda: make_iter_case('ln_iter_relu_mmg', RELU, 24, 4, seed=515, mm_groups=2),
    'ln_iter_dyn': lambda: make_iter_case('ln_iter_dyn', RELU, 21, 4, seed=603, pol_ln=False, dyn_ln=True),
    'ln_mcp': lambda: make_mcp_case('ln_mcp', TANH, 21, 4, 3, seed=530),
}


if __name__ == '__main__':
    mg.CASES = CASES
    if '--out' not in sys.argv:
        sys.argv += ['--out', os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'layer_norm')]
    mg.main()
