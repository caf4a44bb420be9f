"""fp64 oracle of the learned reward head (reward_func=None, a dynamics head 2 (D + 1) wide): the reference's
DynamicsModel.forward with D taken from prev_states (models/core.py:265-303), its rollout loop (utils/rollout.py:62-163)
and mc_pilco's loss (algorithms/mc_pilco.py:134-197).  The pieces that do not depend on the head come from
oracle.ref_torch."""
import os

import numpy as np
import torch

from oracle.ref_torch import (clamp_log_std, flat_grad, get_z_rnd, load_fixture, mlp_forward, mm_resample, policy_forward,
                              policy_params, policy_regularization, to_complex, value_forward)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'learned_reward')


def names(kind=None):
    """Fixtures of one kind: 'iter' (one rollout + gradient, frozen noise), 'step' (the same with the head's noise
    redrawn at every step: dyn_z [H, B, D + 1]), 'mcp' (iterations of the real mc_pilco); None: all."""
    ns = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith('.npz'))
    if kind is None:
        return ns
    pre = {'mcp': 'lr_mcp', 'step': 'lr_step'}.get(kind)
    return [n for n in ns if n.startswith(pre)] if pre else [n for n in ns if not n.startswith(('lr_mcp', 'lr_step'))]


def load(name):
    return load_fixture(os.path.join(GOLDEN, name + '.npz'))


def problem(d, dtype=torch.float64):
    """(x0, pol, dyn, meta, z_mm, z_rr, gamma) of a tests/golden/learned_reward fixture."""
    T = lambda k: torch.tensor(np.asarray(d[k]), dtype=dtype)  # noqa: E731
    nets = {}
    for pre in ('pol', 'dyn'):
        n = int(d[pre + '_n_layers'])
        nets[pre] = dict(weights=[(T('%s_W%d' % (pre, i)), T('%s_b%d' % (pre, i))) for i in range(n)],
                         masks=[T('%s_mask%d' % (pre, i)) for i in range(n - 1)],
                         keep=[float(s) for s in np.asarray(d[pre + '_keep'])], z=T(pre + '_z'),
                         angle_dims=[int(a) for a in np.asarray(d[pre + '_angle_dims'])])
    nets['pol'].update(scale=T('pol_scale'), bias=T('pol_bias'))
    nets['dyn'].update(mx=T('dyn_mx'), iSx=T('dyn_iSx'), my=T('dyn_my'), Sy=T('dyn_Sy'))
    G = int(d['mm_groups'])
    meta = dict(H=int(d['H']), mm_states=bool(d['mm_states']), mm_rewards=bool(d['mm_rewards']),
                mm_groups=G if G > 0 else None, maximize=bool(d['maximize']))
    z_mm = T('z_mm') if 'z_mm' in d else None
    z_rr = T('z_rr') if 'z_rr' in d else None
    return T('x0'), nets['pol'], nets['dyn'], meta, z_mm, z_rr, T('gamma')


def dynamics_forward(x, a, dyn, t=None):
    """(x + state change, reward) from one sample of DiagGaussianDensity(D + 1) with scaling (my, Sy)."""
    D = x.shape[-1]
    xa = torch.cat([x, a], -1)
    if len(dyn.get('angle_dims', [])) > 0:
        xa = to_complex(xa, dyn['angle_dims'])
    o = mlp_forward((xa - dyn['mx']) * dyn['iSx'], dyn['weights'], dyn['masks'], dyn['keep'], t)
    mean, log_std = o.split(D + 1, -1)
    log_std = clamp_log_std(log_std) + dyn['Sy'].log()
    B = x.shape[0]
    z = (dyn['z'][t] if dyn['z'].dim() == 3 else dyn['z'])[:B]     # [H, B, D + 1]: a fresh draw per step
    e = log_std.exp()
    zg = dyn.get('z_grad')
    # z_grad: the noise the derivative of the noise term is taken with.  The reference's sampler swaps the storage of the
    # saved z at every redraw (models/densities.py:113-117), so its autograd uses the LAST step's noise at every step;
    # None: each step's own noise (the device's gradient)
    noise = z * e if zg is None else ((z - zg[:B]) * e).detach() + zg[:B] * e
    y = mean * dyn['Sy'] + dyn['my'] + noise
    return x + y[:, :D], y[:, D:]


def rollout(x0, pol, dyn, H, mm_states=False, mm_rewards=False, mm_groups=None, z_mm=None, z_rr=None):
    B, D = x0.shape
    x, S, A, R = x0, [], [], []
    for i in range(H):
        a = policy_forward(x, pol, i)
        xn, r = dynamics_forward(x, a, dyn, i)
        G = mm_groups or 1
        if mm_states:
            xn = mm_resample(xn.view(G, -1, D), get_z_rnd(z_mm, i, B).view(G, -1, D),
                             1e-12 * torch.eye(D, dtype=x0.dtype)).view(-1, D)
        if mm_rewards:
            r = mm_resample(r.view(G, -1, 1), get_z_rnd(z_rr, i, B).view(G, -1, 1),
                            1e-12 * torch.eye(1, dtype=x0.dtype)).view(-1, 1)
        S.append(x)
        A.append(a)
        R.append(r)
        x = xn
    S.append(x)
    return S, A, R


def iteration(x0, pol, dyn, meta, gamma, z_mm=None, z_rr=None, n_steps=None, value=None, gamma_H=None, cvar_eps=0.0,
              reg_weight=0.0):
    """Rollout, the loss and its policy gradient (the discount vector stays the full horizon's on a truncated one);
    value / gamma_H: terminal-value bootstrap, cvar_eps, reg_weight: as algorithms/mc_pilco.py:136-154,193-194."""
    for p in policy_params(pol):
        p.requires_grad_(True)
        p.grad = None
    S, A, R = rollout(x0, pol, dyn, meta['H'] if n_steps is None else n_steps, meta['mm_states'], meta['mm_rewards'],
                      meta['mm_groups'], z_mm, z_rr)
    disc = torch.stack([r * gamma[i] for i, r in enumerate(R)])
    if value is not None:
        disc = torch.cat([disc, gamma_H * value_forward(S[-1], value).unsqueeze(0)], 0)
    returns = -disc.sum(0) if meta['maximize'] else disc.sum(0)
    if cvar_eps != 0:
        rd = returns.detach().numpy()
        returns = returns[rd < np.quantile(rd, cvar_eps)] if cvar_eps > 0 else returns[rd > np.quantile(rd, -cvar_eps)]
    loss = returns.mean()
    if reg_weight > 0:
        loss = loss + reg_weight * policy_regularization(pol)
    loss.backward()
    return loss.detach(), flat_grad(pol).detach().clone(), (S, A, R)
