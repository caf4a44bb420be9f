#!/usr/bin/env python
"""What a torch callable as the reward costs, at the C2 shape (2 500 rows, H = 40, 2 x 200 networks, cart-pole widths):
milliseconds per mc_pilco iteration of

  analytic   rewards.CartpoleReward: the reward launch of the library (pm_reward_all_kernel)
  callable   the same reward written as a plain torch function of (states, actions): evaluated by the host between
             pmbrl_rollout_fwd and pmbrl_rollout_rewards, its Jacobians by one torch.autograd.grad
  stepwise   the callable on the stepwise rollout (what served any callable before: rollout(on_pol_eval=...) + the
             reference's loss + backward + clip + Adam in torch), for scale: fewer blocks, it is a hundred times slower

Blocks of --iters iterations (one mc_pilco call each, its set-up included in both cases alike), timed from a device
synchronise to a device synchronise, analytic and callable alternating block by block.  Also counts the device launches
of the torch reward and of its backward (torch.profiler; None where the profiler cannot be had).  One JSON line.

    python tools/external_reward_cost.py [--blocks 25] [--iters 10] [--warmup 2] [--stepwise-blocks 3]
"""
import argparse
import json
import math
import os
import sys
import time
from functools import partial

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prob_mbrl_amd as pm  # noqa: E402

DEV = 'cuda:0'
D, U, H, B = 4, 1, 40, 2500


def cartpole_reward_fn(pole_length=0.5, q=16.0, r=1e-4):
    """envs/cartpole/env.py:41-86 as a user would write it: tip position from (x, theta), distance to the upright
    target, exp(-cost / 2)."""
    l = float(pole_length)

    def fn(x, u):
        dx = (x[:, 0:1] + l * torch.sin(x[:, 2:3])) / (2 * l)                 # target tip: (0, l): theta = pi
        dy = (-l * torch.cos(x[:, 2:3]) - l) / (2 * l)
        return torch.exp(-0.5 * (q * (dx * dx + dy * dy) + r * (u * u).sum(-1, keepdim=True)))
    return fn


def build(reward):
    torch.manual_seed(0)
    np.random.seed(0)
    dyn = pm.models.DynamicsModel(
        pm.models.mlp(D + U, 2 * D, [200, 200], dropout_layers=[pm.models.CDropout(0.1 * np.ones(200)) for _ in range(2)],
                      nonlin=torch.nn.ReLU),
        reward_func=reward, output_density=pm.models.DiagGaussianDensity(D)).float()
    pol = pm.models.Policy(
        pm.models.mlp(D, 2 * U, [200, 200], dropout_layers=[pm.models.BDropout(0.1) for _ in range(2)], nonlin=torch.nn.ReLU,
                      output_nonlin=partial(pm.models.DiagGaussianDensity, U)),
        np.array([10.0], np.float32), np.array([-10.0], np.float32)).float()
    dyn.set_dataset(torch.randn(300, D + U), 0.01 * torch.randn(300, D))
    dyn, pol = dyn.to(DEV), pol.to(DEV)
    return dyn, pol, torch.optim.Adam(pol.parameters(), 1e-4)


def launches_of(fn):
    """(device launches of r = fn(x, u), of autograd.grad(r.sum(), (x, u))) at the C2 row count, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        x = torch.randn(H * B, D, device=DEV, requires_grad=True)
        u = torch.randn(H * B, U, device=DEV, requires_grad=True)
        for _ in range(2):
            torch.autograd.grad(fn(x, u).sum(), (x, u))
        counts = []
        for part in ('fwd', 'bwd'):
            r = fn(x, u) if part == 'bwd' else None
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                if part == 'fwd':
                    fn(x, u)
                else:
                    torch.autograd.grad(r.sum(), (x, u))
                torch.cuda.synchronize()
            counts.append(sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')))
        return counts
    except Exception as e:      # noqa: BLE001 -- a count that cannot be had is reported as such
        return 'unavailable: %s' % e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=25)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--stepwise-blocks', type=int, default=3)
    ap.add_argument('--stepwise-iters', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs a HIP device')
    fn = cartpole_reward_fn()
    cases = {'analytic': build(pm.rewards.CartpoleReward(pole_length=torch.tensor(0.5))), 'callable': build(fn)}
    x0 = 0.1 * torch.randn(B, D, device=DEV)
    # the two rewards are the same function: the first iteration's losses agree
    first = {}
    for k, (dyn, pol, opt) in cases.items():
        seen = []
        torch.manual_seed(1)      # (the same dropout masks in both: mc_pilco draws them from torch's generator)
        pm.algorithms.mc_pilco(x0, dyn, pol, H, opt, None, 1, on_iteration=lambda i, loss, *r: seen.append(float(loss)),
                               frozen_noise=dict(z_mm=torch.zeros(H + B, D), z_rr=torch.zeros(H + B, 1)))
        first[k] = seen[0] if seen else math.nan

    def block(k, n):
        dyn, pol, opt = cases[k]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pm.algorithms.mc_pilco(x0, dyn, pol, H, opt, None, n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for k in cases:
        for _ in range(a.warmup):
            block(k, a.iters)
    times = {k: [] for k in cases}
    for _ in range(a.blocks):
        for k in cases:
            times[k].append(block(k, a.iters))
    # the stepwise rollout with the callable: rollout(on_pol_eval=identity) + loss + backward + clip + step, in torch
    dyn, pol, opt = build(fn)
    dyn.eval()
    step_ms = []

    def stepwise():
        states, actions, rewards = pm.utils.rollout(x0, dyn, pol, H, resample_state_noise=False, resample_action_noise=False,
                                                    on_pol_eval=lambda i, s, u: (s, u))
        loss = -torch.stack(rewards).sum(0).mean() / H
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(pol.parameters(), 1.0)
        opt.step()

    stepwise()
    for _ in range(a.stepwise_blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.stepwise_iters):
            stepwise()
        torch.cuda.synchronize()
        step_ms.append((time.perf_counter() - t0) * 1e3 / a.stepwise_iters)
    out = dict(shape=dict(rows=B, H=H, pol=[D, 200, 200, 2 * U], dyn=[D + U, 200, 200, 2 * D]), blocks=a.blocks,
               iters_per_block=a.iters, first_loss=first, reward_launches_fwd_bwd=launches_of(fn))
    times['stepwise'] = step_ms
    for k, t in times.items():
        t = np.asarray(t)
        out[k] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()), blocks=int(t.size))
    out['callable_minus_analytic_ms'] = out['callable']['ms_median'] - out['analytic']['ms_median']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
