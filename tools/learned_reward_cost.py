#!/usr/bin/env python
"""What a learned reward head costs on the device, at the C2 shape (2 500 rows, H = 40, 2 x 200 networks, cart-pole
widths): a full iteration -- forward sweep, rewards, adjoint sweep, dW GEMM, clip and Adam -- of

  learned   the learned reward head (PMBRL_REWARD_LEARNED; the general kernel family)
  generic   the analytic cart-pole reward on the same networks, forced onto the general family (PMBRL_FLAG_FORCE_GENERIC)
  default   the analytic reward with the plan the library chooses (the register-resident family)
  mixture   the analytic reward on a two-component Gaussian-mixture dynamics head (the general family)
  mixture_learned   the learned reward head on that mixture head: a density of D + 1 dimensions (left out, and said so,
            by a library that refuses the combination)

Blocks of --iters iterations, timed from a device synchronise to a device synchronise, the three cases interleaved
block by block; prints the median, min and max milliseconds per iteration of each as one JSON line.

    python tools/learned_reward_cost.py [--blocks 30] [--iters 10] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from prob_mbrl_amd import engine as E  # noqa: E402
from prob_mbrl_amd import problem as PB  # noqa: E402


def learned_problem(d, seed=1):
    """d with a dynamics head one output wider on each half ([means | mean_r | log-stds | ls_r]) and the reward
    column's scaling and noise."""
    d = dict(d)
    D = d['x0'].shape[1]
    n = int(d['dyn_n_layers'])
    W, b = np.asarray(d['dyn_W%d' % (n - 1)]), np.asarray(d['dyn_b%d' % (n - 1)])
    rng = np.random.default_rng(seed)
    wr = (0.05 * rng.standard_normal((2, W.shape[1]))).astype(np.float32)
    d['dyn_W%d' % (n - 1)] = np.concatenate([W[:D], wr[:1], W[D:], wr[1:]], 0)
    d['dyn_b%d' % (n - 1)] = np.concatenate([b[:D], [0.0], b[D:], [-1.0]]).astype(np.float32)
    d['dyn_my'] = np.concatenate([np.asarray(d['dyn_my']).reshape(-1), [0.5]]).astype(np.float32)
    d['dyn_Sy'] = np.concatenate([np.asarray(d['dyn_Sy']).reshape(-1), [0.8]]).astype(np.float32)
    z = np.asarray(d['dyn_z'])
    d['dyn_z'] = np.concatenate([z, rng.standard_normal(z.shape[:-1] + (1,)).astype(np.float32)], -1)
    return d


def mixture_problem(d, n=2, seed=2):
    """d (analytic or learned_problem's) with a mixture head of n components over its density: every component starts
    from the diagonal head's mean and log-std rows plus a small spread, [means | log-stds] component-fastest, then n
    logits and the log-temperature; frozen Gumbel noise, and a uniform and Gaussian noise per row-step."""
    d = dict(d)
    B, H = d['x0'].shape[0], int(d['H'])
    nl = int(d['dyn_n_layers'])
    W, b = np.asarray(d['dyn_W%d' % (nl - 1)]), np.asarray(d['dyn_b%d' % (nl - 1)])
    Dh = W.shape[0] // 2
    rng = np.random.default_rng(seed)
    rows = np.repeat(W, n, 0) + (0.02 * rng.standard_normal((2 * Dh * n, W.shape[1]))).astype(np.float32)
    extra = (0.05 * rng.standard_normal((n + 1, W.shape[1]))).astype(np.float32)
    d['dyn_W%d' % (nl - 1)] = np.concatenate([rows, extra], 0).astype(np.float32)
    d['dyn_b%d' % (nl - 1)] = np.concatenate([np.repeat(b, n), np.zeros(n + 1)]).astype(np.float32)
    d['dyn_gmm_n'] = n
    d['dyn_zpi'] = -np.log(-np.log(rng.uniform(1e-6, 1.0, (B, n)))).astype(np.float32)
    d['dyn_ucat'] = rng.uniform(0.0, 1.0, (H, B)).astype(np.float32)
    d['dyn_z'] = rng.standard_normal((H, B, Dh)).astype(np.float32)
    return d


def case(d, learned=False, force_generic=False):
    eng, args, _ = PB.engine_from_problem(d, force_generic=force_generic,
                                          reward_spec=E.LEARNED_REWARD if learned else None)
    B = d['x0'].shape[0]
    gw = torch.tensor(PB.loss_weights(d, B), device=eng.device)
    n = eng.n_pol_params
    adam = dict(params=args['pol_flat'], exp_avg=torch.zeros(n, device=eng.device),
                exp_avg_sq=torch.zeros(n, device=eng.device), step=torch.zeros(1, dtype=torch.int64, device=eng.device),
                lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0)

    def it():
        eng.forward(**args)
        eng.backward(gw, adam=adam)
    return eng, it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=30)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs a HIP device')
    d = PB.synthetic_problem('cartpole_nomm')
    cases = {'learned': case(learned_problem(d), learned=True), 'generic': case(d, force_generic=True),
             'default': case(d), 'mixture': case(mixture_problem(d))}
    refused = None
    try:
        cases['mixture_learned'] = case(mixture_problem(learned_problem(d)), learned=True)
    except Exception as e:      # (a library from before the combination was offered)
        refused = str(e)
    times = {k: [] for k in cases}
    for _, f in cases.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    for _ in range(a.blocks):
        for k, (_, f) in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
    out = dict(shape=dict(rows=int(d['x0'].shape[0]), H=int(d['H']), pol=PB.layer_dims(d, 'pol'),
                          dyn=PB.layer_dims(d, 'dyn')), blocks=a.blocks, iters_per_block=a.iters)
    for k, (eng, _) in cases.items():
        t = np.asarray(times[k])
        out[k] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()),
                      fast=eng.info['fast'], reg=eng.info['reg'], precision=eng.info['precision'],
                      valid_steps=eng.valid_steps())
    if refused:
        out['mixture_learned'] = dict(refused=refused)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
