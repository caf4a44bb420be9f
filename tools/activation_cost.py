#!/usr/bin/env python
"""What hidden layers other than ReLU cost on the device, at the C2 shape (2 500 rows, H = 40, 2 x 200 networks, cart-pole
widths): a full iteration -- forward sweep, rewards, adjoint sweep, dW GEMM, clip and Adam -- on the general kernel
family with

  relu   ReLU networks forced onto the general family (PMBRL_FLAG_FORCE_GENERIC): activity bits for the adjoint
  tanh   both networks Tanh (the family's ACT instances: act' x mask / keep per hidden unit and row-step, 4 bytes)
  silu   both networks SiLU
  sin | exp | sinlu | hhsinlu | none   likewise (prob_mbrl_amd.activations.NAMES)

--acts names the cases to run (default: all eight; relu is always among them).
Blocks of --iters iterations, timed from a device synchronise to a device synchronise, the cases interleaved
block by block; prints the median, min and max milliseconds per iteration of each and the extra stash bytes per
row-step as one JSON line.

    python tools/activation_cost.py [--acts relu,sin,hhsinlu] [--blocks 25] [--iters 10] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from prob_mbrl_amd import activations as ACT  # noqa: E402
from prob_mbrl_amd import problem as PB  # noqa: E402


def case(d, act):
    d = dict(d)
    d['pol_act'] = d['dyn_act'] = act
    eng, args, _ = PB.engine_from_problem(d, force_generic=True)
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
    ap.add_argument('--blocks', type=int, default=25)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--acts', type=str, default=','.join(ACT.NAMES), help='comma list of %s' % ', '.join(ACT.NAMES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs a HIP device')
    d = PB.synthetic_problem('cartpole_nomm')
    names = ['relu'] + [k for k in a.acts.split(',') if k != 'relu']
    cases = {k: case(d, ACT.NAMES[k]) for k in names}
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
    tiles = sum((h + 15) // 16 for p in ('pol', 'dyn') for h in PB.layer_dims(d, p)[1:-1])
    out = dict(shape=dict(rows=int(d['x0'].shape[0]), H=int(d['H']), pol=PB.layer_dims(d, 'pol'),
                          dyn=PB.layer_dims(d, 'dyn')), blocks=a.blocks, iters_per_block=a.iters,
               stash_bytes_per_row_step=dict(relu=2 * tiles, other=64 * tiles))
    for k, (eng, _) in cases.items():
        t = np.asarray(times[k])
        out[k] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()),
                      fast=eng.info['fast'], reg=eng.info['reg'], precision=eng.info['precision'],
                      valid_steps=eng.valid_steps())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
