#!/usr/bin/env python
"""Throughput of the BNN training step: utils.train_regressor's iteration body on
the example shape (dynamics model 5 -> 200 -> 200 -> 8, minibatch 100, Adam), device path vs the
torch-CPU oracle.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--N', type=int, default=1000)
    ap.add_argument('--hidden', type=int, default=200)
    ap.add_argument('--cpu-iters', type=int, default=60)
    ap.add_argument('--dropout', default='concrete', choices=['concrete', 'bernoulli'],
                    help='dropout kind of both hidden layers (bernoulli: fixed keep probability 0.9)')
    ap.add_argument('--n-in', type=int, default=5)
    ap.add_argument('--n-out', type=int, default=4)
    ap.add_argument('--repeats', type=int, default=1, help='timed repetitions of the fused leg (all reported)')
    a = ap.parse_args()
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import engine as E
    dev = torch.device('cuda:0')
    D, U, h = 4, 1, a.hidden
    torch.manual_seed(0)
    np.random.seed(0)
    bern = a.dropout == 'bernoulli'
    dims = [a.n_in, h, h, 2 * a.n_out]
    Xn = torch.randn(a.N, a.n_in, device=dev)
    Yn = torch.randn(a.N, a.n_out, device=dev)
    parts = []
    for l in range(3):
        parts += [torch.randn(dims[l + 1], dims[l], device=dev).reshape(-1) / np.sqrt(dims[l]),
                  torch.zeros(dims[l + 1], device=dev)]
        if l < 2 and not bern:
            parts.append(torch.full((dims[l + 1],), 1.1, device=dev))
    flat = torch.cat(parts).contiguous()
    if bern:
        step = E.BnnStep(dims, [0.0, 0.0], [0.5, 0.5], [0.0, 0.0], a.batch, a.N, 1.0, device=dev, bernoulli_keep=[0.9, 0.9])
    else:
        step = E.BnnStep(dims, [0.1, 0.1], [0.5, 0.5], [1.0, 1.0], a.batch, a.N, 1.0, device=dev)
    m, v, g = torch.zeros_like(flat), torch.zeros_like(flat), torch.empty_like(flat)
    sum_h = 2 * h

    def it(i):
        idx = torch.randint(0, a.N, (a.batch,), device=dev, dtype=torch.int32)
        u = torch.rand(a.batch * sum_h, device=dev)
        b = torch.rand(a.batch * sum_h, device=dev)
        step.loss_grad(Xn, Yn, idx, flat, u, b, g)
        E.clip_adam(flat, g, m, v, i + 1, 1e-4, max_norm=None)

    # round 5: whole iterations in two launches each, queued 100 at a time by one library call (pmbrl_bnn_train_steps:
    # in-kernel dropout noise, Adam on the device; the minibatch rows of a chunk drawn by ONE torch.randint); the
    # launch-per-piece path above is kept as `unfused` in the line
    for i in range(20):
        it(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.iters // 4):
        it(20 + i)
    torch.cuda.synchronize()
    dt_unfused = (time.perf_counter() - t0) / (a.iters // 4)
    stepc = torch.zeros(1, dtype=torch.int64, device=dev)
    CH = 100

    def chunk(k):
        idx = torch.randint(0, a.N, (CH, a.batch), device=dev, dtype=torch.int32)
        step.train_steps(Xn, Yn, idx, flat, m, v, stepc, 1e-4, seed=7, first_step=k * CH)

    chunk(0)
    torch.cuda.synchronize()
    n_chunks = max(1, a.iters // CH)
    runs = []
    for r in range(a.repeats):
        t0 = time.perf_counter()
        for k in range(n_chunks):
            chunk(1 + r * n_chunks + k)
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    dt = float(np.median(runs))
    a.iters = n_chunks * CH
    assert bool(torch.isfinite(flat).all()) and int(stepc.item()) == (a.repeats * n_chunks + 1) * CH
    # CPU leg: bench.py's cpu_baseline code times the oracle's step on the host (bounded sample)
    from bench import cpu_baseline_bnn
    rate_cpu, cores = cpu_baseline_bnn(dims, h, Xn.cpu(), Yn.cpu(), a.N, a.batch, a.cpu_iters)
    print(json.dumps(dict(metric='bnn_training_iterations_per_sec', value=a.iters / dt, unit='it/s',
                          us_per_iteration=dt / a.iters * 1e6, launches_per_iteration=2,
                          us_per_iteration_runs=[r / a.iters * 1e6 for r in runs],
                          unfused=dict(value=1.0 / dt_unfused, us_per_iteration=dt_unfused * 1e6, launches_per_iteration=10),
                          config=dict(workload='dynamics BNN %s, minibatch %d of %d rows, %s dropout, '
                                               'Gaussian NLL + regulariser, Adam' % (dims, a.batch, a.N, a.dropout)),
                          cpu_baseline=dict(value=rate_cpu, unit='it/s', cores=cores,
                                            kind='port', sample='%d iterations' % a.cpu_iters))))


if __name__ == '__main__':
    main()
