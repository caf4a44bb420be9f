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


def cpu_leg(dims, Xc, Yc, N, batch, iters):
    """bench.cpu_baseline_bnn for any number of hidden layers: the oracle's step (torch autograd on the host + its Adam) on
    the same shapes; returns (iterations/s, threads used)."""
    from oracle import ref_torch as R
    nh = len(dims) - 2
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    W = [(torch.randn(dims[l + 1], dims[l]) / np.sqrt(dims[l]), torch.zeros(dims[l + 1])) for l in range(nh + 1)]
    lp = [torch.full((dims[l + 1],), 1.1) for l in range(nh)]
    params = [t for pair in W for t in pair] + lp
    for p in params:
        p.requires_grad_(True)
    ms = [torch.zeros_like(p) for p in params]
    vs = [torch.zeros_like(p) for p in params]

    def cpu_it(i):
        idx = torch.randint(0, N, (batch,))
        us = [torch.rand(batch, dims[l + 1]) for l in range(nh)]
        for p in params:
            p.grad = None
        with torch.no_grad():
            hs = [torch.bernoulli(torch.full((batch, dims[l + 1]), 0.7)) for l in range(nh)]
        loss, _, _ = R.bnn_loss(W, lp, [0.1] * nh, [0.5] * nh, [1.0] * nh, Xc[idx], Yc[idx], us, hs, N)
        loss.backward()
        with torch.no_grad():
            for p, mm, vv in zip(params, ms, vs):
                R.adam_step(p, p.grad, mm, vv, i + 1, 1e-4)

    for i in range(3):
        cpu_it(i)
    t0 = time.perf_counter()
    for i in range(iters):
        cpu_it(3 + i)
    return iters / (time.perf_counter() - t0), torch.get_num_threads()


def prof_phases(step, nh):
    """{phase: shader-clock cycles} of workgroup 0 of the plan's last forward + backward launch (either kernel form stamps
    the same places; the scratch region is the workspace's last 4 KB, the stamps its second half)."""
    torch.cuda.synchronize()
    ws = step.ws.cpu().numpy()
    st = ws[len(ws) - 2048:len(ws) - 2048 + 21 * 8].view(np.int64)
    marks = [(0, 'entry'), (1, 'gather')] + [(2 + l, 'fwd L%d' % l) for l in range(nh)] + [(10, 'head'), (11, 'loss')]
    marks += [(12 + k, 'bwd L%d' % (nh - k)) for k in range(nh)] + [(20, 'end')]
    out, prev = {}, None
    for k, name in marks:
        if prev is not None:
            out[name] = int(st[k] - st[prev])
        prev = k
    out['total'] = int(st[20] - st[0])
    return out


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
    ap.add_argument('--hidden-layers', type=int, default=2, help='hidden layers, all --hidden wide (3 x 512: the spill form)')
    ap.add_argument('--form', default='auto', choices=['auto', 'resident', 'spill'],
                    help="kernel form of the forward + backward launch (BnnStep's form; the line reports what the plan took)")
    a = ap.parse_args()
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import engine as E
    dev = torch.device('cuda:0')
    D, U, h = 4, 1, a.hidden
    torch.manual_seed(0)
    np.random.seed(0)
    bern = a.dropout == 'bernoulli'
    nh = a.hidden_layers
    dims = [a.n_in] + [h] * nh + [2 * a.n_out]
    Xn = torch.randn(a.N, a.n_in, device=dev)
    Yn = torch.randn(a.N, a.n_out, device=dev)
    parts = []
    for l in range(nh + 1):
        parts += [torch.randn(dims[l + 1], dims[l], device=dev).reshape(-1) / np.sqrt(dims[l]),
                  torch.zeros(dims[l + 1], device=dev)]
        if l < nh and not bern:
            parts.append(torch.full((dims[l + 1],), 1.1, device=dev))
    flat = torch.cat(parts).contiguous()
    if bern:
        step = E.BnnStep(dims, [0.0] * nh, [0.5] * nh, [0.0] * nh, a.batch, a.N, 1.0, device=dev, bernoulli_keep=[0.9] * nh,
                         form=a.form)
    else:
        step = E.BnnStep(dims, [0.1] * nh, [0.5] * nh, [1.0] * nh, a.batch, a.N, 1.0, device=dev, form=a.form)
    m, v, g = torch.zeros_like(flat), torch.zeros_like(flat), torch.empty_like(flat)
    sum_h = nh * h

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
    if nh == 2:
        from bench import cpu_baseline_bnn
        rate_cpu, cores = cpu_baseline_bnn(dims, h, Xn.cpu(), Yn.cpu(), a.N, a.batch, a.cpu_iters)
    else:
        rate_cpu, cores = cpu_leg(dims, Xn.cpu(), Yn.cpu(), a.N, a.batch, a.cpu_iters)
    # PMBRL_BNN_PROF=1: the cycle stamps workgroup 0 of the last forward + backward launch left in the plan's scratch
    # (pmbrl_bnn_train_steps), as the cycles between them: gather, the forward layers, head, loss, the backward layers
    phases = None
    if os.environ.get('PMBRL_BNN_PROF'):
        phases = prof_phases(step, nh)
    print(json.dumps(dict(metric='bnn_training_iterations_per_sec', value=a.iters / dt, unit='it/s',
                          us_per_iteration=dt / a.iters * 1e6, launches_per_iteration=2,
                          us_per_iteration_runs=[r / a.iters * 1e6 for r in runs], form=step.form,
                          **(dict(phase_cycles=phases) if phases else {}),
                          unfused=dict(value=1.0 / dt_unfused, us_per_iteration=dt_unfused * 1e6, launches_per_iteration=10),
                          config=dict(workload='dynamics BNN %s, minibatch %d of %d rows, %s dropout, '
                                               'Gaussian NLL + regulariser, Adam' % (dims, a.batch, a.N, a.dropout)),
                          cpu_baseline=dict(value=rate_cpu, unit='it/s', cores=cores,
                                            kind='port', sample='%d iterations' % a.cpu_iters))))


if __name__ == '__main__':
    main()
