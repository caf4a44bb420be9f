#!/usr/bin/env python
"""Host-side cost of a sharded iteration: the separate calls against the fused tail.

Two ranks on ONE device (gloo for bootstrap, PMBRL_P2P=1: the one-hop peer-to-peer exchange is the gradient transport --
RCCL refuses two ranks on one GPU), each holding the rows of bench.py's flagship configuration (weak scaling).  The
iteration body is bench.py's Leg.step:
  separate   forward, weighted_sum, backward, all-reduce of the gradient, clip_adam            (five library calls)
  fused      forward, backward with the optimiser and the collective inside                    (two library calls;
             Engine.attach_grad_comm -> pmbrl_plan_set_grad_comm)
Blocks of --steps iterations between barrier + synchronize, the two forms by turns so that both see the same clocks;
per block the slower rank counts.  Prints the median, minimum and maximum ms per iteration of both and their ratio as
one JSON line (rank 0).

    python tools/bench_sharded_tail.py [--config cartpole_nomm] [--steps 20] [--blocks 25] [--warmup 5]
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Leg:
    def __init__(self, d, dev, Bg, row_offset, transport, fused):
        import torch
        from prob_mbrl_amd import engine as E
        from prob_mbrl_amd import problem as PB
        self.E, self.transport, self.fused = E, transport, fused
        self.B = d['x0'].shape[0]
        self.eng, self.args, _ = PB.engine_from_problem(d, dev, B_global=Bg, row_offset=row_offset)
        self.gw = torch.tensor(PB.loss_weights(d, Bg)[:, :self.B].copy(), device=dev)
        self.params = self.args['pol_flat'].clone()
        self.params0 = self.params.clone()
        self.args['pol_flat'] = self.params
        self.m, self.v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.loss_buf = torch.zeros(1, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.n = 0
        if fused:
            self.eng.attach_grad_comm(transport)
            self.adam = dict(params=self.params, exp_avg=self.m, exp_avg_sq=self.v, step=self.step_dev, lr=1e-4,
                             betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, loss_out=self.loss_buf)

    def step(self):
        self.n += 1
        if self.fused:
            self.eng.forward(**self.args)
            self.eng.backward(self.gw, adam=self.adam)
            return
        _, _, R = self.eng.forward(**self.args)
        self.eng.weighted_sum(R, self.gw, out=self.loss_buf)
        g, _, _ = self.eng.backward(self.gw)
        self.transport.allreduce_(g)
        self.E.clip_adam(self.params, g, self.m, self.v, self.n, 1e-4, max_norm=1.0)

    def restart(self):
        self.params.copy_(self.params0)
        self.m.zero_()
        self.v.zero_()
        self.step_dev.zero_()
        self.n = 0


def worker(rank, world, port, a, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['PMBRL_P2P'] = '1'
    import torch
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from prob_mbrl_amd import _lib
        from prob_mbrl_amd import distributed as D
        from prob_mbrl_amd import problem as PB
        dev = torch.device('cuda:0')
        torch.cuda.set_device(dev)
        d = PB.synthetic_problem(a.config, seed=0, data_seed=rank)
        B = d['x0'].shape[0]
        tr = D.tail_transport(dist.group.WORLD, dev)
        assert isinstance(tr, D.P2PComm), 'the peer-to-peer transport is what this tool measures'
        legs = dict(separate=Leg(d, dev, B * world, rank * B, tr, False), fused=Leg(d, dev, B * world, rank * B, tr, True))

        def sync():
            torch.cuda.synchronize()
            dist.barrier()
            torch.cuda.synchronize()

        for leg in legs.values():
            for _ in range(a.warmup):
                leg.step()
        sync()
        ms = dict(separate=[], fused=[])
        for _ in range(a.blocks):
            for name, leg in legs.items():
                leg.restart()
                sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    leg.step()
                sync()
                t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                ms[name].append(1e3 * float(t[0]) / a.steps)
        for leg in legs.values():
            assert leg.eng.valid_steps() == int(d['H']) and bool(torch.isfinite(leg.params).all())
        assert int(legs['fused'].step_dev.item()) == a.steps and legs['fused'].eng.tail_calls() > 0
        assert not tr.failed()
        # (the same work: both forms end a block on the same parameters up to the host / device bias corrections)
        dp = float((legs['fused'].params - legs['separate'].params).abs().max())
        if rank == 0:
            res = dict(tool='bench_sharded_tail', config=a.config, ranks=world, rows_per_rank=B, steps=a.steps,
                       blocks=a.blocks, build_id=_lib.load().pmbrl_build_id().decode(), max_param_diff=dp)
            for name in ms:
                res[name + '_ms'] = dict(median=float(np.median(ms[name])), min=float(np.min(ms[name])),
                                         max=float(np.max(ms[name])))
            res['fused_over_separate'] = res['fused_ms']['median'] / res['separate_ms']['median']
            out.put(res)
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--config', default='cartpole_nomm')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, 2, port, a, out)) for r in range(2)]
    for p in procs:
        p.start()
    import queue
    res, deadline = None, time.monotonic() + 600
    try:
        while res is None and time.monotonic() < deadline and all(p.exitcode in (None, 0) for p in procs):
            try:
                res = out.get(timeout=0.5)
            except queue.Empty:
                pass        # (a worker that died ends the wait: its exit code is checked above)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    if res is None:
        print('bench_sharded_tail: no result (worker exit codes %s)' % [p.exitcode for p in procs], file=sys.stderr)
        return 1
    print(json.dumps(res))
    return 0 if all(p.exitcode == 0 for p in procs) else 1


if __name__ == '__main__':
    sys.exit(main())
