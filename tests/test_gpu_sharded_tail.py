"""GPU (-m gpu): the iteration tail of a sharded run in ONE call -- pmbrl_rollout_bwd_adam with the gradient transport
attached (pmbrl_plan_set_grad_comm): horizon agreement, adjoint sweep, dW GEMM, one sum of [gradient | loss | failure
flag] over the ranks, clip + Adam on the sum, nothing returning to the host in between.  Two (or three) processes on
cuda:0, gloo for bootstrap, the one-hop peer-to-peer exchange as the transport (RCCL refuses two ranks on one GPU: its
branch is covered by the one-rank case below).  Shapes: D = 4, U = 1, H = 8; 2 x 32 networks with 32 rows a rank
(general family) and 2 x 200 networks with one row a rank (register-resident family: tests/reg_envelope_cases.py
'rows1')."""
import os

import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu
H = 8
LR, CLIP = 1e-3, 0.05
N_IT = 3
SMALL, REG = 32, 200        # hidden widths of the two shapes


def _problem(width, rows, groups=0, seed=3):
    from prob_mbrl_amd import problem as PB
    P = groups if groups else rows
    cfg = dict(D=4, U=1, pol_hid=[width, width], dyn_hid=[width, width], P=P, S=rows // P, H=H, mm=groups > 0,
               reward='cartpole', maxU=10.0)
    return PB.synthetic_problem(cfg, seed=seed)


def _decouple(d, k=3):
    """State dimension k out of the networks and the reward (tests/reg_envelope_cases.py, 'drift'): a dynamics-mean
    offset in it then overflows fp32 at a step the offset chooses, and nothing else notices"""
    d = dict(d)
    for key in ('pol_W0', 'dyn_W0'):
        W = np.asarray(d[key]).copy()
        W[:, k] = 0.0
        d[key] = W
    C = np.asarray(d['rew_C']).copy()
    assert bool(d['rew_expand'])
    C[:, 2] = 0.0
    d['rew_C'] = C
    return d


def _rank_engine(d, lo, hi, precision=None):
    """rows [lo, hi) of problem d as one rank's engine: whole moment-matching groups, global noise rows"""
    from prob_mbrl_amd import problem as PB
    B = d['x0'].shape[0]
    sub = dict(d)
    for k, v in d.items():
        if k in ('x0', 'pol_z', 'dyn_z') or ('_mask' in k and getattr(v, 'ndim', 0) == 2 and v.shape[0] == B):
            sub[k] = np.asarray(v)[lo:hi]
    sub['mm_groups'] = int(d['mm_groups']) * (hi - lo) // B
    eng, args, _ = PB.engine_from_problem(sub, 'cuda:0', B_global=B, row_offset=lo, precision=precision)
    return eng, args


class _Opt:
    def __init__(self, p0):
        dev = p0.device
        self.p = p0.clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.loss, self.norm = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        self.losses, self.norms, self.status = [], [], []

    def adam(self):
        return dict(params=self.p, exp_avg=self.m, exp_avg_sq=self.v, step=self.step, lr=LR, betas=(0.9, 0.999),
                    eps=1e-8, max_norm=CLIP, norm_out=self.norm, expect=min(H, 6), loss_out=self.loss)

    def record(self, eng):
        self.losses.append(self.loss.clone())
        self.norms.append(self.norm.clone())
        self.status.append(eng.status.clone())

    def result(self):
        torch.cuda.synchronize()
        return dict(p=self.p.cpu().numpy(), m=self.m.cpu().numpy(), v=self.v.cpu().numpy(), step=int(self.step.item()),
                    loss=torch.cat(self.losses).cpu().numpy(), norm=torch.cat(self.norms).cpu().numpy(),
                    status=torch.stack(self.status).cpu().numpy())


def _walk_fused(eng, args, gw, n_it=N_IT):
    """forward + backward-with-the-collective-inside: two library calls an iteration, no host sync in between"""
    o = _Opt(args['pol_flat'])
    args = dict(args, pol_flat=o.p)
    for _ in range(n_it):
        eng.forward(**args)
        eng.backward(gw, adam=o.adam())
        o.record(eng)
    return o.result()


def _walk_separate(eng, args, gw, p2p, group, n_it=N_IT):
    """the same iterations through the separate calls: host agreement on the horizon, weighted_sum, backward, the
    all-reduces of loss and gradient, the guarded step"""
    import torch.distributed as dist
    from prob_mbrl_amd import engine as E
    o = _Opt(args['pol_flat'])
    args = dict(args, pol_flat=o.p)
    for _ in range(n_it):
        _, _, R = eng.forward(**args)
        n = eng.valid_steps()
        if p2p is not None:
            nv = torch.tensor([n], dtype=torch.int32)
            dist.all_reduce(nv, op=dist.ReduceOp.MIN, group=group)
            if int(nv[0]) < n:
                eng.status[0] = int(nv[0])
        eng.weighted_sum(R, gw, out=o.loss)
        g, _, _ = eng.backward(gw)
        if p2p is not None:
            p2p.allreduce_(o.loss)
            p2p.allreduce_(g)
        E.clip_adam_guarded(o.p, g, o.m, o.v, o.step, LR, eng.status, min(H, 6), max_norm=CLIP, norm_out=o.norm)
        o.record(eng)
    return o.result()


def _worker(rank, world, port, case, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['PMBRL_P2P'] = '1'
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from prob_mbrl_amd import distributed as D
        from prob_mbrl_amd import problem as PB
        tr = D.tail_transport(dist.group.WORLD, torch.device('cuda:0'))
        assert isinstance(tr, D.P2PComm)
        kind = case['kind']
        res = dict(rank=rank)
        if kind in ('pair', 'horizon'):
            d = _problem(case['width'], case['rows'], case.get('groups', 0))
            prec = None
            if kind == 'horizon':
                d, prec = _decouple(d), 'f32'
            lo, hi = D.shard_bounds(case['rows'], case.get('groups') or None, world, rank)
            res['rows'] = (lo, hi)
            gw = torch.tensor(PB.loss_weights(d, case['rows'])[:, lo:hi].copy(), device='cuda:0')
            engs = []
            for _ in range(2):
                eng, args = _rank_engine(d, lo, hi, prec)
                if kind == 'horizon' and rank == case['bad_rank']:
                    my = args['my'].clone()
                    my[3] = case['drift']
                    args['my'] = my
                engs.append((eng, args))
            if kind == 'horizon':      # what this rank's device finds on its own
                engs[1][0].forward(**engs[1][1])
                res['own_steps'] = engs[1][0].valid_steps()
            engs[0][0].attach_grad_comm(tr)
            res['fused'] = _walk_fused(engs[0][0], engs[0][1], gw)
            res['tail_calls'] = engs[0][0].tail_calls()
            res['reg_calls'] = engs[0][0].reg_calls()
            res['mm_mode'] = engs[0][0].info['mm_mode']
            res['separate'] = _walk_separate(engs[1][0], engs[1][1], gw, tr, dist.group.WORLD)
            res['p0'] = engs[0][1]['pol_flat'].cpu().numpy()
        res['p2p_failed'] = tr.failed()
        out.put(res)
    finally:
        dist.destroy_process_group()


def _run(world, case, target=_worker):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = common.free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, case, out)) for r in range(world)]
    for p in procs:
        p.start()
    import queue
    import time
    res, deadline = [], time.monotonic() + 180
    try:
        while len(res) < world:
            try:
                res.append(out.get(timeout=0.5))
            except queue.Empty:
                # a dead or late worker fails the test: no retry, and no waiting for the others once one is gone
                assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
                assert time.monotonic() < deadline, 'a worker did not answer in time'
        res.sort(key=lambda r: r['rank'])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for p in procs:
        assert p.exitcode == 0
    return res


def _same_bits(a, b, keys=('p', 'm', 'v', 'loss', 'norm')):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a['step'] == b['step']


# ---------------------------------------------------------------------------------------------------------------------
# 1. fused against the separate calls
@pytest.mark.parametrize('world,width,rows,groups', [(2, SMALL, 64, 0), (2, REG, 2, 0), (3, SMALL, 95, 0), (2, SMALL, 8224, 2)],
                         ids=['small-2', 'reg-2', 'small-3-uneven', 'local-group-in-span-form'])
def test_fused_sharded_tail_walks_the_separate_calls_bit_for_bit(world, width, rows, groups):
    """(local-group-in-span-form: one LOCAL moment-matching group of 4 112 rows a rank -- more workgroups than CUs, which
    the plan runs in the form built for groups spread over ranks, with one rank; the transport must take such a plan)"""
    res = _run(world, dict(kind='pair', width=width, rows=rows, groups=groups))
    if rows == 95:
        assert [r['rows'] for r in res] == [(0, 32), (32, 64), (64, 95)]
    for r in res:
        assert not r['p2p_failed'] and r['tail_calls'] == N_IT
        assert r['fused']['step'] == N_IT and not np.array_equal(r['fused']['p'], r['p0'])
        assert np.all(np.isfinite(r['fused']['loss'])) and np.all(r['fused']['norm'] > 0)
        _same_bits(r['fused'], r['separate'])
        _same_bits(r['fused'], res[0]['fused'])            # ... and the replicas hold the same bits
        if groups:
            assert r['mm_mode'] == 2, r['mm_mode']          # the span form, chosen by the plan itself
        if width == REG:
            assert r['reg_calls'][0] >= N_IT and r['reg_calls'][1] >= N_IT, r['reg_calls']
        else:
            assert r['reg_calls'] == (0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. against one process
def test_two_ranks_of_local_groups_against_one_process():
    """Two moment-matching groups of 32 rows, one a rank, against one process holding both through today's
    pmbrl_rollout_bwd_adam: the same operations up to the order of the sums over rows (per rank, then over ranks).
    The yardstick is the distance the EXISTING separate-call sharded path has from the one process on this case; the
    fused tail stays within twice that.  Measured on the MI355X (relative L2, worst of parameters / moments / loss after
    three iterations): separate calls 3.859e-07, fused tail 3.859e-07 -- DESIGN_LOG.md, "Sharded iteration tail in one
    call"."""
    from prob_mbrl_amd import problem as PB
    res = _run(2, dict(kind='pair', width=SMALL, rows=64, groups=2))
    d = _problem(SMALL, 64, 2)
    eng, args, _ = PB.engine_from_problem(d, 'cuda:0')
    gw = torch.tensor(PB.loss_weights(d, 64), device='cuda:0')
    one = _walk_fused(eng, args, gw)
    assert eng.tail_calls() == 0 and one['step'] == N_IT

    def dist_to_one(r):
        return max(common.rel(r[k], one[k]) for k in ('p', 'm', 'v', 'loss'))
    for r in res:
        d_sep, d_fused = dist_to_one(r['separate']), dist_to_one(r['fused'])
        dp_sep = common.rel(r['separate']['p'] - r['p0'], one['p'] - r['p0'])
        dp_fused = common.rel(r['fused']['p'] - r['p0'], one['p'] - r['p0'])
        print('rank %d: separate-call sharded path vs one process %.3e (parameter UPDATE %.3e); fused tail %.3e (%.3e)'
              % (r['rank'], d_sep, dp_sep, d_fused, dp_fused))
        assert r['tail_calls'] == N_IT
        assert d_fused <= 2 * d_sep and dp_fused <= 2 * dp_sep


# ---------------------------------------------------------------------------------------------------------------------
# 3. mc_pilco(process_group=...) on a reference-recorded fixture
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
        if case.get('mode') == 'opt-out':
            os.environ['PMBRL_SHARDED_TAIL'] = '0'
        elif case.get('mode') == 'small-slots':
            # the peer-to-peer object of this group with slots the flat gradient does not fit: no transport for the
            # fused tail (gloo: no RCCL behind it), and the separate calls' all-reduce takes its own way round it
            dev0 = torch.device('cuda:0')
            D._P2PS[(id(dist.group.WORLD), str(dev0))] = D.P2PComm(dist.group.WORLD, dev0, max_bytes=1024)
        d = dict(common.load(name))
        B = d['x0'].shape[0]
        lo, hi = D.shard_bounds(B, None, world, rank)
        for k in list(d):
            if k == 'x0' or k in ('pol_z', 'dyn_z') or '_mask' in k:
                d[k] = d[k][lo:hi]
        dyn, pol = common.modules_from_fixture(d, name, 'cuda:0')
        opt = torch.optim.Adam(pol.parameters(), float(d['mcp_lr']))
        losses = []
        pm.algorithms.mc_pilco(
            torch.tensor(d['x0'], device='cuda:0'), dyn, pol, int(d['H']), opt, None,
            int(d['mcp_n_iters']), maximize=True, clip_grad=float(d['mcp_clip']),
            on_iteration=lambda i, loss, *a: losses.append(float(loss)),
            frozen_noise=dict(z_mm=torch.zeros(1, 4), z_rr=torch.zeros(1, 1)),
            mm_states=bool(d['mm_states']), mm_rewards=bool(d['mm_rewards']),
            discount=None if np.allclose(d['gamma'], d['gamma'][0]) else float(d['gamma'][1] / d['gamma'][0]),
            process_group=dist.group.WORLD)
        lins = [m for m in pol.model._modules.values() if isinstance(m, torch.nn.Linear)]
        final = torch.cat([t.detach().reshape(-1) for l in lins for t in (l.weight, l.bias)])
        out.put(dict(rank=rank, losses=losses, final=final.cpu().numpy(), n_iters=int(d['mcp_n_iters']),
                     tail_calls=sum(e.tail_calls() for e in RO._ENGINES.values()),
                     opt_steps=int(pm.algorithms.policy_update_counter[pol]),
                     adam_step=int(opt.state[next(iter(pol.parameters()))]['step'])))
    finally:
        dist.destroy_process_group()


def test_mc_pilco_two_ranks_through_the_fused_sharded_tail_match_reference():
    """tests/test_gpu_two_ranks.py::test_mc_pilco_two_ranks_match_reference with the peer-to-peer transport: the same
    reference-recorded losses and final parameters under the same tolerances, every iteration served by the backward
    call with the collective inside, and both ranks counting the same optimiser steps."""
    name = 'mcp_nomm'
    res = _run(2, dict(name=name), target=_mcp_worker)
    d = common.load(name)
    for r in res:
        assert r['tail_calls'] == r['n_iters'] > 0
        assert r['opt_steps'] == r['n_iters'] and r['adam_step'] == r['n_iters']
        assert np.allclose(r['losses'], d['ref32_mcp_losses'], rtol=5e-5)
        assert np.allclose(r['final'], d['ref32_mcp_final'], rtol=1e-4, atol=2e-6)
    assert np.array_equal(res[0]['final'], res[1]['final'])      # replicas stay bit-identical
    assert res[0]['losses'] == res[1]['losses']


@pytest.mark.parametrize('mode', ['small-slots', 'opt-out'])
def test_mc_pilco_keeps_the_separate_calls_where_the_fused_tail_cannot_or_shall_not_run(mode):
    """A flat gradient beyond the peer-to-peer slots (and no RCCL behind them), or PMBRL_SHARDED_TAIL=0: the sharded run
    goes through the separate calls as it did before the fused tail existed -- the same reference-recorded result, no
    backward call with the collective inside."""
    name = 'mcp_nomm'
    res = _run(2, dict(name=name, mode=mode), target=_mcp_worker)
    d = common.load(name)
    for r in res:
        assert r['tail_calls'] == 0 and r['opt_steps'] == r['n_iters'] and r['adam_step'] == r['n_iters']
        assert np.allclose(r['losses'], d['ref32_mcp_losses'], rtol=5e-5)
        assert np.allclose(r['final'], d['ref32_mcp_final'], rtol=1e-4, atol=2e-6)
    assert np.array_equal(res[0]['final'], res[1]['final'])


# ---------------------------------------------------------------------------------------------------------------------
# 4. horizon agreement
@pytest.mark.parametrize('drift,late', [(5e37, True), (1.5e38, False)], ids=['late-failure', 'early-failure'])
def test_ranks_agree_on_the_horizon_inside_the_call(drift, late):
    """Rank 1's rollout overflows fp32 in a state dimension nothing reads (a numerical failure its status word reports);
    rank 0's is clean.  Inside the call both ranks take rank 1's horizon: after step k >= 6 both optimise over k steps
    and hold the separate-call path's bits; before step 6 neither steps."""
    res = _run(2, dict(kind='horizon', width=SMALL, rows=64, drift=drift, bad_rank=1))
    k = res[1]['own_steps']
    assert res[0]['own_steps'] == H and ((6 <= k < H) if late else (0 < k < 6)), (res[0]['own_steps'], k)
    for r in res:
        assert not r['p2p_failed'] and r['tail_calls'] == N_IT
        assert np.all(r['fused']['status'][:, 0] == k) and np.all(r['fused']['status'][:, 1] == 0)
        assert np.all(r['separate']['status'][:, 0] == k)
        _same_bits(r['fused'], r['separate'])
        _same_bits(r['fused'], res[0]['fused'])
        if late:
            assert r['fused']['step'] == N_IT and np.all(np.isfinite(r['fused']['p']))
        else:
            assert r['fused']['step'] == 0 and np.array_equal(r['fused']['p'], r['p0'])
            assert not r['fused']['m'].any() and not r['fused']['v'].any()


# ---------------------------------------------------------------------------------------------------------------------
# 5. no transport, and a transport of one rank
def _one_rank_worker(rank, world, port, case, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from prob_mbrl_amd import _lib
        from prob_mbrl_amd import distributed as D
        from prob_mbrl_amd import problem as PB
        d = _problem(case['width'], case['rows'])
        gw = torch.tensor(PB.loss_weights(d, case['rows']), device='cuda:0')
        res = dict(rank=rank)
        eng, args, _ = PB.engine_from_problem(d, 'cuda:0')
        res['plain'] = _walk_fused(eng, args, gw)
        res['plain_calls'] = eng.tail_calls()
        p2p = D.P2PComm(dist.group.WORLD, torch.device('cuda:0'))
        eng, args, _ = PB.engine_from_problem(d, 'cuda:0')
        eng.attach_grad_comm(p2p)
        res['p2p'] = _walk_fused(eng, args, gw)
        res['p2p_calls'] = eng.tail_calls()
        eng.attach_grad_comm(None)
        res['detached'] = _walk_fused(eng, args, gw)
        res['detached_calls'] = eng.tail_calls()
        # slots the flat gradient does not fit: refused, and the plan goes on without a transport
        tiny = D.P2PComm(dist.group.WORLD, torch.device('cuda:0'), max_bytes=64)
        eng.attach_grad_comm(p2p)
        try:
            eng.attach_grad_comm(tiny)
            res['refused'] = None
        except _lib.PmbrlError as e:
            res['refused'] = str(e)
        res['after_refusal'] = _walk_fused(eng, args, gw)
        res['after_refusal_calls'] = eng.tail_calls()
        res['p2p_failed'] = p2p.failed()
        res['rccl'] = None
        try:
            comm = D.GradComm(dist.group.WORLD, torch.device('cuda:0'))
        except Exception as e:      # noqa: BLE001 -- no RCCL here: said, not hidden (the assertion below names it)
            res['rccl_error'] = str(e)
        else:
            eng, args, _ = PB.engine_from_problem(d, 'cuda:0')
            eng.attach_grad_comm(comm)
            res['rccl'] = _walk_fused(eng, args, gw, n_it=N_IT)
            res['rccl_calls'] = eng.tail_calls()
            eng.attach_grad_comm(None)
            del eng
            comm.close()
        out.put(res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('width,rows', [(SMALL, 32), (REG, 1)], ids=['small', 'reg'])
def test_no_transport_and_one_rank_transports_reproduce_todays_bits(width, rows):
    r = _run(1, dict(width=width, rows=rows), target=_one_rank_worker)[0]
    assert r['plain_calls'] == 0 and r['p2p_calls'] == N_IT and r['detached_calls'] == N_IT and not r['p2p_failed']
    assert r['plain']['step'] == N_IT
    _same_bits(r['p2p'], r['plain'])
    _same_bits(r['detached'], r['plain'])
    assert r['refused'] is not None and '(-2)' in r['refused'] and r['after_refusal_calls'] == N_IT
    _same_bits(r['after_refusal'], r['plain'])
    assert r['rccl'] is not None, r.get('rccl_error')
    assert r['rccl_calls'] == N_IT
    _same_bits(r['rccl'], r['plain'])
