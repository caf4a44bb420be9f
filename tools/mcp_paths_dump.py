"""Dump what mc_pilco leaves behind on each of its iteration paths, for bit comparison between two checkouts:

    python tools/mcp_paths_dump.py --out DIR        (on each checkout, same device)
    python tools/mcp_paths_dump.py --compare DIR_A DIR_B

Forms: the six of tests/test_gpu_mc_pilco_routes.py (pipelined, separate calls, autograd twice, the fp16-range failure
on the pipelined path and on the separate calls, failed rollouts) and two with rows sharded over two processes on one
device (the fused sharded tail over the peer-to-peer transport; separate calls with CVaR and the regulariser).  Per
form one .npz: final flat policy, Adam's exp_avg / exp_avg_sq / step, the losses on_iteration saw, captured stdout.
The reductions are fixed-order: one device gives the same bits twice."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import common  # noqa: E402

DEV = 'cuda:0'
SEED = 1234


def _state(pol, opt, losses, out):
    ps = [p for p in pol.parameters() if p.requires_grad]
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()  # noqa: E731
    st = [opt.state[p] for p in ps if 'exp_avg' in opt.state.get(p, {})]
    return dict(policy=cat(ps), exp_avg=cat([s['exp_avg'] for s in st]) if st else np.zeros(0),
                exp_avg_sq=cat([s['exp_avg_sq'] for s in st]) if st else np.zeros(0),
                step=np.array(int(st[0]['step']) if st else 0), losses=np.array(losses, np.float64), stdout=np.array(out))


def _single(d, name, frozen=False, **kw):
    import prob_mbrl_amd as pm
    torch.manual_seed(SEED)
    dyn, pol = common.modules_from_fixture(d, name, DEV)
    opt = torch.optim.Adam(pol.parameters(), 1e-4)
    x0, H = torch.tensor(d['x0'], device=DEV), int(d['H'])
    if frozen:
        kw['frozen_noise'] = dict(z_mm=torch.zeros(H + x0.shape[0], 4), z_rr=torch.zeros(H + x0.shape[0], 1))
    losses, buf = [], io.StringIO()
    with contextlib.redirect_stdout(buf):
        pm.algorithms.mc_pilco(x0, dyn, pol, H, opt, None, 3, on_iteration=lambda i, loss, *a: losses.append(float(loss)),
                               **kw)
    return _state(pol, opt, losses, buf.getvalue())


def single_forms():
    from tests.test_gpu_mc_pilco_routes import _out_of_fp16_range
    nomm = common.load('nomm_d4')
    yield 'a_pipelined', _single(nomm, 'nomm_d4')
    yield 'b_separate', _single(nomm, 'nomm_d4', on_rollout=lambda *a: None)
    yield 'c_autograd_cvar_reg', _single(nomm, 'nomm_d4', cvar_eps=0.3, reg_weight=1e-3)
    yield 'd_autograd_unit_rates', _single(common.load('unit_rates_d4'), 'unit_rates_d4')
    yield 'e_fp16_pipelined', _single(_out_of_fp16_range(), 'nomm_d4', frozen=True)
    yield 'e_fp16_separate', _single(_out_of_fp16_range(), 'nomm_d4', frozen=True, on_rollout=lambda *a: None)
    yield 'f_failed_rollouts', _single(common.load('mmg_d4'), 'mmg_d4', mm_states=True, mm_rewards=True, mm_groups=20)


def _two_rank_worker(rank, world, port, case, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    if case['p2p']:
        os.environ['PMBRL_P2P'] = '1'
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import prob_mbrl_amd as pm
        from prob_mbrl_amd import distributed as D
        torch.manual_seed(SEED)
        name = case['name']
        d = dict(common.load(name))
        lo, hi = D.shard_bounds(d['x0'].shape[0], None, world, rank)
        for k in list(d):
            if k == 'x0' or k in ('pol_z', 'dyn_z') or '_mask' in k:
                d[k] = d[k][lo:hi]
        dyn, pol = common.modules_from_fixture(d, name, DEV)
        opt = torch.optim.Adam(pol.parameters(), float(d['mcp_lr']))
        losses, buf = [], io.StringIO()
        with contextlib.redirect_stdout(buf):
            pm.algorithms.mc_pilco(
                torch.tensor(d['x0'], device=DEV), dyn, pol, int(d['H']), opt, None, int(d['mcp_n_iters']), maximize=True,
                clip_grad=float(d['mcp_clip']), on_iteration=lambda i, loss, *a: losses.append(float(loss)),
                frozen_noise=(dict(z_mm=torch.tensor(d['z_mm']), z_rr=torch.tensor(d['z_rr'])) if bool(d['mm_states'])
                              else dict(z_mm=torch.zeros(1, 4), z_rr=torch.zeros(1, 1))),
                mm_states=bool(d['mm_states']), mm_rewards=bool(d['mm_rewards']),
                discount=None if np.allclose(d['gamma'], d['gamma'][0]) else float(d['gamma'][1] / d['gamma'][0]),
                cvar_eps=float(d['mcp_cvar_eps']) if 'mcp_cvar_eps' in d else 0.0,
                reg_weight=float(d['mcp_reg_weight']) if 'mcp_reg_weight' in d else 0.0, process_group=dist.group.WORLD)
        from prob_mbrl_amd import rollout as RO
        res = _state(pol, opt, losses, buf.getvalue())
        res['tail_calls'] = np.array(sum(e.tail_calls() for e in RO._ENGINES.values()))
        out.put(dict(rank=rank, state=res))
    finally:
        dist.destroy_process_group()


def two_rank_forms():
    from tests.test_gpu_sharded_tail import _run
    for tag, case in (('w2_fused_tail_p2p', dict(name='mcp_nomm', p2p=True)),
                      ('w2_separate_cvar_reg', dict(name='mcp_cvar_neg_reg', p2p=False))):
        for r in _run(2, case, target=_two_rank_worker):
            yield '%s_rank%d' % (tag, r['rank']), r['state']


def compare(dir_a, dir_b):
    names = sorted(f for f in os.listdir(dir_a) if f.endswith('.npz'))
    assert names and names == sorted(f for f in os.listdir(dir_b) if f.endswith('.npz')), 'different sets of forms'
    bad = 0
    for n in names:
        a, b = np.load(os.path.join(dir_a, n)), np.load(os.path.join(dir_b, n))
        diff = [k for k in a.files if k not in b.files or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
        print('%-36s %s' % (n, 'equal (%s)' % ', '.join(a.files) if not diff else 'DIFFERENT: %s' % ', '.join(diff)))
        bad += bool(diff)
    return bad


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(1 if compare(*args.compare) else 0)
    os.makedirs(args.out, exist_ok=True)
    for forms in (single_forms, two_rank_forms):
        for tag, state in forms():
            np.savez(os.path.join(args.out, tag + '.npz'), **state)
            print('%s: step %d, losses %s' % (tag, int(state['step']), state['losses'].tolist()))
