"""`mc_pilco()` with the reference's call surface (algorithms/mc_pilco.py:13-267).

Two execution paths, same semantics:
 * fused (default): rollout forward -> loss -> adjoint sweep -> dW GEMM ->
   [gradient all-reduce] -> clip + Adam are C-ABI calls on flat buffers; no
   autograd graph, no torch.nn op, one host sync per iteration (status + loss).
   Used when the optimiser is a torch.optim.Adam or AdamW over the policy's Linear
   parameters (any groups, weight decay, amsgrad, maximize: optim.py) and no option needs autograd (CVaR, regulariser, value_func,
   prioritized_replay).
 * autograd: `rollout()`'s single autograd node (the stepwise rollout for a train-mode concrete-dropout policy, whose
   logit_p the optimiser then updates too, and for a policy or dynamics model with layer norm) + torch's loss / clip /
   optimiser
   for everything else the reference signature allows.  value_func is evaluated by
   pmbrl_mlp_forward and differentiated by pmbrl_mlp_grad_input; the priorities of
   prioritized_replay come from pmbrl_rollout_bwd's action_grad_norms output.
"""
import traceback
from collections import defaultdict
from dataclasses import dataclass

import numpy as np
import torch

from . import engine as E
from . import optim as OPT
from . import rollout as RO
from ._lib import PmbrlError
from .utils import tile

policy_update_counter = defaultdict(lambda: 0)   # algorithms/mc_pilco.py:8
x0_tree = None          # SumTree(2**20) of start states, built on first use (mc_pilco.py:9)
episode_counter = 0     # episodes of `exp` already in x0_tree (mc_pilco.py:10)


def _discount_fn(discount, steps):
    """algorithms/mc_pilco.py:46-50."""
    if discount is None:
        return lambda i: 1.0 / steps
    if not callable(discount):
        factor = discount
        return lambda i: factor**i
    return discount


def _adam_flat_state(opt, params, flat):
    """The one translator from a torch optimiser to the device-side steps.  If `opt` is a torch.optim.Adam or AdamW whose
    1 to 8 groups hold exactly the trainable `params` (optim.layout), return the flat optimiser state: m, v, vmax
    (amsgrad's running maximum, where a group asks for it), step, segments (the runs of the flat vector each group
    owns), plain (the plain kernels' own rule: they serve it as before), group (the first group) -- the per-parameter
    state of torch re-pointed at the flat buffers (views), existing state imported on first use.  Else None.
    optim.rule_of(cache) is the rule of one step."""
    segments = OPT.layout(opt, params)
    if segments is None:
        return None
    cache = getattr(opt, '_pmbrl_flat', None)
    if cache is not None and cache['flat_ptr'] == flat.data_ptr() and cache['segments'] == segments:
        st = opt.state.get(params[0], {})
        if 'step' in st:   # torch may have stepped this optimiser in between
            cache['step'] = int(st['step'])
        cache['plain'] = OPT.is_plain(opt)
        if cache['vmax'] is None and any(g.get('amsgrad', False) for g in opt.param_groups):
            cache['vmax'] = cache['v'].clone()       # (amsgrad switched on between two calls: torch starts it from zero)
            cache['vmax'].zero_()
        return cache
    m = torch.zeros_like(flat)
    v = torch.zeros_like(flat)
    vmax = torch.zeros_like(flat) if any(g.get('amsgrad', False) for g in opt.param_groups) else None
    step, off = 0, 0
    for p in params:
        n = p.numel()
        st = opt.state.get(p, {})
        if 'exp_avg' in st:
            m[off:off + n] = st['exp_avg'].reshape(-1)
            v[off:off + n] = st['exp_avg_sq'].reshape(-1)
            if vmax is not None and 'max_exp_avg_sq' in st:
                vmax[off:off + n] = st['max_exp_avg_sq'].reshape(-1)
            step = max(step, int(st['step']) if not torch.is_tensor(st['step']) else int(st['step'].item()))
        off += n
    cache = dict(m=m, v=v, vmax=vmax, step=step, group=opt.param_groups[0], flat_ptr=flat.data_ptr(), opt=opt,
                 params=list(params), segments=segments, plain=OPT.is_plain(opt))
    opt._pmbrl_flat = cache
    return cache


def _sync_adam_state(opt, params, cache):
    """Expose the flat Adam state through opt.state (views) so state_dict()/later
    opt.step() calls keep working (max_exp_avg_sq for the parameters of an amsgrad group)."""
    ams = {id(p) for g in opt.param_groups if g.get('amsgrad', False) for p in g['params']}
    off = 0
    for p in params:
        n = p.numel()
        st = opt.state[p]
        st['step'] = torch.tensor(float(cache['step']))
        st['exp_avg'] = cache['m'][off:off + n].view(p.shape)
        st['exp_avg_sq'] = cache['v'][off:off + n].view(p.shape)
        if id(p) in ams and cache.get('vmax') is not None:
            st['max_exp_avg_sq'] = cache['vmax'][off:off + n].view(p.shape)
        off += n


@dataclass
class Pending:
    """A pipelined iteration in flight: the host reads its status word one iteration late (_settle)."""
    i: int
    ev: object          # recorded behind the status snapshot
    snap: object        # pinned [valid steps, failure flag summed over the ranks]
    loss: object
    S: object
    A: object
    R: object
    tail: object        # the transport inside its backward call, or None
    precision: str      # arithmetic its sweeps ran on


class _Run:
    """One mc_pilco call: its arguments under their own names, what _setup_run derives from them once (H, disc,
    gamma_full, sign, min_steps, dev, world, rank, N, Bg, mm_span, dist_kw, z_mm, z_rr, replay, cvar, need_autograd,
    tail_eligible), and the state its stages share."""

    def __init__(self, **args):
        self.__dict__.update(args)
        self.n_opt_steps = 0
        self.n_resamples = 0        # (sharded pipelined loop: compared over the ranks at the end)
        # arithmetic of the sweeps: the library default, until a rollout fails under fp16 pieces -- whose
        # range, not the rollout, may be what failed: the rest of this call then runs on the bf16 pieces
        self.precision = None
        # the two slots of the pipelined path (iteration i uses slot i & 1), allocated by its first iteration
        self.snap = self.ev = self.loss = None
        self.step_dev = None        # Adam's step count while it lives on the device ...
        self.cache = None           # ... and the flat Adam state it returns to
        self.tail_of = {}           # id(engine) -> (engine, its transport or None)
        self.tail_used = None


def mc_pilco(init_states, dynamics, policy, steps, opt=None, exp=None, opt_iters=1000,
             value_func=None, pegasus=True, mm_states=False, mm_rewards=False, mm_groups=None,
             maximize=True, clip_grad=1.0, cvar_eps=0.0, reg_weight=0.0, discount=None,
             on_rollout=None, on_iteration=None, step_idx_to_sample=None, init_state_noise=0.0,
             resampling_period=99, prioritized_replay=False, priority_alpha=0.6,
             priority_eps=1e-8, init_priority_beta=1.0, priority_beta_increase=0.0, debug=False,
             rollout_kwargs={}, process_group=None, frozen_noise=None, progress=False):
    """Monte-Carlo PILCO policy search.  Mutates `policy` parameters and `opt` state in place.

    Extra keyword arguments (not in the reference): `process_group` -- a torch.distributed
    group over which the particle rows are sharded (this rank passes ITS rows; the flat policy
    gradient is all-reduced over RCCL before the identical clip + Adam on every rank);
    `frozen_noise` -- dict(z_mm=..., z_rr=...) to inject captured PEGASUS noise (tests);
    `progress` -- print the reference's tqdm-style line every 50 iterations."""
    global x0_tree
    if prioritized_replay and x0_tree is None:
        from .experience import SumTree
        x0_tree = SumTree(2**20)
    dynamics.eval()
    policy.train()
    H = int(steps)
    disc = _discount_fn(discount, H)
    if opt is None:
        opt = torch.optim.Adam(filter(lambda p: p.requires_grad, policy.parameters()))
    run = _Run(dynamics=dynamics, policy=policy, opt=opt, value_func=value_func, pegasus=pegasus, mm_states=mm_states,
               mm_rewards=mm_rewards, mm_groups=mm_groups, maximize=maximize, clip_grad=clip_grad, cvar_eps=cvar_eps,
               reg_weight=reg_weight, on_rollout=on_rollout, on_iteration=on_iteration,
               step_idx_to_sample=step_idx_to_sample, prioritized_replay=prioritized_replay,
               priority_beta_increase=priority_beta_increase, rollout_kwargs=rollout_kwargs,
               process_group=process_group, frozen_noise=frozen_noise, progress=progress, H=H, disc=disc)
    _setup_run(run, init_states, init_priority_beta, priority_eps, priority_alpha)
    _resample(run)
    run.n_opt_steps = policy_update_counter[policy]
    pending = None
    for i in range(opt_iters):
        if pending is not None:
            _settle(run, pending)
            pending = None
        if not pegasus or run.n_opt_steps % resampling_period == 0:
            _resample(run)
        x0_ = run.x0
        if mm_groups is not None and x0_.shape[0] == mm_groups:
            x0_ = tile(x0_, int(run.N / mm_groups))
        x0_ = x0_.to(run.dev, torch.float32)
        if not (isinstance(init_state_noise, float) and init_state_noise == 0.0):
            x0_ = x0_ + torch.as_tensor(init_state_noise, device=run.dev) * torch.randn_like(x0_)
        try:
            if RO.stepwise_networks(dynamics, policy) is not None:
                # learned policy dropout rates, layer norm in either network: the stepwise rollout, torch's clip and step
                # over policy.parameters() (logit_p, ln*.weight and ln*.bias among them); the fused and pipelined paths
                # never see such networks
                path = 'autograd'
            else:
                bundle = _make_bundle(run, x0_, run.precision)
                path, cache, tail = _route(run, bundle)
            if path == 'autograd':
                loss, states, actions, rewards = _autograd_iteration(run, x0_, i)
            elif path == 'pipelined':
                pending = _iterate_pipelined(run, bundle, x0_, cache, tail, i)
            else:
                loss, states, actions, rewards = _iterate_separate(run, bundle, x0_, cache, i)
        except NotImplementedError:      # an option the device path does not offer: not a failed rollout
            raise
        except RuntimeError:
            # algorithms/mc_pilco.py:122-131: print, draw new random numbers, skip the step
            traceback.print_exc()
            print('RuntimeError')
            _resample(run)
            opt.zero_grad()
            continue
        if path != 'pipelined':     # (a pipelined iteration is counted and handed to the hook by _settle)
            run.n_opt_steps += 1
            if progress and i % 50 == 0:
                print(_progress_line(maximize, rewards))
            if callable(on_iteration):
                on_iteration(i, loss, states, actions, rewards, disc)
        _next_start_states(run, exp)

    if pending is not None:
        _settle(run, pending)
    if run.step_dev is not None:
        run.cache['step'] = int(run.step_dev.item())
    _check_replicas_in_step(run)
    cache = getattr(opt, '_pmbrl_flat', None)
    if cache is not None and type(opt) in (torch.optim.Adam, torch.optim.AdamW):
        _sync_adam_state(opt, cache['params'], cache)
    policy.eval()
    dynamics.eval()
    policy_update_counter[policy] = run.n_opt_steps


def _setup_run(run, init_states, init_priority_beta, priority_eps, priority_alpha):
    """World and rank, the moment-matching span the ranks agree on, the PEGASUS noise buffers, the replay record and
    the switches _route reads."""
    run.dev = dev = next(run.policy.parameters()).device
    if dev.type != 'cuda':
        raise RuntimeError('prob_mbrl_amd.mc_pilco needs the modules on a HIP device')
    H, D = run.H, init_states.shape[-1]
    run.N = N = init_states.shape[0]
    run.world, run.rank = 1, 0
    run.mm_span = None      # one moment-matching group over the particles of all ranks (sharded runs, mm_groups=None)
    if run.process_group is not None:
        import torch.distributed as dist
        from .distributed import ints_over_ranks
        run.world, run.rank = dist.get_world_size(run.process_group), dist.get_rank(run.process_group)
        if run.world > 1 and (run.mm_states or run.mm_rewards) and run.mm_groups is None:
            # one Gaussian over ALL particles (the examples' default): the per-step sufficient statistics are
            # summed over the ranks (pmbrl_config.mm_span_rows) -- fitting one Gaussian per rank
            # instead would silently be different mathematics.  Needs the same particle count on every rank.
            cnt = ints_over_ranks([N, -N], 'max', run.process_group, dev)
            if cnt[0] != -cnt[1]:
                raise ValueError('moment matching over one global group on a sharded run needs the same number of '
                                 'particles on every rank')
            run.mm_span = (N * run.world, run.rank * N, run.world, run.rank)
    world, rank = run.world, run.rank
    run.Bg = N * world
    run.dist_kw = dict(B_global=run.Bg if world > 1 else None, row_offset=rank * N if world > 1 else 0,
                       mm_span=run.mm_span, process_group=run.process_group if run.mm_span else None)
    run.z_mm = torch.randn(H + run.Bg, D, device=dev)
    run.z_rr = torch.randn(H + run.Bg, 1, device=dev)
    if run.frozen_noise is not None:
        run.z_mm = run.frozen_noise['z_mm'].to(dev, torch.float32)
        run.z_rr = run.frozen_noise['z_rr'].to(dev, torch.float32)
    run.x0 = run.init_states = init_states
    run.cvar = run.cvar_eps > -1.0 and run.cvar_eps < 1.0 and run.cvar_eps != 0
    # sharded runs: CVaR is a row mask on dL/dr once the returns of ALL ranks are known, the regulariser touches only
    # the (replicated) parameters -- both fit the fused path; one process keeps the reference's own
    # sequence of autograd operations for them
    run.need_autograd = (((run.cvar or run.reg_weight > 0) and world == 1) or run.value_func is not None
                         or run.prioritized_replay or bool(run.rollout_kwargs))
    run.replay = None
    if run.prioritized_replay:      # algorithms/mc_pilco.py:80-84
        run.replay = dict(idxs=None, weights=None, beta=init_priority_beta, eps=priority_eps, alpha=priority_alpha,
                          tree=x0_tree, N=N, world=world, rank=rank, group=run.process_group)
    run.gamma_full = [float(run.disc(i)) for i in range(H)]
    run.sign = -1.0 if run.maximize else 1.0
    # a rollout that failed after more than 5 steps is optimised on its truncated horizon
    # (utils/rollout.py:154-157); earlier failures skip the step (algorithms/mc_pilco.py:122-131)
    run.min_steps = min(H, 6)
    from .distributed import sharded_tail_wanted
    run.tail_eligible = (world > 1 and not callable(run.on_rollout) and not run.need_autograd and not run.cvar
                         and not run.reg_weight > 0 and run.mm_span is None and sharded_tail_wanted())


def _resample(run):
    run.n_resamples += 1
    if run.frozen_noise is not None:
        return
    seed = torch.randint(2**32, [1])
    if run.world > 1:   # every rank must draw different masks: offset the seed by the rank
        seed = seed + 7919 * run.rank
    run.dynamics.resample(seed=seed)
    run.policy.resample(seed=seed)
    if run.value_func is not None:
        run.value_func.resample(seed=seed)
    run.z_mm.normal_()
    run.z_rr.normal_()
    if run.mm_span is not None:
        # one group over all ranks: one cyclic noise buffer, as one process would hold it
        import torch.distributed as dist
        src = dist.get_global_rank(run.process_group, 0)
        dist.broadcast(run.z_mm, src, group=run.process_group)
        dist.broadcast(run.z_rr, src, group=run.process_group)


def _make_bundle(run, x0_, precision):
    return RO.Bundle(run.dynamics, run.policy, x0_.shape[0], run.H, not run.pegasus, not run.pegasus, run.mm_states,
                     run.mm_rewards, run.mm_groups, run.z_mm if run.pegasus else None,
                     run.z_rr if run.pegasus else None, precision=precision, **run.dist_kw)


def _route(run, bundle):
    """('autograd' | 'pipelined' | 'separate', flat Adam state, transport): the path of this iteration.

    Pipelined fused path (single process, no on_rollout hook): the optimiser step is decided on
    the device from the rollout's status word (pmbrl_clip_adam_guarded) and the host reads that
    word one iteration late, from a pinned snapshot queued right behind the forward sweep.  The
    host then never waits for a whole iteration: while it prepares iteration i+1 the device still
    has the adjoint sweep, the dW GEMM and the Adam step of iteration i to run.
    Rows sharded over ranks take the same two-call loop when the gradient exchange can run INSIDE the backward call
    (pmbrl_plan_set_grad_comm: RCCL, or the peer-to-peer transport with PMBRL_P2P=1): the ranks agree on the horizon,
    sum gradient, loss and failure flag and decide the step on the device; the host reads the AGREED status one iteration
    late, so every rank resamples, switches arithmetic and counts optimiser steps in the same iterations.  Anything
    that needs the host between the sweeps (CVaR, regulariser, groups spread over ranks, hooks) keeps the separate calls.
    Decided per engine, the same way on every rank (_tail_for): a plan that cannot take the transport -- a flat gradient
    beyond the peer-to-peer slots with no RCCL behind them, a refusal by the library -- keeps the separate calls.
    PMBRL_SHARDED_TAIL=0 keeps them everywhere (tools/bench_sharded_tail.py measured the fused call SLOWER than bench.py's
    separate calls with two ranks on one device; this loop's own separate calls, with their host round trips, have
    not been timed against it -- DESIGN_LOG.md)."""
    # (per-unit dropout rates: the kernels run on scaled copies of the parameters -- the device-side Adam step
    #  would update the wrong numbers; the autograd form scales the gradient back)
    if run.need_autograd or bundle.unit_scaled:
        return 'autograd', None, None
    cache = _adam_flat_state(run.opt, bundle.pol_params, bundle.pol_flat)
    if cache is None:
        return 'autograd', None, None
    tail = _tail_for(run, bundle.engine, bundle.pol_flat.numel()) if run.tail_eligible else None
    if tail is not None or (run.world == 1 and not callable(run.on_rollout)):
        return 'pipelined', cache, tail
    return 'separate', cache, None


def _tail_for(run, eng, n_params):
    """The transport `eng` carries inside its backward call, or None: keep the separate calls.  Collective the first
    time an engine is seen (the ranks meet new engines in the same iterations)."""
    hit = run.tail_of.get(id(eng))
    if hit is not None and hit[0] is eng:
        return hit[1]
    from .distributed import ints_over_ranks, tail_transport
    tr = tail_transport(run.process_group, run.dev, n_params=n_params)
    ok = 0
    if tr is not None:
        try:
            eng.attach_grad_comm(tr)
            ok = 1
        except PmbrlError as e:
            print('prob_mbrl_amd: rank %d keeps the separate calls of the sharded iteration (%s)' % (run.rank, e))
    if ints_over_ranks([ok], 'min', run.process_group, run.dev)[0] == 0:
        if ok:
            eng.attach_grad_comm(None)
        tr = None
    run.tail_of[id(eng)] = (eng, tr)
    return tr


def _iterate_pipelined(run, bundle, x0_, cache, tail, i):
    """Forward call, then ONE backward call that ends in the guarded clip + Adam: nothing returns to the host; the
    status word travels to a pinned snapshot that _settle reads one iteration late."""
    eng, dev = bundle.engine, run.dev
    run.tail_used = tail if tail is not None else run.tail_used
    if run.snap is None:
        run.snap = [torch.zeros(2, dtype=torch.int32).pin_memory() for _ in range(2)]
        run.ev = [torch.cuda.Event() for _ in range(2)]
        run.loss = [torch.zeros(1, dtype=torch.float32, device=dev) for _ in range(2)]
    if run.step_dev is None:
        run.step_dev = torch.tensor([cache['step']], dtype=torch.int64, device=dev)
        run.cache = cache
    S, A, R = bundle.forward(x0_)
    k = i & 1
    if tail is None:
        run.snap[k][0:1].copy_(eng.status[0:1], non_blocking=True)
        run.ev[k].record()
    gw = _loss_weights(eng, run.gamma_full, run.sign, run.Bg, dev)
    # (the loss: formed by the backward call's gradient reduction, written by its optimiser launch --
    #  pmbrl_adam::loss_out_d; two buffers: the host reads iteration i's one iteration late)
    grp = cache['group']
    # adjoint sweep, dW GEMM, then reduction + global norm + clip + Adam, taken on the device only if the
    # rollout completed (pmbrl_rollout_bwd_adam)
    eng.backward(gw, adam=dict(params=bundle.pol_flat, exp_avg=cache['m'], exp_avg_sq=cache['v'], step=run.step_dev,
                               lr=grp['lr'], betas=grp['betas'], eps=grp['eps'], max_norm=run.clip_grad,
                               expect=run.min_steps, loss_out=run.loss[k], rule=OPT.rule_of(cache)))
    if tail is not None:
        # (the horizon the ranks agreed on and the summed failure flag exist only behind the backward call)
        run.snap[k].copy_(eng.status, non_blocking=True)
        run.ev[k].record()
    return Pending(i, run.ev[k], run.snap[k], run.loss[k][0], S, A, R, tail, eng.info['precision'])


def _settle(run, pend):
    """Host side of a pipelined iteration, once its status word has arrived."""
    pend.ev.synchronize()
    if pend.tail is not None and int(pend.snap[1]) != 0:
        # the failure flag summed over the ranks with the gradient: an adjoint sweep that reported a failure of its
        # own, or a peer-to-peer wait that had timed out before the exchange, on ANY rank -- the device skipped the
        # step on every rank, and every rank raises here, in the same iteration.  (A wait that timed out INSIDE the
        # gradient exchange: the rank it happened on skipped alone and raises here now -- its own status word says
        # so, pm_tail_finish_kernel; the others raise one iteration later, from the sticky error word.)
        raise RuntimeError('sharded iteration %d: the adjoint sweep or the gradient exchange failed on a rank (a '
                           'barrier between workgroups or a wait for a peer timed out; PMBRL_P2P_TIMEOUT_SPINS sets '
                           'the latter)' % pend.i)
    n_valid = min(int(pend.snap[0]), run.H)
    if n_valid < run.H and run.precision is None and E.safe_precision(pend.precision) is not None:
        # (the device skipped or truncated this step on its own; no resampling: same random numbers,
        #  wider exponent range from now on)
        run.precision = E.safe_precision(pend.precision)
        print('rollout failed at step %d under %s arithmetic (iteration %d): continuing with %s' %
              (n_valid, pend.precision, pend.i, run.precision))
        if n_valid < run.min_steps:
            return
    elif n_valid < run.min_steps:
        # algorithms/mc_pilco.py:122-131: report, draw new random numbers; the device already
        # skipped the optimiser step
        print('RuntimeError: rollout failed at step %d (iteration %d)' % (n_valid, pend.i))
        _resample(run)
        return
    run.n_opt_steps += 1
    shown = run.progress and pend.i % 50 == 0
    if shown or callable(run.on_iteration):
        # fresh tensors, like the reference hands out: the engine's buffers are overwritten by the
        # next iteration -- cloned only here, where somebody reads them
        states, actions, rewards = _as_lists(pend.S, pend.A, pend.R, n_valid, clone=True)
        if shown:
            print(_progress_line(run.maximize, rewards))
        if callable(run.on_iteration):      # (the loss buffer is reused two iterations on)
            run.on_iteration(pend.i, pend.loss.clone(), states, actions, rewards, run.disc)


def _progress_line(maximize, rewards):
    msg = 'Pred. Cumm. rewards: %f' if maximize else 'Pred. Cumm. costs: %f'
    return (msg % float(torch.stack(rewards).sum(0).mean())) + ' [{0}]'.format(len(rewards))


def _as_lists(S, A, R, n_valid, clone):
    """(states, actions, rewards) of the first n_valid steps as the reference's lists of per-step tensors -- views of
    the engine's buffers, or tensors of their own."""
    own = (lambda t: t.clone()) if clone else (lambda t: t)
    return tuple(list(own(t).unbind(0)) for t in (S[:n_valid + 1], A[:n_valid], R[:n_valid]))


def _cvar_select(ret, rd_all, cvar_eps):
    """algorithms/mc_pilco.py:146-154: (mask of the rows of `ret` beyond the cvar_eps quantile of ALL returns rd_all,
    how many of rd_all are)."""
    q = np.quantile(rd_all, abs(cvar_eps))
    if cvar_eps > 0:
        return ret < float(q), int((rd_all < q).sum())
    return ret > float(q), int((rd_all > q).sum())


def _agreed_steps(run, eng):
    """Valid steps of the sweep just run -- on a sharded run the MIN over the ranks: every rank must take
    the same branch and the same horizon, a failure anywhere truncates (or fails) the rollout
    everywhere, like one process would."""
    n = eng.valid_steps()           # the one host sync of the iteration
    if run.world > 1:
        from .distributed import ints_over_ranks
        n_all = ints_over_ranks([n], 'min', run.process_group, run.dev)[0]
        if n_all < n:
            eng.status[0:1].fill_(n_all)          # what the adjoint sweep and the loss read
        n = n_all
    return n


def _iterate_separate(run, bundle, x0_, cache, i):
    """Forward, host agreement on the horizon, loss, on_rollout, backward, gradient all-reduce, regulariser, clip +
    Adam as separate calls: what a hook, CVaR, the regulariser or a plan without a transport need."""
    eng, dev, H, world = bundle.engine, run.dev, run.H, run.world
    if run.step_dev is not None:
        # (an engine that keeps the separate calls behind one that ran the fused tail: the step count moves
        #  back to the host)
        cache['step'] = int(run.step_dev.item())
        run.step_dev = None
    S, A, R = bundle.forward(x0_)
    n_valid = _agreed_steps(run, eng)
    if n_valid < H and run.precision is None and E.safe_precision(eng.info['precision']) is not None:
        # fp16 pieces: their range may be what failed -- decide on the bf16 / fp32 path.  (n_valid is the
        # ranks' minimum, so all of them switch together and stay switched.)
        run.precision = E.safe_precision(eng.info['precision'])
        bundle = _make_bundle(run, x0_, run.precision)
        eng = bundle.engine
        S, A, R = bundle.forward(x0_)
        n_valid = _agreed_steps(run, eng)
    if n_valid < run.min_steps:
        raise RuntimeError('rollout failed at step %d' % n_valid)
    gw = _loss_weights(eng, run.gamma_full, run.sign, run.Bg, dev)
    if run.cvar:
        # algorithms/mc_pilco.py:146-154 over the rows of all ranks: the returns are gathered in rank (=
        # row) order, the quantile is the one process' quantile, every rank keeps its own rows' mask
        gcol = torch.tensor(run.gamma_full[:n_valid], dtype=torch.float32, device=dev)
        ret = run.sign * (R[:n_valid, :, 0] * gcol[:, None]).sum(0)
        sel, n_sel = _cvar_select(ret, _gather_rows(ret, run.process_group, world).cpu().numpy(), run.cvar_eps)
        gfull = torch.tensor(run.gamma_full, dtype=torch.float64) * (run.sign / max(n_sel, 1))
        gw = (gfull.float().to(dev)[:, None] * sel.float()[None, :]).contiguous()
    loss = eng.weighted_sum(R, gw)[0]
    if world > 1:
        from .distributed import allreduce_sum_
        loss = allreduce_sum_(loss.reshape(1).clone(), run.process_group)[0]
    # the hooks get tensors of their own, cloned before the backward call (the engine's buffers are reused by the
    # next iteration; the reference hands out fresh tensors)
    states, actions, rewards = _as_lists(S, A, R, n_valid,
                                         clone=callable(run.on_rollout) or callable(run.on_iteration))
    if callable(run.on_rollout):
        run.on_rollout(i, states, actions, rewards, run.disc)
    g, _, _ = eng.backward(gw)
    if eng.info.get('mm_grid') or eng.info.get('mm_parts', 1) > 1:
        # sweeps whose workgroups meet at barriers: a barrier that timed out (workgroups not co-resident
        # after all -- another process on the device) leaves a garbage gradient and says so in status[1]
        bad = eng.sweep_failed()
        if world > 1:
            from .distributed import ints_over_ranks
            bad = bool(ints_over_ranks([1 if bad else 0], 'max', run.process_group, dev)[0])
        if bad:
            raise RuntimeError('adjoint sweep: a barrier between workgroups timed out')
    if world > 1:
        from .distributed import grad_allreduce, p2p_check
        grad_allreduce(run.process_group, dev)(g)     # RCCL on the compute stream (C ABI)
        # (peer-to-peer transport: a wait that timed out anywhere -- this gradient, or the per-step
        #  statistics of groups spread over the ranks -- fails the iteration on every rank)
        p2p_check(run.process_group, dev)
    if run.reg_weight > 0:
        # algorithms/mc_pilco.py:193-194: a function of the parameters alone, the same on every rank
        run.policy.zero_grad()
        regl = run.policy.regularization_loss()
        regl.backward()
        g.add_(torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                          for p in bundle.pol_params]), alpha=float(run.reg_weight))
        loss = loss + run.reg_weight * regl.detach()
    cache['step'] += 1
    grp = cache['group']
    E.clip_adam(bundle.pol_flat, g, cache['m'], cache['v'], cache['step'], grp['lr'],
                grp['betas'], grp['eps'], max_norm=run.clip_grad, rule=OPT.rule_of(cache))
    return loss, states, actions, rewards


def _next_start_states(run, exp):
    """New initial states for the next iteration (algorithms/mc_pilco.py:222-263)."""
    global episode_counter
    if exp is None:
        run.x0 = run.init_states.detach()
        return
    dev, world, rank, replay = run.dev, run.world, run.rank, run.replay
    n_draw = run.mm_groups if run.mm_groups is not None else run.N
    if not run.prioritized_replay:
        run.x0 = run.init_states = exp.sample_states(n_draw, timestep=run.step_idx_to_sample).to(dev, torch.float32)
        return
    # grow the tree with the episodes it has not seen (mc_pilco.py:224-231)
    if exp.n_samples() > x0_tree.size:
        for idx in range(episode_counter, exp.n_episodes()):
            for x in torch.as_tensor(np.asarray(exp.states[idx])):
                x0_tree.append(x, x0_tree.max_p)
                x0_tree.renormalize()
        episode_counter = exp.n_episodes()
    # sharded run: every rank holds the same tree and uses the same GLOBAL sample (drawn by rank 0), then keeps
    # its slice of the start states and importance weights; the priorities of the whole sample are updated
    # on every rank from the gathered norms (_update_priorities), so the replicas of the tree stay identical
    if world > 1:
        # ONE draw for all ranks: rank 0's (the replicas' numpy generators are not assumed in step -- a
        # single user draw on one rank would silently give the ranks different samples, weights and,
        # through _update_priorities, different trees)
        import torch.distributed as dist
        box = [None]
        if rank == 0:
            xs, idxs0, w = x0_tree.sample(n_draw * world, beta=replay['beta'])
            box = [(np.asarray(idxs0), np.asarray(w))]
        dist.broadcast_object_list(box, src=dist.get_global_rank(run.process_group, 0), group=run.process_group)
        replay['idxs'], w = box[0]
        if rank != 0:
            xs = x0_tree.replay_sample(replay['idxs'])
    else:
        xs, replay['idxs'], w = x0_tree.sample(n_draw * world, beta=replay['beta'])
    # (sic) max, not min: beta never drops below 1 (mc_pilco.py:240-241)
    replay['beta'] = max(1.0, replay['beta'] + run.priority_beta_increase)
    lo_r, hi_r = rank * n_draw, (rank + 1) * n_draw
    run.x0 = torch.stack([torch.as_tensor(x) for x in xs[lo_r:hi_r]]).to(dev, torch.float32)
    # (the reference multiplies the [B, 1] returns with the [B] weights -- a [B, B] product, mc_pilco.py:156-158:
    #  every row meets the weights of ALL sampled states, so a rank keeps the whole weight vector)
    replay['weights'] = torch.as_tensor(np.stack(w)).to(dev, torch.float32)


def _check_replicas_in_step(run):
    """End of a run that used the fused sharded tail: the replicas must have walked the same iterations -- a rank that
    resampled, switched arithmetic or stepped alone has different parameters from here on, and nothing later would
    notice."""
    tail = run.tail_used
    if tail is None:
        return
    from .distributed import P2PComm, ints_over_ranks
    mine = [run.n_opt_steps, run.n_resamples, 0 if run.precision is None else 1,
            int(run.cache['step']) if run.cache else 0,
            1 if (isinstance(tail, P2PComm) and tail.failed()) else 0]
    both = ints_over_ranks(mine + [-x for x in mine], 'max', run.process_group, run.dev)
    hi, lo = both[:len(mine)], [-x for x in both[len(mine):]]
    if hi[4]:
        raise RuntimeError('peer-to-peer exchange: a rank waited for a peer that did not arrive in time '
                           '(PMBRL_P2P_TIMEOUT_SPINS sets the wait)')
    if hi != lo:
        raise RuntimeError('sharded run: the ranks did not walk the same iterations (optimiser steps, resamplings, '
                           'arithmetic switches, Adam steps: max %s, min %s)' % (hi[:4], lo[:4]))


def _gather_rows(t, group, world):
    """The rows of every rank's `t` ([n, ...], the same n on every rank) in rank order, on every rank -- a tensor
    collective (no pickling, no host round trip beyond what the backend needs)."""
    import torch.distributed as dist
    parts = [torch.empty_like(t) for _ in range(world)]
    if dist.get_backend(group) == 'nccl':
        dist.all_gather(parts, t.contiguous(), group=group)
        return torch.cat(parts, 0)
    host = [torch.empty(t.shape, dtype=t.dtype) for _ in range(world)]     # (gloo groups: the CPU-transport tests)
    dist.all_gather(host, t.detach().cpu().contiguous(), group=group)
    return torch.cat(host, 0).to(t.device)


_GW_CACHE = {}


def _loss_weights(eng, gamma, sign, B_global, dev):
    """dL/dr[t,b] = -/+ gamma_t / B  (algorithms/mc_pilco.py:134-144,190), cached per shape."""
    key = (id(eng), tuple(gamma), sign, B_global)
    gw = _GW_CACHE.get(key)
    if gw is None:
        if len(_GW_CACHE) > 8:
            _GW_CACHE.clear()
        col = torch.tensor(gamma, dtype=torch.float64) * (sign / B_global)
        gw = col.float().to(dev)[:, None].expand(eng.H, eng.B).contiguous()
        _GW_CACHE[key] = gw
    return gw


def _update_priorities(replay, m_norms, mm_groups):
    """New priorities of the sampled start states from the per-step ||dL/da_t|| of their
    particles (mc_pilco.py:163-182; the reference collects the same norms with tensor hooks on
    actions[t], here they are an output of the adjoint sweep)."""
    tree, idxs = replay['tree'], replay['idxs']
    world = replay.get('world', 1)
    if world > 1:      # [H, B_local] -> [H, B_global] in rank (= row) order
        m_norms = _gather_rows(m_norms.t().contiguous(), replay['group'], world).t()
    if mm_groups is not None:
        m_norms = m_norms.reshape(-1, mm_groups * world, int(replay['N'] / mm_groups)).mean(-1)
    scores = m_norms.mean(0).detach().cpu().numpy() / tree.counts[idxs - tree.max_size + 1]
    priorities = (scores + replay['eps'])**replay['alpha']
    for idx, p in zip(idxs, priorities):
        tree.update(idx, p)
    tree.renormalize()



def _autograd_iteration(run, x0_, i):
    """The reference loop body on top of the autograd rollout.  On a sharded run (world > 1) this rank's rows are a
    slice of one global batch: the loss is the mean over the GLOBAL batch (CVaR: over the rows its global quantile
    keeps), the flat gradient is summed over the ranks before the clip, the regulariser -- a function of the
    replicated parameters -- counts once."""
    policy, pegasus, world, replay, disc = run.policy, run.pegasus, run.world, run.replay, run.disc
    dkw = {}
    if world > 1:
        dkw = {k: v for k, v in run.dist_kw.items() if v is not None}
        # every rank keeps the horizon of the slowest one and retries / raises with it (rollout(): agree_group)
        dkw['agree_group'] = run.process_group
    policy.zero_grad()
    run.opt.zero_grad()
    weighted = replay is not None and replay['idxs'] is not None
    norms_out = [] if weighted else None
    states, actions, rewards = RO.rollout(
        x0_, run.dynamics, policy, run.H, resample_state_noise=not pegasus,
        resample_action_noise=not pegasus, mm_states=run.mm_states, mm_rewards=run.mm_rewards,
        z_mm=run.z_mm if pegasus else None, z_rr=run.z_rr if pegasus else None, mm_groups=run.mm_groups,
        action_grad_norms_out=norms_out, **dkw, **run.rollout_kwargs)
    if callable(run.on_rollout):
        run.on_rollout(i, states, actions, rewards, disc)
    discounted = torch.stack([r * disc(t) for t, r in enumerate(rewards)])
    if run.value_func is not None:
        # terminal-value bootstrap (mc_pilco.py:136-140); dV/ds_H comes from pmbrl_mlp_grad_input
        # and enters the adjoint sweep as grad_states[H]
        Vend = run.value_func(states[-1], resample=False, return_samples=True)
        discounted = torch.cat([discounted, disc(run.H) * Vend.unsqueeze(0)], 0)
    returns = -discounted.sum(0) if run.maximize else discounted.sum(0)
    n_global = returns.shape[0] * world
    if run.cvar:
        rd = returns.detach()
        rd_all = (_gather_rows(rd, run.process_group, world) if world > 1 else rd).cpu().numpy()
        sel, n_global = _cvar_select(rd, rd_all, run.cvar_eps)
        returns = returns[sel]
    if weighted:
        # importance-sampling weights, broadcast exactly as the reference does ([B,1] * [n],
        # mc_pilco.py:156-158)
        returns = returns * replay['weights']
    if world == 1:
        loss = returns.mean()
        if run.reg_weight > 0:
            loss = loss + run.reg_weight * policy.regularization_loss()
        loss.backward()
    else:
        if weighted and returns.dim() == 2:
            n_global = n_global * returns.shape[1]     # (the reference's [B, 1] * [B] broadcast: a mean over [B, B])
        loss = returns.sum() / max(n_global, 1)
        if run.reg_weight > 0:
            loss = loss + (run.reg_weight / world) * policy.regularization_loss()
        loss.backward()
        from .distributed import grad_allreduce, p2p_check
        params = [p for p in policy.parameters() if p.requires_grad]
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])
        tot = torch.cat([flat, loss.detach().reshape(1)])
        grad_allreduce(run.process_group, tot.device)(tot)
        p2p_check(run.process_group, tot.device)
        off = 0
        for p in params:
            p.grad = tot[off:off + p.numel()].reshape(p.shape).clone()
            off += p.numel()
        loss = tot[-1]
    if weighted:
        _update_priorities(replay, norms_out[0][:len(actions)], run.mm_groups)
    if run.clip_grad is not None:
        torch.nn.utils.clip_grad_norm_(policy.parameters(), run.clip_grad)
    run.opt.step()
    return loss.detach(), states, actions, rewards
