"""The launch sequence of pmbrl_rollout_fwd / pmbrl_rollout_bwd(_adam), pinned per call form (pmbrl.hip: SweepForm, the
stage functions of the two calls).  Each form records the forward call alone in one engine.Graph and the adjoint call
alone in another; the graphs' node counts -- kernels, memsets, event record / wait pairs -- are constants measured
before the two calls were split into stages (DESIGN_LOG.md), exact, and three replayed iterations leave parameters, Adam
moments, loss and status bit-equal to three eager iterations of a second engine.  Uses the Python surface only.

Wide external moment matching (6 < D <= 32, pm_mmw_*_kernel) is the form `wide_ext` below; the two-rank span forms
are tests/test_gpu_span.py and tests/test_gpu_two_ranks.py (a host collective cannot be recorded)."""
import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

ONE_GROUP = dict(mm_groups=0)      # one moment-matching group over all rows: it spans workgroups
# ... of the cart-pole shape (2 x 200 units: the sweeps' prologue form needs their wide activation rows), 80 rows, 6 steps
SPANNING = ('synthetic/cartpole_mm', dict(P=1, S=80, H=6))
NO_REG = {'PMBRL_REG': '0'}        # the latency-optimised family where the register-resident one would serve the plan
# id: (fixture, fixture overrides, environment, engine arguments, optimiser in the call, what plan_info must say)
FORMS = {
    'reg_plain': ('full200_nomm', {}, {}, {}, True, dict(reg=1, mm_mode=0)),
    'reg_split_groups': ('full200_mmg', {}, {}, {}, True, dict(reg=1, mm_mode=1, mm_parts=2)),
    'fast_plain': ('nomm_d4', {}, {}, {}, True, dict(fast=1, mm_mode=0)),
    'fast_mm': ('mmg_d4', {}, {}, {}, True, dict(fast=1, mm_mode=1, mm_parts=1)),
    'fast_mm_parts2': ('mmg_d4', {}, {'PMBRL_MM_PARTS': '2'}, {}, True, dict(fast=1, mm_mode=1, mm_parts=2)),
    'general': ('nomm_d4', {}, {}, dict(force_generic=True), True, dict(fast=0, mm_mode=0)),
    'learned_reward': ('learned_reward/lr_mcp_mmg', {}, {}, {}, True, dict(fast=0, mm_mode=1)),
    'perstep_switches_d4': ('mmg_d4', {}, {'PMBRL_MM_PERSTEP': '1', 'PMBRL_MM_PARTS': '1'}, {}, True, dict(mm_parts=1)),
    'external_perstep': ('mmg_h40', ONE_GROUP, {'PMBRL_MM_MODE2': '1', 'PMBRL_MM_PARTS': '1'}, {}, True, dict(mm_mode=2)),
    'wide_ext': ('c5_mm_d12', ONE_GROUP, {'PMBRL_MM_PARTS': '1'}, {}, True, dict(mm_mode=2)),
    'spanning_perstep': SPANNING + ({'PMBRL_MM_PERSTEP': '1', 'PMBRL_MM_PARTS': '1'}, {}, True, dict(mm_mode=3, mm_grid=0)),
    'spanning_barrier': SPANNING + ({'PMBRL_MM_PARTS': '1'}, {}, True, dict(mm_mode=3, mm_grid=1)),
    'pipelined_dw': ('nomm_d4', {}, {'PMBRL_DW_PIPE': '5,4,3'}, {}, True, dict(dw_pipe=3)),
    'loss_launch': ('full200_nomm', {}, {'PMBRL_FUSE_LOSS': '0'}, {}, True, dict(reg=1)),
    'no_optimiser': ('full200_nomm', {}, {}, {}, False, dict(reg=1)),
    # ... and one form per instance table that the forms above leave out, shape-specialised and generic (KERNELS below)
    'lo_shaped_lean': ('full200_nomm', {}, NO_REG, {}, True, dict(fast=1, reg=0, mm_mode=0, precision='split_f16', stages=(4, 3))),
    'lo_shaped_mm_parts2': ('full200_mmg', {}, NO_REG, {}, True, dict(fast=1, reg=0, mm_mode=1, mm_parts=2, precision='split_f16')),
    'lo_split_bf16': ('full200_nomm', {}, {}, dict(precision='split'), True, dict(fast=1, reg=0, precision='split', stages=(4, 3))),
    'lo_f32_shaped': ('full200_nomm', {}, {}, dict(precision='f32'), True, dict(fast=1, reg=0, precision='f32', stages=(7, 6))),
    'lo_f32_generic': ('nomm_d4', {}, {}, dict(precision='f32'), True, dict(fast=1, precision='f32', stages=(2, 2))),
    'general_f32': ('nomm_d4', {}, {}, dict(force_generic=True, precision='f32'), True, dict(fast=0, mm_mode=0, precision='f32')),
    'general_tanh': ('activations/act_tanh_d4', {}, {}, {}, True, dict(fast=0, mm_mode=0, precision='split_f16')),
    'lo_rows64_split': ('dcp200_mmg50', {}, {'PMBRL_MM_PARTS': '1'}, {}, True, dict(fast=1, row_tiles=4, mm_mode=1, mm_parts=1, precision='split_f16')),
    'lo_tree': ('synthetic/cartpole_mm', dict(P=1, S=144, H=6), NO_REG, {}, True, dict(fast=1, reg=0, mm_mode=1, mm_parts=9, precision='split_f16')),
}
# graph nodes of (forward call, adjoint call), measured on the commit before the split: exact, no margin
NODES = {
    'external_perstep': (84, 85),
    'fast_mm': (5, 5),
    'fast_mm_parts2': (7, 7),
    'fast_plain': (4, 4),
    'general': (4, 4),
    'learned_reward': (5, 5),
    'loss_launch': (4, 6),
    'no_optimiser': (4, 4),
    'perstep_switches_d4': (5, 5),
    'pipelined_dw': (4, 10),
    'reg_plain': (4, 5),
    'reg_split_groups': (6, 7),
    'spanning_barrier': (6, 8),
    'spanning_perstep': (11, 12),
    'wide_ext': (24, 25),
    # (the forms added with the instance tables: counted on the commit before them)
    'general_f32': (4, 4),
    'general_tanh': (4, 4),
    'lo_f32_generic': (4, 4),
    'lo_f32_shaped': (4, 4),
    'lo_rows64_split': (5, 6),
    'lo_shaped_lean': (4, 5),
    'lo_shaped_mm_parts2': (7, 8),
    'lo_split_bf16': (4, 5),
    'lo_tree': (8, 8),
}
# The sweep kernels of each form's forward and adjoint call, (variant of Engine.sweep_kernels(), name) each: what the
# commit before the instance tables launched, from a rocprofv3 --kernel-trace of every form there (mangled names; the
# trace names the kernel descriptor, NAME.kd, the runtime the kernel, NAME)
KERNELS = {
    'external_perstep': (('ext', '_Z19pm_rollout_fwd_fastILi1ELi1ELi1ELi1E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs'),
                          ('ext', '_Z19pm_rollout_bwd_fastILi1ELi1ELi1ELi1E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs')),
    'fast_mm': (('mm', '_Z19pm_rollout_fwd_fastILi1ELi1ELi1ELi2E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs'),
                 ('mm', '_Z19pm_rollout_bwd_fastILi1ELi1ELi1ELi2E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs')),
    'fast_mm_parts2': (('mm', '_Z19pm_rollout_fwd_fastILi1ELi1ELi1ELi2E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs'),
                        ('mm', '_Z19pm_rollout_bwd_fastILi1ELi1ELi1ELi2E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs')),
    'fast_plain': (('lean', '_Z19pm_rollout_fwd_fastILi1ELi1ELi1ELi0E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs'),
                    ('lean', '_Z19pm_rollout_bwd_fastILi1ELi1ELi1ELi0E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs')),
    'general': (('lean', '_Z14pm_rollout_fwdILi1ELi2ELi0ELb0EEv11RolloutArgs'),
                 ('lean', '_Z14pm_rollout_bwdILi1ELi2ELi0ELb0EEv11RolloutArgs')),
    'general_f32': (('lean', '_Z14pm_rollout_fwdILi1ELi0ELi0ELb0EEv11RolloutArgs'),
                     ('lean', '_Z14pm_rollout_bwdILi1ELi0ELi0ELb0EEv11RolloutArgs')),
    'general_tanh': (('lean', '_Z14pm_rollout_fwdILi1ELi2ELi0ELb1EEv11RolloutArgs'),
                      ('lean', '_Z14pm_rollout_bwdILi1ELi2ELi0ELb1EEv11RolloutArgs')),
    'learned_reward': (('lean', '_Z14pm_rollout_fwdILi1ELi2ELi0ELb0EEv11RolloutArgs'),
                        ('lean', '_Z14pm_rollout_bwdILi1ELi2ELi0ELb0EEv11RolloutArgs')),
    'lo_f32_generic': (('lean', '_Z19pm_rollout_fwd_fastILi1ELi2ELi2ELi0E7PfShapeILi0ELi0ELi0ELi0ELi0EELi0EEv11RolloutArgs'),
                        ('lean', '_Z19pm_rollout_bwd_fastILi1ELi2ELi2ELi0E7PfShapeILi0ELi0ELi0ELi0ELi0EELi0EEv11RolloutArgs')),
    'lo_f32_shaped': (('lean', '_Z19pm_rollout_fwd_fastILi1ELi7ELi6ELi0E7PfShapeILi5ELi1ELi216ELi3ELi13EELi0EEv11RolloutArgs'),
                       ('lean', '_Z19pm_rollout_bwd_fastILi1ELi7ELi6ELi0E7PfShapeILi5ELi1ELi216ELi3ELi13EELi0EEv11RolloutArgs')),
    'lo_rows64_split': (('mm', '_Z19pm_rollout_fwd_fastILi4ELi4ELi3ELi2E7PfShapeILi6ELi1ELi240ELi3ELi13EELi2EEv11RolloutArgs'),
                         ('mm', '_Z19pm_rollout_bwd_fastILi4ELi4ELi3ELi2E7PfShapeILi6ELi1ELi240ELi3ELi13EELi2EEv11RolloutArgs')),
    'lo_shaped_lean': (('lean', '_Z19pm_rollout_fwd_fastILi1ELi4ELi3ELi0E7PfShapeILi5ELi1ELi240ELi3ELi13EELi2EEv11RolloutArgs'),
                        ('lean', '_Z19pm_rollout_bwd_fastILi1ELi4ELi3ELi0E7PfShapeILi5ELi1ELi240ELi3ELi13EELi2EEv11RolloutArgs')),
    'lo_shaped_mm_parts2': (('mm', '_Z19pm_rollout_fwd_fastILi1ELi4ELi3ELi2E7PfShapeILi4ELi1ELi240ELi3ELi13EELi2EEv11RolloutArgs'),
                             ('mm', '_Z19pm_rollout_bwd_fastILi1ELi4ELi3ELi2E7PfShapeILi4ELi1ELi240ELi3ELi13EELi2EEv11RolloutArgs')),
    'lo_split_bf16': (('lean', '_Z19pm_rollout_fwd_fastILi1ELi4ELi3ELi0E7PfShapeILi5ELi1ELi360ELi3ELi13EELi1EEv11RolloutArgs'),
                       ('lean', '_Z19pm_rollout_bwd_fastILi1ELi4ELi3ELi0E7PfShapeILi5ELi1ELi360ELi3ELi13EELi1EEv11RolloutArgs')),
    'lo_tree': (('mm', '_Z19pm_rollout_fwd_fastILi1ELi4ELi3ELi2E11PfShapeTreeILi4ELi1ELi240ELi3ELi13EELi2EEv11RolloutArgs'),
                 ('mm', '_Z19pm_rollout_bwd_fastILi1ELi4ELi3ELi2E11PfShapeTreeILi4ELi1ELi240ELi3ELi13EELi2EEv11RolloutArgs')),
    'loss_launch': (('reg', '_Z17pm_reg_fwd_kernelILb0ELi0ELb0EEv7RegArgs'),
                     ('reg', '_Z17pm_reg_bwd_kernelILb0ELi0ELb0EEv7RegArgs')),
    'no_optimiser': (('reg', '_Z17pm_reg_fwd_kernelILb0ELi0ELb0EEv7RegArgs'),
                      ('reg', '_Z17pm_reg_bwd_kernelILb0ELi0ELb0EEv7RegArgs')),
    'perstep_switches_d4': (('mm', '_Z19pm_rollout_fwd_fastILi1ELi1ELi1ELi2E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs'),
                             ('mm', '_Z19pm_rollout_bwd_fastILi1ELi1ELi1ELi2E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs')),
    'pipelined_dw': (('lean', '_Z19pm_rollout_fwd_fastILi1ELi1ELi1ELi0E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs'),
                      ('ext', '_Z19pm_rollout_bwd_fastILi1ELi1ELi1ELi1E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs')),
    'reg_plain': (('reg', '_Z17pm_reg_fwd_kernelILb0ELi0ELb0EEv7RegArgs'),
                   ('reg', '_Z17pm_reg_bwd_kernelILb0ELi0ELb0EEv7RegArgs')),
    'reg_split_groups': (('reg', '_Z17pm_reg_fwd_kernelILb0ELi4ELb0EEv7RegArgs'),
                          ('reg', '_Z17pm_reg_bwd_kernelILb0ELi4ELb0EEv7RegArgs')),
    'spanning_barrier': (('mmg', '_Z19pm_rollout_fwd_fastILi1ELi4ELi3ELi3E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs'),
                          ('mmg', '_Z19pm_rollout_bwd_fastILi1ELi4ELi3ELi3E7PfShapeILi0ELi0ELi0ELi0ELi0EELi2EEv11RolloutArgs')),
    'spanning_perstep': (('mm', '_Z19pm_rollout_fwd_fastILi1ELi4ELi3ELi2E7PfShapeILi4ELi1ELi240ELi3ELi13EELi2EEv11RolloutArgs'),
                          ('mm', '_Z19pm_rollout_bwd_fastILi1ELi4ELi3ELi2E7PfShapeILi4ELi1ELi240ELi3ELi13EELi2EEv11RolloutArgs')),
    'wide_ext': (('lean', '_Z14pm_rollout_fwdILi1ELi2ELi0ELb0EEv11RolloutArgs'),
                  ('lean', '_Z14pm_rollout_bwdILi1ELi2ELi0ELb0EEv11RolloutArgs')),
}


def check_kernels(form, eng):
    """The plan resolved the sweep kernels that the parent of the instance tables launched for this form.  The names
    are what plan creation resolved (pmbrl_plan_sweep_kernel), not what a launch used: that the launches use the resolved
    pointer was checked once, by tracing every form on both trees (DESIGN_LOG.md)."""
    got = eng.sweep_kernels()
    for adjoint, (variant, name) in enumerate(KERNELS[form]):
        assert got.get(variant, ('', ''))[adjoint] == name, (form, variant, got)


def build(form, monkeypatch):
    name, over, env, kw, with_adam, want = FORMS[form] if isinstance(form, str) else form
    from prob_mbrl_amd import engine as E
    from prob_mbrl_amd import problem as PB
    learned = name.startswith('learned_reward/')
    if name.startswith('synthetic/'):
        d = PB.synthetic_problem(name.split('/')[1], seed=0, data_seed=0, **over)
    else:
        d = dict(common.load(name.split('/')[-1]))
        for k, v in over.items():
            d[k] = np.asarray(v)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if learned:
        kw = dict(kw, reward_spec=E.LEARNED_REWARD)
    eng, args, _ = common.engine_from_fixture(d, torch.device(DEV), **kw)
    for k, v in want.items():
        assert eng.info[k] == v, (form, k, eng.info)
    H, B = int(d['H']), d['x0'].shape[0]
    gw = torch.tensor(common.loss_weights(d, B), device=DEV)
    params = args['pol_flat'].clone()
    args['pol_flat'] = params
    st = dict(params=params, exp_avg=torch.zeros_like(params), exp_avg_sq=torch.zeros_like(params),
              step=torch.zeros(1, dtype=torch.int64, device=DEV), loss=torch.full((1,), float('nan'), device=DEV))
    adam = dict(params=params, exp_avg=st['exp_avg'], exp_avg_sq=st['exp_avg_sq'], step=st['step'], lr=1e-3,
                betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, loss_out=st['loss']) if with_adam else None
    out = (torch.empty((H + 1, B, eng.D), device=DEV), torch.empty((H, B, eng.U), device=DEV),
           torch.empty((H, B, 1), device=DEV))
    fwd = lambda: eng.forward(**args, out=out)       # noqa: E731
    bwd = lambda: eng.backward(gw, adam=adam)        # noqa: E731
    return eng, st, fwd, bwd


def results(eng, st):
    torch.cuda.synchronize()
    return [t.clone() for t in (st['params'], st['exp_avg'], st['exp_avg_sq'], st['step'], st['loss'], eng.status,
                                eng.grad_flat)]


def same(a, b):
    # (bit equality: the loss of a call without the optimiser stays the NaN it was set to)
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def eager(form, monkeypatch, n=3):
    eng, st, fwd, bwd = build(form, monkeypatch)
    for _ in range(n):
        fwd()
        bwd()
    assert eng.valid_steps() == eng.H
    return results(eng, st)


@pytest.mark.parametrize('form', sorted(FORMS))
def test_call_form_records_the_same_launches_and_replays_bit_equal(form, monkeypatch):
    from prob_mbrl_amd import engine as E
    want = eager(form, monkeypatch)
    eng, st, fwd, bwd = build(form, monkeypatch)
    check_kernels(form, eng)
    p0 = st['params'].clone()
    gf = E.Graph(fwd, warmup=1)
    gb = E.Graph(bwd, warmup=1)
    counts = [(gf.num_nodes(), gb.num_nodes())]
    if form == 'reg_split_groups':
        # the recording taken twice in a row: a recording always carries the fill of the exchange granules, so the second
        # one has the same nodes
        gf, gb = E.Graph(fwd, warmup=0), E.Graph(bwd, warmup=0)
        counts.append((gf.num_nodes(), gb.num_nodes()))
    print('call-form nodes %r: %r,' % (form, counts[0]))
    # the warm-up calls took an optimiser step: back to the start, then three iterations from the recordings
    torch.cuda.synchronize()
    st['params'].copy_(p0)
    for k in ('exp_avg', 'exp_avg_sq', 'step'):
        st[k].zero_()
    for _ in range(3):
        gf.replay()
        gb.replay()
    got = results(eng, st)
    assert eng.valid_steps() == eng.H
    assert same(got, want)
    assert all(c == NODES.get(form) for c in counts), (form, counts, NODES.get(form))


def test_one_rank_span_is_deterministic(monkeypatch):
    """mm_span_ranks = 1: the exchange is the identity, no collective attached.  Replay is refused with a span, so eager
    only: two engines, bit-equal."""
    form = ('mmg_d4', {}, {}, dict(mm_span=(10, 0, 1, 0)), True, dict(mm_mode=2))
    a = eager(form, monkeypatch)
    b = eager(form, monkeypatch)
    assert same(a, b) and int(a[3]) == 3 and bool(torch.isfinite(a[4]).all())


@pytest.mark.parametrize('form,text', [
    ('external_perstep', 'grad_states with external moment matching: not offered'),
    ('spanning_perstep', 'grad_states with moment-matching groups spanning workgroups: not offered')])
def test_refused_adjoint_call_queues_nothing(form, text, monkeypatch):
    """grad_states where the moment matching runs between or across the sweep launches: refused with code -3 and the same
    message as ever.  The one intended change of the split into stages: the refusal used to come after the clearing
    of the gradient carry buffer (and, with reward moment matching, its adjoint launch) had been queued -- inside a
    recording under pmbrl_plan_set_replay -- and now comes before anything is: workspace and gradient keep the
    sentinel bytes written before the call."""
    from prob_mbrl_amd._lib import PmbrlError
    eng, st, fwd, bwd = build(form, monkeypatch)
    fwd()
    torch.cuda.synchronize()
    gw = torch.ones((eng.H, eng.B), device=DEV)
    gs = torch.zeros((eng.H + 1, eng.B, eng.D), device=DEV)
    # (nothing reads the workspace again: the call is refused)
    eng.workspace.fill_(0x55)
    eng.grad_flat.fill_(-7.0)
    status = eng.status.clone()
    with pytest.raises(PmbrlError) as e:
        eng.backward(gw, grad_states=gs)
    assert '(-3)' in str(e.value) and text in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert bool((eng.workspace == 0x55).all()) and bool((eng.grad_flat == -7.0).all())
    assert torch.equal(eng.status, status)
