"""The envelope of the register-resident sweep family (csrc/pmbrl_reg.h, pmbrl_reg_mm.h; the host side's
pm_reg_shape_ok / pm_reg_mm_shape_ok / pm_reg_plan_ok in csrc/pmbrl_reg.hip) as a table of small synthetic problems,
and the arithmetic both envelope tests judge them with:

  tests/test_reg_envelope_cases.py   (CPU) every case is well conditioned: the oracle's own fp32 run stays within a
                                     quarter of each bar of its fp64 run
  tests/test_gpu_reg_envelope.py     (GPU) every case against the fp64 oracle, on the family and with it switched off

One axis varies per case around the centre every other test of the family sits on (hidden width 200, D = 4, U = 1),
plus a few combined corners.  Cases are generated (prob_mbrl_amd.problem.synthetic_problem from a shape dictionary),
nothing is stored.  `inside` says on which side of the envelope the case lies; for a moment-matching case `layout` is
the (mm_parts, rows_per_wg, n_wg) the case was written for."""
import numpy as np
import torch

from oracle import ref_torch as R
from prob_mbrl_amd import problem as PB
from tests.common import rel  # noqa: F401  (the envelope tests use it through this module too)

# the project's bars (tests/test_gpu_kernels.py: TOL_TRAJ, TOL_GRAD)
TOL_TRAJ = 2e-5
TOL_GRAD = 1e-4
# the family against the latency-optimised kernels on the same problem: tests/test_gpu_kernels.py::test_rollout_parity_lean
# (no moment matching), tests/test_gpu_full_size.py::test_instantiations_agree_bitwise (with)
TOL_PAIR_PLAIN = 2e-5
TOL_PAIR_MM = 6e-5
# a slice (one parameter tensor, one state dimension, one step) below this share of the whole quantity's fp64 norm is
# judged on the global norm alone
SLICE_FLOOR = 1e-3


def _shape(width=200, D=4, U=1, rows=40, groups=0, H=5, reward=None, mm_rewards=None):
    """rows: the batch; groups > 0: moment matching of the states in that many groups of rows / groups"""
    if reward is None:
        reward = {4: 'cartpole', 5: 'cartpole', 6: 'double_cartpole'}.get(D, 'generic') if U == 1 else 'generic'
    mm = groups > 0
    P = groups if mm else rows
    assert rows % P == 0
    cfg = dict(D=D, U=U, pol_hid=[width, width], dyn_hid=[width, width], P=P, S=rows // P, H=H, mm=mm, reward=reward,
               maxU={'cartpole': 10.0, 'double_cartpole': 20.0, 'generic': 2.0}[reward])
    if mm_rewards is not None:
        cfg['mm_rewards'] = mm_rewards
    return cfg


def _case(cid, seed, inside=True, layout=None, hint=0, mods=(), **shape):
    return dict(id=cid, seed=seed, inside=inside, layout=layout, hint=hint, mods=tuple(mods), cfg=_shape(**shape))


def _mm(cid, seed, D, M, G, parts, H=4, inside=True, hint=0, **kw):
    """G groups of M rows; parts: workgroups per group the plan is expected to choose (1: one workgroup per group)"""
    rpw = -(-M // parts)
    layout = dict(mm_parts=parts, rows_per_wg=rpw, n_wg=G * parts) if inside else None
    return _case(cid, seed, inside=inside, layout=layout, hint=hint, D=D, rows=M * G, groups=G, H=H, **kw)


CASES = [
    # ---- hidden width: 13 output tiles = 193 .. 208 (net_plan: nt = (width + 15) / 16); 192 is 12 tiles, 209 is 14
    _case('w193', 1, width=193),                  # last tile: 1 valid column
    _case('w194', 0, width=194),
    _case('w207', 2, width=207),
    _case('w208', 0, width=208),                  # last tile full
    _case('w192-out', 3, inside=False, width=192),
    _case('w209-out', 0, inside=False, width=209),
    # ---- (D, U) without moment matching: D + U <= 8
    _case('d1u1', 4, D=1, U=1),
    _case('d2u1', 0, D=2, U=1),
    _case('d3u2', 5, D=3, U=2),
    _case('d4u4', 0, D=4, U=4),
    _case('d7u1', 6, D=7, U=1),
    _case('d1u7', 0, D=1, U=7),
    _case('d5u3', 7, D=5, U=3),
    _case('d5u1-cartpole', 0, D=5, U=1),          # the cart-pole reward on the expanded state
    _case('d8u1-out', 8, inside=False, D=8, U=1),
    _case('d5u4-out', 0, inside=False, D=5, U=4),
    # ---- rows: 16-row workgroups, ragged last workgroup
    _case('rows1', 9, rows=1),
    _case('rows15', 0, rows=15),
    _case('rows16', 10, rows=16),
    _case('rows17', 0, rows=17),
    _case('rows77', 11, rows=77),
    # ---- horizon: first and last steps are the special ones
    _case('h1', 0, H=1),
    _case('h2', 12, H=2),
    _case('h3', 0, H=3),
    _case('h12', 13, H=12),
    # ---- moment matching of the states, D = 4
    _mm('mm4-m16', 0, 4, 16, 3, 1),
    _mm('mm4-m7', 14, 4, 7, 4, 1, hint=7),        # one group per workgroup on request (two 7-row groups would fit 16 rows)
    _mm('mm4-m25', 0, 4, 25, 3, 2),               # 13 + 12
    _mm('mm4-m17', 15, 4, 17, 2, 2),              # 9 + 8
    _mm('mm4-m121', 0, 4, 121, 1, 8),             # 7 x 16 + 9
    _mm('mm4-m25-norr', 16, 4, 25, 2, 2, mm_rewards=False),
    # ---- D = 5
    _mm('mm5-m16', 17, 5, 16, 3, 1),
    _mm('mm5-m7', 0, 5, 7, 4, 1, hint=7, mm_rewards=False),
    _mm('mm5-m25-h1', 18, 5, 25, 3, 2, H=1),
    _mm('mm5-m25-h2', 0, 5, 25, 3, 2, H=2),
    _mm('mm5-m25-h10', 19, 5, 25, 3, 2, H=10),
    _mm('mm5-m17', 0, 5, 17, 2, 2),
    _mm('mm5-m121', 20, 5, 121, 1, 8),
    # ---- D = 6 (the double cart-pole reward)
    _mm('mm6-m16', 0, 6, 16, 3, 1),
    _mm('mm6-m25', 21, 6, 25, 3, 2),
    _mm('mm6-m17-norr', 0, 6, 17, 2, 2, mm_rewards=False),
    _mm('mm6-m121', 22, 6, 121, 1, 8, H=3),
    _mm('mm6-m16-h1', 23, 6, 16, 2, 1, H=1),
    # ---- ONE group over the batch, D = 4: the two-level exchange (25 parts of 16 rows, 2 collectors)
    _mm('mm4-tree-b400', 24, 4, 400, 1, 25, H=4),
    # ---- moment matching just outside
    _mm('mm3-m16-out', 25, 3, 16, 3, 1, inside=False),
    _mm('mm7-m16-out', 0, 7, 16, 3, 1, inside=False),
    _mm('mm5-m130-out', 26, 5, 130, 1, 9, inside=False, H=3),     # more than 8 parts of 16 rows, no two-level form at D = 5
    _mm('mm4-m7x2-out', 0, 4, 7, 4, 1, inside=False),             # two whole groups per workgroup: the other family's
    # ---- combined corners
    _case('w193-d5u3-rows17-h3', 27, width=193, D=5, U=3, rows=17, H=3),
    _case('w208-d1u7-rows77-h2', 28, width=208, D=1, U=7, rows=77, H=2),
    _mm('w207-mm6-m25-h2', 29, 6, 25, 2, 2, H=2, width=207),
    _mm('w194-mm5-m17', 30, 5, 17, 2, 2, width=194),
    _mm('w193-mm4-m16-h1', 31, 4, 16, 2, 1, H=1, width=193),
]

# ---- saturation of the family's own transcendentals (pr_tanh, pr_sigmoid_neg), on one plain and one moment-matching case
SAT_POLICY_FACTOR = 10.0
SAT_NOISE_SCALES = (0.3, 8.0, 30.0)
SAT_LOGSTD_FACTOR = 10.0
SAT_LOGSTD_SHIFT = (110.0, -110.0, 0.0)
SAT_CASES = [
    _case('sat-tanh-w193', 32, width=193, rows=48, H=6, mods=('sat_policy',)),
    _mm('sat-tanh-mm5-m25', 33, 5, 25, 2, 2, H=6, mods=('sat_policy',)),
    _case('sat-logstd-w193-d4u3', 34, width=193, D=4, U=3, rows=48, H=6, mods=('sat_logstd',)),
    _mm('sat-logstd-mm5u3-m25', 35, 5, 25, 2, 2, H=6, U=3, mods=('sat_logstd',)),
]
# ---- a non-finite value mid horizon: one state dimension, decoupled from both networks and the reward, drifts by 5e37 a step
DRIFT_DIM = 3
OVERFLOW_CASES = [
    _case('overflow-plain', 36, rows=40, H=12, mods=('drift',)),
    _mm('overflow-mm4-m16', 37, 4, 16, 3, 1, H=12, mods=('drift',)),
]

ALL_CASES = CASES + SAT_CASES + OVERFLOW_CASES
assert len({c['id'] for c in ALL_CASES}) == len(ALL_CASES)
assert 2 * sum(c['seed'] != 0 for c in ALL_CASES) >= len(ALL_CASES)


def ids(cases):
    return [c['id'] for c in cases]


def problem(case, drift=5e37):
    """drift: what the decoupled dimension of an overflow case gains per step"""
    d = PB.synthetic_problem(case['cfg'], seed=case['seed'])
    D, U = case['cfg']['D'], case['cfg']['U']
    for m in case['mods']:
        if m == 'sat_policy':
            # the policy's last layer (weights and bias) scaled, and the rows of the policy's frozen noise scaled in three
            # classes: the head output u = mean + z std covers |u| < 2 .. |u| > 44 in ONE run.  (The layer's scale alone
            # moves all rows together -- u is its bias plus a few per cent of spread: a factor that puts a tenth of the
            # entries beyond 44 leaves none below 2)
            d['pol_W2'] = d['pol_W2'] * np.float32(SAT_POLICY_FACTOR)
            d['pol_b2'] = d['pol_b2'] * np.float32(SAT_POLICY_FACTOR)
            B = d['pol_z'].shape[0]
            d['pol_z'] = d['pol_z'] * np.asarray(SAT_NOISE_SCALES, dtype=np.float32)[np.arange(B) % len(SAT_NOISE_SCALES)][:, None]
        elif m == 'sat_logstd':
            # the log-std half of both heads: scaled, and its biases moved to +-SAT_LOGSTD_SHIFT by turns (every third unit
            # stays where it was): ls - max_log_std from below -80 to above +80, whole units at either end of the clamp
            for pre, n in (('pol', U), ('dyn', D)):
                W, b = d[pre + '_W2'].copy(), d[pre + '_b2'].copy()
                W[n:] *= np.float32(SAT_LOGSTD_FACTOR)
                b[n:] = b[n:] * np.float32(SAT_LOGSTD_FACTOR) + np.asarray(SAT_LOGSTD_SHIFT, dtype=np.float32)[np.arange(n) % 3]
                d[pre + '_W2'], d[pre + '_b2'] = W, b
        elif m == 'drift':
            # (tests/test_gpu_full_size.py::test_device_detects_a_mid_horizon_failure_..., on this family's shapes)
            k = DRIFT_DIM
            assert D == 4 and bool(d['rew_expand'])
            for key in ('pol_W0', 'dyn_W0'):
                W = d[key].copy()
                W[:, k] = 0.0
                d[key] = W
            C = np.asarray(d['rew_C']).copy()
            C[:, 2] = 0.0      # columns of the expanded state [others (0, 1, 3) | sin | cos]: dimension 3 is column 2
            d['rew_C'] = C
            my = d['dyn_my'].copy()
            my[k] = drift
            d['dyn_my'] = my
        else:
            raise KeyError(m)
    return d


def oracle(d, dtype, n_steps=None):
    """oracle/ref_torch.py: iteration on problem d -> dict of numpy arrays (states [n + 1, B, D], actions [n, B, U],
    rewards [n, B], loss, grad) and the policy head's pre-squash output u [n, B, U], log-std arguments
    ls - max_log_std of the policy [n, B, U] and of the dynamics [n, B, D] head"""
    x0, pol, dyn, spec, meta, z_mm, z_rr, gamma = R.problem_from_npz(d, dtype)
    loss, g, (S, A, Rw) = R.iteration(x0, pol, dyn, spec, meta['H'], gamma, meta['maximize'], meta['mm_states'],
                                      meta['mm_rewards'], meta['mm_groups'], z_mm, z_rr, meta['infer_ns'], n_steps=n_steps)
    out = dict(states=torch.stack(S).detach().numpy(), actions=torch.stack(A).detach().numpy(),
               rewards=torch.stack(Rw).detach().numpy()[..., 0], loss=float(loss), grad=g.numpy())
    with torch.no_grad():
        us, lp, ld = [], [], []
        # (angle features and activations as policy_forward / dynamics_forward apply them: tests/general_envelope_cases.py
        #  has cases with both; none of this module's has either)
        for t in range(len(A)):
            o = R.mlp_forward(R.to_complex(S[t], pol.get('angle_dims', [])), pol['weights'], pol['masks'], pol['keep'], t,
                              pol.get('act', 0))
            U = o.shape[-1] // 2
            us.append(o[:, :U] + pol['z'][:o.shape[0]] * R.clamp_log_std(o[:, U:]).exp())
            lp.append(o[:, U:] - R.LOG_MAX_STD)
            xin = (R.to_complex(torch.cat([S[t], A[t]], -1), dyn.get('angle_dims', [])) - dyn['mx']) * dyn['iSx']
            o = R.mlp_forward(xin, dyn['weights'], dyn['masks'], dyn['keep'], t, dyn.get('act', 0))
            ld.append(o[:, o.shape[-1] // 2:] - R.LOG_MAX_STD)
        out.update(u=torch.stack(us).numpy(), ls_pol=torch.stack(lp).numpy(), ls_dyn=torch.stack(ld).numpy())
    return out


def split_drift(o):
    """an overflow case's run with the drifting dimension taken out of the states (it would be their whole norm) and
    kept as a quantity of its own"""
    o = dict(o)
    keep = [j for j in range(o['states'].shape[-1]) if j != DRIFT_DIM]
    o['drift'] = o['states'][..., DRIFT_DIM]
    o['states'] = o['states'][..., keep]
    return o


def param_slices(d):
    """(name, slice) of every policy tensor inside the flat gradient: the order of problem.flat_params"""
    out, o = [], 0
    for i in range(int(d['pol_n_layers'])):
        for k in ('W', 'b'):
            n = int(np.asarray(d['pol_%s%d' % (k, i)]).size)
            out.append(('%s%d' % (k, i), slice(o, o + n)))
            o += n
    return out


def global_errors(got, ref):
    """got, ref: dicts with states / actions / rewards / loss / grad -> relative errors on the whole quantities"""
    e = {k: rel(got[k], ref[k]) for k in ('states', 'actions', 'rewards', 'grad')}
    e['loss'] = abs(got['loss'] - ref['loss']) / max(abs(ref['loss']), 1e-300)
    return e


BARS = dict(states=TOL_TRAJ, actions=TOL_TRAJ, rewards=TOL_TRAJ, loss=TOL_TRAJ, grad=TOL_GRAD)


def slice_errors(d, got, ref):
    """Each policy tensor of the gradient, each state dimension, each step of the states / actions / rewards: the
    relative error on the slice's OWN fp64 norm -> {slice name: (error, bar)}.  Slices whose fp64 norm is below
    SLICE_FLOOR of the whole quantity's are left to the global norm."""
    out = {}

    def put(name, a, b, whole, bar):
        nb = np.linalg.norm(np.asarray(b, dtype=np.float64))
        if nb >= SLICE_FLOOR * whole and nb > 0.0:
            out[name] = (rel(a, b), bar)
    ng = np.linalg.norm(ref['grad'])
    for name, sl in param_slices(d):
        put('grad.' + name, got['grad'][sl], ref['grad'][sl], ng, TOL_GRAD)
    ns = np.linalg.norm(ref['states'])
    for j in range(ref['states'].shape[-1]):
        put('states.dim%d' % j, got['states'][..., j], ref['states'][..., j], ns, TOL_TRAJ)
    for k in ('states', 'actions', 'rewards'):
        nk = np.linalg.norm(ref[k])
        for t in range(ref[k].shape[0]):
            put('%s.step%d' % (k, t), got[k][t], ref[k][t], nk, TOL_TRAJ)
    return out


def worst(sl, prefix):
    """(name, error) of the worst slice whose name starts with prefix"""
    items = [(k, v[0]) for k, v in sl.items() if k.startswith(prefix)]
    return max(items, key=lambda kv: kv[1]) if items else ('-', 0.0)


def saturation_shares(case, o64):
    """What share of the fp64 oracle's head values lies where: the conditions the saturation cases are written for
    (asserted on the CPU, tests/test_reg_envelope_cases.py)"""
    if 'sat_policy' in case['mods']:
        u = np.abs(o64['u'])
        return {'|u| > 44': float(np.mean(u > 44)), '15 < |u| <= 44': float(np.mean((u > 15) & (u <= 44))),
                '|u| < 2': float(np.mean(u < 2))}
    if 'sat_logstd' in case['mods']:
        return {'%s: ls - max %s' % (k, s): float(np.mean(o64['ls_' + k] < -80 if s == '< -80' else o64['ls_' + k] > 80))
                for k in ('pol', 'dyn') for s in ('< -80', '> 80')}
    return {}
