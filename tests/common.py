"""Shared helpers for the parity tests: the fixture lists, fixture -> oracle call, fixture -> Engine inputs,
fixture -> reference-shaped modules, and the bars more than one file asserts."""
import glob
import math
import os
import socket

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SUBDIRS = ('', 'activations', 'learned_reward', 'bdropout')
# tests/golden/activations (tools/make_golden_activations.py), by kind
ACT_ITER = ['act_tanh_d4', 'act_silu_d4', 'act_mixed_nets_d4', 'act_silu_mmg_d4', 'act_tanh_mm1_d4', 'act_silu_full200',
            'act_tanh_w48_24', 'act_silu_angles_d4', 'act_tanh_sat']
ACT_MCP = ['act_mcp_tanh', 'act_mcp_silu_mmg', 'act_critic_tanh']
ACT_BNN = ['act_bnn_tanh', 'act_bnn_silu']
# tests/golden/bdropout (tools/make_golden_bdropout.py)
BD_FIT = ['bd_nll_relu', 'bd_unit_tanh', 'bd_mixed_silu', 'bd_gmm', 'bd_resample_off']      # per-iteration idx and losses
BD_OPTS = ['bd_nll_relu_decoupled', 'bd_nll_relu_prioritized']
BD_CRITIC = ['bd_critic']


def fixture_names(kind=None):
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, '*.npz')))
    if kind == 'iter':
        return [n for n in names if not n.startswith(('mcp_', 'ext_', 'standalone_', 'bnn_', 'experience_', 'critic_', 'bnnopt_',
                                                      'trunc_', 'draw_', 'unit_'))]
    if kind == 'bnn':
        return [n for n in names if n.startswith('bnn_')]
    if kind == 'standalone':
        return [n for n in names if n.startswith('standalone_')]
    if kind == 'mcp':
        return [n for n in names if n.startswith('mcp_')]
    return names


def lr_names(kind=None):
    """Fixtures of tests/golden/learned_reward (tools/make_golden_learned_reward.py) of one kind: 'iter' (one rollout +
    gradient, frozen noise), 'step' (the same with the head's noise redrawn at every step: dyn_z [H, B, D + 1]), 'mcp'
    (iterations of the real mc_pilco); None: all."""
    ns = sorted(f[:-4] for f in os.listdir(os.path.join(GOLDEN, 'learned_reward')) if f.endswith('.npz'))
    if kind is None:
        return ns
    pre = {'mcp': 'lr_mcp', 'step': 'lr_step'}.get(kind)
    return [n for n in ns if n.startswith(pre)] if pre else [n for n in ns if not n.startswith(('lr_mcp', 'lr_step'))]


def path_of(name):
    """The fixture's file, in tests/golden or one of its sub-directories."""
    paths = [os.path.join(GOLDEN, sub, name + '.npz') for sub in SUBDIRS]
    return next(p for p in paths if os.path.exists(p))


def load(name):
    from oracle import ref_torch
    d = ref_torch.load_fixture(path_of(name))
    if 'dyn_gmm_n' in d and int(d['dyn_gmm_n']) > 1 and 'dyn_ucat' not in d:
        d = dict(d)
        d['dyn_ucat'] = gmm_uniforms(d)
    return d


def gmm_uniforms(d):
    """Mixture head: the reference draws the component of every (step, row) from torch's generator and the fixture
    records the INDEX; the device draws by inverse CDF from a uniform.  The uniforms that reproduce the recorded
    indices: midpoints of the drawn component's CDF interval, the softmax taken from the fp64 oracle run."""
    k_soft = []
    oracle_iteration(d, dyn_update=dict(k_soft_out=k_soft))
    ks = torch.stack(k_soft[:int(d['H'])]).numpy()          # [H, B, n]
    kidx = np.asarray(d['dyn_kidx'])
    cdf = np.cumsum(ks, -1)
    hi = np.take_along_axis(cdf, kidx[..., None], -1)[..., 0]
    lo = hi - np.take_along_axis(ks, kidx[..., None], -1)[..., 0]
    assert np.all(hi - lo > 1e-4), 'a drawn component has (almost) no probability: midpoint not robust'
    return np.clip(0.5 * (lo + hi), 0.0, 1.0 - 1e-7).astype(np.float32)


from prob_mbrl_amd.problem import engine_from_problem as engine_from_fixture  # noqa: E402,F401
from prob_mbrl_amd.problem import loss_weights  # noqa: E402,F401


def oracle_iteration(d, dtype=torch.float64, with_value=False, dyn_update=None, **kw):
    """oracle.ref_torch.iteration on a rollout fixture, with its activations and its reward (analytic or learned):
    (loss, flat gradient, (S, A, R)).  with_value: bootstrap with the fixture's critic where it has one; dyn_update:
    entries put into the dynamics dict first (z, z_grad, k_soft_out); kw: iteration's own (n_steps, cvar_eps, ...)."""
    from oracle import ref_torch as R
    x0, pol, dyn, spec, meta, z_mm, z_rr, gamma = R.problem_from_npz(d, dtype)
    dyn.update(dyn_update or {})
    if with_value and 'val_n_layers' in d:
        kw.update(value=R.value_from_npz(d, dtype), gamma_H=float(gamma[-1]))
    return R.iteration(x0, pol, dyn, spec, meta['H'], gamma, meta['maximize'], meta['mm_states'], meta['mm_rewards'],
                       meta['mm_groups'], z_mm, z_rr, meta['infer_ns'], **kw)


def dyn_first_layer_max(d, S, A):
    """Largest |pre-activation| of the dynamics model's first layer over a trajectory (lists of fp64 tensors)."""
    mx, iSx = (torch.tensor(np.asarray(d[k]), dtype=torch.float64) for k in ('dyn_mx', 'dyn_iSx'))
    W, b = (torch.tensor(np.asarray(d[k]), dtype=torch.float64) for k in ('dyn_W0', 'dyn_b0'))
    return max(float((((torch.cat([s, a], -1) - mx) * iSx) @ W.t() + b).abs().max()) for s, a in zip(S, A))


def kink_margin(d):
    """The smallest |pre-activation| among the units that a replay of the fit d keeps (mask 1, or no dropout), over all
    hidden layers and iterations.  ReLU's derivative jumps at 0: a kept unit whose pre-activation lies closer to 0 than
    single precision resolves it takes either side there, and the gradient of everything in front of it with it."""
    from oracle import ref_torch as R
    pre = []
    R.bnn_train(d, torch.float64, pre=pre)
    small = math.inf
    for it, zs in enumerate(pre):
        for l, z in enumerate(zs):
            kept = np.ones(z.shape, bool) if int(d['kind%d' % l]) == R.NONE else np.asarray(d['hard%d_it%d' % (l, it)]) > 0
            small = min(small, float(np.abs(z.numpy())[kept].min()))
    return small


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def flat_grad(pol):
    """The gradient of a Policy module's Linear layers, flat in the order of problem.flat_params."""
    lins = [m for m in pol.model._modules.values() if isinstance(m, torch.nn.Linear)]
    return torch.cat([t.grad.reshape(-1) for l in lins for t in (l.weight, l.bias)]).cpu().numpy()


def loss_of(rewards, d):
    """mc_pilco's loss (algorithms/mc_pilco.py:134-144,190) of a list of reward tensors, with the fixture's discounts."""
    gamma = [float(g) for g in d['gamma']]
    disc = torch.stack([r * gamma[i] for i, r in enumerate(rewards)])
    return (-disc.sum(0) if bool(d['maximize']) else disc.sum(0)).mean()


def assert_mcp_update(final, init, d):
    """The policy parameters `final` after an mc_pilco fixture's iterations, started from `init`, against the
    reference's.  Returns (err, g_abs, cos) for what a caller reports or asserts beyond this.

    Adam divides by |g_i|: an element whose gradient is tiny against the gradient's rms moves by up to lr per step on
    the SIGN of rounding noise -- in any fp32-class arithmetic, the reference's own included.  The bar per element is
    the north star's 1e-4 (of the gradient's rms) pushed through Adam's normalisation: n lr eps_g / (|g_i| + eps),
    capped at n lr; |g_i| from the reference's second-moment estimate.  (The 32-unit fixtures never need the term:
    2e-6 covers them; of the 41 602 parameters of the 2 x 200 policy a few dozen have |g_i| < 1e-3 rms.)
    FROZEN (round 6): these bars may only tighten.  The per-element bar admits whatever Adam can reach for an element
    whose gradient is rounding noise; what guards against a systematic error is the update direction, a quantity
    rounding does not move: the cosine between this run's total parameter update and the reference's."""
    final, init = np.asarray(final, np.float64), np.asarray(init, np.float64)
    ref = np.asarray(d['ref32_mcp_final'], np.float64)
    n_it, lr = int(d['mcp_n_iters']), float(d['mcp_lr'])
    g_abs = np.sqrt(np.asarray(d['ref32_mcp_exp_avg_sq'], np.float64) / (1.0 - 0.999 ** n_it))
    eps_g = 1e-4 * np.sqrt(np.mean(g_abs ** 2))
    tol = 1e-4 * np.abs(ref) + 2e-6 + n_it * lr * np.minimum(1.0, eps_g / (g_abs + 1e-8))
    err = np.abs(final - ref)
    assert np.all(err <= tol), (int((err > tol).sum()), float((err - tol).max()), float(err.max()))
    upd, upd_ref = final - init, ref - init
    cos = float(upd @ upd_ref / (np.linalg.norm(upd) * np.linalg.norm(upd_ref)))
    assert cos > 1.0 - 1e-7, cos          # (measured: 1 - 6.3e-9 at worst, mcp_mm1)
    return err, g_abs, cos


def act_module(code):
    """The torch module class of an activation code of prob_mbrl_amd/activations.py."""
    from prob_mbrl_amd import activations as ACT
    return {ACT.RELU: torch.nn.ReLU, ACT.TANH: torch.nn.Tanh, ACT.SILU: ACT.Swish}[int(code)]


def modules_from_fixture(d, name, device='cuda:0', learned=False):
    """Build prob_mbrl_amd Policy / DynamicsModel (reference-shaped modules) holding the
    fixture's weights, normalisation, frozen masks and noise, with its activations (pol_act / dyn_act; none: ReLU), its
    mixture head and its per-unit rates where it has them.  learned: reward_func=None, the head 2 (D + 1) wide over
    DiagGaussianDensity(D + 1); else the reward module is chosen by the fixture's name."""
    from functools import partial

    import prob_mbrl_amd as pm
    dev = torch.device(device)
    B, D = d['x0'].shape
    U = d['pol_z'].shape[1]
    npl, ndl = int(d['pol_n_layers']), int(d['dyn_n_layers'])
    pol_hid = [d['pol_W%d' % i].shape[0] for i in range(npl - 1)]
    dyn_hid = [d['dyn_W%d' % i].shape[0] for i in range(ndl - 1)]
    pad = [int(a) for a in np.asarray(d['pol_angle_dims'])]
    dad = [int(a) for a in np.asarray(d['dyn_angle_dims'])]
    if learned:
        rew = None
    elif name.startswith(('dcp', 'angles_dcp', 'gmm_d6')):
        rew = pm.rewards.DoubleCartpoleReward(pole1_length=torch.tensor(0.6),
                                              pole2_length=torch.tensor(0.6))
    elif name.startswith('pend'):
        rew = pm.rewards.PendulumReward(pole_length=torch.tensor(1.0))
    elif name.startswith('rdv') or name.endswith('_u4'):
        rew = pm.rewards.RendezvousReward()
    elif name.startswith('c5'):
        rew = pm.rewards.LinearFeatureReward(torch.tensor(np.asarray(d['rew_C'], dtype=np.float32)),
                                             torch.tensor(np.asarray(d['rew_tip_target'], dtype=np.float32)),
                                             torch.tensor(np.asarray(d['rew_Q'], dtype=np.float32)),
                                             torch.tensor(np.asarray(d['rew_R'], dtype=np.float32)))
    else:
        rew = pm.rewards.CartpoleReward(pole_length=torch.tensor(0.5))
    n_comp = int(d['dyn_gmm_n']) if 'dyn_gmm_n' in d else 0
    Dy = D + 1 if learned else D
    dyn = pm.models.DynamicsModel(
        pm.models.mlp(D + U + len(dad), (2 * D + 1) * n_comp + 1 if n_comp > 1 else 2 * Dy, dyn_hid,
                      dropout_layers=[pm.models.CDropout(0.1 * np.ones(h)) for h in dyn_hid],
                      nonlin=act_module(d['dyn_act'] if 'dyn_act' in d else 0)),
        reward_func=rew, angle_dims=dad,
        output_density=(pm.models.GaussianMixtureDensity(D, n_comp) if n_comp > 1
                        else pm.models.DiagGaussianDensity(Dy))).float()
    maxU = np.asarray(d['pol_scale'], dtype=np.float32)
    pol = pm.models.Policy(
        pm.models.mlp(D + len(pad), 2 * U, pol_hid,
                      # (per-unit rates where the fixture recorded them: models/modules.py:19-27 takes a tensor)
                      dropout_layers=[pm.models.BDropout(torch.tensor(np.asarray(d['pol_rate%d' % i], dtype=np.float32))
                                                         if 'pol_rate%d' % i in d else 0.1)
                                      for i in range(len(pol_hid))],
                      nonlin=act_module(d['pol_act'] if 'pol_act' in d else 0),
                      output_nonlin=partial(pm.models.DiagGaussianDensity, U)), maxU, -maxU, angle_dims=pad).float()
    fill_modules(dyn, pol, d)
    dyn = dyn.to(dev)
    pol = pol.to(dev)
    dyn.eval()
    return dyn, pol


def fill_modules(dyn, pol, d):
    """Copy the fixture's weights, normalisation, frozen masks and noise into reference-shaped modules (on the CPU,
    before they are moved to the device)."""
    import prob_mbrl_amd as pm
    B, D = d['x0'].shape
    npl, ndl = int(d['pol_n_layers']), int(d['dyn_n_layers'])
    dyn_hid = [d['dyn_W%d' % i].shape[0] for i in range(ndl - 1)]
    n_comp = int(d['dyn_gmm_n']) if 'dyn_gmm_n' in d else 0
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))  # noqa: E731
    with torch.no_grad():
        for pre, mod, n in (('pol', pol.model, npl), ('dyn', dyn.model, ndl)):
            lins = [m for m in mod._modules.values() if isinstance(m, torch.nn.Linear)]
            for i, lin in enumerate(lins):
                lin.weight.copy_(T(d['%s_W%d' % (pre, i)]))
                lin.bias.copy_(T(d['%s_b%d' % (pre, i)]))
        for i in range(npl - 1):
            getattr(pol.model, 'drop%d' % i).noise.data = T(d['pol_mask%d' % i])
        for i in range(ndl - 1):
            dr = getattr(dyn.model, 'drop%d' % i)
            dr.noise.data = torch.rand(B, dyn_hid[i])
            dr.concrete_noise = T(d['dyn_mask%d' % i])
        pol.model.fc_nonlin.z.data = T(d['pol_z'])
        if n_comp > 1:    # mixture head: frozen Gumbel noise; the per-step draws are replayed (rollout.Bundle)
            dyn.output_density.z_pi.data = T(d['dyn_zpi'])
            dyn.output_density._forced_draws = (T(d['dyn_z']), T(d['dyn_ucat']))
        else:
            dyn.output_density.z.data = T(d['dyn_z'])
        for k in ('mx', 'iSx', 'my', 'Sy'):
            getattr(dyn, k).data = T(d['dyn_' + k]).reshape(1, -1)
        dyn.Sx.data = dyn.iSx.reciprocal()


def value_from_fixture(d, device='cuda:0'):
    """The critic of examples/deep_pilco_no_mm_with_value.py:269-278 (no output density, concrete dropout, eval mode)
    holding the fixture's weights and masks, with its activation (val_act; none: ReLU)."""
    import prob_mbrl_amd as pm
    n = int(d['val_n_layers'])
    hid = [d['val_W%d' % i].shape[0] for i in range(n - 1)]
    D = d['val_W0'].shape[1]
    V = pm.models.Regressor(pm.models.mlp(D, 1, hid, dropout_layers=[pm.models.CDropout(0.1 * np.ones(h)) for h in hid],
                                          nonlin=act_module(d['val_act'] if 'val_act' in d else 0))).float()
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))  # noqa: E731
    with torch.no_grad():
        lins = [m for m in V.model._modules.values() if isinstance(m, torch.nn.Linear)]
        for i, lin in enumerate(lins):
            lin.weight.copy_(T(d['val_W%d' % i]))
            lin.bias.copy_(T(d['val_b%d' % i]))
        for i in range(n - 1):
            dr = getattr(V.model, 'drop%d' % i)
            dr.noise.data = torch.rand(d['val_mask%d' % i].shape)
            dr.concrete_noise = T(d['val_mask%d' % i])
        for k in ('mx', 'iSx', 'my', 'Sy'):
            getattr(V, k).data = T(d['val_' + k]).reshape(1, -1)
    return V.to(device).eval()
