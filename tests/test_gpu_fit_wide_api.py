"""GPU (-m gpu): networks behind the resident form's LDS edge through the public calls -- BnnStep's default form='auto'
turns to the spill form, so train_regressor (fused chunks, _replay, prioritised sampling, decoupled_reg, the mixture head),
critic.update_value_function and examples/deep_pilco.py take them with no change of their own.  Against the fp64 oracle
where the existing tests of these calls hold a fixture, at those tests' bars."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from tests import common
from tests import fit_envelope_cases as FE
from tests.test_gpu_bernoulli_fit import DEV, Scalars, dynamics_from_fixture

pytestmark = pytest.mark.gpu

WIDE = FE._case('api_w272', 3, [5, 272, 272, 8], 24, FE.RELU, [FE.C, FE.B])      # mlp(5, 8, [272, 272]), N = 60, batch 24
NP_SEED = 11


@functools.lru_cache(maxsize=None)
def regressor_fit():
    """WIDE's fit with the minibatches train_regressor draws under np.random.seed(NP_SEED), and the fp64 oracle's run of
    it: (fit, losses [2, 3], final parameters by key)."""
    from prob_mbrl_amd.train_regressor import iterate_minibatches
    d = dict(FE.generate(WIDE))
    np.random.seed(NP_SEED)
    it = iterate_minibatches(WIDE['N'], WIDE['M'])
    for k in range(2):
        d['idx_it%d' % k] = np.array(next(it))
    assert FE.lds_bytes(WIDE['dims'], WIDE['act']) > FE.LDS_LIMIT
    o = FE.run_oracle(d, torch.float64)
    return d, o['losses'], dict(zip(FE.keys_of(d), o['params']))


def wide_dynamics(d):
    """The DynamicsModel of the fit d (tests/test_gpu_bernoulli_fit.py::dynamics_from_fixture) on its normalised data, the
    normalisation switched off and the concrete layers' logits set."""
    dyn, lins = dynamics_from_fixture(dict(d, X=d['Xn'], Y=d['Yn']))
    with torch.no_grad():
        for l in range(int(d['n_layers']) - 1):
            if int(d['kind%d' % l]) == R.CONCRETE:
                getattr(dyn.model, 'drop%d' % l).logit_p.copy_(torch.tensor(d['logit_p%d_init' % l]))
        for k, v in (('mx', 0.0), ('Sx', 1.0), ('iSx', 1.0), ('my', 0.0), ('Sy', 1.0), ('iSy', 1.0)):
            getattr(dyn, k).data.fill_(v)
    return dyn, lins


def forms_of(fn):
    """Run fn() and return the forms of the BnnStep plans it created."""
    from prob_mbrl_amd import engine as E
    made, keep = [], E.BnnStep.__init__

    def init(self, *a, **k):
        keep(self, *a, **k)
        made.append(self.form)
    E.BnnStep.__init__ = init
    try:
        out = fn()
    finally:
        E.BnnStep.__init__ = keep
    return made, out


def test_train_regressor_replays_the_oracle_on_a_wide_model():
    """Two iterations with the recorded draws (_replay) on the fused path: losses and -E[lml] of both iterations, every
    weight and bias after them, at the bars of test_gpu_bernoulli_fit.py::test_train_regressor_matches_reference."""
    import prob_mbrl_amd as pm
    d, want, final = regressor_fit()
    assert common.kink_margin(d) > FE.KINK_MARGIN
    dyn, lins = wide_dynamics(d)
    opt = torch.optim.Adam([p for p in dyn.parameters() if p.requires_grad], float(d['lr']))
    dyn = dyn.to(DEV)
    n = int(d['n_layers'])
    replay = dict(u=[[d.get('u%d_it%d' % (l, it)) for l in range(n - 1)] for it in range(2)],
                  hard=[[d['hard%d_it%d' % (l, it)] for l in range(n - 1)] for it in range(2)])
    writer = Scalars()
    np.random.seed(NP_SEED)
    made, _ = forms_of(lambda: pm.utils.train_regressor(dyn, 1, WIDE['M'], True, opt, summary_writer=writer, _replay=replay))
    assert made == ['spill']
    got = np.array([[writer.rows[it]['training_loss'], -writer.rows[it]['E_lml']] for it in range(2)])
    print('losses', got, want[:, :2])
    assert np.allclose(got, want[:, :2], rtol=3e-5, atol=2e-6)
    for i, lin in enumerate(lins):
        for t, key in ((lin.weight, 'W%d' % i), (lin.bias, 'b%d' % i)):
            err = np.abs(t.detach().cpu().numpy() - final[key]).max()
            print(key, 'max |got - want| %.2e' % err)
            assert np.allclose(t.detach().cpu().numpy(), final[key], rtol=1e-4, atol=2e-6), (key, err)


@pytest.mark.parametrize('option', ['prioritized_sampling', 'decoupled_reg'])
def test_train_regressor_options_run_on_a_wide_model(option):
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import train_regressor as TR
    d, _, _ = regressor_fit()
    dyn, lins = wide_dynamics(d)
    opt = torch.optim.Adam([p for p in dyn.parameters() if p.requires_grad], 1e-3)
    dyn = dyn.to(DEV)
    writer = Scalars()
    TR.priority_tree.clear()
    np.random.seed(NP_SEED)
    torch.manual_seed(0)
    made, _ = forms_of(lambda: pm.utils.train_regressor(dyn, 5, WIDE['M'], True, opt, summary_writer=writer,
                                                         _warmup_iters=2, **{option: True}))
    assert made and set(made) == {'spill'}
    losses = [writer.rows[it]['training_loss'] for it in sorted(writer.rows)]
    assert len(losses) == 6 and all(np.isfinite(losses)) and losses[0] != losses[-1]
    assert all(bool(torch.isfinite(lin.weight).all()) for lin in lins)
    assert not np.array_equal(lins[0].weight.detach().cpu().numpy(), d['W0_init'])


def test_mixture_head_fits_on_a_wide_body():
    import prob_mbrl_amd as pm
    D, U, n = 4, 1, 3
    torch.manual_seed(0)
    np.random.seed(0)
    dyn = pm.models.DynamicsModel(
        pm.models.mlp(D + U, (2 * D + 1) * n + 1, [272, 272],
                      dropout_layers=[pm.models.CDropout(0.1 * np.ones(272)), pm.models.BDropout(0.1)], nonlin=torch.nn.ReLU),
        reward_func=None, output_density=pm.models.GaussianMixtureDensity(D, n)).float().to(DEV)
    X = torch.randn(60, D + U, device=DEV)
    Y = 0.3 * torch.randn(60, D, device=DEV) + 0.5 * X[:, :D] * X[:, D:D + 1]
    dyn.set_dataset(X, Y)
    opt = torch.optim.Adam(dyn.parameters(), 1e-3)
    ll = pm.losses.gaussian_mixture_log_likelihood
    made, first = forms_of(lambda: pm.utils.train_regressor(dyn, 2, 24, True, opt, log_likelihood=ll))
    assert made and set(made) == {'spill'}
    last = pm.utils.train_regressor(dyn, 40, 24, True, opt, log_likelihood=ll)
    print('-E[lml]', float(first[1]), '->', float(last[1]))
    assert np.isfinite(float(last[1])) and float(last[1]) < float(first[1]), (first, last)


CRITIC = dict(hid=[272, 272, 272], D=4, B=20, H=3, gamma=0.95, keep=0.9, lr=1e-3, reg_weight=1e-4, seed=3)


@functools.lru_cache(maxsize=None)
def critic_problem():
    """One update of a [4, 272, 272, 272, 1] critic with Bernoulli layers, every float an fp32 value, and the fp64 oracle's
    weights after it (oracle.ref_torch.critic_loss + its Adam step): (problem, parameters after the step, kink margin)."""
    c = CRITIC
    rs = np.random.RandomState(c['seed'])
    dims = [c['D']] + c['hid'] + [1]
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    p = dict(W=[f32(rs.randn(dims[l + 1], dims[l]) * np.sqrt(2.0 / dims[l])) for l in range(len(dims) - 1)],
             b=[f32(rs.uniform(-0.1, 0.1, dims[l + 1])) for l in range(len(dims) - 1)],
             x0=f32(rs.randn(c['B'], c['D'])), xH=f32(rs.randn(c['B'], c['D'])),
             rewards=[f32(rs.rand(c['B'], 1)) for _ in range(c['H'])],
             hards=[f32(rs.rand(c['B'], h) < c['keep']) for h in c['hid'] * 2],
             norm=dict(mx=f32(0.1 * rs.randn(1, c['D'])), iSx=f32(1.0 + 0.1 * rs.rand(1, c['D'])), my=f32([[0.3]]), Sy=f32([[1.5]])))
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    weights = [(T(W).requires_grad_(True), T(b).requires_grad_(True)) for W, b in zip(p['W'], p['b'])]
    layers = [dict(kind=R.BERNOULLI, keep=T([np.float32(c['keep'])]), reg_scale=0.5) for _ in c['hid']]
    nd = len(layers)
    norm = {k: T(v) for k, v in p['norm'].items()}
    hs = [T(h) for h in p['hards']]
    loss = R.critic_loss(weights, layers, [None] * nd, [None] * nd, norm, T(p['x0']), T(p['xH']), [T(r) for r in p['rewards']],
                         float(np.float32(c['gamma'])), c['H'], hs, reg_weight=c['reg_weight'])
    loss.backward()
    after = []
    with torch.no_grad():
        for W, b in weights:
            for t in (W, b):
                m, v = torch.zeros_like(t), torch.zeros_like(t)
                R.adam_step(t, t.grad, m, v, 1, c['lr'])
                after.append(t.detach().numpy().copy())
    # the kept pre-activations of both passes, for the distance to ReLU's kink
    margin = np.inf
    with torch.no_grad():
        for x, hh in ((p['x0'], hs[:nd]), (p['xH'], hs[nd:])):
            pre = []
            R.bnn_forward((T(x) - norm['mx']) * norm['iSx'], weights, layers, [None] * nd, [None] * nd, hh, 0, pre)
            margin = min([margin] + [float(z.abs()[h > 0].min()) for z, h in zip(pre, hh)])
    return p, after, margin


def test_critic_update_matches_the_oracle_on_a_wide_critic():
    """critic.update_value_function, one step, at the bars of test_gpu_api.py::test_critic_fit_matches_reference."""
    import prob_mbrl_amd as pm
    from prob_mbrl_amd.critic import update_value_function
    c = CRITIC
    p, after, margin = critic_problem()
    assert margin > FE.KINK_MARGIN
    C = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))  # noqa: E731
    V = pm.models.Regressor(pm.models.mlp(c['D'], 1, c['hid'], nonlin=torch.nn.ReLU, dropout_layers=[
        pm.models.BDropout(float(1 - np.float32(c['keep']))) for _ in c['hid']])).float()
    lins = [m for m in V.model._modules.values() if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for i, lin in enumerate(lins):
            lin.weight.copy_(C(p['W'][i]))
            lin.bias.copy_(C(p['b'][i]))
        for k in ('mx', 'iSx', 'my', 'Sy'):
            getattr(V, k).data = C(p['norm'][k]).reshape(1, -1)
    V = V.to(DEV)
    opt = torch.optim.Adam(V.parameters(), c['lr'])
    states = [None] * (c['H'] + 1)
    states[0], states[c['H']] = C(p['x0']).to(DEV), C(p['xH']).to(DEV)
    rewards = [C(r).to(DEV) for r in p['rewards']]
    gam = float(np.float32(c['gamma']))
    made, _ = forms_of(lambda: update_value_function(V, opt, c['H'], 0, states, None, rewards, lambda i: gam ** i,
                                                      reg_weight=c['reg_weight'], _bernoulli=list(p['hards'])))
    assert made == ['spill']
    for i, lin in enumerate(lins):
        for t, want, name in ((lin.weight, after[2 * i], 'W%d' % i), (lin.bias, after[2 * i + 1], 'b%d' % i)):
            got = t.detach().cpu().numpy()
            print(name, 'max |got - want| %.2e' % np.abs(got - want).max())
            assert np.allclose(got, want, rtol=5e-4, atol=5e-6), (name, np.abs(got - want).max())
            assert not np.array_equal(got, p['W'][i] if t is lin.weight else p['b'][i])
    assert not V.training


def test_deep_pilco_runs_with_a_wide_dynamics_model(tmp_path):
    """examples/deep_pilco.py --dyn_shape 272,272 at tiny sizes, in a fresh child process with a time limit of its own: it
    died in its first train_regressor call before the spill form."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import sys; sys.path.insert(0, %r); import json; from examples import deep_pilco; '
            'folder, hist = deep_pilco.main(sys.argv[1:]); print("RESULT", json.dumps([folder, hist]))' % root)
    args = ['--dyn_shape', '272,272', '--pol_shape', '32,32', '--ps_iters', '1', '--pol_opt_iters', '3', '--dyn_opt_iters', '20',
            '--control_H', '20', '--pred_H', '6', '--pol_batch_size', '20', '-o', str(tmp_path)]
    r = subprocess.run([sys.executable, '-c', code] + args, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    folder, hist = json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
    assert len(hist) == 1 and all(np.isfinite(h['first_loss']) and np.isfinite(h['last_loss']) for h in hist)
