#!/usr/bin/env python
"""Generate the fixtures tests/golden/bdropout/bd_*.npz: the REAL reference's utils.train_regressor and the example's
update_value_function (examples/deep_pilco_no_mm_with_value.py:14-66) on networks with fixed-rate Bernoulli dropout
(models.modules.BDropout, models/modules.py:14-70), alone and mixed with concrete dropout and with layers that have none.
Runs through tools/make_golden.py's import shims; the existing fixtures are not touched.

The reference's modules are switched to .double() (as make_golden does for its ref64 arrays), so what is recorded is the
reference's arithmetic without its fp32 rounding; the uniform noise of concrete layers is rounded to fp32 as it is drawn,
so that a replay in fp32 sees the very numbers.  Nothing else is substituted: the minibatch indices come from the
reference's iterate_minibatches / SumTree under a numpy seed (with N = 60 and a batch size of 24 the third minibatch of
an epoch has 12 rows), the masks from torch.bernoulli, intercepted as they are drawn.

Per case:  W{l}_init / b{l}_init / logit_p{l}_init, kind{l} (0 none, 1 concrete, 2 Bernoulli), keep{l} (Bernoulli: p = 1 -
rate, one value or one per unit), reg_scale{l}, temp{l}, drop_reg{l}; Xn, Yn, X, Y; per iteration idx_it{i}, hard{l}_it{i}
(the mask, or the concrete layer's Bernoulli outcome), u{l}_it{i} (concrete layers); losses [iters][3] = loss, -E[lml], reg;
the gradients of iteration 0 (gW{l}_it0, gb{l}_it0, glogit_p{l}_it0) and the parameters after the last step (*_final).

Usage:  python tools/make_golden_bdropout.py [--out tests/golden/bdropout] [--only name]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (import shims, the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from prob_mbrl import losses, models  # noqa: E402
from prob_mbrl.models.activations import Swish  # noqa: E402
from prob_mbrl.models.modules import BDropout, CDropout  # noqa: E402

RELU, TANH, SILU = 0, 1, 2
MODULES = {RELU: torch.nn.ReLU, TANH: torch.nn.Tanh, SILU: Swish}
f = lambda t: t.detach().double().cpu().numpy().copy()  # noqa: E731  (a copy: a double tensor's array aliases it)


def B(rate):
    return lambda h: BDropout(rate if np.isscalar(rate) else torch.tensor(np.asarray(rate(h), dtype=np.float32)))


def Cc(rate):
    return lambda h: CDropout(rate * np.ones(h))


class _Scalars:
    """stand-in for the tensorboardX writer: keeps what train_regressor reports per iteration"""

    def __init__(self):
        self.rows = {}

    def add_scalar(self, name, value, i):
        self.rows.setdefault(int(i), {})[name] = float(value)


class _Draws:
    """torch.rand_like / torch.bernoulli with every draw recorded, in call order"""

    def __init__(self):
        self.u, self.b = [], []

    def __enter__(self):
        self.orig = torch.rand_like, torch.bernoulli

        def rand_like(x, *a, **k):
            out = self.orig[0](x, *a, **k).float().to(x.dtype)      # fp32 values: a replay in fp32 sees the same numbers
            self.u.append(out.clone())
            return out

        def bern(p, *a, **k):
            out = self.orig[1](p, *a, **k)
            self.b.append(out.clone())
            return out

        torch.rand_like, torch.bernoulli = rand_like, bern
        return self

    def __exit__(self, *exc):
        torch.rand_like, torch.bernoulli = self.orig


def describe(d, lins, drops):
    d['n_layers'] = len(lins)
    for i, m in enumerate(lins):
        d['W%d_init' % i] = f(m.weight)
        d['b%d_init' % i] = f(m.bias)
    for i, m in enumerate(drops):
        d['kind%d' % i] = 0 if m is None else (1 if isinstance(m, CDropout) else 2)
        if m is None:
            continue
        d['reg_scale%d' % i] = float(m.regularizer_scale)
        if isinstance(m, CDropout):
            d['logit_p%d_init' % i] = f(m.logit_p)
            d['temp%d' % i] = float(m.temp)
            d['drop_reg%d' % i] = float(m.dropout_regularizer)
        else:
            d['keep%d' % i] = f(1 - m.rate).reshape(-1)


def finals(d, lins, drops, suffix='_final'):
    for i, m in enumerate(lins):
        d['W%d%s' % (i, suffix)] = f(m.weight)
        d['b%d%s' % (i, suffix)] = f(m.bias)
    for i, m in enumerate(drops):
        if isinstance(m, CDropout):
            d['logit_p%d%s' % (i, suffix)] = f(m.logit_p)


def make_fit_case(name, dims, drop, act, iters, M=24, N=60, n_comp=0, resample=True, mode=None, lr=1e-3, seed=301,
                  reg_weight=1.0, warmup=2):
    """utils.train_regressor (utils/train_regressor.py:58-165) for `iters` steps.  dims: input, hidden..., n_out;
    drop: one builder per hidden layer (B / Cc / None); mode: None, 'decoupled' or 'prioritized'."""
    print('[bdropout] %s' % name)
    TR = sys.modules['prob_mbrl.utils.train_regressor']
    torch.manual_seed(seed)
    hid, D = list(dims[1:-1]), dims[-1]
    layers = [b(h) if b is not None else None for b, h in zip(drop, hid)]
    net = models.mlp(dims[0], (2 * D + 1) * n_comp + 1 if n_comp > 1 else 2 * D, hid, dropout_layers=layers,
                     nonlin=MODULES[act])
    dyn = models.DynamicsModel(net, reward_func=None, output_density=(
        models.GaussianMixtureDensity(D, n_comp) if n_comp > 1 else models.DiagGaussianDensity(D))).double()
    lins = [m for m in dyn.model._modules.values() if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        if n_comp > 1:
            lins[-1].bias.add_(0.5 * torch.randn_like(lins[-1].bias))
        for m in layers:
            if isinstance(m, CDropout):
                m.logit_p.add_(0.3 * torch.randn_like(m.logit_p))
    Xd = torch.randn(N, dims[0]).double()
    Yd = (0.3 * torch.randn(N, D) + 0.5 * Xd[:, :D].float() * Xd[:, D:D + 1].float()).double()
    dyn.set_dataset(Xd, Yd)
    d = dict(act=act, N=N, M=M, iters=iters, lr=lr, reg_weight=reg_weight, np_seed=seed + 7, resample=int(resample),
             warmup=warmup, max_log_std=float(dyn.output_density.max_log_std), X=f(Xd), Y=f(Yd),
             Xn=f((dyn.X - dyn.mx) * dyn.iSx), Yn=f((dyn.Y - dyn.my) * dyn.iSy))
    if n_comp > 1:
        d['n_components'] = n_comp
    describe(d, lins, layers)
    opt = torch.optim.Adam([p for p in dyn.parameters() if p.requires_grad], lr)
    idxs, writer = [], _Scalars()
    orig_it, orig_step = TR.iterate_minibatches, opt.step

    def iterate_minibatches(inputs, targets, batchsize):
        for x, y, idx in orig_it(inputs, targets, batchsize):
            if mode != 'prioritized':
                idxs.append(np.array(idx, dtype=np.int64))
            yield x, y, idx

    def step(*a, **k):
        if 'gW0_it0' not in d:
            for i, m in enumerate(lins):
                d['gW%d_it0' % i], d['gb%d_it0' % i] = f(m.weight.grad), f(m.bias.grad)
            for i, m in enumerate(layers):
                if isinstance(m, CDropout):
                    d['glogit_p%d_it0' % i] = f(m.logit_p.grad)
        return orig_step(*a, **k)

    opt.step = step
    TR.iterate_minibatches = iterate_minibatches
    old_defaults = TR.iterate_priority_tree.__defaults__
    TR.iterate_priority_tree.__defaults__ = (warmup,)
    TR.priority_tree.clear()
    TR.decoupled_optimizers.clear()
    np.random.seed(seed + 7)
    ll = losses.gaussian_mixture_log_likelihood if n_comp > 1 else losses.gaussian_log_likelihood
    try:
        with _Draws() as rec:
            # (the reference runs iters + 1 steps: `if i == iters: break` after the step)
            TR.train_regressor(dyn, iters - 1, M, resample, opt, log_likelihood=ll, reg_weight=reg_weight,
                               pbar_class=mg._QuietBar, summary_writer=writer, decoupled_reg=(mode == 'decoupled'),
                               prioritized_sampling=(mode == 'prioritized'))
    finally:
        TR.iterate_minibatches = orig_it
        TR.iterate_priority_tree.__defaults__ = old_defaults
        opt.step = orig_step
    with_drop = [i for i, m in enumerate(layers) if m is not None]
    concrete = [i for i, m in enumerate(layers) if isinstance(m, CDropout)]
    assert len(rec.u) == iters * len(concrete), len(rec.u)
    if resample:
        assert len(rec.b) == iters * len(with_drop), len(rec.b)
    else:
        # one stored mask per Bernoulli layer, drawn by the first forward; every iteration applies its leading rows
        assert not concrete and len(rec.b) == len(with_drop), len(rec.b)
    for it in range(iters):
        if mode != 'prioritized':
            d['idx_it%d' % it] = idxs[it]
        rows = M if mode == 'prioritized' else len(idxs[it])
        for k, i in enumerate(with_drop):
            d['hard%d_it%d' % (i, it)] = f(rec.b[it * len(with_drop) + k]) if resample else f(layers[i].noise[:rows])
        for k, i in enumerate(concrete):
            d['u%d_it%d' % (i, it)] = f(rec.u[it * len(concrete) + k])
    d['losses'] = np.array([[writer.rows[it]['training_loss'], -writer.rows[it]['E_lml'], writer.rows[it]['reg_loss']]
                            for it in range(iters)])
    finals(d, lins, layers)
    if mode == 'prioritized':
        tree = TR.priority_tree[dyn]
        d['tree_counts'] = tree.counts[:N].copy()
        d['tree_leaves'] = tree.sum_tree[tree.max_size - 1:tree.max_size - 1 + N].copy()
    return d


def make_critic_case(name, D=4, hid=(40, 24), Bn=24, H=5, n_updates=2, lr=1e-3, seed=331, rate=0.1):
    """The reference example's update_value_function on a critic with Bernoulli layers (resample=False, its default:
    V0 and V_tgt = V apply the stored masks, recorded here as hard{k}_it{i}: V0's layers, then V_tgt's)."""
    import importlib.util
    print('[bdropout critic] %s' % name)
    spec = importlib.util.spec_from_file_location(
        'ref_example_with_value', os.path.join(os.path.dirname(models.__file__), '..', '..', 'examples',
                                               'deep_pilco_no_mm_with_value.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    torch.manual_seed(seed)
    np.random.seed(seed)
    layers = [BDropout(rate) for _ in hid]
    V = models.Regressor(models.mlp(D, 1, list(hid), dropout_layers=layers, nonlin=torch.nn.ReLU)).double()
    V.set_dataset((0.3 * torch.randn(200, D)).double(), (0.4 + 0.25 * torch.randn(200, 1)).double())
    states = [(0.3 * torch.randn(Bn, D)).double() for _ in range(H + 1)]
    rewards = [torch.rand(Bn, 1).double() for _ in range(H)]
    gam = 0.9
    V.train()
    with torch.no_grad():
        V(states[0], resample=False)          # stores the masks for Bn rows
    lins = [m for m in V.model._modules.values() if isinstance(m, torch.nn.Linear)]
    d = dict(act=RELU, gamma=gam, H=H, lr=lr, n_updates=n_updates, reg_weight=1e-4, states0=f(states[0]),
             statesH=f(states[H]), rewards=f(torch.stack(rewards)))
    describe(d, lins, layers)
    for k in ['mx', 'iSx', 'my', 'Sy']:
        d[k] = f(getattr(V, k)).reshape(-1)
    opt = torch.optim.Adam(V.parameters(), lr)
    for it in range(n_updates):
        with _Draws() as rec:
            ex.update_value_function(V, opt, H, it, states, None, rewards, lambda i: gam**i)
        assert not rec.b and not rec.u      # the stored masks served
        for k in range(2 * len(layers)):
            d['hard%d_it%d' % (k, it)] = f(layers[k % len(layers)].noise[:Bn])
        finals(d, lins, layers, '_it%d' % it)
    return d


_lin = lambda h: np.linspace(0.05, 0.5, h)  # noqa: E731
CASES = {
    'bd_nll_relu': lambda: make_fit_case('bd_nll_relu', [6, 40, 24, 4], [B(0.1), B(0.25)], RELU, 4, seed=301),
    'bd_unit_tanh': lambda: make_fit_case('bd_unit_tanh', [6, 40, 40, 4], [B(_lin), B(0.1)], TANH, 4, seed=302),
    'bd_mixed_silu': lambda: make_fit_case('bd_mixed_silu', [5, 32, 40, 16, 3], [B(0.2), Cc(0.1), None], SILU, 4, M=20,
                                           N=50, seed=303),
    'bd_gmm': lambda: make_fit_case('bd_gmm', [6, 40, 24, 4], [B(0.1), B(0.1)], RELU, 3, n_comp=2, seed=304),
    'bd_critic': lambda: make_critic_case('bd_critic'),
    'bd_resample_off': lambda: make_fit_case('bd_resample_off', [6, 40, 24, 4], [B(0.1), B(0.25)], RELU, 3, resample=False,
                                             seed=305),
    'bd_nll_relu_decoupled': lambda: make_fit_case('bd_nll_relu_decoupled', [6, 40, 24, 4], [B(0.1), B(0.25)], RELU, 4,
                                                   mode='decoupled', seed=306),
    'bd_nll_relu_prioritized': lambda: make_fit_case('bd_nll_relu_prioritized', [6, 40, 24, 4], [B(0.1), B(0.25)], RELU, 6,
                                                     mode='prioritized', seed=307),
}


if __name__ == '__main__':
    mg.CASES = CASES
    if '--out' not in sys.argv:
        sys.argv += ['--out', os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'bdropout')]
    mg.main()
