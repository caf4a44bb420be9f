"""fp64 restatement of BNN fits whose hidden layers carry fixed-rate Bernoulli dropout, alone or mixed with concrete
dropout and with layers that have none (fixtures tests/golden/bdropout, tools/make_golden_bdropout.py).

  BDropout.forward, training mode                          models/modules.py:46-61     out = x * m / p,  m ~ Bernoulli(p)
  BDropout.weights_regularizer / biases_regularizer        models/modules.py:30-35     rs (sum_j p_j sum_o W[o, j]^2), rs sum_o b[o]^2
  CDropout.forward, training branch, and its regulariser   models/modules.py:102-118,120-160,88-93
  BSequential.regularization_loss                          models/modules.py:234-274   a layer regularises the Linear behind it
  DiagGaussianDensity.forward (return_samples=False)       models/densities.py:87-121
  losses.gaussian_log_likelihood                           losses.py:16-37
  GaussianMixtureDensity.forward / the mixture likelihood  models/densities.py:173-207, losses.py:40-64
  the critic fit (mse_loss + reg_weight * reg)             examples/deep_pilco_no_mm_with_value.py:14-66
  utils.train_regressor's step (loss = -E[lml] + reg / N)  utils/train_regressor.py:108-137
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bdropout')
RELU, TANH, SILU = 0, 1, 2
NONE, CONCRETE, BERNOULLI = 0, 1, 2
FN = {RELU: torch.relu, TANH: torch.tanh, SILU: lambda x: x * torch.sigmoid(x)}
FIT = ['bd_nll_relu', 'bd_unit_tanh', 'bd_mixed_silu', 'bd_gmm', 'bd_resample_off']      # per-iteration idx and losses
OPTS = ['bd_nll_relu_decoupled', 'bd_nll_relu_prioritized']
CRITIC = ['bd_critic']


def load(name):
    raw = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    return {k: raw[k] for k in raw.files}


def T(a):
    return torch.tensor(np.asarray(a, dtype=np.float64))


def layers_of(d):
    """Per hidden layer: dict(kind, and keep [h] / reg_scale for Bernoulli, temp / reg_scale / drop_reg for concrete)."""
    out = []
    for l in range(int(d['n_layers']) - 1):
        kind = int(d['kind%d' % l])
        L = dict(kind=kind)
        if kind != NONE:
            L['reg_scale'] = float(d['reg_scale%d' % l])
        if kind == BERNOULLI:
            L['keep'] = T(d['keep%d' % l]).reshape(-1)
        if kind == CONCRETE:
            L['temp'], L['drop_reg'] = float(d['temp%d' % l]), float(d['drop_reg%d' % l])
        out.append(L)
    return out


def hidden(x, weights, layers, logit_ps, act, us, hards, pre=None):
    """The network up to its last Linear (models/core.py:169-187 over BSequential.forward, models/modules.py:215-232).
    pre: a list that receives the hidden layers' pre-activations."""
    h = x
    for l, (W, b) in enumerate(weights[:-1]):
        z = h @ W.t() + b
        if pre is not None:
            pre.append(z.detach())
        h = FN[int(act)](z)
        L = layers[l]
        if L['kind'] == BERNOULLI:
            h = (h * hards[l]) / L['keep']                                   # models/modules.py:58,61
        elif L['kind'] == CONCRETE:
            cp = logit_ps[l] + ((us[l] + 1e-7) / (1 - (us[l] - 1e-7))).log()      # models/modules.py:108-112
            probs = (cp / L['temp']).sigmoid()
            h = h * ((hards[l] - probs).detach() + probs)                    # models/modules.py:116-117,160
    W, b = weights[-1]
    return h @ W.t() + b


def regulariser(weights, layers, logit_ps):
    reg = 0.0
    for l, L in enumerate(layers):
        if L['kind'] == NONE:
            continue
        W, b = weights[l + 1]
        p = L['keep'] if L['kind'] == BERNOULLI else logit_ps[l].sigmoid()
        reg = reg + L['reg_scale'] * (p * (W**2).sum(0)).sum() + L['reg_scale'] * (b**2).sum()      # :30-35, :88-90
        if L['kind'] == CONCRETE:
            reg = reg + (L['drop_reg'] * (p * p.log() + (1 - p) * (1 - p).log())).sum()             # :91-92
    return reg


def row_log_likelihood(o, y, max_log_std, n_components=0):
    if n_components > 1:      # models/densities.py:173-207 (return_samples=False), losses.py:40-64
        n = int(n_components)
        D = ((o.shape[-1] - 1) // n - 1) // 2
        nD = n * D
        mean, log_std, extras = o[:, :nD], o[:, nD:2 * nD], o[:, 2 * nD:]
        logit_pi, log_temperature = extras[:, :n], extras[:, n:]
        log_std = -torch.nn.functional.softplus(-log_std + max_log_std) + max_log_std
        mean, log_std = mean.reshape(-1, D, n), log_std.reshape(-1, D, n)
        logit_pi = logit_pi / (1e-1 + torch.nn.functional.softplus(log_temperature))
        deltas = mean - y.unsqueeze(-1)
        log_norm = -D * 0.5 * math.log(2 * math.pi) - log_std.sum(-2)
        dists = -0.5 * ((deltas * log_std.exp().reciprocal())**2).sum(-2)
        return torch.logsumexp(torch.log_softmax(logit_pi, -1) + log_norm + dists, dim=-1)
    D = o.shape[-1] // 2      # models/densities.py:87-121, losses.py:16-37
    mean, log_std = o.split(D, -1)
    log_std = -torch.nn.functional.softplus(-log_std + max_log_std) + max_log_std
    return -0.5 * (((mean - y) * log_std.exp().reciprocal())**2).sum(-1) - log_std.sum(-1) - D * 0.5 * math.log(2 * math.pi)


def fit_loss(weights, layers, logit_ps, act, x, y, us, hards, N, reg_weight=1.0, max_log_std=1.0, n_components=0, pre=None):
    """(loss, -E[lml], reg) of one utils.train_regressor iteration (utils/train_regressor.py:111-133)."""
    o = hidden(x, weights, layers, logit_ps, act, us, hards, pre)
    Enlml = -row_log_likelihood(o, y, max_log_std, n_components).mean()
    reg = reg_weight * regulariser(weights, layers, logit_ps)
    return Enlml + reg / N, Enlml, reg


def mse_term(weights, layers, logit_ps, act, x, y, us, hards):
    """mean squared error of the mean head (the critic fit's loss on normalised rows; pmbrl_bnn_config.loss_kind 1)."""
    o = hidden(x, weights, layers, logit_ps, act, us, hards)
    return ((o[:, :y.shape[1]] - y)**2).mean()


def adam_step(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam with its defaults."""
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    denom = (v.sqrt() / math.sqrt(1 - b2**step)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / (1 - b1**step))


def problem(d, suffix='_init'):
    nl = int(d['n_layers'])
    weights = [(T(d['W%d%s' % (i, suffix)]), T(d['b%d%s' % (i, suffix)])) for i in range(nl)]
    logit_ps = [T(d['logit_p%d%s' % (i, suffix)]) if int(d['kind%d' % i]) == CONCRETE else None for i in range(nl - 1)]
    return weights, logit_ps


def param_keys(d):
    """The flat parameter order of the module: W0, b0, [logit_p0], W1, ... (logit_p_l for concrete layers only)."""
    nl = int(d['n_layers'])
    keys = []
    for l in range(nl):
        keys += ['W%d' % l, 'b%d' % l]
        if l < nl - 1 and int(d['kind%d' % l]) == CONCRETE:
            keys.append('logit_p%d' % l)
    return keys


def draws(d, it):
    nl = int(d['n_layers'])
    us = [T(d['u%d_it%d' % (l, it)]) if int(d['kind%d' % l]) == CONCRETE else None for l in range(nl - 1)]
    hs = [T(d['hard%d_it%d' % (l, it)]) if int(d['kind%d' % l]) != NONE else None for l in range(nl - 1)]
    return us, hs


def train(d, Xn=None, Yn=None, idx=None, hards=None, iters=None, pre=None):
    """Replay a fit fixture's iterations with Adam: ({key: parameter}, losses [iters][3], {key: gradient of iteration 0}).
    Xn / Yn / idx (per iteration) / hards (per iteration, per layer) replace the fixture's when given.  pre: a list that
    receives, per iteration, the list of the hidden layers' pre-activations."""
    weights, logit_ps = problem(d)
    layers = layers_of(d)
    keys = param_keys(d)
    named = {}
    for l, (W, b) in enumerate(weights):
        named['W%d' % l], named['b%d' % l] = W, b
    for l, lp in enumerate(logit_ps):
        if lp is not None:
            named['logit_p%d' % l] = lp
    params = [named[k].requires_grad_(True) for k in keys]
    ms, vs = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    Xn = T(d['Xn']) if Xn is None else Xn
    Yn = T(d['Yn']) if Yn is None else Yn
    losses, g0 = [], None
    for it in range(int(d['iters']) if iters is None else iters):
        ix = torch.as_tensor(np.asarray(d['idx_it%d' % it] if idx is None else idx[it]), dtype=torch.int64)
        us, hs = draws(d, it) if hards is None else ([None] * len(layers), hards[it])
        for p in params:
            p.grad = None
        zs = None if pre is None else []
        if pre is not None:
            pre.append(zs)
        loss, Enlml, reg = fit_loss(weights, layers, logit_ps, d['act'], Xn[ix], Yn[ix], us, hs, int(d['N']),
                                    float(d['reg_weight']), float(d['max_log_std']),
                                    int(d['n_components']) if 'n_components' in d else 0, zs)
        loss.backward()
        if it == 0:
            g0 = {k: p.grad.clone() for k, p in zip(keys, params)}
        with torch.no_grad():
            for p, m, v in zip(params, ms, vs):
                adam_step(p, p.grad, m, v, it + 1, float(d['lr']))
        losses.append([float(loss.detach()), float(Enlml.detach()), float(reg.detach())])
    return dict(zip(keys, params)), np.asarray(losses), g0


def kink_margin(d):
    """The smallest |pre-activation| among the units that a replay of d keeps (mask 1, or no dropout), over all hidden
    layers and iterations.  ReLU's derivative jumps at 0: a kept unit whose pre-activation lies closer to 0 than single
    precision resolves it takes either side there, and the gradient of everything in front of it with it."""
    pre = []
    train(d, pre=pre)
    small = math.inf
    for it, zs in enumerate(pre):
        for l, z in enumerate(zs):
            kept = np.ones(z.shape, bool) if int(d['kind%d' % l]) == NONE else np.asarray(d['hard%d_it%d' % (l, it)]) > 0
            small = min(small, float(np.abs(z.numpy())[kept].min()))
    return small


def critic_train(d):
    """Replay the critic fixture's updates (examples/deep_pilco_no_mm_with_value.py:14-66, no output density):
    list over updates of {key: parameter after it}."""
    weights, logit_ps = problem(d)
    layers = layers_of(d)
    keys = param_keys(d)
    nd = len(layers)
    named = {}
    for l, (W, b) in enumerate(weights):
        named['W%d' % l], named['b%d' % l] = W, b
    params = [named[k].requires_grad_(True) for k in keys]
    ms, vs = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    mx, iSx, my, Sy = (T(d[k]) for k in ('mx', 'iSx', 'my', 'Sy'))
    x0, xH, rewards = T(d['states0']), T(d['statesH']), T(d['rewards'])
    gam, H = float(d['gamma']), int(d['H'])
    out = []
    for it in range(int(d['n_updates'])):
        hs = [T(d['hard%d_it%d' % (k, it)]) for k in range(2 * nd)]
        V = lambda x, h: hidden((x - mx) * iSx, weights, layers, logit_ps, d['act'], [None] * nd, h) * Sy + my  # noqa: E731
        V0, VH = V(x0, hs[:nd]), V(xH, hs[nd:]).detach()
        targets = sum(rewards[j] * gam**j for j in range(H)) + gam**H * VH
        loss = torch.nn.functional.mse_loss(V0, targets) + float(d['reg_weight']) * regulariser(weights, layers, logit_ps)
        for p in params:
            p.grad = None
        loss.backward()
        with torch.no_grad():
            for p, m, v in zip(params, ms, vs):
                adam_step(p, p.grad, m, v, it + 1, float(d['lr']))
        out.append({k: p.detach().clone() for k, p in zip(keys, params)})
    return out


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
