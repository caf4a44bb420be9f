"""Train-mode concrete dropout restated in plain torch, at any dtype, and the loader of tests/golden/concrete_policy
(tools/make_golden_concrete_policy.py).

For a hidden layer l followed by a CDropout in train() mode (models/modules.py:102-118,151-153):

    a     = act(h_{l-1} W_l^T + b_l)
    c     = logit_p[j] + log((u[r, j] + 1e-7) / (1 - (u[r, j] - 1e-7)))
    probs = sigmoid(c / temp)
    hard  ~ Bernoulli(probs)                 exactly {0, 1}: an INPUT here (the recorded draw)
    h_l   = a * hard                         no division by p

and the backward goes through probs: the mask is (hard - probs).detach() + probs.  Everything behind the policy network
(the head, the dynamics model, the reward, moment matching, the loss) is oracle.ref_torch's."""
import math
import os

import numpy as np
import torch

from oracle import ref_torch as R
from tests import common

DIR = os.path.join(common.GOLDEN, 'concrete_policy')
ITER = ['cp_iter_tanh', 'cp_iter_relu_mmg', 'cp_iter_resample']
MCP = ['cp_mcp_noreg', 'cp_mcp_reg']
RELU = 0


def load(name):
    return R.load_fixture(os.path.join(DIR, name + '.npz'))


def concrete_mask(logit_p, u, temp, hard):
    """The mask of one call: the value of `hard`, the gradient of sigmoid(c / temp)."""
    c = logit_p + ((u + 1e-7) / (1 - (u - 1e-7))).log()
    probs = (c / temp).sigmoid()
    return (hard - probs).detach() + probs


def mlp(x, weights, act, logits, us, temps, hards, margin=None):
    """Linear -> act -> concrete dropout ... -> Linear.  logits / us / temps / hards: per hidden layer, None where the
    layer has no concrete dropout (hards[l] is then a constant mask or None).  margin: a list that receives the smallest
    |pre-activation| among the kept units of every hidden layer."""
    h, n = x, len(weights)
    for l, (W, b) in enumerate(weights):
        v = h @ W.t() + b
        if l == n - 1:
            return v
        a = R.ACT[int(act[l] if isinstance(act, (list, tuple)) else act)](v)
        if logits[l] is not None:
            m = concrete_mask(logits[l], us[l], temps[l], hards[l])
        else:
            m = hards[l]
        if margin is not None:
            kept = v.detach().abs()[hards[l] > 0] if hards[l] is not None else v.detach().abs()
            margin.append(float(kept.min()))
        h = a * m if m is not None else a


class Problem:
    """A fixture as tensors of `dtype`: the policy's Linear parameters and logits are leaves that require grad."""

    def __init__(self, d, dtype=torch.float64):
        self.d, self.dtype = d, dtype
        self.x0, self.pol, self.dyn, self.spec, self.meta, self.z_mm, self.z_rr, self.gamma = R.problem_from_npz(d, dtype)
        T = lambda k: torch.tensor(np.asarray(d[k]), dtype=dtype)  # noqa: E731
        self.n_hidden = int(d['pol_n_layers']) - 1
        self.logits = [T('pol_logit_p%d' % l).requires_grad_(True) for l in range(self.n_hidden)]
        self.u = [T('pol_u%d' % l) for l in range(self.n_hidden)]            # [B, h], or [H, B, h]: one per call
        self.hard = [T('pol_hard%d' % l) for l in range(self.n_hidden)]      # [iterations, H, B, h]
        self.temp = [float(d['pol_temp%d' % l]) for l in range(self.n_hidden)]
        self.act = int(d['pol_act'])
        for p in R.policy_params(self.pol):
            p.requires_grad_(True)
        self.margin = []

    def leaves(self):
        """In the order of policy.parameters(): fc0.weight, fc0.bias, drop0.logit_p, fc1.weight, ..."""
        out = []
        for l, (W, b) in enumerate(self.pol['weights']):
            out += [W, b] + ([self.logits[l]] if l < self.n_hidden else [])
        return out

    def policy(self, x, it, t):
        us = [u[t] if u.dim() == 3 else u for u in self.u]
        o = mlp(x, self.pol['weights'], self.act, self.logits, us, self.temp, [h[it, t] for h in self.hard], self.margin)
        U = o.shape[-1] // 2
        mean, log_std = o.split(U, -1)
        s = mean + self.pol['z'][:x.shape[0]] * R.clamp_log_std(log_std).exp()
        return self.pol['scale'] * s.tanh() + self.pol['bias']

    def regulariser(self):
        """models/modules.py:88-93,234-274: every dropout layer regularises the NEXT Linear, p = sigmoid(logit_p)."""
        d, reg = self.d, 0.0
        for l in range(self.n_hidden):
            W, b = self.pol['weights'][l + 1]
            p = self.logits[l].sigmoid()
            rs, dr = float(d['pol_reg_scale%d' % l]), float(d['pol_drop_reg%d' % l])
            reg = reg + (rs * (p * (W ** 2).sum(0)) + dr * (p * p.log() + (1 - p) * (1 - p).log())).sum() + rs * (b ** 2).sum()
        return reg

    def iteration(self, it=0, reg_weight=0.0):
        """One rollout, loss and backward with the draws of iteration `it`: (states [H + 1, B, D], loss); the gradients
        are on the leaves."""
        m, D = self.meta, self.x0.shape[1]
        B, G = self.x0.shape[0], self.meta['mm_groups']
        j1, j2 = 1e-12 * torch.eye(D, dtype=self.dtype), 1e-12 * torch.eye(1, dtype=self.dtype)

        def mm(t, z, j):
            w = t.shape[-1]
            if G is not None:
                return R.mm_resample(t.view(G, -1, w), z.view(G, -1, w), j, m['infer_ns']).view(-1, w)
            return R.mm_resample(t, z, j, m['infer_ns'])

        for p in self.leaves():
            p.grad = None
        states, S, Rw = self.x0, [], []
        for t in range(m['H']):
            actions = self.policy(states, it, t)
            nxt, rew = R.dynamics_forward(states, actions, self.dyn, self.spec, t)
            if m['mm_states']:
                nxt = mm(nxt, R.get_z_rnd(self.z_mm, t, B), j1)
            if m['mm_rewards']:
                rew = mm(rew, R.get_z_rnd(self.z_rr, t, B), j2)
            S.append(states)
            Rw.append(rew)
            states = nxt
        S.append(states)
        loss = R.mc_loss(Rw, self.gamma, m['maximize'])
        if reg_weight > 0:
            loss = loss + reg_weight * self.regulariser()
        loss.backward()
        return torch.stack(S).detach(), loss.detach()

    def flat_grad(self):
        return torch.cat([p.grad.reshape(-1) for p in R.policy_params(self.pol)])

    def flat_params(self):
        return torch.cat([p.detach().reshape(-1) for p in R.policy_params(self.pol)])

    def mc_pilco(self):
        """The fixture's iterations of algorithms/mc_pilco.py:86-216: loss (+ regulariser), clip over all policy
        parameters, Adam.  Returns the losses; the leaves hold the final parameters."""
        d = self.d
        opt = torch.optim.Adam(self.leaves(), float(d['mcp_lr']))
        losses = []
        for it in range(int(d['mcp_n_iters'])):
            _, loss = self.iteration(it, float(d['mcp_reg_weight']))
            torch.nn.utils.clip_grad_norm_(self.leaves(), float(d['mcp_clip']))
            opt.step()
            losses.append(float(loss))
        return losses

    def kink_margin(self):
        return min(self.margin) if self.margin else math.inf


def standalone(dims, act, B, seed, temp, kinds, saturate=None):
    """Inputs of a stand-alone network call (CPU tensors, fp32 values), drawn once per argument set.  kinds: per hidden
    layer 'c' (concrete), 'b' (Bernoulli, keep 0.8) or None.  saturate = (layer, unit): that unit's u is 0 in every
    row, so that probs is 0 to the last bit and its logit has no gradient."""
    g = torch.Generator().manual_seed(seed)
    nl, n_out = len(dims) - 1, dims[-1] // 2
    c = dict(B=B, dims=list(dims), act=act, nl=nl, n_out=n_out, kinds=list(kinds))
    c['Ws'] = [torch.randn(dims[i + 1], dims[i], generator=g) / np.sqrt(dims[i]) for i in range(nl)]
    c['bs'] = [0.1 * torch.randn(dims[i + 1], generator=g) for i in range(nl)]
    c['x'] = torch.randn(B, dims[0], generator=g)
    c['z'] = torch.randn(B, n_out, generator=g)
    c['shift'], c['iscale'] = torch.randn(dims[0], generator=g), 0.5 + torch.rand(dims[0], generator=g)
    c['osc'], c['osh'] = 0.5 + torch.rand(n_out, generator=g), torch.randn(n_out, generator=g)
    c['sqs'], c['sqb'] = 1.0 + torch.rand(n_out, generator=g), 0.1 * torch.randn(n_out, generator=g)
    c['up'] = [torch.randn(B, n_out, generator=g) for _ in range(3)]
    c['logit'], c['u'], c['hard'], c['keep'], c['temp'] = [], [], [], [], []
    for l, k in enumerate(kinds):
        h = dims[l + 1]
        if k == 'c':
            lg = math.log(9.0) + 0.3 * torch.randn(h, generator=g)          # keep probabilities around 0.9
            u = torch.rand(B, h, generator=g)
            if saturate is not None and saturate[0] == l:
                u[:, saturate[1]] = 0.0
            probs = ((lg + ((u + 1e-7) / (1 - (u - 1e-7))).log()) / temp).sigmoid()
            c['logit'].append(lg), c['u'].append(u), c['hard'].append(torch.bernoulli(probs, generator=g))
            c['keep'].append(1.0), c['temp'].append(temp)
        elif k == 'b':
            c['logit'].append(None), c['u'].append(None), c['temp'].append(None), c['keep'].append(0.8)
            c['hard'].append((torch.rand(B, h, generator=g) < 0.8).float())
        else:
            c['logit'].append(None), c['u'].append(None), c['temp'].append(None), c['keep'].append(1.0)
            c['hard'].append(None)
    return c


def standalone_reference(c, dtype=torch.float64, mls=float(np.log(5.0))):
    """(grad_x, [grad W0, grad b0, ...], [grad logit_p per hidden layer or None], smallest kept |pre-activation|) of
    sum(sample * up0 + mean * up1 + log_std * up2) by torch autograd in `dtype`."""
    d = lambda t: t.to(dtype)  # noqa: E731
    x = d(c['x']).requires_grad_(True)
    weights = [(d(W).requires_grad_(True), d(b).requires_grad_(True)) for W, b in zip(c['Ws'], c['bs'])]
    logits = [d(t).requires_grad_(True) if t is not None else None for t in c['logit']]
    us = [d(t) if t is not None else None for t in c['u']]
    # a Bernoulli layer's constant mask carries its 1 / keep
    hards = [None if h is None else (d(h) if k == 'c' else d(h) / keep) for h, k, keep in zip(c['hard'], c['kinds'], c['keep'])]
    margin = []
    o = mlp((x - d(c['shift'])) * d(c['iscale']), weights, c['act'], logits, us, c['temp'], hards, margin)
    n = c['n_out']
    mu, ls = o[:, :n], o[:, n:]
    ls = -torch.nn.functional.softplus(-ls + mls) + mls + d(c['osc']).log()
    mu = mu * d(c['osc']) + d(c['osh'])
    smp = d(c['sqs']) * torch.tanh(mu + d(c['z']) * ls.exp()) + d(c['sqb'])
    sum((t * d(up)).sum() for t, up in zip((smp, mu, ls), c['up'])).backward()
    return (x.grad, [t.grad for pair in weights for t in pair], [t.grad if t is not None else None for t in logits],
            min(margin))
