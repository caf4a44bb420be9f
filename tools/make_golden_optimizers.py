#!/usr/bin/env python
"""Generate the optimiser fixtures tests/golden/optimizers/opt_*.npz by running the REAL reference (algorithms.mc_pilco,
the body of utils.train_regressor, the example's update_value_function) through tools/make_golden.py's import shims,
cases and capture code, stepping with the optimiser the case names in place of the plain torch.optim.Adam its case
builders construct.  The existing fixtures are not touched.

The one thing substituted is the optimiser: make_golden's builders call torch.optim.Adam(params, lr); while a case is
built here that name hands out a torch.optim.Adam or AdamW over the same parameters, split into the groups the case
describes (by the kind of every tensor: weight, bias, dropout logit), with lr as the base learning rate.  Every fixture
records the choice as numbers -- opt_class (0 Adam, 1 AdamW), the groups' lr / betas / eps / weight_decay / flags
(1 decoupled, 2 amsgrad, 4 maximize), the segments of the flat parameter vector (opt_seg_end, opt_seg_group: neighbours
of one group merged) -- and the optimiser's final state, flat in parameter order (opt_exp_avg, opt_exp_avg_sq,
opt_max_exp_avg_sq where a group has amsgrad), next to the arrays the existing fixtures have.  mcp_lr is the largest
group's (the bar of the parameter update scales with it).

The fixtures live in tests/golden/optimizers/, beside (not among) the fixtures the existing parity tests collect.

Usage:  python tools/make_golden_optimizers.py [--out tests/golden/optimizers] [--only name]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (import shims, the reference, the capture code)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ADAM, ADAMW = 0, 1
_Adam, _AdamW = torch.optim.Adam, torch.optim.AdamW
W, B, LOGIT = 'weight', 'bias', 'logit'


def kinds(params):
    """weight / bias / logit of every tensor of a network's parameter list (fc.weight, fc.bias, [drop.logit_p], ...)."""
    out = []
    for p in params:
        if p.dim() == 2:
            out.append(W)
        else:
            out.append(B if out and out[-1] == W else LOGIT)
    return out


def with_optimizer(fn, cls, groups, **common_kw):
    """Run a make_golden case builder with torch.optim.Adam handing out `cls` over the groups `groups`: a list of
    (kinds, overrides) -- a tensor goes to the first group that lists its kind; overrides: lr_scale, weight_decay, ..."""
    made = []

    def factory(params, lr=1e-3, **kw):
        params = [p for p in params if p.requires_grad]
        ks = kinds(params)
        spec = []
        for which, over in groups:
            over = dict(over)
            g = dict(params=[p for p, k in zip(params, ks) if k in which and not any(p is q for s in spec for q in s['params'])])
            if 'lr_scale' in over:
                g['lr'] = lr * over.pop('lr_scale')
            g.update(over)
            spec.append(g)
        assert sum(len(g['params']) for g in spec) == len(params)
        opt = (_AdamW if cls == ADAMW else _Adam)(spec, lr, **common_kw, **kw)
        made.append((opt, params))
        return opt

    torch.optim.Adam = factory
    try:
        d = fn()
    finally:
        torch.optim.Adam = _Adam
    assert len(made) == 1
    opt, params = made[0]
    owner = {id(p): k for k, g in enumerate(opt.param_groups) for p in g['params']}
    seg_end, seg_group, off = [], [], 0
    for p in params:
        off += p.numel()
        if seg_group and seg_group[-1] == owner[id(p)]:
            seg_end[-1] = off
        else:
            seg_end.append(off)
            seg_group.append(owner[id(p)])
    gs = opt.param_groups
    d['opt_class'] = cls
    d['opt_n_groups'] = len(gs)
    d['opt_group_lr'] = np.array([g['lr'] for g in gs], dtype=np.float64)
    d['opt_group_betas'] = np.array([g['betas'] for g in gs], dtype=np.float64)
    d['opt_group_eps'] = np.array([g['eps'] for g in gs], dtype=np.float64)
    d['opt_group_weight_decay'] = np.array([g['weight_decay'] for g in gs], dtype=np.float64)
    d['opt_group_flags'] = np.array([(1 if cls == ADAMW else 0) | (2 if g['amsgrad'] else 0) | (4 if g['maximize'] else 0)
                                     for g in gs], dtype=np.int64)
    d['opt_seg_end'] = np.array(seg_end, dtype=np.int64)
    d['opt_seg_group'] = np.array(seg_group, dtype=np.int64)
    flat = lambda key: torch.cat([opt.state[p][key].reshape(-1) for p in params]).numpy().astype(np.float32)  # noqa: E731
    d['opt_exp_avg'], d['opt_exp_avg_sq'] = flat('exp_avg'), flat('exp_avg_sq')
    if any(g['amsgrad'] for g in gs):
        d['opt_max_exp_avg_sq'] = torch.cat([(opt.state[p]['max_exp_avg_sq'] if 'max_exp_avg_sq' in opt.state[p]
                                              else torch.zeros_like(p)).reshape(-1) for p in params]).numpy().astype(np.float32)
    d['opt_steps'] = int(max(float(opt.state[p]['step']) for p in params))
    if 'mcp_lr' in d:
        d['mcp_lr'] = float(max(g['lr'] for g in gs))
    return d


def _mcp(name, B, H, n_iters, seed, **kw):
    return lambda: mg.make_mcpilco_case(name, 4, 1, [32, 32], [32, 32], mg._cartpole, 10.0, B, H, n_iters, seed=seed, **kw)


CASES = {
    # weights decayed, biases not, two learning rates
    'opt_mcp_adamw_groups': lambda: with_optimizer(_mcp('opt_mcp_adamw_groups', 40, 12, 4, 301), ADAMW,
                                                   [((W,), dict(weight_decay=1e-2)),
                                                    ((B,), dict(weight_decay=0.0, lr_scale=3.0))]),
    'opt_mcp_adam_l2_amsgrad': lambda: with_optimizer(_mcp('opt_mcp_adam_l2_amsgrad', 30, 10, 4, 302), ADAM,
                                                      [((W, B), dict())], weight_decay=1e-2, amsgrad=True),
    # moment-matching groups: the one-launch-per-step form, which replays
    'opt_mcp_adamw_mmg': lambda: with_optimizer(_mcp('opt_mcp_adamw_mmg', 32, 10, 3, 303, mm=True, mm_groups=4), ADAMW,
                                                [((W,), dict(weight_decay=1e-2)), ((B,), dict(weight_decay=0.0))]),
    # weights, biases, and the dropout logits at 10 x lr.  The decay is large enough to show within three steps at the
    # bars the fits are held to (lr wd |w| = 3e-4 x 0.5 x 0.3 = 4.5e-5 a step against rtol 1e-4 of |w|, atol 2e-6).  The base rate keeps the regulariser's VALUE
    # away from zero over the recorded iterations: at 1e-3 (logits at 1e-2) it falls 0.49, 0.24, -3.5e-4 -- in the third
    # iteration the difference of two sums of O(1), which fp32 (the reference's own included) resolves to a few 1e-6
    # absolute, so that the relative part of the loss bar (rtol 3e-5, atol 2e-6) has nothing left to act on.
    'opt_bnn_adamw_logit_lr': lambda: with_optimizer(
        lambda: mg.make_bnn_case('opt_bnn_adamw_logit_lr', 4, 1, [32, 32], 80, 30, 3, 3e-4, seed=304), ADAMW,
        [((W,), dict(weight_decay=0.5)), ((B,), dict(weight_decay=0.0)), ((LOGIT,), dict(weight_decay=0.0, lr_scale=10.0))]),
    'opt_bnn_adam_amsgrad': lambda: with_optimizer(
        lambda: mg.make_bnn_case('opt_bnn_adam_amsgrad', 4, 1, [32, 32], 80, 30, 4, 1e-3, seed=305), ADAM,
        [((W, B, LOGIT), dict())], amsgrad=True),
    'opt_critic_adamw': lambda: with_optimizer(
        lambda: mg.make_critic_case('opt_critic_adamw', hid=(32, 32), seed=306), ADAMW,
        [((W, B, LOGIT), dict())], weight_decay=0.5),      # (large enough to show within three updates at the fit's bars)
}


if __name__ == '__main__':
    mg.CASES = CASES
    if '--out' not in sys.argv:
        sys.argv += ['--out', os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'optimizers')]
    mg.main()
