"""Optimiser rules: what a torch.optim.Adam / AdamW object asks for, in the form the device-side optimiser steps take it
(pmbrl_opt_rule of include/pmbrl.h) -- parameter groups with their own lr / betas / eps / weight_decay, L2 or decoupled
decay, amsgrad, maximize, and the segments of the flat parameter vector each group owns.

`layout(opt, params)` is the translation (pure Python, no device); `Rule` carries one step's numbers to the library.
algorithms._adam_flat_state builds on both."""
import ctypes as C

import torch

from . import _lib

OFFERED = 'torch.optim.Adam or torch.optim.AdamW (1 to 8 parameter groups; weight_decay, amsgrad and maximize are honoured)'


class Rule:
    """groups: dicts with lr, betas, eps, weight_decay, flags (_lib.OPT_*); segments: (end, group) pairs, ascending, the
    last end = n; vmax: amsgrad's running maximum (flat fp32, n elements) where a group asks for it."""

    def __init__(self, groups, segments, vmax=None):
        self.groups, self.segments, self.vmax = list(groups), list(segments), vmax

    def struct(self):
        r = _lib.OptRule()
        r.n_groups = len(self.groups)
        for k, g in enumerate(self.groups[:_lib.OPT_MAX_GROUPS]):
            r.group[k] = _lib.OptGroup(float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']),
                                       float(g.get('weight_decay', 0.0)), int(g.get('flags', 0)))
        r.n_segments = len(self.segments)
        for q, (end, grp) in enumerate(self.segments[:_lib.OPT_MAX_SEGMENTS]):
            r.seg_end[q], r.seg_group[q] = int(end), int(grp)
        r.max_exp_avg_sq_d = self.vmax.data_ptr() if self.vmax is not None else None
        return r

    def check(self, n):
        """pmbrl_opt_rule_check: raises PmbrlError with the library's message."""
        _lib.check(_lib.load().pmbrl_opt_rule_check(C.byref(self.struct()), int(n)), 'pmbrl_opt_rule_check')


def group_flags(opt, g):
    decoupled = g.get('decoupled_weight_decay', type(opt) is torch.optim.AdamW)
    return ((_lib.OPT_DECOUPLED if decoupled else 0) | (_lib.OPT_AMSGRAD if g.get('amsgrad', False) else 0)
            | (_lib.OPT_MAXIMIZE if g.get('maximize', False) else 0))


def layout(opt, params):
    """The segments [(end, group index)] of the flat vector of `params` (in that order, neighbours of one group merged)
    if `opt` is an optimiser the device steps serve, else None: another class than Adam / AdamW, more than 8 groups, a
    tensor lr, capturable or differentiable groups, a trainable parameter of `params` in no group or in two, a trainable
    parameter of a group that is not in `params`, more than 32 segments."""
    if type(opt) not in (torch.optim.Adam, torch.optim.AdamW):
        return None
    if not 1 <= len(opt.param_groups) <= _lib.OPT_MAX_GROUPS:
        return None
    owner, count = {}, {}
    for k, g in enumerate(opt.param_groups):
        if torch.is_tensor(g['lr']) or g.get('capturable', False) or g.get('differentiable', False):
            return None
        # frozen tensors (e.g. the reward module's constants inside DynamicsModel.parameters()) sit in a group but never
        # receive a gradient: Adam skips them, so do we
        for p in g['params']:
            if p.requires_grad:
                owner[id(p)] = k
                count[id(p)] = count.get(id(p), 0) + 1
    if len(owner) != len(params) or any(count.get(id(p), 0) != 1 for p in params):
        return None
    segments, off = [], 0
    for p in params:
        off += p.numel()
        if segments and segments[-1][1] == owner[id(p)]:
            segments[-1] = (off, owner[id(p)])
        else:
            segments.append((off, owner[id(p)]))
    return segments if len(segments) <= _lib.OPT_MAX_SEGMENTS else None


def is_plain(opt):
    """One group whose rule is the plain kernels' own: no decay, no amsgrad, no maximize."""
    if len(opt.param_groups) != 1:
        return False
    g = opt.param_groups[0]
    return g.get('weight_decay', 0) == 0 and not g.get('amsgrad', False) and not g.get('maximize', False)


def rule_of(cache):
    """This step's Rule of a flat optimiser state (algorithms._adam_flat_state), the groups' numbers read NOW -- a
    torch.optim.lr_scheduler between two steps is honoured; None for the plain rule, which the plain calls serve."""
    if cache['plain']:
        return None
    opt = cache['opt']
    groups = [dict(lr=g['lr'], betas=g['betas'], eps=g['eps'], weight_decay=g.get('weight_decay', 0.0),
                   flags=group_flags(opt, g)) for g in opt.param_groups]
    return Rule(groups, cache['segments'], cache['vmax'])
