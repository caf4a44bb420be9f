"""Helpers of the tests of the activations beyond ReLU / Tanh / SiLU and of per-layer activation lists: the fixtures of
tests/golden/activations/per_layer (tools/make_golden_activations.py --new), the stated formulas in fp64, and what lets
the fp64 oracle (oracle/ref_torch.py, untouched) evaluate them.

The oracle looks a network's activation up in its ACT tuple and calls it once per hidden layer, in layer order.  Here the
tuple is rebound with entries 3 .. 7 appended -- Sin, Exp, SinLU, hhSinLU, none, written from the formulas of
include/pmbrl.h -- and a network whose hidden layers differ gets one more entry of its own: a callable that applies the
layers' codes in turn (layered).  load() puts that entry's index where the oracle reads the network's code."""
import os

import numpy as np
import torch

from oracle import ref_torch as R
from tests import common

DIR = os.path.join(common.GOLDEN, 'activations', 'per_layer')
RELU, TANH, SILU, SIN, EXP, SINLU, HHSINLU, NONE = range(8)
NEW_ITER = ['act_sin_d4', 'act_exp_d4', 'act_sinlu_d4', 'act_hhsinlu_d4', 'act_layers_d4', 'act_sin_mmg_d4',
            'act_hhsinlu_full200', 'act_sin_sat']
NEW_MCP = ['act_mcp_hhsinlu']
NEW_BNN = ['act_bnn_sin', 'act_bnn_layers']


def hhsinlu(a):
    """unit j of n: s_j = -1 for even j, +1 for odd j; sin(s_j a) for j < ceil(n / 2), relu(s_j a) behind"""
    n = a.shape[-1]
    j = torch.arange(n)
    sa = a * torch.where(j % 2 == 0, -1.0, 1.0).to(a.dtype)
    return torch.where(j < -(-n // 2), torch.sin(sa), torch.relu(sa))


FORMULAS = {RELU: torch.relu, TANH: torch.tanh, SILU: lambda a: a * torch.sigmoid(a), SIN: torch.sin,
            EXP: lambda a: torch.exp(-0.5 * a * a), SINLU: lambda a: torch.where(a > 0, a, torch.sin(a)),
            HHSINLU: hhsinlu, NONE: lambda a: a}
if len(R.ACT) == 3:
    R.ACT = R.ACT + tuple(FORMULAS[c] for c in range(3, 8))
_LAYERED = {}      # index in R.ACT -> the layers' codes


class _Layered:
    def __init__(self, codes):
        self.codes, self.calls = [int(c) for c in codes], 0

    def __call__(self, a):
        fn = FORMULAS[self.codes[self.calls % len(self.codes)]]
        self.calls += 1
        return fn(a)


def layered(codes):
    """Index of a fresh R.ACT entry that applies these codes, one per hidden layer, in the order the oracle's forward
    passes call it (every pass walks all hidden layers)."""
    R.ACT = R.ACT + (_Layered(codes),)
    _LAYERED[len(R.ACT) - 1] = [int(c) for c in codes]
    return len(R.ACT) - 1


def codes_of(d, key, n_hidden):
    """The per-layer codes of network `key` ('pol' | 'dyn' | 'val' | '') of a fixture."""
    if key + ('_acts' if key else 'acts') in d:
        return [int(c) for c in np.asarray(d[key + ('_acts' if key else 'acts')])]
    k = key + ('_act' if key else 'act')
    return [int(d[k]) if k in d else RELU] * n_hidden


def load(name):
    """A fixture of per_layer/ as the oracle and the engine builders read it: a per-layer network (pol_acts / dyn_acts /
    acts) gets its scalar key too, the index of its layered() entry -- prob_mbrl_amd reads the list, the oracle the index."""
    d = dict(R.load_fixture(os.path.join(DIR, name + '.npz')))
    for key in ('pol_act', 'dyn_act', 'val_act', 'act'):
        if key + 's' in d:
            d[key] = layered(np.asarray(d[key + 's']))
    return d


def module_classes(code):
    """The `nonlin` argument of mlp() for a fixture's scalar activation key (a code, or a layered() index)."""
    from prob_mbrl_amd import activations as ACT
    cls = {RELU: torch.nn.ReLU, TANH: torch.nn.Tanh, SILU: ACT.Swish, SIN: ACT.Sin, EXP: ACT.Exp, SINLU: ACT.SinLU,
           HHSINLU: ACT.hhSinLU, NONE: None}
    code = int(code)
    return [cls[c] for c in _LAYERED[code]] if code in _LAYERED else cls[code]


def modules_from_fixture(d, name, device='cuda:0'):
    """common.modules_from_fixture with every activation of prob_mbrl_amd.activations (its act_module knows three)."""
    keep = common.act_module
    common.act_module = module_classes
    try:
        return common.modules_from_fixture(d, name, device)
    finally:
        common.act_module = keep


def mlp64(x, weights, masks, keep, codes):
    """Linear -> activation of layer l -> mask / keep ... -> Linear in the dtype of x, the layers' codes given."""
    h = x
    for l, (W, b) in enumerate(weights):
        h = h @ W.t() + b
        if l < len(weights) - 1:
            h = FORMULAS[codes[l]](h)
            if masks is not None and masks[l] is not None:
                h = h * masks[l][:h.shape[0]] / keep[l]
    return h
