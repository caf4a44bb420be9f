"""fp64 oracle for networks whose hidden layers are not ReLU (tests/golden/activations, tools/make_golden_activations.py):
oracle.ref_torch with the activation substituted for the duration of a call.  ref_torch applies torch.relu to every
hidden layer; here its mlp_forward looks up the activation of the network it is handed (by the identity of the weight
list, so the policy and the dynamics model of one rollout can differ) and, for the BNN loss that calls torch.relu
itself, torch.relu is the activation while the call lasts."""
import os
from contextlib import contextmanager

import numpy as np
import torch

from oracle import ref_torch as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'activations')
RELU, TANH, SILU = 0, 1, 2
FN = {RELU: torch.relu, TANH: torch.tanh, SILU: lambda x: x * torch.sigmoid(x)}
# the fixtures of the issue's table, by kind
ITER = ['act_tanh_d4', 'act_silu_d4', 'act_mixed_nets_d4', 'act_silu_mmg_d4', 'act_tanh_mm1_d4', 'act_silu_full200',
        'act_tanh_w48_24', 'act_silu_angles_d4', 'act_tanh_sat']
MCP = ['act_mcp_tanh', 'act_mcp_silu_mmg', 'act_critic_tanh']
BNN = ['act_bnn_tanh', 'act_bnn_silu']


def load(name):
    return R.load_fixture(os.path.join(GOLDEN, name + '.npz'))


@contextmanager
def relu_is(act):
    """torch.relu is the activation `act` inside the block (ref_torch.bnn_loss / critic_update call it directly)."""
    orig = torch.relu
    torch.relu = FN[int(act)]
    try:
        yield
    finally:
        torch.relu = orig


@contextmanager
def activations(*nets):
    """nets: (network dict of ref_torch, activation code) pairs; inside the block ref_torch.mlp_forward runs each of
    them with its own activation (any other network: ReLU)."""
    table = {id(n['weights']): int(a) for n, a in nets}
    orig = R.mlp_forward

    def mlp_forward(x, weights, masks, keep, t=None):
        with relu_is(table.get(id(weights), RELU)):
            return orig(x, weights, masks, keep, t)

    R.mlp_forward = mlp_forward
    try:
        yield
    finally:
        R.mlp_forward = orig


def iteration(d, dtype=torch.float64, n_steps=None, **kw):
    """ref_torch.iteration on a rollout fixture with its pol_act / dyn_act (/ val_act): (loss, flat gradient, (S, A, R))."""
    x0, pol, dyn, spec, meta, z_mm, z_rr, gamma = R.problem_from_npz(d, dtype)
    nets = [(pol, d['pol_act']), (dyn, d['dyn_act'])]
    if kw.pop('with_value', False) and 'val_n_layers' in d:
        val = R.value_from_npz(d, dtype)
        nets.append((val, d['val_act']))
        kw.update(value=val, gamma_H=float(gamma[-1]))
    with activations(*nets):
        return R.iteration(x0, pol, dyn, spec, meta['H'], gamma, meta['maximize'], meta['mm_states'], meta['mm_rewards'],
                           meta['mm_groups'], z_mm, z_rr, meta['infer_ns'], n_steps=n_steps, **kw)


def net_forward(x, net, act):
    """The raw head outputs of one network on the rows x (fp64 tensors)."""
    with relu_is(act):
        return R.mlp_forward(x, net['weights'], net['masks'], net['keep'])


def bnn_train(d, dtype=torch.float64):
    with relu_is(d['act']):
        return R.bnn_train(d, dtype)


def dyn_first_layer_max(d, S, A):
    """Largest |pre-activation| of the dynamics model's first layer over a trajectory (lists of fp64 tensors)."""
    mx, iSx = (torch.tensor(np.asarray(d[k]), dtype=torch.float64) for k in ('dyn_mx', 'dyn_iSx'))
    W, b = (torch.tensor(np.asarray(d[k]), dtype=torch.float64) for k in ('dyn_W0', 'dyn_b0'))
    return max(float((((torch.cat([s, a], -1) - mx) * iSx) @ W.t() + b).abs().max()) for s, a in zip(S, A))
