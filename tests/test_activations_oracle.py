"""CPU: the fp64 oracle (oracle/ref_torch.py) on Tanh / SiLU hidden layers -- the activation is the `act` entry of a
network's dict, filled from the fixture's pol_act / dyn_act / val_act / act -- against the reference's own fp32 and fp64
outputs recorded in tests/golden/activations/ (tools/make_golden_activations.py); the Python layer's parsing of the
activation and its refusals, which need no device."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch
from tests import common
from tests.common import rel


@pytest.mark.parametrize('name', common.ACT_ITER)
def test_oracle_reproduces_reference(name):
    d = common.load(name)
    loss, g, (S, A, R) = common.oracle_iteration(d)
    states, rewards = torch.stack(S).detach().numpy(), torch.stack(R).detach().numpy()
    # the 1e-6 of tests/test_oracle_golden.py against the reference's fp64 run
    assert rel(states, d['ref64_states']) < 1e-6
    assert rel(rewards, d['ref64_rewards']) < 1e-6
    assert rel(torch.stack(A).detach().numpy(), d['ref64_actions']) < 1e-6
    assert abs(float(loss) - float(d['ref64_loss'])) <= 1e-6 * abs(float(d['ref64_loss']))
    assert rel(g.numpy(), d['ref64_grad']) < 1e-6
    if name == 'act_tanh_sat':      # what the fixture is for: pre-activations of 50 and beyond
        assert common.dyn_first_layer_max(d, [s.detach() for s in S], [a.detach() for a in A]) >= 50.0


@pytest.mark.parametrize('name', common.ACT_MCP)
def test_oracle_first_mc_pilco_loss(name):
    d = common.load(name)
    loss, _, _ = common.oracle_iteration(d, with_value=True, cvar_eps=float(d['mcp_cvar_eps']), reg_weight=float(d['mcp_reg_weight']))
    assert abs(float(loss) - float(d['ref32_mcp_losses'][0])) <= 2e-6 * abs(float(d['ref32_mcp_losses'][0]))


@pytest.mark.parametrize('name', common.ACT_BNN)
def test_oracle_bnn_training(name):
    d = common.load(name)
    params, losses, g0 = ref_torch.bnn_train(d, torch.float64)
    assert np.allclose(np.asarray(losses), d['losses'], rtol=1e-5, atol=1e-7)
    nl = int(d['n_layers'])
    k = 0
    for l in range(nl):
        assert rel(g0[k].numpy(), d['gW%d_it0' % l]) < 1e-5 and rel(params[k].detach().numpy(), d['W%d_final' % l]) < 1e-5
        k += 3 if l < nl - 1 else 2


def test_fixtures_hold_numeric_arrays_only():
    golden = os.path.join(common.GOLDEN, 'activations')
    names = sorted(f[:-4] for f in os.listdir(golden) if f.endswith('.npz'))
    assert set(names) == set(common.ACT_ITER + common.ACT_MCP + common.ACT_BNN)
    for name in names:
        raw = np.load(os.path.join(golden, name + '.npz'), allow_pickle=False)
        for k in raw.files:
            assert raw[k].dtype.kind in 'biufU', (name, k, raw[k].dtype)     # (U: the reward's kind, a name)


def test_activation_is_parsed_per_network():
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import activations as ACT
    for cls, code in ((torch.nn.ReLU, ACT.RELU), (torch.nn.Tanh, ACT.TANH), (torch.nn.SiLU, ACT.SILU), (ACT.Swish, ACT.SILU)):
        net = pm.models.mlp(5, 8, [16, 16], nonlin=cls, dropout_layers=pm.models.BDropout(0.1))
        lin, drops, dens = net.layer_spec()
        assert len(lin) == 3 and len(drops) == 2 and dens is None and net.activation() == code
    x = torch.linspace(-60.0, 60.0, 25)
    assert torch.equal(ACT.Swish()(x), x * x.sigmoid())


def test_refusals_name_what_is_offered():
    import prob_mbrl_amd as pm
    offered = 'torch.nn.Tanh'
    with pytest.raises(NotImplementedError, match=offered):       # mixed activations in one network
        pm.models.mlp(5, 8, [16, 16], nonlin=[torch.nn.Tanh, torch.nn.ReLU]).layer_spec()
    with pytest.raises(NotImplementedError, match=offered):       # an activation that is not offered
        pm.models.mlp(5, 8, [16, 16], nonlin=torch.nn.ELU).layer_spec()
    rates = [pm.models.BDropout(torch.linspace(0.05, 0.35, 16)) for _ in range(2)]
    with pytest.raises(NotImplementedError, match='only valid for ReLU.*' + offered):     # per-unit rates need ReLU
        pm.models.mlp(5, 8, [16, 16], nonlin=torch.nn.Tanh, dropout_layers=rates).layer_spec()
    pm.models.mlp(5, 8, [16, 16], nonlin=torch.nn.ReLU, dropout_layers=rates).layer_spec()
    pm.models.mlp(5, 8, [16, 16], nonlin=torch.nn.Tanh, dropout_layers=pm.models.BDropout(0.2)).layer_spec()
