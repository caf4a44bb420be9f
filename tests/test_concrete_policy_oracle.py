"""CPU: the plain-torch restatement of train-mode concrete dropout (tests/concrete_policy_ref.py) in fp64 against the
fp64 results of the reference recorded in tests/golden/concrete_policy, at test_oracle_golden.py's bar (1e-6), and the
rule of test_gpu_mlp_backward.py for ReLU: no kept unit of the fp64 run closer to the kink than 1e-4."""
import numpy as np
import pytest
import torch

from tests import common
from tests import concrete_policy_ref as CP

BAR = 1e-6


def hold(name, what, got, ref):
    e = common.rel(got, ref)
    print('%s %s: %.2e' % (name, what, e))
    assert e < BAR, (name, what, e)


@pytest.mark.parametrize('name', CP.ITER + CP.MCP)
def test_iteration_matches_the_reference_fp64(name):
    d = CP.load(name)
    P = CP.Problem(d, torch.float64)
    S, loss = P.iteration(0, float(d['mcp_reg_weight']) if 'mcp_reg_weight' in d else 0.0)
    hold(name, 'states', S.numpy(), d['ref64_states'])
    assert abs(float(loss) - float(d['ref64_loss'])) <= BAR * abs(float(d['ref64_loss']))
    hold(name, 'gradient', P.flat_grad().numpy(), d['ref64_grad'])
    for l, lg in enumerate(P.logits):
        assert float(np.linalg.norm(d['ref64_glogit%d' % l])) > 0
        hold(name, 'logit_p%d gradient' % l, lg.grad.numpy(), d['ref64_glogit%d' % l])


@pytest.mark.parametrize('name', CP.MCP)
def test_mc_pilco_matches_the_reference_fp64(name):
    d = CP.load(name)
    P = CP.Problem(d, torch.float64)
    losses = P.mc_pilco()
    assert np.allclose(losses, d['ref64_mcp_losses'], rtol=BAR, atol=0)
    hold(name, 'final parameters', P.flat_params().numpy(), d['ref64_mcp_final'])
    for l, lg in enumerate(P.logits):
        hold(name, 'final logit_p%d' % l, lg.detach().numpy(), d['ref64_mcp_logit_final%d' % l])
        # the rates were learned: three Adam steps of lr move a logit by up to 3 lr
        moved = np.abs(lg.detach().numpy() - np.asarray(d['pol_logit_p%d' % l], np.float64))
        assert moved.max() > float(d['mcp_lr'])


def test_fp32_results_are_the_same_run():
    """The recorded fp32 results belong to the same draws as the fp64 ones (the generator replays them)."""
    for name in CP.ITER + CP.MCP:
        d = CP.load(name)
        assert common.rel(d['ref32_states'], d['ref64_states']) < 1e-5 if 'ref32_states' in d else True
    for name in CP.MCP:
        d = CP.load(name)
        assert np.allclose(d['ref32_mcp_losses'], d['ref64_mcp_losses'], rtol=5e-5)


def test_relu_cases_stay_clear_of_the_kink():
    for name in CP.ITER + CP.MCP:
        d = CP.load(name)
        if int(d['pol_act']) != CP.RELU:
            continue
        P = CP.Problem(d, torch.float64)
        P.iteration(0)
        print('%s: smallest kept |pre-activation| %.2e' % (name, P.kink_margin()))
        assert P.kink_margin() > 1e-4, name
