"""CPU: the plain-torch restatement of layer-normalised networks (tests/layer_norm_ref.py) in fp64 against the fp64 results
of the reference recorded in tests/golden/layer_norm, at test_oracle_golden.py's bar (1e-6), and the rule of
test_gpu_mlp_backward.py for ReLU: no kept unit of the fp64 run closer to the kink than 1e-4."""
import numpy as np
import pytest
import torch

from tests import common
from tests import layer_norm_ref as LN

BAR = 1e-6


def hold(name, what, got, ref):
    e = common.rel(got, ref)
    print('%s %s: %.2e' % (name, what, e))
    assert e < BAR, (name, what, e)


@pytest.mark.parametrize('name', LN.ITER + LN.MCP)
def test_iteration_matches_the_reference_fp64(name):
    d = LN.load(name)
    P = LN.Problem(d, torch.float64)
    S, loss = P.iteration()
    hold(name, 'states', S.numpy(), d['ref64_states'])
    assert abs(float(loss) - float(d['ref64_loss'])) <= BAR * abs(float(d['ref64_loss']))
    hold(name, 'gradient', P.flat_grad().numpy(), d['ref64_grad'])
    # every tensor on its own, the LayerNorm's among them
    got, ref = P.split(P.flat_grad().numpy()), P.split(d['ref64_grad'])
    for k in got:
        assert float(np.linalg.norm(ref[k])) > 0, k
        hold(name, k + ' gradient', got[k], ref[k])
    has_ln = any(k.startswith('ln') for k in got)
    assert has_ln == (name != 'ln_iter_dyn')
    assert any(n is not None for n in P.dyn_norms) == (name == 'ln_iter_dyn')


@pytest.mark.parametrize('name', LN.MCP)
def test_mc_pilco_matches_the_reference_fp64(name):
    d = LN.load(name)
    P = LN.Problem(d, torch.float64)
    init = P.flat_params().numpy().copy()
    losses, opt = P.mc_pilco()
    assert np.allclose(losses, d['ref64_mcp_losses'], rtol=BAR, atol=0)
    hold(name, 'final parameters', P.flat_params().numpy(), d['ref64_mcp_final'])
    v = torch.cat([opt.state[p]['exp_avg_sq'].reshape(-1) for p in P.leaves()]).numpy()
    hold(name, 'exp_avg_sq', v, d['ref64_mcp_exp_avg_sq'])
    # gamma and beta were trained: three Adam steps of lr move an element by up to 3 lr
    moved = P.split(np.abs(P.flat_params().numpy() - init))
    for k in ('ln0.weight', 'ln0.bias', 'ln1.weight', 'ln1.bias'):
        assert moved[k].max() > float(d['mcp_lr']), k


def test_fp32_results_are_the_same_run():
    for name in LN.ITER:
        d = LN.load(name)
        assert common.rel(d['ref32_states'], d['ref64_states']) < 1e-5
        assert common.rel(d['ref32_grad'], d['ref64_grad']) < 1e-5
    for name in LN.MCP:
        d = LN.load(name)
        assert np.allclose(d['ref32_mcp_losses'], d['ref64_mcp_losses'], rtol=5e-5)


def test_relu_cases_stay_clear_of_the_kink():
    for name in LN.ITER + LN.MCP:      # (every dynamics model is ReLU, and two of the policies)
        d = LN.load(name)
        P = LN.Problem(d, torch.float64)
        P.iteration()
        print('%s: smallest kept |y| %.2e' % (name, P.kink_margin()))
        assert P.kink_margin() > 1e-4, name


def test_the_written_out_normalisation_is_torchs():
    g = torch.Generator().manual_seed(0)
    v = 3.0 + torch.randn(9, 40, generator=g, dtype=torch.float64)
    gamma, beta = torch.randn(40, generator=g, dtype=torch.float64), torch.randn(40, generator=g, dtype=torch.float64)
    want = torch.nn.functional.layer_norm(v, (40,), gamma, beta, LN.EPS)
    assert common.rel(LN.layer_norm(v, gamma, beta, LN.EPS).numpy(), want.numpy()) < 1e-14
