"""CPU: the fp64 oracle of the learned reward head (tests/lr_oracle.py) against the reference's own fp32 and fp64
outputs recorded in tests/golden/learned_reward/ (tools/make_golden_learned_reward.py)."""
import numpy as np
import pytest
import torch

from tests import lr_oracle as LR


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize('name', LR.names('iter') + LR.names('step'))
def test_oracle_reproduces_reference(name):
    d = LR.load(name)
    x0, pol, dyn, meta, z_mm, z_rr, gamma = LR.problem(d)
    if dyn['z'].dim() == 3:
        # per-step noise: the reference's autograd differentiates every step's noise term with the last draw
        dyn['z_grad'] = dyn['z'][-1]
    assert dyn['z'].shape[-1] == x0.shape[1] + 1 and dyn['weights'][-1][0].shape[0] == 2 * (x0.shape[1] + 1)
    loss, g, (S, A, R) = LR.iteration(x0, pol, dyn, meta, gamma, z_mm, z_rr)
    states = torch.stack(S).detach().numpy()
    rewards = torch.stack(R).detach().numpy()
    assert states.shape == d['ref32_states'].shape and rewards.shape == d['ref32_rewards'].shape
    # against the reference's fp32 run: its rounding only
    assert rel(states, d['ref32_states']) < 1e-6
    assert rel(rewards, d['ref32_rewards']) < 1e-6
    assert rel(torch.stack(A).detach().numpy(), d['ref32_actions']) < 1e-6
    assert abs(float(loss) - float(d['ref32_loss'])) <= 1e-6 * abs(float(d['ref32_loss']))
    assert rel(g.numpy(), d['ref32_grad']) < 1e-6
    # against the reference's fp64 run of the same modules (whose constants, e.g. log(max_noise_std), were fp32)
    assert rel(states, d['ref64_states']) < 1e-7
    assert abs(float(loss) - float(d['ref64_loss'])) <= 1e-7 * abs(float(d['ref64_loss']))
    assert rel(g.numpy(), d['ref64_grad']) < 1e-7


@pytest.mark.parametrize('name', [n for n in LR.names('mcp') if n != 'lr_mcp_replay'])
def test_oracle_first_mc_pilco_loss(name):
    """mc_pilco fixtures: the first iteration's loss is the oracle's at the recorded initial parameters (value bootstrap,
    CVaR and the regulariser included where the run used them; the replay run starts from sampled states)."""
    from oracle.ref_torch import value_from_npz
    d = LR.load(name)
    x0, pol, dyn, meta, z_mm, z_rr, gamma = LR.problem(d)
    kw = {}
    if 'val_n_layers' in d:
        kw = dict(value=value_from_npz(d, torch.float64), gamma_H=float(gamma[-1]))
    loss, _, _ = LR.iteration(x0, pol, dyn, meta, gamma, z_mm, z_rr, cvar_eps=float(d['mcp_cvar_eps']),
                              reg_weight=float(d['mcp_reg_weight']), **kw)
    assert abs(float(loss) - float(d['ref32_mcp_losses'][0])) <= 2e-6 * abs(float(d['ref32_mcp_losses'][0]))


def test_fixtures_hold_numeric_arrays_only():
    names = LR.names()
    assert len(names) >= 10 and LR.names('step') and LR.names('mcp') and LR.names('iter')
    for name in names:
        raw = np.load(LR.os.path.join(LR.GOLDEN, name + '.npz'), allow_pickle=False)
        for k in raw.files:
            assert raw[k].dtype.kind in 'biuf', (name, k, raw[k].dtype)
