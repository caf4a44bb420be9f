"""CPU: the fp64 oracle (oracle/ref_torch.py) on the learned reward head -- reward_spec {'kind': 'learned'}, what
problem_from_npz gives for a fixture without rew_kind -- against the reference's own fp32 and fp64 outputs recorded in
tests/golden/learned_reward/ (tools/make_golden_learned_reward.py)."""
import numpy as np
import pytest
import torch

from oracle import ref_torch
from tests import common
from tests.common import rel


@pytest.mark.parametrize('name', common.lr_names('iter') + common.lr_names('step'))
def test_oracle_reproduces_reference(name):
    d = common.load(name)
    x0, _, dyn, spec, _, _, _, _ = ref_torch.problem_from_npz(d, torch.float64)
    assert spec == {'kind': 'learned'}
    assert dyn['z'].shape[-1] == x0.shape[1] + 1 and dyn['weights'][-1][0].shape[0] == 2 * (x0.shape[1] + 1)
    # per-step noise: the reference's autograd differentiates every step's noise term with the last draw
    loss, g, (S, A, R) = common.oracle_iteration(d, dyn_update=dict(z_grad=dyn['z'][-1]) if dyn['z'].dim() == 3 else None)
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


@pytest.mark.parametrize('name', [n for n in common.lr_names('mcp') if n != 'lr_mcp_replay'])
def test_oracle_first_mc_pilco_loss(name):
    """mc_pilco fixtures: the first iteration's loss is the oracle's at the recorded initial parameters (value bootstrap,
    CVaR and the regulariser included where the run used them; the replay run starts from sampled states)."""
    d = common.load(name)
    loss, _, _ = common.oracle_iteration(d, with_value=True, cvar_eps=float(d['mcp_cvar_eps']),
                                         reg_weight=float(d['mcp_reg_weight']))
    assert abs(float(loss) - float(d['ref32_mcp_losses'][0])) <= 2e-6 * abs(float(d['ref32_mcp_losses'][0]))


def test_fixtures_hold_numeric_arrays_only():
    names = common.lr_names()
    assert len(names) >= 10 and common.lr_names('step') and common.lr_names('mcp') and common.lr_names('iter')
    for name in names:
        raw = np.load(common.path_of(name), allow_pickle=False)
        for k in raw.files:
            assert raw[k].dtype.kind in 'biuf', (name, k, raw[k].dtype)
