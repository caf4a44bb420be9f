#!/usr/bin/env python
"""Generate the learned-reward fixtures tests/golden/learned_reward/lr_*.npz by running the REAL reference (utils.rollout,
mm_resample_, Regressor.forward, DiagGaussianDensity, algorithms.mc_pilco) through tools/make_golden.py's import
shims, cases and capture code.  The existing fixtures are not touched.

The dynamics model predicts the reward in an extra output column (examples/deep_pilco_mm.py:94-99,117:
reward_func=None, mlp(D + U, 2 (D + 1)), DiagGaussianDensity(D + 1)).  The reference's DynamicsModel.forward
cannot run that case with tuple inputs (models/core.py:296 splits by a D only assigned on the concatenated-input
path: UnboundLocalError from utils.rollout); LearnedRewardDynamicsModel below is the ONE deviation:
that call, with the state width taken from the states.  Everything else runs as the reference has it.

The fixtures live in tests/golden/learned_reward/, beside (not among) the analytic-reward fixtures that the
existing parity tests collect from tests/golden/*.npz.

Usage:  python tools/make_golden_learned_reward.py [--out tests/golden/learned_reward] [--only name]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (import shims, the reference, the capture code)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from prob_mbrl import models  # noqa: E402


class LearnedRewardDynamicsModel(models.DynamicsModel):
    """The one deviation.  Only the call the reference cannot serve -- tuple inputs, samples, a learned reward -- is
    handled here, with the width of the state part taken from the states handed in; every other call goes to the
    reference's own DynamicsModel.forward."""

    def forward(self, inputs, separate_outputs=False, deltas=True, **kwargs):
        learned_tuple = (isinstance(inputs, (tuple, list)) and kwargs.get('return_samples', False)
                         and not callable(self.reward_func))
        if not learned_tuple:
            return super().forward(inputs, separate_outputs=separate_outputs, deltas=deltas, **kwargs)
        x, u = inputs
        sample = models.Regressor.forward(self, torch.cat([x, u], -1), **kwargs)
        n = x.shape[-1]
        step, r = sample[..., :n], sample[..., n:]
        nxt = step if deltas else x + step
        return (nxt, r) if separate_outputs else torch.cat([nxt, r], -1)


_build_analytic = mg.build


def build_learned(D, U, dyn_hid, pol_hid, rew, maxU, seed, pol_drop=0.1, dyn_drop=0.1, n_data=300, y_scale=0.01,
                  pol_angle_dims=(), dyn_angle_dims=(), pol_unit_rates=False):
    """make_golden.build with the learned reward head in place of the dynamics model (rew is not used)."""
    _, pol = _build_analytic(D, U, dyn_hid, pol_hid, None, maxU, seed, pol_drop, dyn_drop, n_data, y_scale,
                             pol_angle_dims, dyn_angle_dims, pol_unit_rates)
    torch.manual_seed(seed + 500)
    dyn_angle_dims = list(dyn_angle_dims or ())
    dyn_model = models.mlp(
        D + U + len(dyn_angle_dims), 2 * (D + 1), dyn_hid,
        dropout_layers=[models.modules.CDropout(dyn_drop * np.ones(h)) if dyn_drop > 0 else None for h in dyn_hid],
        nonlin=torch.nn.ReLU)
    dyn = LearnedRewardDynamicsModel(dyn_model, reward_func=None, angle_dims=dyn_angle_dims,
                                     output_density=models.DiagGaussianDensity(D + 1)).float()
    X = torch.randn(n_data, D + U)
    Y = torch.cat([y_scale * torch.randn(n_data, D), 0.5 + 0.2 * torch.randn(n_data, 1)], -1)
    dyn.set_dataset(X, Y)        # (DynamicsModel.set_dataset: maxR / minR from the reward column)
    return dyn, pol


def _no_reward():
    return torch.nn.Module()     # (make_case converts its reward module to fp64; nothing else uses it)


def make_step_noise_case(name, D=4, U=1, hid=(32, 32), B=24, H=10, seed=108):
    """utils.rollout(resample_state_noise=True): the head's noise [B, D + 1] redrawn at every step by the reference's
    DiagGaussianDensity.forward.  The draws are recorded as dyn_z [H, B, D + 1]; the fp64 run replays them."""
    hid = list(hid)
    dyn, pol = build_learned(D, U, hid, hid, None, 10.0, seed)
    dyn.eval()
    pol.train()
    torch.manual_seed(seed + 1000)
    x0 = 0.1 * torch.randn(B, D)
    gamma = [1.0 / H] * H
    with torch.no_grad():
        mg.utils.rollout(x0, dyn, pol, 1, resample_state_noise=False, resample_action_noise=False)
    seed_t = torch.tensor([seed + 77])
    dyn.resample(seed=seed_t)
    pol.resample(seed=seed_t)
    torch.manual_seed(seed + 5)
    pol.model.fc_nonlin.z.data = torch.randn_like(pol.model.fc_nonlin.z)
    d = mg.capture_inputs(dyn, pol, x0, H, gamma, False, False, None, None, None, True, False, None)

    def run(replay=None):
        draws = []
        hook = dyn.output_density.register_forward_hook(lambda m, i, o: draws.append(m.z.detach().clone()))
        orig = torch.randn_like
        if replay is not None:
            it = iter(replay)
            torch.randn_like = lambda t, *a, **k: next(it).to(t.dtype)
        try:
            pol.zero_grad()
            states, actions, rewards = mg.utils.rollout(x0.to(pol.scale.dtype), dyn, pol, H, resample_state_noise=True,
                                                        resample_action_noise=False)
            loss = -torch.stack([r * gamma[i] for i, r in enumerate(rewards)]).sum(0).mean()
            loss.backward()
        finally:
            torch.randn_like = orig
            hook.remove()
        assert len(draws) == H
        g = torch.cat([p.grad.reshape(-1) for p in pol.parameters()])
        return draws, dict(states=torch.stack(states).detach().numpy(), actions=torch.stack(actions).detach().numpy(),
                           rewards=torch.stack(rewards).detach().numpy(), loss=float(loss), grad=g.detach().numpy().copy())

    torch.manual_seed(seed + 9)
    draws, r32 = run()
    _, r32b = run(draws)
    assert np.array_equal(r32['grad'], r32b['grad']), 'replayed draws differ from the recorded run'
    d['dyn_z'] = torch.stack(draws).double().numpy()
    dyn.double()
    pol.double()
    _, r64 = run(draws)
    for k, v in r32.items():
        d['ref32_' + k] = np.asarray(v, dtype=np.float32)
    for k, v in r64.items():
        d['ref64_' + k] = np.asarray(v, dtype=np.float64)
    print('%-22s B=%d H=%d loss32=%.7f loss64=%.7f' % (name, B, H, r32['loss'], r64['loss']))
    return d


CASES = {
    'lr_nomm_d4': lambda: mg.make_case('lr_nomm_d4', 4, 1, [32, 32], [32, 32], _no_reward, 10.0, 40, 12, seed=101, P=8),
    'lr_mmg_d4': lambda: mg.make_case('lr_mmg_d4', 4, 1, [32, 32], [32, 32], _no_reward, 10.0, 40, 12, mm=True,
                                      mm_groups=4, seed=102, P=4),
    'lr_mm1_d4': lambda: mg.make_case('lr_mm1_d4', 4, 1, [32, 32], [32, 32], _no_reward, 10.0, 30, 10, mm=True,
                                      seed=103),
    'lr_angles_d4': lambda: mg.make_case('lr_angles_d4', 4, 1, [32, 32], [32, 32], _no_reward, 10.0, 40, 12, seed=104,
                                         P=8, x0_scale=1.0, dyn_angle_dims=[2]),
    'lr_full200': lambda: mg.make_case('lr_full200', 4, 1, [200, 200], [200, 200], _no_reward, 10.0, 200, 8, mm=True,
                                       mm_groups=4, seed=105, P=4),
    'lr_mcp': lambda: mg.make_mcpilco_case('lr_mcp', 4, 1, [32, 32], [32, 32], _no_reward, 10.0, 30, 10, 4, seed=106),
    'lr_mcp_mmg': lambda: mg.make_mcpilco_case('lr_mcp_mmg', 4, 1, [32, 32], [32, 32], _no_reward, 10.0, 32, 10, 3,
                                               mm=True, mm_groups=4, seed=107),
    'lr_step_d4': lambda: make_step_noise_case('lr_step_d4'),
    # the options of algorithms/mc_pilco.py on top of a learned reward: value bootstrap + CVaR + regulariser, and
    # prioritised replay of the start states
    'lr_mcp_ext': lambda: mg.make_mcpilco_case('lr_mcp_ext', 4, 1, [32, 32], [32, 32], _no_reward, 10.0, 40, 10, 3,
                                               seed=109, value_hid=[24, 24], cvar_eps=0.3, reg_weight=1e-2),
    'lr_mcp_replay': lambda: mg.make_mcpilco_case('lr_mcp_replay', 4, 1, [32, 32], [32, 32], _no_reward, 10.0, 36, 8,
                                                  4, seed=110, replay=True),
}


if __name__ == '__main__':
    mg.build = build_learned
    mg.reward_spec = lambda rew, D: {}      # (no reward constants: numeric arrays only)
    mg.CASES = CASES
    if '--out' not in sys.argv:
        sys.argv += ['--out', os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden',
                                           'learned_reward')]
    mg.main()
