#!/usr/bin/env python
"""What a user of the reference's examples/deep_pilco_mm.py keeps when switching to this build: the SAME import
line and the same calls -- `from prob_mbrl import utils, models, algorithms, envs`, `utils.load_csv` as the argparse
type of the network shapes, `envs.__dict__[name]()`, `models.modules.CDropout / BDropout` inside `models.mlp(...)`,
`models.DynamicsModel(dyn_model, reward_func=env.reward_func, output_density=...)`, `models.Policy(pol_model, maxU,
minU)`, `utils.ExperienceDataset / apply_controller / train_regressor`, `algorithms.mc_pilco(...)` -- with
`<repo>/compat` on the path in front of the reference.  (Reference lines: model construction 111-151, the loop
201-264.  tensorboardX logging and plotting are left out: neither is installed / in scope here.)

    PYTHONPATH=compat:. python examples/deep_pilco_mm_compat.py --ps_iters 2 --pol_opt_iters 50

`--reference_shaped_reward` swaps the environment's reward for a module shaped like the reference's own
(envs/cartpole/env.py:27-40: a torch module called CartpoleReward holding Q, R, target and pole_length as
parameters), which is what `env.reward_func` is when the environment object comes from the reference."""
import argparse
import copy
import os
import sys
from functools import partial

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, 'compat')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from prob_mbrl import utils, models, algorithms, envs  # noqa: E402


class CartpoleReward(torch.nn.Module):
    """Stand-in with the attribute contract of the reference's reward module (class name + constants as frozen
    parameters); the build reads the constants and evaluates its own closed form (prob_mbrl_amd.rewards.from_module)."""

    def __init__(self, pole_length, Q, R, target):
        super().__init__()
        frozen = lambda t: torch.nn.Parameter(torch.as_tensor(t, dtype=torch.float32), requires_grad=False)  # noqa: E731
        self.Q, self.R, self.target, self.pole_length = frozen(Q), frozen(R), frozen(target), frozen(pole_length)


def main(argv=None):
    ap = argparse.ArgumentParser('Deep-PILCO with moment matching, through the prob_mbrl import surface')
    ap.add_argument('-e', '--env', type=str, default='Cartpole')
    ap.add_argument('-s', '--seed', type=int, default=1)
    ap.add_argument('--n_initial_epi', type=int, default=1)
    ap.add_argument('--pred_H', type=int, default=15)
    ap.add_argument('--control_H', type=int, default=40)
    ap.add_argument('--mm_groups', type=int, default=None)
    ap.add_argument('--dyn_lr', type=float, default=1e-4)
    ap.add_argument('--dyn_opt_iters', type=int, default=2000)
    ap.add_argument('--dyn_batch_size', type=int, default=100)
    ap.add_argument('--dyn_drop_rate', type=float, default=0.1)
    ap.add_argument('--dyn_shape', type=utils.load_csv, default=[200, 200])
    ap.add_argument('--pol_lr', type=float, default=1e-3)
    ap.add_argument('--pol_clip', type=float, default=1.0)
    ap.add_argument('--pol_drop_rate', type=float, default=0.1)
    ap.add_argument('--pol_opt_iters', type=int, default=1000)
    ap.add_argument('--pol_batch_size', type=int, default=100)
    ap.add_argument('--ps_iters', type=int, default=100)
    ap.add_argument('--pol_shape', type=utils.load_csv, default=[200, 200])
    ap.add_argument('--resampling_period', type=int, default=499)
    ap.add_argument('--reference_shaped_reward', action='store_true')
    # examples/deep_pilco_mm.py:94-123: the dynamics model predicts the reward too / a mixture-of-Gaussians head
    ap.add_argument('--learn_reward', action='store_true')
    ap.add_argument('--dyn_components', type=int, default=1)
    args = ap.parse_args(argv)

    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    torch.set_flush_denormal(True)
    assert args.env in envs.__all__, 'environments of this build: %s' % envs.__all__
    env = envs.__dict__[args.env]()
    D, U = env.observation_space.shape[0], env.action_space.shape[0]
    maxU, minU = env.action_space.high, env.action_space.low
    reward_func = env.reward_func
    if args.reference_shaped_reward:
        reward_func = CartpoleReward(env.reward_func.pole_length, env.reward_func.Q, env.reward_func.R,
                                     env.reward_func.target)

    if args.learn_reward:
        reward_func = None
    # dynamics model: concrete dropout after every hidden layer, diagonal Gaussian (or a mixture of them) over the
    # next-state deltas -- and the reward, when it is learned
    Dy = D + 1 if args.learn_reward else D
    if args.dyn_components > 1:
        density, dynE = models.GaussianMixtureDensity(Dy, args.dyn_components), (2 * Dy + 1) * args.dyn_components + 1
    else:
        density, dynE = models.DiagGaussianDensity(Dy), 2 * Dy
    dyn_model = models.mlp(D + U, dynE, args.dyn_shape,
                           dropout_layers=[models.modules.CDropout(args.dyn_drop_rate * np.ones(hid))
                                           if args.dyn_drop_rate > 0 else None for hid in args.dyn_shape],
                           nonlin=torch.nn.ReLU)
    dyn = models.DynamicsModel(dyn_model, reward_func=reward_func, output_density=density).float()
    # policy: Bernoulli dropout, Gaussian output squashed to the action range
    pol_model = models.mlp(D, 2 * U, args.pol_shape,
                           dropout_layers=[models.modules.BDropout(args.pol_drop_rate)
                                           if args.pol_drop_rate > 0 else None for hid in args.pol_shape],
                           nonlin=torch.nn.ReLU, output_nonlin=partial(models.DiagGaussianDensity, U))
    pol = models.Policy(pol_model, maxU, minU).float()
    exp = utils.ExperienceDataset()
    opt1 = torch.optim.Adam(dyn.parameters(), args.dyn_lr)
    opt2 = torch.optim.Adam(pol.parameters(), args.pol_lr)
    dyn, pol = dyn.cuda(), pol.cuda()

    env.seed(args.seed)
    rnd = lambda x, t: env.action_space.sample()  # noqa: E731
    for _ in range(args.n_initial_epi):
        exp.append_episode(*utils.apply_controller(env, rnd, args.control_H), policy_params=[])
    act = lambda x, t: np.clip(pol(x), minU, maxU)  # noqa: E731
    log = []
    for ps_it in range(args.ps_iters):
        ret = utils.apply_controller(env, act, args.control_H)
        exp.append_episode(*ret, policy_params=[])
        exp.policy_parameters[-1] = copy.deepcopy(pol.state_dict())
        X, Y = exp.get_dynmodel_dataset(deltas=True, return_costs=args.learn_reward)
        dyn.set_dataset(X.to(dyn.X.device, dyn.X.dtype), Y.to(dyn.X.device, dyn.X.dtype))
        utils.train_regressor(dyn, args.dyn_opt_iters, args.dyn_batch_size, True, opt1,
                              log_likelihood=dyn.output_density.log_prob)
        x0 = exp.sample_states(args.pol_batch_size, timestep=0).to(dyn.X.device, dyn.X.dtype).detach()
        losses = []
        algorithms.mc_pilco(x0, dyn, pol, args.pred_H, opt2, exp, args.pol_opt_iters, pegasus=True,
                            mm_states=True, mm_rewards=True, mm_groups=args.mm_groups, maximize=True,
                            clip_grad=args.pol_clip, resampling_period=args.resampling_period,
                            step_idx_to_sample=0, init_state_noise=1e-2 * x0.std(0),
                            on_iteration=lambda i, loss, *a: losses.append(float(loss)))
        log.append(dict(episode_reward=float(np.sum(ret[2])), losses=losses))
        print('policy search %d: episode reward %.3f, loss %.5f -> %.5f' %
              (ps_it + 1, log[-1]['episode_reward'], losses[0], losses[-1]))
    return dyn, pol, log


if __name__ == '__main__':
    main()
