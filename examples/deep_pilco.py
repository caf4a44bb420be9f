#!/usr/bin/env python
"""Deep-PILCO on the MI355X path: the loop of the reference's examples/deep_pilco_mm.py and
examples/deep_pilco_no_mm.py (collect experience -> fit the BNN dynamics -> MC-PILCO policy
search), written against prob_mbrl_amd.  Same stages, same calls, same checkpoint files
(`experience.pth.tar`, `latest_dynamics.pth.tar`, `latest_policy.pth.tar`); the environment is
the self-contained cart-pole of prob_mbrl_amd.envs (gym / Box2D are not part of this build).

    python examples/deep_pilco.py --ps_iters 5                 # moment matching (deep_pilco_mm)
    python examples/deep_pilco.py --no_mm --pol_batch_size 100 # particles only (deep_pilco_no_mm)
    python examples/deep_pilco.py --learn_reward               # the dynamics model predicts the reward too
"""
import argparse
import copy
import datetime
import os
import sys
from functools import partial

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from prob_mbrl_amd import algorithms, envs, models, utils  # noqa: E402


def nonlin_names(s):
    """--nonlin: a name of prob_mbrl_amd.activations.NAMES, or a comma list of them with one name per hidden layer."""
    from prob_mbrl_amd.activations import NAMES
    for n in s.split(','):
        if n.strip() not in NAMES:
            raise argparse.ArgumentTypeError('%r is not one of %s' % (n, ', '.join(NAMES)))
    return s


def parse(argv=None):
    ap = argparse.ArgumentParser('Deep-PILCO (MI355X build)')
    ap.add_argument('-e', '--env', type=str, default='Cartpole')
    ap.add_argument('-o', '--output_folder', type=str, default='~/.prob_mbrl_amd/')
    ap.add_argument('-s', '--seed', type=int, default=1)
    ap.add_argument('--n_initial_epi', type=int, default=1)
    ap.add_argument('--load_from', type=str, default=None)
    ap.add_argument('--pred_H', type=int, default=15)
    ap.add_argument('--control_H', type=int, default=40)
    ap.add_argument('--discount_factor', type=str, default=None)
    ap.add_argument('--prioritized_replay', action='store_true')
    ap.add_argument('--mm_groups', type=int, default=None)
    ap.add_argument('--no_mm', action='store_true', help='particles only (deep_pilco_no_mm.py)')
    ap.add_argument('--learn_reward', action='store_true',
                    help='a learned reward head: the dynamics model predicts the reward (examples/deep_pilco_mm.py:94-99)')
    ap.add_argument('--reward', type=str, default='analytic', choices=['analytic', 'callable'],
                    help="callable: hand the environment's reward over as a plain torch function of (states, actions) -- how "
                         'a reward of your own reaches the fused rollout (DynamicsModel states the contract)')
    ap.add_argument('--nonlin', type=nonlin_names, default='relu',
                    help='activation of the hidden layers of the dynamics model and the policy: relu | tanh | silu | sin | '
                         'exp | sinlu | hhsinlu | none, or a comma list with one name per hidden layer (relu,sin)')
    ap.add_argument('--dyn_lr', type=float, default=1e-4)
    ap.add_argument('--dyn_opt', type=str, default='adam', choices=['adam', 'adamw'],
                    help='optimiser of the dynamics model: torch.optim.Adam (weight decay as an L2 term) or AdamW (decoupled)')
    ap.add_argument('--dyn_weight_decay', type=float, default=0.0, help='on the weights; biases and dropout logits are not decayed')
    ap.add_argument('--dyn_logit_lr', type=float, default=None,
                    help='a learning rate of their own for the concrete-dropout logits (a parameter group over logit_p)')
    ap.add_argument('--dyn_opt_iters', type=int, default=2000)
    ap.add_argument('--dyn_batch_size', type=int, default=100)
    ap.add_argument('--dyn_drop_rate', type=float, default=0.1)
    ap.add_argument('--dyn_dropout', type=str, default='concrete', choices=['concrete', 'bernoulli'],
                    help='dropout of the dynamics model: concrete (CDropout, rates learned from --dyn_drop_rate) or '
                         'fixed-rate Bernoulli (BDropout at --dyn_drop_rate, the original Deep-PILCO model)')
    ap.add_argument('--dyn_components', type=int, default=1,
                    help='> 1: GaussianMixtureDensity dynamics head (examples/deep_pilco_mm.py:117-121)')
    ap.add_argument('--dyn_shape', type=lambda s: [int(v) for v in s.split(',')], default=[200, 200])
    ap.add_argument('--pol_lr', type=float, default=1e-3)
    ap.add_argument('--pol_opt', type=str, default='adam', choices=['adam', 'adamw'], help='optimiser of the policy')
    ap.add_argument('--pol_weight_decay', type=float, default=0.0, help='on the weights; biases are not decayed')
    ap.add_argument('--pol_clip', type=float, default=1.0)
    ap.add_argument('--pol_drop_rate', type=float, default=0.1)
    ap.add_argument('--pol_dropout', type=str, default='bernoulli', choices=['concrete', 'bernoulli'],
                    help='dropout of the policy: fixed-rate Bernoulli (BDropout at --pol_drop_rate) or concrete (CDropout, '
                         'rates learned by the policy search from --pol_drop_rate; such a search runs at the stepwise '
                         "rollout's cost and does not combine with --prioritized_replay)")
    ap.add_argument('--pol_layer_norm', action='store_true',
                    help='a LayerNorm between every hidden Linear of the policy and its activation (mlp(layer_norm=True)); '
                         "such a search runs at the stepwise rollout's cost and does not combine with --prioritized_replay")
    ap.add_argument('--pol_opt_iters', type=int, default=1000)
    ap.add_argument('--pol_batch_size', type=int, default=100)
    ap.add_argument('--ps_iters', type=int, default=100)
    ap.add_argument('--pol_shape', type=lambda s: [int(v) for v in s.split(',')], default=[200, 200])
    ap.add_argument('--stop_when_done', action='store_true')
    ap.add_argument('--expl_noise', type=float, default=0.0)
    ap.add_argument('--resampling_period', type=int, default=499)
    ap.add_argument('--device', type=str, default='cuda:0')
    return ap.parse_args(argv)


def make_optimizer(net, kind, lr, weight_decay=0.0, logit_lr=None):
    """torch.optim.Adam / AdamW over net.parameters().  With a weight decay or a learning rate for the dropout logits:
    parameter groups -- weights (decayed), biases, and the logit_p tensors at logit_lr -- which the device-side optimiser
    steps serve like the plain optimiser (prob_mbrl_amd/optim.py)."""
    cls = torch.optim.AdamW if kind == 'adamw' else torch.optim.Adam
    if weight_decay == 0.0 and logit_lr is None:
        return cls(net.parameters(), lr, weight_decay=0.0) if kind == 'adamw' else cls(net.parameters(), lr)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    logits = [p for n, p in named if n.endswith('logit_p')] if logit_lr is not None else []
    rest = [p for n, p in named if not any(p is q for q in logits)]
    groups = [dict(params=[p for p in rest if p.dim() > 1], weight_decay=weight_decay),
              dict(params=[p for p in rest if p.dim() <= 1], weight_decay=0.0)]
    if logits:
        groups.append(dict(params=logits, weight_decay=0.0, lr=logit_lr))
    frozen = [p for p in net.parameters() if not p.requires_grad]
    if frozen:
        groups[1]['params'] += frozen
    return cls([g for g in groups if g['params']], lr)


def main(argv=None):
    args = parse(argv)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    dev = torch.device(args.device)
    env = getattr(envs, args.env)()
    results_folder = os.path.join(os.path.expanduser(args.output_folder), 'mc_pilco', args.env,
                                  datetime.datetime.now().strftime('%Y_%m_%d_%H_%M_%S.%f'))
    os.makedirs(results_folder, exist_ok=True)
    results_filename = os.path.join(results_folder, 'experience.pth.tar')
    torch.save(args, os.path.join(results_folder, 'args.pth.tar'))

    D = env.observation_space.shape[0]
    U = env.action_space.shape[0]
    maxU, minU = env.action_space.high, env.action_space.low
    if args.discount_factor is not None:
        args.discount_factor = ((1.0 / args.control_H)**(2.0 / args.control_H)
                                if args.discount_factor == 'auto' else float(args.discount_factor))

    # an environment without an analytic reward takes the learned path too (examples/deep_pilco_mm.py:94-99)
    if args.learn_reward or getattr(env, 'reward_func', None) is None:
        reward_func, args.learn_reward = None, True
    else:
        reward_func = env.reward_func
        if args.reward == 'callable':
            # the same reward as a plain function: nothing tells the library its closed form, so the fused rollout calls it
            # in torch on all row-steps at once.  (A copy on the device: the environment keeps evaluating its own on the host.)
            rew = copy.deepcopy(env.reward_func).to(dev)
            reward_func = lambda states, actions: rew(states, actions)  # noqa: E731
    # (learned reward: the density has one more dimension, examples/deep_pilco_mm.py:94-99,117-121)
    Dy = D + 1 if args.learn_reward else D
    if args.dyn_components > 1:     # mixture-of-Gaussians head: (2 Dy + 1) n + 1 outputs
        density, dynE = models.GaussianMixtureDensity(Dy, args.dyn_components), (2 * Dy + 1) * args.dyn_components + 1
    else:
        density, dynE = models.DiagGaussianDensity(Dy), 2 * Dy
    # --nonlin: the hidden layers' activations of both networks, one name or one per layer
    from prob_mbrl_amd.activations import module_of
    nonlin = module_of(args.nonlin)
    dyn = models.DynamicsModel(
        models.mlp(D + U, dynE, args.dyn_shape,
                   dropout_layers=[None if args.dyn_drop_rate <= 0 else
                                   (models.BDropout(args.dyn_drop_rate) if args.dyn_dropout == 'bernoulli' else
                                    models.CDropout(args.dyn_drop_rate * np.ones(h))) for h in args.dyn_shape],
                   nonlin=nonlin),
        reward_func=reward_func, output_density=density).float()
    pol = models.Policy(
        models.mlp(D, 2 * U, args.pol_shape,
                   dropout_layers=[None if args.pol_drop_rate <= 0 else
                                   (models.BDropout(args.pol_drop_rate) if args.pol_dropout == 'bernoulli' else
                                    models.CDropout(args.pol_drop_rate * np.ones(h))) for h in args.pol_shape], nonlin=nonlin,
                   output_nonlin=partial(models.DiagGaussianDensity, U), layer_norm=args.pol_layer_norm), maxU, minU).float()
    exp = utils.ExperienceDataset()
    if args.load_from is not None:
        utils.load_checkpoint(args.load_from, dyn, pol, exp)
    opt1 = make_optimizer(dyn, args.dyn_opt, args.dyn_lr, args.dyn_weight_decay, args.dyn_logit_lr)
    opt2 = make_optimizer(pol, args.pol_opt, args.pol_lr, args.pol_weight_decay)
    dyn, pol = dyn.to(dev), pol.to(dev)

    env.seed(args.seed)
    rnd = lambda x, t: env.action_space.sample()  # noqa: E731
    initial_experience = args.control_H * args.n_initial_epi
    while exp.n_samples() < initial_experience:
        ret = utils.apply_controller(env, rnd, min(args.control_H, initial_experience - exp.n_samples() + 1),
                                     stop_when_done=args.stop_when_done)
        exp.append_episode(*ret, policy_params=[])
    if initial_experience > 0:
        exp.policy_parameters[-1] = copy.deepcopy(pol.state_dict())
    exp.save(results_filename)

    expl_pol = lambda x, t: (pol(x) + args.expl_noise * rnd(x, t)).clip(minU, maxU)  # noqa: E731
    history = []
    for ps_it in range(args.ps_iters):
        # apply the policy
        new_exp = exp.n_samples() + args.control_H
        while exp.n_samples() < new_exp:
            ret = utils.apply_controller(env, expl_pol, min(args.control_H, new_exp - exp.n_samples() + 1),
                                         stop_when_done=args.stop_when_done)
            exp.append_episode(*ret, policy_params=[])
        exp.policy_parameters[-1] = copy.deepcopy(pol.state_dict())
        exp.save(results_filename)

        # fit the dynamics model
        X, Y = exp.get_dynmodel_dataset(deltas=True, return_costs=args.learn_reward)
        dyn.set_dataset(X.to(dev, torch.float32), Y.to(dev, torch.float32))
        utils.train_regressor(dyn, args.dyn_opt_iters, args.dyn_batch_size, True, opt1,
                              log_likelihood=dyn.output_density.log_prob)
        torch.save(dyn.state_dict(), os.path.join(results_folder, 'latest_dynamics.pth.tar'))

        # policy search
        x0 = exp.sample_states(args.pol_batch_size, timestep=0).to(dev, torch.float32).detach()
        losses = []
        print('Policy search iteration %d' % (ps_it + 1))
        algorithms.mc_pilco(x0, dyn, pol, args.pred_H, opt2, exp, args.pol_opt_iters,
                            discount=args.discount_factor, pegasus=True, mm_states=not args.no_mm,
                            mm_rewards=not args.no_mm, mm_groups=args.mm_groups, maximize=True,
                            clip_grad=args.pol_clip, resampling_period=args.resampling_period,
                            step_idx_to_sample=0, init_state_noise=1e-2 * x0.std(0),
                            prioritized_replay=args.prioritized_replay,
                            on_iteration=lambda i, loss, *a: losses.append(float(loss)))
        torch.save(pol.state_dict(), os.path.join(results_folder, 'latest_policy.pth.tar'))
        history.append(dict(episode_reward=float(np.sum(ret[2])), n_samples=exp.n_samples(),
                            first_loss=losses[0] if losses else None,
                            last_loss=losses[-1] if losses else None))
        print('  episode reward %.3f, predicted return %s -> %s' %
              (history[-1]['episode_reward'], history[-1]['first_loss'], history[-1]['last_loss']))
    return results_folder, history


if __name__ == '__main__':
    main()
