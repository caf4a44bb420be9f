#!/usr/bin/env python
"""Generate the fixtures tests/golden/gmm_reward/gr_*.npz of a learned reward head on a Gaussian-mixture dynamics model
(examples/deep_pilco_mm.py:94-123 with --learn_reward --dyn_components n: reward_func=None, mlp(D + U, (2 (D + 1) + 1) n
+ 1), GaussianMixtureDensity(D + 1, n)) by running the REAL reference (utils.rollout, mm_resample_, Regressor.forward,
GaussianMixtureDensity.forward, utils.train_regressor's body) through tools/make_golden.py's import shims and capture
code.  No existing fixture is touched.

One sample of the density is [state change | reward]: one component draw per row and step serves all D + 1
dimensions.  As for the mixture fixtures of tools/make_golden.py (make_gmm_case), the component index of every step
(Categorical(k_soft).sample()) and the Gaussian noise of every step (the sampler redraws it whatever resample_noise
says) are recorded in call order and replayed for the fp64 run; z_pi stays frozen.  The reference's
DynamicsModel.forward cannot split a learned reward off tuple inputs (models/core.py:296): the one
deviation is tools/make_golden_learned_reward.py's LearnedRewardDynamicsModel, reused here.

gr_step also redraws the dropout masks of both networks at every step (resample_model / resample_policy=True, recorded
as make_golden.make_resample_case records them); gr_fit is make_golden.make_bnn_case on D + 1 targets.

Usage:  python tools/make_golden_gmm_reward.py [--out tests/golden/gmm_reward] [--only name]
"""
import os
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (import shims, the reference, the capture code)
import make_golden_learned_reward as lr  # noqa: E402  (the one deviation)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from prob_mbrl import models, utils  # noqa: E402


def make_gr_case(name, D, U, n_comp, dyn_hid, pol_hid, B, H, seed, mm_groups=None, dyn_angle_dims=(), step_masks=False):
    print('[gmm + learned reward] %s' % name)
    mm = mm_groups is not None
    dyn_angle_dims = list(dyn_angle_dims)
    if dyn_angle_dims:
        mg._patch_build_odims()
    torch.manual_seed(seed)
    np.random.seed(seed)
    Dh = D + 1
    dyn_model = models.mlp(D + U + len(dyn_angle_dims), (2 * Dh + 1) * n_comp + 1, list(dyn_hid),
                           dropout_layers=[models.modules.CDropout(0.1 * np.ones(h)) for h in dyn_hid],
                           nonlin=torch.nn.ReLU)
    dyn = lr.LearnedRewardDynamicsModel(dyn_model, reward_func=None, angle_dims=dyn_angle_dims,
                                        output_density=models.GaussianMixtureDensity(Dh, n_comp)).float()
    pol_model = models.mlp(D, 2 * U, list(pol_hid), dropout_layers=[models.modules.BDropout(0.1) for h in pol_hid],
                           nonlin=torch.nn.ReLU, output_nonlin=partial(models.DiagGaussianDensity, U))
    maxU_t = np.asarray([10.0] * U, dtype=np.float32)
    pol = models.Policy(pol_model, maxU_t, -maxU_t).float()
    X = torch.randn(300, D + U)
    Y = torch.cat([0.01 * torch.randn(300, D), 0.5 + 0.2 * torch.randn(300, 1)], -1)
    dyn.set_dataset(X, Y)
    # a head that actually mixes: spread the component logits and the means
    last = [m for m in dyn.model._modules.values() if isinstance(m, torch.nn.Linear)][-1]
    with torch.no_grad():
        last.bias.add_(0.5 * torch.randn_like(last.bias))
    dyn.eval()
    pol.train()
    torch.manual_seed(seed + 1000)
    x0 = (1.0 if dyn_angle_dims else 0.1) * torch.randn(B, D)
    gamma = [1.0 / H] * H
    with torch.no_grad():   # sizes the noise buffers (z_pi is drawn here and then frozen)
        utils.rollout(x0, dyn, pol, 1, resample_state_noise=False, resample_action_noise=False)
    seed_t = torch.tensor([seed + 77])
    dyn.model.resample(seed=seed_t)
    pol.resample(seed=seed_t)
    torch.manual_seed(seed + 5)
    pol.model.fc_nonlin.z.data = torch.randn_like(pol.model.fc_nonlin.z)
    z_mm = torch.randn(H + B, D) if mm else None
    z_rr = torch.randn(H + B, 1) if mm else None
    d = mg.capture_inputs(dyn, pol, x0, H, gamma, mm, mm, mm_groups, z_mm, z_rr, True, False, None)
    d['dyn_zpi'] = dyn.output_density.z_pi.detach().double().numpy()
    d['dyn_gmm_n'] = n_comp
    rec_k, rec_z, rec_m = [], [], []
    Cat = torch.distributions.Categorical
    orig_sample, orig_randn, orig_bern = Cat.sample, torch.randn, torch.bernoulli

    def run(dt, replay=None):
        pol.zero_grad()
        dyn.zero_grad()
        it_k, it_z, it_m = (iter(r) for r in replay) if replay else (None, None, None)

        def sample(self, *a, **k):
            if it_k is not None:
                return next(it_k)
            out = orig_sample(self, *a, **k)
            rec_k.append(out.detach().clone())
            return out

        def randn(*a, **k):
            if it_z is not None:
                return next(it_z)
            out = orig_randn(*a, **k)
            rec_z.append(out.detach().clone())
            return out

        def bern(p, *a, **k):
            if it_m is not None:
                return next(it_m).to(p.dtype)
            out = orig_bern(p, *a, **k)
            rec_m.append(out.detach().clone())
            return out

        Cat.sample, torch.randn, torch.bernoulli = sample, randn, bern
        try:
            states, actions, rewards = utils.rollout(
                x0.to(dt), dyn, pol, H, resample_model=step_masks, resample_policy=step_masks,
                resample_state_noise=False, resample_action_noise=False, mm_states=mm, mm_rewards=mm,
                mm_groups=mm_groups, z_mm=None if z_mm is None else z_mm.to(dt),
                z_rr=None if z_rr is None else z_rr.to(dt))
        finally:
            Cat.sample, torch.randn, torch.bernoulli = orig_sample, orig_randn, orig_bern
        loss = (-torch.stack([r * gamma[i] for i, r in enumerate(rewards)]).sum(0)).mean()
        loss.backward()
        g = torch.cat([p.grad.reshape(-1) for p in pol.parameters()])
        return dict(states=torch.stack(states).detach().numpy(), actions=torch.stack(actions).detach().numpy(),
                    rewards=torch.stack(rewards).detach().numpy(), loss=float(loss), grad=g.detach().numpy().copy())

    torch.manual_seed(seed + 9)
    r32 = run(torch.float32)
    # per step three torch.randn calls without moment matching (utils/rollout.py:96-97: z1, z2, unused), then the
    # density's z_normal
    per = 1 if mm else 3
    assert len(rec_k) == H and len(rec_z) == per * H, (len(rec_k), len(rec_z))
    zn = rec_z[per - 1::per]
    assert all(z.shape == (B, Dh) for z in zn)
    assert torch.equal(dyn.output_density.z_pi.double(), torch.tensor(d['dyn_zpi'])), 'z_pi was redrawn'
    d['dyn_kidx'] = torch.stack(rec_k).numpy().astype(np.int64)          # [H, B]
    d['dyn_z'] = torch.stack(zn).double().numpy()                        # [H, B, D + 1]
    print('   components drawn: %s' % np.bincount(d['dyn_kidx'].reshape(-1), minlength=n_comp))
    masks = list(rec_m)
    if step_masks:
        # per step: policy drop0, drop1, dynamics drop0, drop1 (make_golden.make_resample_case)
        assert len(masks) == 4 * H, len(masks)
        for k, (pre, i, hid) in enumerate((('pol', 0, pol_hid), ('pol', 1, pol_hid), ('dyn', 0, dyn_hid), ('dyn', 1, dyn_hid))):
            m = torch.stack([masks[4 * t + k] for t in range(H)])
            assert m.shape == (H, B, hid[i]) and bool(((m == 0) | (m == 1)).all())
            d['%s_mask%d' % (pre, i)] = m.double().numpy()
    else:
        assert not masks
    dyn.double()
    pol.double()
    r64 = run(torch.float64, replay=(list(rec_k), list(rec_z), masks))
    for k, v in r32.items():
        d['ref32_' + k] = np.asarray(v, dtype=np.float32)
    for k, v in r64.items():
        d['ref64_' + k] = np.asarray(v, dtype=np.float64)
    gerr = np.linalg.norm(r32['grad'] - r64['grad']) / np.linalg.norm(r64['grad'])
    print('%-22s B=%d H=%d loss32=%.7f loss64=%.7f |g32-g64|/|g64|=%.2e' % (name, B, H, r32['loss'], r64['loss'], gerr))
    return d


CASES = {
    # head 23 wide: two 16-column tiles; hidden 24 / 25: padded widths; 20 rows: a partial 16-row tile
    'gr_d4': lambda: make_gr_case('gr_d4', 4, 1, 2, [24, 25], [24, 25], 20, 4, seed=201),
    'gr_d4_mmg': lambda: make_gr_case('gr_d4_mmg', 4, 1, 2, [24, 25], [24, 25], 20, 4, seed=202, mm_groups=2),
    # PMBRL_MAX_COMP components, head 121 wide, an angle dimension inside the dynamics model
    'gr_8comp': lambda: make_gr_case('gr_8comp', 6, 2, 8, [24, 25], [24, 25], 20, 3, seed=203, dyn_angle_dims=[2]),
    'gr_step': lambda: make_gr_case('gr_step', 4, 1, 2, [24, 25], [24, 25], 20, 4, seed=204, step_masks=True),
    # a fit on D + 1 = 5 targets from D + U = 6 inputs (D = 4, U = 2), three components: head 34 wide
    'gr_fit': lambda: mg.make_bnn_case('gr_fit', 5, 1, [24, 25], 60, 20, 3, 1e-3, seed=205, n_comp=3),
}


if __name__ == '__main__':
    mg.reward_spec = lambda rew, D: {}      # (no reward constants: numeric arrays only)
    mg.CASES = CASES
    if '--out' not in sys.argv:
        sys.argv += ['--out', os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden',
                                           'gmm_reward')]
    mg.main()
