#!/usr/bin/env python
"""Generate the activation fixtures tests/golden/activations/act_*.npz by running the REAL reference (utils.rollout,
mm_resample_, Regressor.forward, algorithms.mc_pilco, the body of utils.train_regressor) through tools/make_golden.py's
import shims, cases and capture code, with nonlin=torch.nn.Tanh / prob_mbrl.models.activations.Swish in place of the
ReLU its model builders pass to models.mlp.  The existing fixtures are not touched.

The one thing substituted is the `nonlin` argument: make_golden's builders call models.mlp(..., nonlin=torch.nn.ReLU);
while a case is built here models.mlp is wrapped so that the policy (the call with an output_nonlin), the critic (one
output) and the dynamics model (every other call) get the activation the case names.  Every fixture records the choice
as integers (pol_act / dyn_act / val_act, or act for the BNN cases: 0 ReLU, 1 Tanh, 2 SiLU) next to the arrays the
existing fixtures have.

The fixtures live in tests/golden/activations/, beside (not among) the fixtures that the existing parity tests collect
from tests/golden/*.npz.

Usage:  python tools/make_golden_activations.py [--out tests/golden/activations] [--only name]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (import shims, the reference, the capture code)

import torch  # noqa: E402

from prob_mbrl import models  # noqa: E402
from prob_mbrl.models.activations import Swish  # noqa: E402

RELU, TANH, SILU = 0, 1, 2
MODULES = {RELU: torch.nn.ReLU, TANH: torch.nn.Tanh, SILU: Swish}
_mlp = models.mlp


def with_acts(fn, pol=RELU, dyn=RELU, val=RELU, first_scale=None):
    """Run a make_golden case builder with models.mlp handing out these activations.  first_scale = (policy, dynamics):
    the first layers' weights and biases multiplied by these factors right after construction (saturation)."""

    def mlp(input_dims, output_dims, *a, **kw):
        which = 'pol' if kw.get('output_nonlin') is not None else ('val' if int(output_dims) == 1 else 'dyn')
        kw['nonlin'] = MODULES[dict(pol=pol, dyn=dyn, val=val)[which]]
        net = _mlp(input_dims, output_dims, *a, **kw)
        if first_scale is not None and which != 'val':
            with torch.no_grad():
                net.fc0.weight.mul_(first_scale[0 if which == 'pol' else 1])
                net.fc0.bias.mul_(first_scale[0 if which == 'pol' else 1])
        return net

    models.mlp = mlp
    try:
        d = fn()
    finally:
        models.mlp = _mlp
    if 'pol_n_layers' in d:
        d['pol_act'], d['dyn_act'] = pol, dyn
        if 'val_n_layers' in d:
            d['val_act'] = val
    else:
        d['act'] = dyn
    return d


def _case(name, hid, B, H, seed, **kw):
    return lambda: mg.make_case(name, 4, 1, list(hid), list(hid), mg._cartpole, 10.0, B, H, seed=seed, **kw)


CASES = {
    'act_tanh_d4': lambda: with_acts(_case('act_tanh_d4', (32, 32), 40, 12, 201, P=8), TANH, TANH),
    'act_silu_d4': lambda: with_acts(_case('act_silu_d4', (32, 32), 40, 12, 202, P=8), SILU, SILU),
    'act_mixed_nets_d4': lambda: with_acts(_case('act_mixed_nets_d4', (32, 32), 40, 12, 203, P=8), TANH, SILU),
    'act_silu_mmg_d4': lambda: with_acts(_case('act_silu_mmg_d4', (32, 32), 40, 12, 204, mm=True, mm_groups=4, P=4),
                                         SILU, SILU),
    'act_tanh_mm1_d4': lambda: with_acts(_case('act_tanh_mm1_d4', (32, 32), 30, 10, 205, mm=True), TANH, TANH),
    'act_silu_full200': lambda: with_acts(_case('act_silu_full200', (200, 200), 64, 8, 206, mm=True, mm_groups=4, P=4),
                                          SILU, SILU),
    'act_tanh_w48_24': lambda: with_acts(_case('act_tanh_w48_24', (48, 24), 40, 12, 207, P=8), TANH, TANH),
    'act_silu_angles_d4': lambda: with_acts(_case('act_silu_angles_d4', (32, 32), 40, 12, 208, P=8, x0_scale=1.0,
                                                  dyn_angle_dims=[2]), SILU, SILU),
    # first-layer pre-activations of 50 and beyond in the dynamics model (both networks run the same epilogues).  The
    # policy's first layer is left alone: scaled by 150 and more, the reference's own fp32 gradient is 7e-3 to 2e-1 away
    # from its fp64 one (1 - tanh^2 cancels), which leaves nothing to hold a kernel to; this way it is 6e-6
    'act_tanh_sat': lambda: with_acts(_case('act_tanh_sat', (32, 32), 40, 12, 209, P=8), TANH, TANH,
                                      first_scale=(1.0, 60.0)),
    'act_mcp_tanh': lambda: with_acts(lambda: mg.make_mcpilco_case('act_mcp_tanh', 4, 1, [32, 32], [32, 32], mg._cartpole,
                                                                   10.0, 30, 10, 4, seed=210), TANH, TANH),
    'act_mcp_silu_mmg': lambda: with_acts(lambda: mg.make_mcpilco_case('act_mcp_silu_mmg', 4, 1, [32, 32], [32, 32],
                                                                       mg._cartpole, 10.0, 32, 10, 3, mm=True,
                                                                       mm_groups=4, seed=211), SILU, SILU),
    'act_bnn_tanh': lambda: with_acts(lambda: mg.make_bnn_case('act_bnn_tanh', 4, 1, [48, 48], 80, 30, 3, 1e-3, seed=212),
                                      dyn=TANH),
    'act_bnn_silu': lambda: with_acts(lambda: mg.make_bnn_case('act_bnn_silu', 4, 1, [48, 48], 80, 30, 3, 1e-3, seed=213,
                                                               n_comp=3), dyn=SILU),
    # value bootstrap through a Tanh critic (the options of lr_mcp_ext: CVaR + regulariser on top)
    'act_critic_tanh': lambda: with_acts(lambda: mg.make_mcpilco_case('act_critic_tanh', 4, 1, [32, 32], [32, 32],
                                                                      mg._cartpole, 10.0, 40, 10, 3, seed=214,
                                                                      value_hid=[24, 24], cvar_eps=0.3, reg_weight=1e-2),
                                         TANH, TANH, TANH),
}


if __name__ == '__main__':
    mg.CASES = CASES
    if '--out' not in sys.argv:
        sys.argv += ['--out', os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden',
                                           'activations')]
    mg.main()
