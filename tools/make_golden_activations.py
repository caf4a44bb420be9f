#!/usr/bin/env python
"""Generate the activation fixtures tests/golden/activations/act_*.npz by running the REAL reference (utils.rollout,
mm_resample_, Regressor.forward, algorithms.mc_pilco, the body of utils.train_regressor) through tools/make_golden.py's
import shims, cases and capture code, with nonlin=torch.nn.Tanh / prob_mbrl.models.activations.Swish in place of the
ReLU its model builders pass to models.mlp -- or, for the fixtures under per_layer/ (NEW_CASES, --new), any of the
reference's models/activations.py (Exp, Sin, SinLU, hhSinLU), one per network or a list with one entry per hidden layer,
None in the list meaning no activation on that layer.  The existing fixtures are not touched.

The one thing substituted is the `nonlin` argument: make_golden's builders call models.mlp(..., nonlin=torch.nn.ReLU);
while a case is built here models.mlp is wrapped so that the policy (the call with an output_nonlin), the critic (one
output) and the dynamics model (every other call) get the activation the case names.  Every fixture records the choice
as integers (pol_act / dyn_act / val_act, or act for the BNN cases: 0 ReLU, 1 Tanh, 2 SiLU, 3 Sin, 4 Exp, 5 SinLU,
6 hhSinLU, 7 none) next to the arrays the existing fixtures have; a network whose hidden layers differ records an integer
array pol_acts / dyn_acts / acts, one code per hidden layer, instead of the scalar.

The fixtures live in tests/golden/activations/, beside (not among) the fixtures that the existing parity tests collect
from tests/golden/*.npz; those of the five further activations and of per-layer lists go to
tests/golden/activations/per_layer/, beside the files the existing tests enumerate.

Usage:  python tools/make_golden_activations.py [--new] [--out DIR] [--only name]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (import shims, the reference, the capture code)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from prob_mbrl import models  # noqa: E402
from prob_mbrl.models.activations import Exp, Sin, SinLU, Swish, hhSinLU  # noqa: E402

RELU, TANH, SILU, SIN, EXP, SINLU, HHSINLU, NONE = range(8)
MODULES = {RELU: torch.nn.ReLU, TANH: torch.nn.Tanh, SILU: Swish, SIN: Sin, EXP: Exp, SINLU: SinLU, HHSINLU: hhSinLU,
           NONE: None}


def _nonlin(a):
    """One code -> its module class; a list of codes -> the list models.mlp takes, one entry per hidden layer."""
    return [MODULES[c] for c in a] if isinstance(a, (list, tuple)) else MODULES[a]
_mlp = models.mlp


def with_acts(fn, pol=RELU, dyn=RELU, val=RELU, first_scale=None):
    """Run a make_golden case builder with models.mlp handing out these activations.  first_scale = (policy, dynamics):
    the first layers' weights and biases multiplied by these factors right after construction (saturation)."""

    def mlp(input_dims, output_dims, *a, **kw):
        which = 'pol' if kw.get('output_nonlin') is not None else ('val' if int(output_dims) == 1 else 'dyn')
        kw['nonlin'] = _nonlin(dict(pol=pol, dyn=dyn, val=val)[which])
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
    def record(key, a):      # (a per-layer list: key + 's', an integer array)
        if isinstance(a, (list, tuple)):
            d[key + 's'] = np.asarray(a, dtype=np.int64)
        else:
            d[key] = a

    if 'pol_n_layers' in d:
        record('pol_act', pol)
        record('dyn_act', dyn)
        if 'val_n_layers' in d:
            record('val_act', val)
    else:
        record('act', dyn)
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


def _sin_sat():
    """act_sin_d4's shape with the dynamics model's first layer scaled as in act_tanh_sat (pre-activations of about
    +-50: a sine on a reduced argument range misses the bars there).  The scale is taken down until the reference's own
    fp32 gradient is within 3e-5 of its fp64 one -- under a third of the gradient bar, so that the fixture can hold a
    kernel to it; the scale and the distance are recorded."""
    scale = 60.0
    while True:
        d = with_acts(_case('act_sin_sat', (24, 25), 20, 4, 228), SIN, SIN, first_scale=(1.0, scale))
        dist = float(np.linalg.norm(d['ref32_grad'] - d['ref64_grad']) / np.linalg.norm(d['ref64_grad']))
        if dist < 3e-5:
            break
        scale *= 0.8
        assert scale > 1.0, 'no scale with a usable reference gradient'
    d['sat_scale'], d['sat_dist'] = scale, dist
    return d


def _bnn_layers():
    """utils.train_regressor on [SinLU, Exp] hidden layers, the first behind fixed-rate Bernoulli dropout and the second
    behind concrete dropout (tools/make_golden_bdropout.py's capture and keys)."""
    import make_golden_bdropout as bd
    bd.MODULES['layers'] = [SinLU, Exp]
    try:
        d = bd.make_fit_case('act_bnn_layers', [5, 24, 25, 3], [bd.B(0.2), bd.Cc(0.1)], 'layers', 4, M=20, N=50, seed=231)
    finally:
        del bd.MODULES['layers']
    del d['act']
    d['acts'] = np.asarray([SINLU, EXP], dtype=np.int64)
    return d


# The five further activations and per-layer lists: D = 4, U = 1; B = 20 leaves a partial second 16-row tile, width 24 has
# padded units, width 25 is odd (hhSinLU's halves: 13 + 12) and has padded units
NEW_CASES = {
    'act_sin_d4': lambda: with_acts(_case('act_sin_d4', (24, 25), 20, 4, 221), SIN, SIN),
    'act_exp_d4': lambda: with_acts(_case('act_exp_d4', (24, 25), 20, 4, 222), EXP, EXP),
    'act_sinlu_d4': lambda: with_acts(_case('act_sinlu_d4', (24, 25), 20, 4, 223), SINLU, SINLU),
    'act_hhsinlu_d4': lambda: with_acts(_case('act_hhsinlu_d4', (24, 25), 20, 4, 224), HHSINLU, HHSINLU),
    'act_layers_d4': lambda: with_acts(_case('act_layers_d4', (24, 25), 20, 4, 225, x0_scale=1.0, pol_angle_dims=[2],
                                             dyn_angle_dims=[2]), [RELU, SIN], [HHSINLU, NONE]),
    'act_sin_mmg_d4': lambda: with_acts(_case('act_sin_mmg_d4', (24, 25), 64, 4, 226, mm=True, mm_groups=4, P=4),
                                        SIN, SIN),
    'act_hhsinlu_full200': lambda: with_acts(_case('act_hhsinlu_full200', (200, 200), 64, 5, 227, P=4), HHSINLU, HHSINLU),
    'act_sin_sat': _sin_sat,
    'act_mcp_hhsinlu': lambda: with_acts(lambda: mg.make_mcpilco_case('act_mcp_hhsinlu', 4, 1, [24, 25], [24, 25],
                                                                      mg._cartpole, 10.0, 20, 4, 3, seed=229),
                                         HHSINLU, HHSINLU),
    'act_bnn_sin': lambda: with_acts(lambda: mg.make_bnn_case('act_bnn_sin', 4, 1, [24, 25], 80, 20, 3, 1e-3, seed=230),
                                     dyn=SIN),
    'act_bnn_layers': _bnn_layers,
}


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    new = '--new' in sys.argv
    if new:
        sys.argv.remove('--new')
    mg.CASES = NEW_CASES if new else CASES
    if '--out' not in sys.argv:
        sys.argv += ['--out', os.path.join(here, '..', 'tests', 'golden', 'activations', *(['per_layer'] if new else []))]
    mg.main()
