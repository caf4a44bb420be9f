#!/usr/bin/env python
"""What the parameter gradient of a stand-alone network call and a hooked rollout cost on the device.

  mlp      pmbrl_mlp_backward (input + parameter gradient) against pmbrl_mlp_grad_input (input gradient only) at
           2 500 rows of a [4, 200, 200, 2] network, all three upstream gradients; and pmbrl_mlp_backward_concrete
           (both hidden layers train-mode concrete dropout: the logit gradient on top) on the same call
  ln       the layer-norm calls on the same network with both hidden layers normalised: pmbrl_mlp_forward_ln,
           pmbrl_mlp_grad_input_ln, pmbrl_mlp_backward_ln, beside pmbrl_mlp_forward; and one mc_pilco iteration with such a
           policy at the C2 shape (the stepwise rollout, torch's clip and Adam)
  --other-lib PATH   a second build of libpmbrl_hip.so (e.g. the parent commit's): its pmbrl_mlp_backward is timed on the
           same call, the two builds alternating block by block in one run
  rollout  rollout(..., on_pol_eval=identity) + loss.backward() at the C2 shape (2 500 rows, H = 40, 2 x 200 networks,
           cart-pole widths, no moment matching): the stepwise path, beside the fused rollout + backward of the same
           modules through the same autograd surface

Blocks timed from a device synchronise to a device synchronise; prints median, min and max milliseconds per call as one
JSON line.

    python tools/param_grad_cost.py [--blocks 20] [--iters 10] [--warmup 3] [--only mlp] [--other-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prob_mbrl_amd as pm  # noqa: E402
from prob_mbrl_amd import engine as E  # noqa: E402


def timed(f, blocks, iters, warmup):
    for _ in range(warmup):
        f()
    out = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    t = np.asarray(out)
    return dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()))


def alternating(fs, blocks, iters, warmup):
    """timed() for several callables, one block of each in turn, so that drift and neighbours hit them alike."""
    for f in fs:
        for _ in range(warmup):
            f()
    out = [[] for _ in fs]
    for _ in range(blocks):
        for k, f in enumerate(fs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3 / iters)
    return [dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t))) for t in out]


def other_build(path):
    """A second build of the library with the two entry points pmbrl_mlp_backward needs, typed as _lib types them."""
    from prob_mbrl_amd import _lib
    mine, lib = _lib.load(), ctypes.CDLL(path)
    for name in ('pmbrl_mlp_backward_workspace_bytes', 'pmbrl_mlp_backward', 'pmbrl_last_error', 'pmbrl_build_id'):
        getattr(lib, name).restype, getattr(lib, name).argtypes = getattr(mine, name).restype, getattr(mine, name).argtypes
    return lib


def ln_case(dev, B=2500, dims=(4, 200, 200, 2)):
    g = torch.Generator().manual_seed(1)
    nl, n_out = len(dims) - 1, dims[-1] // 2
    flat = torch.cat([t.reshape(-1) for i in range(nl) for t in
                      (torch.randn(dims[i + 1], dims[i], generator=g) / np.sqrt(dims[i]), 0.1 * torch.randn(dims[i + 1], generator=g))])
    bits = [E.pack_mask((torch.rand(B, dims[i + 1], generator=g) < 0.9).float().to(dev)) for i in range(nl - 1)]
    ln = [(1.0 + 0.3 * torch.randn(dims[i + 1], generator=g), 0.1 * torch.randn(dims[i + 1], generator=g), 1e-5) for i in range(nl - 1)]
    args = (torch.randn(B, dims[0], generator=g).to(dev), flat.to(dev), list(dims), [0.9] * (nl - 1), bits,
            torch.randn(B, n_out, generator=g).to(dev), None, None, None, None, torch.ones(n_out), torch.zeros(n_out), E.LOG_MAX_STD)
    plain, call = E._MlpCall(*args), E._MlpCall(*args, layer_norm=ln)
    ups = [torch.randn(B, n_out, generator=g).to(dev) for _ in range(3)]
    want = ('sample', 'mean', 'log_std')
    return dict(mlp_forward=lambda: plain.forward(want), mlp_forward_ln=lambda: call.forward(want),
                mlp_grad_input_ln=lambda: call.grad_input(*ups), mlp_backward_ln=lambda: call.backward(*ups))


def mcp_ln_case(dev, B=2500, H=40, D=4, U=1, hidden=(200, 200)):
    """n -> n mc_pilco iterations (no moment matching, as the C2 shape) with a layer-normalised policy."""
    from functools import partial
    torch.manual_seed(0)
    dyn = pm.models.DynamicsModel(
        pm.models.mlp(D + U, 2 * D, list(hidden), dropout_layers=[pm.models.CDropout(0.1 * np.ones(h)) for h in hidden]),
        reward_func=pm.rewards.CartpoleReward(pole_length=torch.tensor(0.5)),
        output_density=pm.models.DiagGaussianDensity(D)).float()
    pol = pm.models.Policy(pm.models.mlp(D, 2 * U, list(hidden), dropout_layers=[pm.models.BDropout(0.1) for _ in hidden],
                                         output_nonlin=partial(pm.models.DiagGaussianDensity, U), layer_norm=True), 10.0).float()
    dyn.set_dataset(torch.randn(300, D + U), 0.01 * torch.randn(300, D))
    dyn, pol = dyn.to(dev), pol.to(dev)
    opt = torch.optim.Adam(pol.parameters(), 1e-4)
    x0 = 0.1 * torch.randn(B, D, device=dev)
    return lambda n: pm.algorithms.mc_pilco(x0, dyn, pol, H, opt, None, n, progress=False)


def mlp_case(dev, B=2500, dims=(4, 200, 200, 2)):
    g = torch.Generator().manual_seed(0)
    nl, n_out = len(dims) - 1, dims[-1] // 2
    flat = torch.cat([t.reshape(-1) for i in range(nl) for t in
                      (torch.randn(dims[i + 1], dims[i], generator=g) / np.sqrt(dims[i]), 0.1 * torch.randn(dims[i + 1], generator=g))])
    bits = [E.pack_mask((torch.rand(B, dims[i + 1], generator=g) < 0.9).float().to(dev)) for i in range(nl - 1)]
    call = E._MlpCall(torch.randn(B, dims[0], generator=g).to(dev), flat.to(dev), list(dims), [0.9] * (nl - 1), bits,
                      torch.randn(B, n_out, generator=g).to(dev), None, None, None, None, torch.ones(n_out), torch.zeros(n_out),
                      E.LOG_MAX_STD)
    ups = [torch.randn(B, n_out, generator=g).to(dev) for _ in range(3)]
    # the same network with concrete layers (keep = 1; the hard samples are the masks above)
    conc_call = E._MlpCall(call.x, call.pf, list(dims), [1.0] * (nl - 1), bits, call.z, None, None, None, None,
                           torch.ones(n_out), torch.zeros(n_out), E.LOG_MAX_STD)
    conc = [(torch.rand(B, dims[i + 1], generator=g).to(dev), torch.full((dims[i + 1],), 2.2, device=dev), 0.1)
            for i in range(nl - 1)]
    return ((lambda: call.backward(*ups)), (lambda: call.grad_input(*ups)), (lambda: conc_call.backward(*ups, concrete=conc)),
            call, ups)


def rollout_case(dev, B=2500, H=40, D=4, U=1, hidden=(200, 200)):
    torch.manual_seed(0)
    dyn = pm.models.DynamicsModel(
        pm.models.mlp(D + U, 2 * D, list(hidden), dropout_layers=[pm.models.CDropout(0.1 * np.ones(h)) for h in hidden]),
        reward_func=pm.rewards.CartpoleReward(pole_length=torch.tensor(0.5)),
        output_density=pm.models.DiagGaussianDensity(D)).float()
    from functools import partial
    pol = pm.models.Policy(pm.models.mlp(D, 2 * U, list(hidden), dropout_layers=[pm.models.BDropout(0.1) for _ in hidden],
                                         output_nonlin=partial(pm.models.DiagGaussianDensity, U)), 10.0).float()
    dyn.Sy.data = torch.full((1, D), 0.05)       # small steps: the trajectory stays bounded over the horizon
    dyn, pol = dyn.to(dev).eval(), pol.to(dev)
    x0 = 0.1 * torch.randn(B, D, device=dev)

    def run(**kw):
        pol.zero_grad()
        _, _, rewards = pm.utils.rollout(x0, dyn, pol, H, resample_state_noise=False, resample_action_noise=False, **kw)
        assert len(rewards) == H
        (-torch.stack(rewards).mean()).backward()
    return (lambda: run(on_pol_eval=lambda i, s, a: (s, a))), run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=20)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default=None, choices=['mlp', 'ln'], help='mlp: the stand-alone calls only; ln: they and the '
                    'layer-norm figures')
    ap.add_argument('--other-lib', default=None, help='a second build of libpmbrl_hip.so to time pmbrl_mlp_backward on')
    ap.add_argument('--mcp-iters', type=int, default=10, help='mc_pilco iterations per timed block of the ln figures')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs a HIP device')
    dev = torch.device('cuda:0')
    bwd, gin, bwd_conc, call, ups = mlp_case(dev)
    out = dict(blocks=a.blocks,
               mlp_backward=timed(bwd, a.blocks, a.iters, a.warmup), mlp_grad_input=timed(gin, a.blocks, a.iters, a.warmup),
               mlp_backward_concrete=timed(bwd_conc, a.blocks, a.iters, a.warmup))
    if a.other_lib:
        import copy
        other = copy.copy(call)      # the same marshalled call, sent to the other build
        other.lib = other_build(a.other_lib)
        t = alternating([bwd, lambda: other.backward(*ups)], a.blocks, a.iters, a.warmup)
        assert torch.equal(call.backward(*ups)[1], other.backward(*ups)[1])
        out.update(mlp_backward_this_build=t[0], mlp_backward_other_build=t[1],
                   other_build_id=other.lib.pmbrl_build_id().decode())
    if a.only == 'ln' or a.only is None:
        fs = ln_case(dev)
        out.update(zip(fs, alternating(list(fs.values()), a.blocks, a.iters, a.warmup)))
        run = mcp_ln_case(dev)
        run(2)
        out['mc_pilco_iteration_ln_policy'] = timed(lambda: run(a.mcp_iters), max(3, a.blocks // 4), 1, 0)
        for k in ('ms_median', 'ms_min', 'ms_max'):
            out['mc_pilco_iteration_ln_policy'][k] /= a.mcp_iters
    if a.only is None:
        hooked, fused = rollout_case(dev)
        out.update(rollout_hooked=timed(hooked, a.blocks, 1, 1),
                   rollout_fused_autograd=timed(fused, a.blocks, a.iters, a.warmup))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
