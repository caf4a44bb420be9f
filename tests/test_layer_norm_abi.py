"""CPU: mlp(layer_norm=True) builds the reference's network, the C ABI of the pmbrl_mlp_*_ln calls validates a call
without a device, and the fused consumers refuse a layer-normalised network by name."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from tests import common  # noqa: F401  (puts the repository root on sys.path)
from tests.test_concrete_grad_abi import PTR, _call, _conc

NAMES = ('pmbrl_mlp_ln_workspace_bytes', 'pmbrl_mlp_forward_ln', 'pmbrl_mlp_grad_input_ln',
         'pmbrl_mlp_backward_ln_workspace_bytes', 'pmbrl_mlp_backward_ln')
BUF = 16 * 216 * 4      # one 16-row LDS buffer of the 2 x 200 network
KB160 = 160 * 1024


def _ln(layers, eps=1e-5, beta=True):
    from prob_mbrl_amd import _lib
    n = _lib.MlpLayerNorm()
    for l in layers:
        n.gamma_d[l] = PTR
        n.beta_d[l] = PTR if beta else None
        n.eps[l] = eps
    return n


def _bytes(lib, call, conc, ln):
    return lib.pmbrl_mlp_backward_ln_workspace_bytes(ctypes.byref(call), ctypes.byref(conc) if conc is not None else None,
                                                     ctypes.byref(ln) if ln is not None else None)


# ---------------------------------------------------------------------------
# the factory
# ---------------------------------------------------------------------------
def test_mlp_builds_the_references_network():
    import prob_mbrl_amd as pm
    torch.manual_seed(0)
    net = pm.models.mlp(4, 2, [24, 40], nonlin=torch.nn.Tanh, layer_norm=True,
                        output_nonlin=partial(pm.models.DiagGaussianDensity, 1))
    assert list(net._modules) == ['fc0', 'ln0', 'nonlin0', 'drop0', 'fc1', 'ln1', 'nonlin1', 'drop1', 'fc_out', 'fc_nonlin']
    assert [n for n, _ in net.named_parameters()] == ['fc0.weight', 'fc0.bias', 'ln0.weight', 'ln0.bias', 'fc1.weight',
                                                      'fc1.bias', 'ln1.weight', 'ln1.bias', 'fc_out.weight', 'fc_out.bias']
    for l, h in enumerate((24, 40)):
        ln = getattr(net, 'ln%d' % l)
        assert isinstance(ln, torch.nn.LayerNorm) and tuple(ln.normalized_shape) == (h,) and ln.eps == 1e-5
        assert bool((ln.weight == 1).all())                       # not touched by weights_initializer (core.py:83-85)
        b = ln.bias.detach()
        assert float(b.abs().max()) <= 0.1 and float(b.std()) > 0.02      # drawn by biases_initializer (core.py:90-92)
    # the parsers keep their shapes; the new accessor names the LayerNorms
    assert len(net.layer_spec()) == 3 and len(net.layers_spec()) == 4
    assert net.layer_norms() == [net.ln0, net.ln1]
    plain = pm.models.mlp(4, 2, [24, 40], output_nonlin=partial(pm.models.DiagGaussianDensity, 1))
    assert plain.layer_norms() == [None, None] and not any(isinstance(m, torch.nn.LayerNorm) for m in plain.modules())
    # the dropout regulariser skips the LayerNorm and lands on the next Linear
    assert float(net.regularization_loss().detach()) > 0


def test_the_other_arguments_stay_refused():
    import prob_mbrl_amd as pm
    for kw in (dict(spectral_norm=True), dict(spectral_norm_output=True), dict(input_dropout=pm.models.BDropout),
               dict(hidden_biases=False), dict(output_biases=False)):
        with pytest.raises(NotImplementedError):
            pm.models.mlp(4, 2, [8, 8], layer_norm=True, **kw)
    # per-unit rates cannot be folded into a Linear in front of a LayerNorm
    net = pm.models.mlp(4, 2, [8, 8], layer_norm=True, dropout_layers=[pm.models.BDropout(torch.linspace(0.1, 0.3, 8))] * 2)
    with pytest.raises(NotImplementedError, match='per-unit'):
        net.layers_spec()
    # a LayerNorm anywhere else is not what the kernels compute
    odd = pm.models.BSequential(torch.nn.Linear(4, 8), torch.nn.ReLU(), torch.nn.LayerNorm(8), torch.nn.Linear(8, 2))
    with pytest.raises(NotImplementedError, match='right behind'):
        odd.layers_spec()


def test_fused_consumers_refuse_layer_norm_by_name():
    import prob_mbrl_amd as pm
    from prob_mbrl_amd import critic, rollout
    D, U = 4, 1
    pol = pm.models.Policy(pm.models.mlp(D, 2 * U, [8, 8], layer_norm=True,
                                         output_nonlin=partial(pm.models.DiagGaussianDensity, U)), 10.0)
    plain_pol = pm.models.Policy(pm.models.mlp(D, 2 * U, [8, 8], output_nonlin=partial(pm.models.DiagGaussianDensity, U)), 10.0)
    mk = lambda ln: pm.models.DynamicsModel(  # noqa: E731
        pm.models.mlp(D + U, 2 * D, [8, 8], layer_norm=ln, dropout_layers=[pm.models.CDropout(0.1 * np.ones(8))] * 2),
        reward_func=pm.rewards.CartpoleReward(pole_length=torch.tensor(0.5)), output_density=pm.models.DiagGaussianDensity(D))
    args = (8, 4, False, False, False, False, None, None, None)
    for dyn, p in ((mk(False), pol), (mk(True), plain_pol)):
        with pytest.raises(NotImplementedError, match=r'layer norm.*param_grad'):
            rollout.Bundle(dyn, p, *args)
    assert rollout.stepwise_networks(mk(False), pol) and rollout.stepwise_networks(mk(True), plain_pol)
    assert rollout.stepwise_networks(mk(False), plain_pol) is None
    dyn = mk(True)
    dyn.set_dataset(torch.randn(20, D + U), torch.randn(20, D))
    with pytest.raises(NotImplementedError, match=r'layer norm.*param_grad'):
        pm.train_regressor.train_regressor(dyn, iters=1)
    V = pm.models.Regressor(pm.models.mlp(D, 1, [8, 8], layer_norm=True, dropout_layers=[pm.models.CDropout(0.1 * np.ones(8))] * 2))
    with pytest.raises(NotImplementedError, match=r'layer norm.*param_grad'):
        critic.update_value_function(V, None, 4, 0, None, None, None, 1.0)


def test_reference_checkpoint_keys_load():
    import prob_mbrl_amd as pm
    mk = lambda: pm.models.Policy(pm.models.mlp(4, 2, [8, 8], layer_norm=True,  # noqa: E731
                                                output_nonlin=partial(pm.models.DiagGaussianDensity, 1)), 10.0)
    a, b = mk(), mk()
    with torch.no_grad():
        a.model.ln0.weight.add_(0.5)
    sd = a.state_dict()
    assert 'model.ln0.weight' in sd and 'model.ln1.bias' in sd
    b.load(sd)
    assert torch.equal(b.model.ln0.weight, a.model.ln0.weight) and torch.equal(b.model.ln1.bias, a.model.ln1.bias)


# ---------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------
def test_layer_norm_symbols_exported():
    from prob_mbrl_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    # the existing structs did not grow for it, and the version the existing tests pin is unchanged
    assert ctypes.sizeof(_lib.MLP) == 4 + 4 * 9 + 4 * 8
    assert ctypes.sizeof(_lib.MlpCall) == 4 + ctypes.sizeof(_lib.MLP) + 4 + 4
    assert ctypes.sizeof(_lib.MlpConcrete) == 8 * 8 + 8 * 8 + 4 * 8
    assert ctypes.sizeof(_lib.MlpLayerNorm) == 8 * 8 + 8 * 8 + 4 * 8
    assert _lib.load().pmbrl_version() == 8


def test_workspace_is_the_backwards_plus_the_ln_slabs():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    dims = [6, 40, 56, 6]
    plain = lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(_call(dims)))
    # ln == NULL: the query of the call it extends
    assert _bytes(lib, _call(dims), None, None) == plain
    conc = lib.pmbrl_mlp_backward_concrete_workspace_bytes(ctypes.byref(_call(dims)), ctypes.byref(_conc([0, 1])))
    assert _bytes(lib, _call(dims), _conc([0, 1]), None) == conc
    # 45 rows are 3 tiles: 3 slabs of 2 x (40 + 56) floats behind the parameter (and logit) slabs
    assert plain + 3 * 4 * 192 <= _bytes(lib, _call(dims), None, _ln([0, 1])) <= plain + 512 + 3 * 4 * 192
    assert plain + 3 * 4 * 112 <= _bytes(lib, _call(dims), None, _ln([1])) <= plain + 512 + 3 * 4 * 112
    assert conc + 3 * 4 * 192 <= _bytes(lib, _call(dims), _conc([0, 1]), _ln([0, 1])) <= conc + 512 + 3 * 4 * 192
    cap = _lib.MLP_BWD_MAX_BLOCKS
    at_cap = _bytes(lib, _call(dims, B=16 * cap), None, _ln([0, 1]))
    assert _bytes(lib, _call(dims, B=16 * cap + 5), None, _ln([0, 1])) == at_cap
    # the forward's and the input gradient's workspace is pmbrl_mlp_forward's
    fwd = lib.pmbrl_mlp_workspace_bytes(ctypes.byref(_call(dims)))
    assert lib.pmbrl_mlp_ln_workspace_bytes(ctypes.byref(_call(dims)), ctypes.byref(_ln([0, 1]))) == fwd
    assert lib.pmbrl_mlp_ln_workspace_bytes(ctypes.byref(_call(dims)), None) == fwd


# buffers of the 2 x 200 backward: 5, + 2 derivative buffers unless ReLU, + 1 per concrete layer, + 1 per LN layer
@pytest.mark.parametrize('act,conc,ln,buffers', [
    (0, [], [0, 1], 7), (0, [0], [0, 1], 8), (0, [0, 1], [0, 1], 9),
    (1, [], [0, 1], 9), (1, [0], [0, 1], 10), (1, [0, 1], [0], 10), (1, [0, 1], [0, 1], 11),
    (2, [0, 1], [0, 1], 11), (2, [], [0, 1], 9),
])
def test_which_two_by_200_combinations_fit(act, conc, ln, buffers):
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    call = _call([5, 200, 200, 2], B=2500, act=act)
    need = buffers * BUF + 24 * 1024
    got = _bytes(lib, call, _conc(conc) if conc else None, _ln(ln))
    if need <= KB160:
        assert got > 0, (need, lib.pmbrl_last_error())
    else:
        assert got == 0 and b'LDS' in lib.pmbrl_last_error()
        rc = lib.pmbrl_mlp_backward_ln(None, ctypes.byref(call), None, None, None, None, *([None] * 12),
                                       ctypes.byref(_conc(conc)) if conc else None, None, ctypes.byref(_ln(ln)), None)
        assert rc == -3 and b'LDS' in lib.pmbrl_last_error()
    assert (buffers, need) in ((7, 121344), (8, 135168), (9, 148992), (10, 162816), (11, 176640))


def test_bad_arguments_give_a_negative_code():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    dims = [6, 40, 56, 6]

    def bwd(call, ln, conc=None, grad_logit=None, ws=PTR):
        return lib.pmbrl_mlp_backward_ln(None, ctypes.byref(call), ws, PTR, PTR, None, *([None] * 7), PTR, None, None,
                                         None, None, ctypes.byref(conc) if conc is not None else None, grad_logit,
                                         ctypes.byref(ln), PTR)

    def fwd(call, ln):
        return lib.pmbrl_mlp_forward_ln(None, ctypes.byref(call), PTR, PTR, PTR, None, *([None] * 7), PTR, None, None,
                                        ctypes.byref(ln))

    def gin(call, ln):
        return lib.pmbrl_mlp_grad_input_ln(None, ctypes.byref(call), PTR, PTR, PTR, None, *([None] * 7), PTR, None, None,
                                           PTR, ctypes.byref(ln))

    for f in (bwd, fwd, gin):
        assert f(_call(dims), _ln([])) == -2 and b'no layer-norm layer' in lib.pmbrl_last_error()
        assert f(_call(dims), _ln([2])) == -2 and b'hidden layer' in lib.pmbrl_last_error()
        assert f(_call(dims), _ln([0], beta=False)) == -1 and b'beta_d' in lib.pmbrl_last_error()
        assert f(_call(dims), _ln([0], eps=0.0)) == -2 and b'eps' in lib.pmbrl_last_error()
        assert f(_call(dims), _ln([1], eps=-1e-5)) == -2 and b'eps' in lib.pmbrl_last_error()
    # the concrete part keeps its own checks
    assert bwd(_call(dims), _ln([0]), _conc([0]), grad_logit=None) == -1
    assert bwd(_call(dims), _ln([0]), _conc([0], temp=0.0), grad_logit=PTR) == -2 and b'temp' in lib.pmbrl_last_error()
    assert bwd(_call(dims), _ln([0]), ws=None) == -1
    assert _bytes(lib, _call(dims), None, _ln([])) == 0
    assert _bytes(lib, _call(dims, act=7), None, _ln([0])) == 0 and b'activation' in lib.pmbrl_last_error()
    # the input gradient's own LDS need: Tanh, 2 x 288 wide -- 6 buffers of 16 x 296 floats fit, 8 do not
    wide = _call([5, 288, 288, 2], act=1)
    assert gin(wide, _ln([0, 1])) == -3 and b'LDS' in lib.pmbrl_last_error()
