"""CPU: the C ABI of the stand-alone network's backward (pmbrl_mlp_backward) validates a call without a device, and
`models.param_grad()` is a proper context (no compute calls -- there is no GPU here)."""
import ctypes
import threading

from tests import common  # noqa: F401  (puts the repository root on sys.path)


def _call(dims, B=45, act=0):
    from prob_mbrl_amd import _lib
    c = _lib.MlpCall()
    c.B = B
    c.net.n_layers = len(dims) - 1
    for i, d in enumerate(dims):
        c.net.dims[i] = d
    for l in range(len(dims) - 2):
        c.net.keep[l] = 1.0
    c.max_log_std = 1.6
    c.act = act
    return c


def test_backward_symbols_exported():
    from prob_mbrl_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pmbrl_mlp_backward_workspace_bytes', 'pmbrl_mlp_backward'):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS


def test_backward_workspace_bytes():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    dims = [6, 40, 56, 6]
    n_params = sum(dims[i + 1] * dims[i] + dims[i + 1] for i in range(3))
    fwd = lib.pmbrl_mlp_workspace_bytes(ctypes.byref(_call(dims)))
    got = lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(_call(dims)))
    assert got > 0
    # the packed weights of the forward, then one gradient slab per workgroup: 45 rows are 3 tiles of 16
    assert fwd + 3 * 4 * n_params <= got <= fwd + 256 + 3 * 4 * n_params
    # the slabs stop growing at the block cap
    cap = _lib.MLP_BWD_MAX_BLOCKS
    at_cap = lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(_call(dims, B=16 * cap)))
    assert lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(_call(dims, B=16 * cap + 5))) == at_cap
    assert lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(_call(dims, B=1000 * cap))) == at_cap
    assert fwd + cap * 4 * n_params <= at_cap <= fwd + 256 + cap * 4 * n_params


def test_backward_block_cap_shrinks_for_large_networks():
    """256 slabs of a [512, 512, 512] network would be 538 MB: the cap comes down to what 64 MB hold."""
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    dims = [512, 512, 512]
    n_params = 2 * (512 * 512 + 512)
    slabs = (64 << 20) // (4 * n_params)
    assert 1 < slabs < _lib.MLP_BWD_MAX_BLOCKS
    fwd = lib.pmbrl_mlp_workspace_bytes(ctypes.byref(_call(dims)))
    got = lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(_call(dims, B=16 * _lib.MLP_BWD_MAX_BLOCKS)))
    assert fwd + slabs * 4 * n_params <= got <= fwd + 256 + slabs * 4 * n_params


def test_backward_refuses_bad_calls_with_a_message():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    assert lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(_call([6, 40, 56, 6], act=7))) == 0
    assert b'activation' in lib.pmbrl_last_error()
    # every Linear's input stays in LDS: 6 buffers of 16 x 520 floats are past the 160 KB of a CU, the forward's 2 are not
    wide = _call([32, 512, 512, 512, 64])
    assert lib.pmbrl_mlp_workspace_bytes(ctypes.byref(wide)) > 0
    assert lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(wide)) == 0
    assert b'LDS' in lib.pmbrl_last_error()
    # ... and Tanh / SiLU keep a derivative buffer per hidden layer on top: four hidden layers of 288 fit with ReLU only
    assert lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(_call([8, 288, 288, 288, 288, 4]))) > 0
    assert lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(_call([8, 288, 288, 288, 288, 4], act=1))) == 0
    assert b'LDS' in lib.pmbrl_last_error()
    # the call itself refuses the same way before it touches the device
    rc = lib.pmbrl_mlp_backward(None, ctypes.byref(wide), None, None, None, None, *([None] * 12))
    assert rc == -3 and b'LDS' in lib.pmbrl_last_error()


def test_param_grad_toggles_nests_and_restores():
    from prob_mbrl_amd import models as M
    assert not M.param_grad_enabled()
    with M.param_grad():
        assert M.param_grad_enabled()
        with M.param_grad(False):
            assert not M.param_grad_enabled()
            with M.param_grad():
                assert M.param_grad_enabled()
            assert not M.param_grad_enabled()
        assert M.param_grad_enabled()
        seen = []
        t = threading.Thread(target=lambda: seen.append(M.param_grad_enabled()))
        t.start()
        t.join()
        assert seen == [False]          # thread-local
    assert not M.param_grad_enabled()
    try:
        with M.param_grad():
            raise KeyError('x')
    except KeyError:
        pass
    assert not M.param_grad_enabled()   # restored on an exception too
