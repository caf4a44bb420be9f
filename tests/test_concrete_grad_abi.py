"""CPU: the C ABI of pmbrl_mlp_backward_concrete (the stand-alone network's backward with train-mode concrete-dropout
layers) validates a call without a device."""
import ctypes

from tests import common  # noqa: F401  (puts the repository root on sys.path)

PTR = 0x1000      # a non-null address: the queries and the argument checks never dereference it


def _call(dims, B=45, act=0, keep=1.0):
    from prob_mbrl_amd import _lib
    c = _lib.MlpCall()
    c.B = B
    c.net.n_layers = len(dims) - 1
    for i, d in enumerate(dims):
        c.net.dims[i] = d
    for l in range(len(dims) - 2):
        c.net.keep[l] = keep
    c.max_log_std = 1.6
    c.act = act
    return c


def _conc(layers, temp=0.1, logit=True):
    from prob_mbrl_amd import _lib
    q = _lib.MlpConcrete()
    for l in layers:
        q.u_d[l] = PTR
        q.logit_d[l] = PTR if logit else None
        q.temp[l] = temp
    return q


def _bytes(lib, call, conc):
    return lib.pmbrl_mlp_backward_concrete_workspace_bytes(ctypes.byref(call), ctypes.byref(conc))


def test_concrete_symbols_exported():
    from prob_mbrl_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pmbrl_mlp_backward_concrete_workspace_bytes', 'pmbrl_mlp_backward_concrete'):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    # the existing structs did not grow for it
    assert ctypes.sizeof(_lib.MLP) == 4 + 4 * 9 + 4 * 8
    assert ctypes.sizeof(_lib.MlpConcrete) == 8 * 8 + 8 * 8 + 4 * 8


def test_workspace_is_the_backwards_plus_the_logit_slabs():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    dims = [6, 40, 56, 6]
    plain = lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(_call(dims)))
    got = _bytes(lib, _call(dims), _conc([0, 1]))
    # 45 rows are 3 tiles: 3 slabs of 40 + 56 logits behind the parameter slabs
    assert plain + 3 * 4 * 96 <= got <= plain + 256 + 3 * 4 * 96
    assert plain + 3 * 4 * 56 <= _bytes(lib, _call(dims), _conc([1])) <= plain + 256 + 3 * 4 * 56
    cap = _lib.MLP_BWD_MAX_BLOCKS
    at_cap = _bytes(lib, _call(dims, B=16 * cap), _conc([0, 1]))
    assert _bytes(lib, _call(dims, B=16 * cap + 5), _conc([0, 1])) == at_cap


def test_two_by_200_with_two_concrete_layers_fits():
    """9 buffers of 16 x 216 floats + 24 KB = 148 992 bytes of LDS with Tanh or SiLU, under the 160 KB of a CU."""
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    for act in (0, 1, 2):
        assert _bytes(lib, _call([5, 200, 200, 2], B=2500, act=act), _conc([0, 1])) > 0, act


def test_a_width_that_cannot_fit_is_refused_with_a_message():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    # Tanh, two hidden layers of 240: pmbrl_mlp_backward's 7 buffers of 16 x 248 floats fit, two more do not
    wide = _call([5, 240, 240, 2], act=1)
    assert lib.pmbrl_mlp_backward_workspace_bytes(ctypes.byref(wide)) > 0
    assert _bytes(lib, wide, _conc([0])) > 0
    assert _bytes(lib, wide, _conc([0, 1])) == 0
    assert b'LDS' in lib.pmbrl_last_error()
    rc = lib.pmbrl_mlp_backward_concrete(None, ctypes.byref(wide), None, None, None, None, *([None] * 12),
                                         ctypes.byref(_conc([0, 1])), None)
    assert rc == -3 and b'LDS' in lib.pmbrl_last_error()


def test_bad_arguments_give_a_negative_code():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    dims = [6, 40, 56, 6]

    def rc(call, conc, grad_logit=PTR, ws=PTR):
        conc = ctypes.byref(conc) if conc is not None else None
        return lib.pmbrl_mlp_backward_concrete(None, ctypes.byref(call), ws, PTR, PTR, None, *([None] * 7), PTR, None, None,
                                               None, None, conc, grad_logit)

    assert rc(_call(dims), None) == -1
    assert rc(_call(dims), _conc([])) == -2 and b'no concrete layer' in lib.pmbrl_last_error()
    assert rc(_call(dims), _conc([2])) == -2 and b'hidden layer' in lib.pmbrl_last_error()
    assert rc(_call(dims), _conc([0], logit=False)) == -1 and b'logit_d' in lib.pmbrl_last_error()
    assert rc(_call(dims), _conc([0], temp=0.0)) == -2 and b'temp' in lib.pmbrl_last_error()
    assert rc(_call(dims, keep=0.8), _conc([1])) == -2 and b'keep' in lib.pmbrl_last_error()
    assert rc(_call(dims), _conc([0, 1]), grad_logit=None) == -1
    assert rc(_call(dims), _conc([0, 1]), ws=None) == -1
    assert _bytes(lib, _call(dims), _conc([])) == 0
    assert _bytes(lib, _call(dims, act=7), _conc([0])) == 0 and b'activation' in lib.pmbrl_last_error()
