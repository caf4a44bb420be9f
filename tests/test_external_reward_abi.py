"""CPU: the C ABI of a reward evaluated by the caller (PMBRL_REWARD_EXTERNAL): the new entry points are exported, no
struct grew, plan creation knows the new kind, and pmbrl_rollout_rewards validates its arguments without a device."""
import ctypes
import re

from tests import common

NAMES = ('pmbrl_plan_reward_input', 'pmbrl_rollout_rewards')
PTR = ctypes.c_void_p(256)      # a non-null pointer that is never dereferenced: the calls below fail before any launch


def test_new_names_are_exported_and_listed():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    header = open(common.ROOT + '/include/pmbrl.h').read()
    for name in NAMES:
        assert hasattr(lib, name), 'missing export %s' % name
        assert name in _lib.EXPORTS
        assert re.search(r'\bint %s\(' % name, header)
    assert re.search(r'#define PMBRL_REWARD_EXTERNAL 3\b', header) and _lib.REWARD_EXTERNAL == 3


def test_no_struct_grew_and_the_version_stays():
    from prob_mbrl_amd import _lib
    assert ctypes.sizeof(_lib.Reward) == 4 * (3 + 8 + 1) + 4 * (8 * 64 + 8 + 2 + 64 + 64 * 64)
    # pmbrl_config: 10 scalars, two pmbrl_mlp, the reward, then 2 + (1 + 8) + (1 + 8) + 1 + 4 + 2 int32 fields
    mlp = 4 + 4 * 9 + 4 * 8
    assert ctypes.sizeof(_lib.MLP) == mlp
    assert ctypes.sizeof(_lib.Config) == 4 * 10 + 2 * mlp + ctypes.sizeof(_lib.Reward) + 4 * (2 + 9 + 9 + 1 + 4 + 2)
    assert _lib.load().pmbrl_version() == 8


def _create(kind):
    """pmbrl_plan_create on a configuration that is empty but for its sizes and the reward's kind: (code, message)."""
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    cfg = _lib.Config()
    cfg.B, cfg.D, cfg.U, cfg.H = 32, 4, 1, 8
    cfg.reward.kind = kind
    cfg.reward.k = 1
    plan = ctypes.c_void_p()
    rc = lib.pmbrl_plan_create(ctypes.byref(cfg), 0, ctypes.byref(plan))
    assert not plan.value
    return rc, lib.pmbrl_last_error().decode()


def test_plan_create_knows_the_external_kind():
    rc, msg = _create(3)
    assert rc < 0 and 'unknown reward kind' not in msg, msg      # (the networks are empty: that is what it fails on)
    assert 'n_layers' in msg, msg
    rc, msg = _create(9)
    assert rc == -2 and 'unknown reward kind' in msg, msg
    # the constants of an external reward are ignored: k = 0 is no reason to refuse it
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    cfg = _lib.Config()
    cfg.B, cfg.D, cfg.U, cfg.H = 32, 4, 1, 8
    cfg.reward.kind = 3
    plan = ctypes.c_void_p()
    assert lib.pmbrl_plan_create(ctypes.byref(cfg), 0, ctypes.byref(plan)) < 0
    assert 'reward.k' not in lib.pmbrl_last_error().decode()


def test_rewards_call_refuses_null_arguments():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    rc = lib.pmbrl_rollout_rewards(None, None, PTR, PTR, PTR, PTR, PTR, PTR)
    assert rc == -1 and b'null' in lib.pmbrl_last_error()
    assert lib.pmbrl_rollout_rewards(None, None, None, None, None, None, None, None) == -1
    off = ctypes.c_int64(7)
    assert lib.pmbrl_plan_reward_input(None, ctypes.byref(off)) == -1 and off.value == 7
    assert lib.pmbrl_plan_reward_input(PTR, None) == -1
