"""CPU: the C ABI of the sharded iteration tail (the gradient exchange inside pmbrl_rollout_bwd_adam) is there -- the
setter is declared, exported and bound, and the library says it is the version that has it.  No compute calls."""
import ctypes
import os
import re

from tests import common


def test_grad_comm_setter_is_declared_exported_and_bound():
    from prob_mbrl_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    header = open(os.path.join(common.ROOT, 'include', 'pmbrl.h')).read()
    assert re.search(r'int\s+pmbrl_plan_set_grad_comm\s*\(\s*pmbrl_plan\s*\*\s*plan\s*,\s*pmbrl_comm\s*\*\s*comm\s*,'
                     r'\s*pmbrl_p2p\s*\*\s*p2p\s*\)', header)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'pmbrl_plan_set_grad_comm')
    assert 'pmbrl_plan_set_grad_comm' in _lib.EXPORTS
    lib = _lib.load()
    assert lib.pmbrl_plan_set_grad_comm.argtypes == [ctypes.c_void_p] * 3


def test_version_and_info_count_are_the_bumped_ones():
    from prob_mbrl_amd import _lib
    assert _lib.load().pmbrl_version() == 8
    header = open(os.path.join(common.ROOT, 'include', 'pmbrl.h')).read()
    assert int(re.search(r'PMBRL_INFO_TAIL_CALLS\s*=\s*(\d+)', header).group(1)) == 21
    assert int(re.search(r'PMBRL_INFO_COUNT\s*=\s*(\d+)', header).group(1)) == _lib.INFO_COUNT == 22


def test_setter_rejects_a_null_plan_without_gpu():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    assert lib.pmbrl_plan_set_grad_comm(None, None, None) < 0
    assert b'null' in lib.pmbrl_last_error()
