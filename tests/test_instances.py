"""The sweep-kernel instance lists (prob_mbrl_amd/csrc/pmbrl_instances.h) without a device: tests/instances_check.cpp
includes the header, is compiled by the host compiler alone and checks that the stage pairs derived from the lists are
the ones the plan always chose among, that whatever pair the chooser returns has its instances, and that the
shape-specialised rows the plan's predicates ask for exist."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_instance_lists(tmp_path):
    exe = str(tmp_path / 'instances_check')
    subprocess.check_call([HIPCC, '-x', 'c++', '-std=c++17', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'),
                           '-I' + os.path.join(ROOT, 'prob_mbrl_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'instances_check.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout
