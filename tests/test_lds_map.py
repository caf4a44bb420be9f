"""The LDS maps of the general and the latency-optimised sweeps (prob_mbrl_amd/csrc/pmbrl_lds_map.h) without a device:
tests/lds_map_check.cpp includes the header, is compiled by the host compiler alone and checks, for one smallest shape
per branch of the two walks -- K-split tails, the head partials aliased, split precision, whole and split groups, the
LDS-resident tiles, networks of different depth, the general family's aliased partials and in-place form -- that the
regions follow each other without overlap, end at the total and sit at offsets worked out by hand from the region list."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_lds_map(tmp_path):
    exe = str(tmp_path / 'lds_map_check')
    subprocess.check_call([HIPCC, '-x', 'c++', '-std=c++17', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'),
                           '-I' + os.path.join(ROOT, 'prob_mbrl_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'lds_map_check.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout
