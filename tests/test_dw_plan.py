"""The dW GEMM's planner (prob_mbrl_amd/csrc/pmbrl_dw_plan.h) without a device: tests/dw_plan_check.cpp includes the
header, is compiled by the host compiler alone and checks, for one smallest shape per form, what the planner decides --
block tables, wide and pre-split units, the whole-layer kernel, the pipelined ranges, the streamed form's cut and
consumers, the head in the consumers -- against values worked out by hand from the rules, and what build_dw_blocks
guarantees of every table."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_dw_planner(tmp_path):
    exe = str(tmp_path / 'dw_plan_check')
    subprocess.check_call([HIPCC, '-x', 'c++', '-std=c++17', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'),
                           '-I' + os.path.join(ROOT, 'prob_mbrl_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'dw_plan_check.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout
