"""CPU: the C ABI of the training step's kernel forms (pmbrl_bnn_plan_create_form, pmbrl_bnn_plan_form) -- validation
comes before the first device call -- and the spill form's LDS map: its mirror (tests/fit_wide_cases.py) against the byte
table of DESIGN.md 4d and against what plan creation refuses."""
import ctypes
import os
import re

import pytest

from tests import common
from tests import fit_envelope_cases as FE
from tests import fit_wide_cases as FW
from tests.test_fit_envelope_cases import _config


def create(form, dims, act=FE.RELU):
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    plan = ctypes.c_void_p()
    rc = lib.pmbrl_bnn_plan_create_form(ctypes.byref(_config(dims, act)), 0, form, ctypes.byref(plan))
    return rc, plan, lib.pmbrl_last_error()


def test_symbols_are_exported_and_the_version_stays():
    from prob_mbrl_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(common.ROOT, 'include', 'pmbrl.h')).read()
    for name in ('pmbrl_bnn_plan_create_form', 'pmbrl_bnn_plan_form'):
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, header)
    assert lib.pmbrl_version() == 8
    assert (_lib.BNN_FORM_RESIDENT, _lib.BNN_FORM_SPILL, _lib.BNN_FORM_AUTO) == (0, 1, 2)
    for k, v in (('RESIDENT', 0), ('SPILL', 1), ('AUTO', 2)):
        assert re.search(r'#define PMBRL_BNN_FORM_%s %d\b' % (k, v), header)
    assert lib.pmbrl_bnn_plan_form(None) == -1


@pytest.mark.parametrize('form', [-1, 3, 7])
def test_unknown_form_is_refused(form):
    rc, plan, msg = create(form, [6, 40, 24, 8])
    assert rc == -2 and b'form' in msg and not plan


@pytest.mark.parametrize('dims, act', [([6, 272, 272, 8], FE.RELU), ([6, 256, 256, 8], FE.TANH)])
def test_resident_form_keeps_its_edge(dims, act):
    from prob_mbrl_amd import _lib
    rc, plan, msg = create(_lib.BNN_FORM_RESIDENT, dims, act)
    assert rc == -3 and b'LDS' in msg and not plan
    assert FW.spill_fits(dims)      # (what 'auto' turns to: accepted by the GPU tests)


@pytest.mark.parametrize('form', ['SPILL', 'AUTO'])
@pytest.mark.parametrize('dims', [[6, FW.WIDEST + 1, 8], [FW.WIDEST + 1, 40, 8], [6, 40, 2 * (FW.WIDEST // 2 + 1)],
                                  [40, 512, 1024, 512, 64]])
def test_spill_form_refuses_behind_its_edge(form, dims):
    """The first width past the edge -- as a hidden layer, as the input, as the head -- and the plan's width limit: -3 and a
    message that names LDS, no plan."""
    from prob_mbrl_amd import _lib
    assert not FW.spill_fits(dims)
    rc, plan, msg = create(getattr(_lib, 'BNN_FORM_' + form), dims, FE.SILU)
    assert rc == -3 and b'LDS' in msg and not plan


def design_table():
    text = open(os.path.join(common.ROOT, 'DESIGN.md')).read()
    sec = text[text.index('## 4d.'):]
    sec = sec[:sec.index('\n## ', 4)]
    rows = re.findall(r'^\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*([\d ]+?)\s*\|\s*(yes|no)\s*\|$', sec, re.M)
    return [(int(w), int(ld), int(b.replace(' ', '')), fits == 'yes') for w, ld, b, fits in rows]


def test_mirror_of_the_map_agrees_with_the_design_table():
    rows = design_table()
    assert len(rows) >= 6 and {256, 272, 512, FW.WIDEST, FW.WIDEST + 16} <= {r[0] for r in rows}
    for width, ld, nbytes, fits in rows:
        for dims in ([6, width, 8], [40, width, width, width, 64], [5, 24, width, 24, 24, 24, 24, 24, 6]):
            assert FW.leading_dim(dims) == ld and FW.spill_lds_bytes(dims) == nbytes and FW.spill_fits(dims) == fits, (width, dims)
    # the figures the map is made of: 3 x 512 is 126 464 bytes; the edge is the last width whose map, with what the loss
    # sections declare on top, stays within the 160 KB of a workgroup
    assert FW.spill_lds_bytes([40, 512, 512, 512, 64]) == 3 * 33280 + 24 * 1024 + 2 * 1024 == 126464
    assert FW.spill_lds_bytes([6, FW.WIDEST, 8]) + FW.LDS_STATIC <= FE.LDS_LIMIT < FW.spill_lds_bytes([6, FW.WIDEST + 1, 8]) + FW.LDS_STATIC
    # the static part is no guess: the mixture's responsibilities and softmax [16][MAX_COMP] each, temperature and
    # log-likelihood [16] each, and the Gaussian section's row sums [16]
    assert 4 * (2 * 16 * FE.MAX_COMP + 2 * 16 + 16) <= FW.LDS_STATIC
    assert FW.spill_stash_bytes([40, 512, 512, 512, 64], 100) == 7 * 3 * 2 * 33280
