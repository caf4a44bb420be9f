"""Fits only the spill form of the training step takes (csrc/pmbrl_bnn_spill.h: pm_bnn_fwd_bwd_spill): networks behind
the LDS edge of the resident form, as a table of small synthetic fits in the manner of tests/fit_envelope_cases.py, whose
generator, oracle runs and bars these are made and judged with.

  tests/test_fit_wide_cases.py   (CPU) every case is refused by the resident form's map and taken by the spill form's,
                                 every ReLU case is clear of the kink, every case is well conditioned
  tests/test_gpu_fit_spill.py    (GPU) pmbrl_bnn_loss_grad and pmbrl_bnn_train_steps on every case against the fp64 oracle

Also the spill form's LDS map, mirrored (pm_bnn_spill_lds_floats, pmbrl_bnn_parts.h), and its edge."""
import functools

from prob_mbrl_amd import activations as ACT
from tests import act_layers as AL
from tests import fit_envelope_cases as FE
from tests.fit_envelope_cases import B, C, N, RELU, SILU, TANH, _case


def _layered_case(cid, seed, dims, M, acts, kinds):
    """A case whose hidden layers differ: `acts`, their codes.  The oracle reads such a network's activation as an entry of
    its own in its table (tests/act_layers.py::layered), the device as the packed field: problem() / for_device()."""
    case = _case(cid, seed, dims, M, RELU, kinds)
    case['acts'] = [int(c) for c in acts]
    return case


CASES = [
    _case('w272_refused', 2, [6, 272, 272, 8], 20, RELU, [B, C]),                  # the shape plan creation was pinned to refuse
    _case('w256_tanh_refused', 3, [6, 256, 256, 8], 20, TANH, [C, B]),             # ... and the other: the derivative buffer
    _case('w512x3_silu', 4, [40, 512, 512, 512, 64], 20, SILU, [C, B, C]),         # the baseline's dynamics shape
    _case('w512x3_m1', 5, [40, 512, 512, 512, 64], 1, SILU, [C, B, C]),            # ... one row
    _case('w512x3_m33_relu', 6, [40, 512, 512, 512, 64], 33, RELU, [B, N, C]),     # ... two tiles and a row, the ReLU instances
    _layered_case('per_layer_hhsinlu', 7, [6, 272, 272, 272, 8], 20, [TANH, SILU, ACT.HHSINLU], [C, N, B]),
    _case('gmm_w320', 9, [6, 320, 320, 53], 24, RELU, [B, C], n_components=4),     # a mixture head on a wide body
    _case('w688_edge', 9, [6, 688, 8], 20, TANH, [C]),                             # the widest layer the map admits
]
assert len({c['id'] for c in CASES}) == len(CASES)
GAUSSIAN = [c for c in CASES if c['n_components'] <= 1]


def all_relu(case):
    return 'acts' not in case and case['act'] == RELU


def generate(case, seed=None):
    """FE.generate; a per-layer case with `act` as the oracle reads it."""
    d = FE.generate(case, seed)
    if 'acts' in case:
        d['act'] = AL.layered(case['acts'])
    return d


def for_device(case, fit):
    """A fit of the case (problem(case), reference(case)['second']) with `act` as BnnStep takes it."""
    return dict(fit, act=ACT.pack(case['acts'])) if 'acts' in case else fit


@functools.lru_cache(maxsize=None)
def _problem(cid):
    return generate(next(c for c in CASES if c['id'] == cid))


def problem(case):
    """The case's fit, generated once and shared (leave it unchanged)."""
    return _problem(case['id'])


@functools.lru_cache(maxsize=None)
def _reference(cid):
    return FE.reference_of(_problem(cid))


def reference(case):
    """FE.reference of a case of this table (shared, leave it unchanged)."""
    return _reference(case['id'])


# ---- the spill form's LDS map, mirrored (pmbrl_bnn_parts.h, pmbrl_bnn.hip)
LDS_STATIC = 2048        # PM_BNN_LDS_STATIC: what the loss sections declare on top of the map, rounded up
WIDEST = 688             # the widest layer (input and head included) the map admits


def leading_dim(dims):
    return 16 * max(FE.tiles(w) for w in dims) + 8


def spill_lds_bytes(dims):
    """pm_bnn_spill_lds_floats * 4 of a plan: three [16][LD] buffers, the K-split scratch, the loss scratch -- whatever the
    depth, the activations and the dropout kinds."""
    return 4 * (3 * 16 * leading_dim(dims) + FE.PM_NW * FE.PM_KS_NT * 256 + FE.PM_NW * 64)


def spill_fits(dims):
    return spill_lds_bytes(dims) + LDS_STATIC <= FE.LDS_LIMIT


def spill_stash_bytes(dims, M):
    """The stashes a spill plan's workspace ends with: per workgroup and hidden layer two [16][LD] blocks."""
    return 4 * (-(-M // 16)) * (len(dims) - 2) * 2 * 16 * leading_dim(dims)
