"""The per-tensor bar of the parameter-gradient tests: common.rel < 2e-5 -- the input-gradient bar of the stand-alone
network kernels -- for EVERY tensor on its own, so that a thin layer cannot hide behind a wide one.  A tensor whose
fp64 norm is below 1e-12 of the largest tensor's has no scale of its own (it is zero up to rounding): its error is
measured against the largest norm instead."""
import numpy as np

from tests import common

BAR = 2e-5


def errors(got, ref, labels=None):
    """[(label, error)] of the tensors `got` against their fp64 expectations `ref` (sequences of arrays)."""
    got = [np.asarray(g, np.float64) for g in got]
    ref = [np.asarray(r, np.float64) for r in ref]
    assert len(got) == len(ref) and all(g.shape == r.shape for g, r in zip(got, ref))
    labels = labels or ['%s%d' % ('Wb'[i % 2], i // 2) for i in range(len(ref))]
    big = max(float(np.linalg.norm(r)) for r in ref)
    out = []
    for label, g, r in zip(labels, got, ref):
        if float(np.linalg.norm(r)) < 1e-12 * big:
            out.append((label + ' (abs)', float(np.linalg.norm(g - r)) / max(big, 1e-300)))
        else:
            out.append((label, common.rel(g, r)))
    return out


def hold(what, errs, bar=BAR):
    """Print every figure, then hold each to the bar."""
    print('%s: %s' % (what, ', '.join('%s %.2e' % e for e in errs)))
    for label, e in errs:
        assert e < bar, (what, label, e)
