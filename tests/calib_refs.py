"""References and error bounds for the calibration sums (vm_pair_calib_sums, voicemap_amd/calibration.py), shared by
test_calibration_cpu.py and test_gpu_calibration.py.

``sums_ref`` evaluates the per-trial statement of include/voicemap_hip.h with z and t in float64 exactly as stated (products and sums
of doubles are correctly rounded on the host and, with contraction off, on the device: the same bits) and everything after t -- exp,
1 + e, log1p, the divisions, the products with s -- in ``np.longdouble`` (x87 extended, 64 significand bits), summed with ``math.fsum``
over exact splits of the extended values.  What a float64 evaluation may differ by is then a count of roundings after t, in units of
u = 2^-53 relative to the term (every term is positive, or has the sign of s):

    e = exp(-|t|)                       X   (the library's exp, in ulp: |error| <= X ulp <= 2 X u relative; counted as 2 X)
    d = 1 + e                           1
    loss = max(t, 0) + log1p(e)         e's error enters log1p with a factor <= 1; log1p itself Y ulp -> 2 Y; the sum 1
    p = 1 / d  or  e / d                e's error, d's, the division: 2 X + 1 + 1
    w = e / (d d)                       e's error with factor |1 - 2 e / d| <= 1; d twice, the product, the division: 2 X + 4
    p s, w s, (w s) s                   one rounding per product

X = Y = 1: no accuracy table of the device math library is on the build machine, so -- as an ASSUMPTION -- the device's float64
exp / log1p are taken to be as good as the host's, whose measured term errors test_calibration_cpu.py holds to these same counts.
A sum of n such terms accumulated in float64 in any order adds at most (n - 1) u (1 + O(n u)) sum|term|; the bound used is
(n + K) u sum|term| with K the count above plus 1 for the second-order terms.
"""
import math

import numpy as np

U = 2.0 ** -53
EXP_ULP, LOG1P_ULP = 1, 1
_X, _Y = 2 * EXP_ULP, 2 * LOG1P_ULP
# K per sum, in the order L, P0, P1, W0, W1, W2 (+ 1: second-order terms)
K = {"L": _X + _Y + 1 + 1, "P0": _X + 2 + 1, "P1": _X + 3 + 1, "W0": _X + 4 + 1, "W1": _X + 5 + 1, "W2": _X + 6 + 1}
NAMES = ("L", "P0", "P1", "W0", "W1", "W2")


def have_extended() -> bool:
    return np.finfo(np.longdouble).eps <= 2.0 ** -63


def terms_ref(scores, target, a, b, tau):
    """(finite mask, target mask, six (n,) longdouble term arrays L, P0, P1, W0, W1, W2 of the finite trials)."""
    s32 = np.asarray(scores, dtype=np.float32).ravel()
    tg = np.asarray(target, dtype=bool).ravel()
    fin = np.isfinite(s32)
    s = s32[fin].astype(np.float64)
    z = np.float64(a) * s + np.float64(b) + np.float64(tau)   # float64, as stated
    t = np.where(tg[fin], -z, z)
    tl, sl = t.astype(np.longdouble), s.astype(np.longdouble)
    e = np.exp(-np.abs(tl))
    d = 1 + e
    p = np.where(tl >= 0, 1 / d, e / d)
    w = e / (d * d)
    loss = np.maximum(tl, 0) + np.log1p(e)
    return fin, tg, (loss, p, p * sl, w, w * sl, w * sl * sl)


def _fsum_ld(x) -> float:
    """Sum of longdouble values, correctly rounded to float64: each value is split exactly into two doubles."""
    x = np.asarray(x, dtype=np.longdouble)
    hi = x.astype(np.float64)
    lo = (x - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


def sums_ref(scores, target, a, b, tau):
    """((2, 8) float64 reference sums, (2, 8) float64 bounds on |float64 evaluation - reference|; 0 for the two counts)."""
    fin, tg, terms = terms_ref(scores, target, a, b, tau)
    ref, bound = np.zeros((2, 8)), np.zeros((2, 8))
    for c, cls in enumerate((tg, ~tg)):
        sel = cls[fin]
        n = int(sel.sum())
        ref[c, 0], ref[c, 1] = n, int((cls & ~fin).sum())
        for k, name in enumerate(NAMES):
            v = terms[k][sel]
            ref[c, 2 + k] = _fsum_ld(v)
            bound[c, 2 + k] = (n + K[name]) * U * _fsum_ld(np.abs(v))
    return ref, bound


def assert_sums_close(got, scores, target, a, b, tau, what=""):
    """Counts exact, the six sums within ``sums_ref``'s bound; prints the worst ratio error / bound before it asserts."""
    got = np.asarray(got, dtype=np.float64)
    ref, bound = sums_ref(scores, target, a, b, tau)
    assert np.array_equal(got[:, :2], ref[:, :2]), (what, got[:, :2], ref[:, :2])
    err = np.abs(got[:, 2:] - ref[:, 2:])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound[:, 2:], 0.0)
    print("calib sums %s: worst error / bound = %.3g" % (what, float(ratio.max()) if ratio.size else 0.0))
    assert np.all(err <= bound[:, 2:]), (what, got, ref, bound)
    return ref, bound
