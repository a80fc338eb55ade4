"""CPU checks of score calibration and detection costs (voicemap_amd/calibration.py, verification.py): the float64 statement of the
calibration sums against an extended-precision reference (the error the device bound of test_gpu_calibration.py is built on), the
Newton fit on score arrays, the minimum detection cost against brute force and through the zoom, the new C-ABI symbols and the
experiment script's flags."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import calib_refs as R
from voicemap_amd import _lib
from voicemap_amd import calibration as C
from voicemap_amd import verification as V

POINTS = [(0.5, 1, 1), (0.01, 1, 1), (0.001, 1, 1), (0.05, 10, 1)]
# moderate; a = 0; saturating (|z| > 750: exp underflows to 0); |z| about 40
ABT = [(-0.8, 2.5, -1.0), (0.0, 0.3, 0.7), (-0.5, 800.0, 0.0), (-2.0, 40.0, 1.5)]


def _gauss(seed, n=4000, gap=1.5, p_target=0.3):
    r = np.random.default_rng(seed)
    tg = r.random(n) < p_target
    return (r.normal(3.0, 1.0, n) - gap * tg).astype(np.float32), tg


@pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64 here")
@pytest.mark.parametrize("abt", ABT)
def test_float64_sums_lie_within_the_rounding_count_of_the_extended_reference(abt):
    s, tg = _gauss(1)
    s[::97] = np.nan
    s[5::301] = np.inf
    s[7::311] = -np.inf
    got = C.calib_sums_numpy(s, tg, *abt)
    ref, _ = R.assert_sums_close(got, s, tg, *abt, what="numpy %r" % (abt,))
    assert ref[:, 1].sum() == np.sum(~np.isfinite(s)) and ref[:, :2].sum() == len(s)
    # the single terms: the float64 statement's own error, in u = 2^-53 relative, against the counts the device bound uses
    fin, _, terms = R.terms_ref(s, tg, *abt)
    sf = s[fin].astype(np.float64)
    z = np.float64(abt[0]) * sf + np.float64(abt[1]) + np.float64(abt[2])
    t = np.where(tg[fin], -z, z)
    e = np.exp(-np.abs(t))
    d = 1.0 + e
    w = e / (d * d)
    p = np.where(t >= 0.0, 1.0 / d, e / d)
    mine = (np.maximum(t, 0.0) + np.log1p(e), p, p * sf, w, w * sf, (w * sf) * sf)
    for name, m, x in zip(R.NAMES, mine, terms):
        nz = np.abs(x) >= 2.0 ** -1000   # relative error has no meaning where float64 underflows (the saturating case: e = 0)
        rel = np.abs((m[nz].astype(np.longdouble) - x[nz]) / x[nz]).astype(np.float64) / R.U
        worst = float(rel.max()) if rel.size else 0.0
        print("term %s at %r: worst error %.2f u (count %d)" % (name, abt, worst, R.K[name] - 1))
        assert worst <= R.K[name] - 1
        assert np.all(np.abs(m[~nz]) <= 2.0 ** -999)


def test_sums_at_zero_are_counts_and_moments():
    s = np.array([1, 2, 3, 4, -2, np.nan], np.float32)
    tg = np.array([1, 1, 0, 0, 0, 1], bool)
    S = C.calib_sums_numpy(s, tg, 0.0, 0.0, 0.0)
    assert S[0].tolist()[:2] == [2, 1] and S[1].tolist()[:2] == [3, 0]
    assert S[0, 3:].tolist() == [1.0, 1.5, 0.5, 0.75, 1.25] and S[1, 3:].tolist() == [1.5, 2.5, 0.75, 1.25, 7.25]
    assert S[0, 2] == 2 * math.log1p(1.0) and C.cllr_of(S) == pytest.approx(1.0, abs=1e-15)


@pytest.mark.parametrize("seed,prior", [(0, 0.5), (1, 0.5), (2, 0.1), (3, 0.01)])
def test_fit_converges_on_overlapping_gaussians(seed, prior):
    s, tg = _gauss(10 + seed)
    cal = C.fit_calibration_numpy(s, tg, prior=prior)
    assert cal.converged and cal.iterations <= 50 and cal.stop == C.NEWTON_STOP and cal.a < 0
    # optimality at the result: the gradient, measured as the criterion measures it (its norm in the inverse Hessian: the Newton
    # decrement, which bounds the distance to the minimiser), is below the stopping constant
    Cv, g, H = C.objective_terms(C.calib_sums_numpy(s, tg, cal.a, cal.b, C.logit(prior)), prior)
    assert math.sqrt(C.newton_decrement2(g, H)) < cal.stop
    assert Cv == cal.objective and 0 < cal.cllr_train < 1
    # a minimum: nearby points are no better
    for da, db in ((1e-3, 0), (-1e-3, 0), (0, 1e-3), (0, -1e-3)):
        assert C.objective_terms(C.calib_sums_numpy(s, tg, cal.a + da, cal.b + db, C.logit(prior)), prior)[0] >= Cv
    # equal-variance Gaussians with unit variance and means 1.5 apart: llr = -1.5 s + const
    if prior == 0.5:
        assert abs(cal.a + 1.5) < 0.15
    assert np.array_equal(C.llr(cal, s[:5]), cal.a * s[:5].astype(np.float64) + cal.b)


def test_fit_on_separable_scores_does_not_converge_and_ends():
    r = np.random.default_rng(0)
    tg = r.random(500) < 0.4
    s = np.where(tg, r.uniform(0, 1, 500), r.uniform(2, 3, 500)).astype(np.float32)
    cal = C.fit_calibration_numpy(s, tg, max_iter=50)
    assert not cal.converged and cal.iterations <= 50 and cal.a < 0 and cal.cllr_train < 0.01
    with pytest.raises(ValueError):
        C.fit_calibration_numpy(s[tg], tg[tg])   # one class only


# ---- detection costs -----------------------------------------------------------------------------------------------------------------
def _brute_dcf(s, tg, point):
    """min over thresholds (distinct finite scores and +inf, accept iff s < t) of the cost as an exact rational, by plain loops."""
    pt, cm, cf = (Fraction(float(x)) for x in point)
    ok = ~np.isnan(s)
    st, sn = s[ok & tg].tolist(), s[ok & ~tg].tolist()
    best = None
    for t in sorted(set(float(v) for v in s[ok & np.isfinite(s)])) + [math.inf]:
        miss, fa = sum(1 for v in st if not v < t), sum(1 for v in sn if v < t)
        cost = (cm * pt * Fraction(miss, len(st)) + cf * (1 - pt) * Fraction(fa, len(sn))) / min(cm * pt, cf * (1 - pt))
        if best is None or cost < best[0]:
            best = (cost, t, fa / len(sn), miss / len(st))
    return best


def test_sorted_dcf_equals_a_brute_force_loop_over_thresholds():
    r = np.random.default_rng(4)
    for trial in range(4):
        n = 300
        tg = r.random(n) < (0.3, 0.05, 0.5, 0.2)[trial]
        s = (r.normal(1, 0.4, n) - 0.6 * tg).astype(np.float32)
        if trial % 2:
            s = np.round(s * 4).astype(np.float32)   # ties
        s[r.random(n) < 0.03] = np.nan
        s[r.random(n) < 0.03] = np.inf
        for pt, d in zip(POINTS, V.sorted_dcf(s, tg, POINTS)):
            cost, t, far, frr = _brute_dcf(s, tg, pt)
            assert (d["min_dcf_threshold"], d["far_at_min_dcf"], d["frr_at_min_dcf"]) == (t, far, frr), (trial, pt)
            assert d["min_dcf"] == V.dcf_value(pt, far, frr) and abs(d["min_dcf"] - float(cost)) <= 4 * 2.0 ** -53 * float(cost)
            assert d["min_dcf"] <= 1.0   # accepting nothing (or everything) costs 1 at the most


def _sweep(s, tg, lo, hi, points=POINTS):
    return V.exact_sweep(lambda wins, bins: V.bin_scores(s, tg, wins, bins), V.pass1_window(lo, hi), dcf_points=points)


def _check_dcf(s, tg, lo, hi):
    got, ref = _sweep(s, tg, lo, hi), V.sorted_dcf(s, tg, POINTS)
    assert len(got["dcf"]) == len(POINTS)
    for g, r_ in zip(got["dcf"], ref):
        assert g.keys() == r_.keys()
        for k in r_:
            assert g[k] == r_[k] or (np.isnan(g[k]) and np.isnan(r_[k])), (k, g, r_)
    sm = V.sorted_metrics(s, tg)
    for k in ("eer", "eer_threshold", "best_balanced_accuracy", "best_threshold"):   # the other metrics are untouched
        assert got[k] == sm[k] or (np.isnan(got[k]) and np.isnan(sm[k]))
    return got


@pytest.mark.parametrize("seed", range(5))
def test_sweep_dcf_equals_sort_on_random_scores(seed):
    r = np.random.default_rng(seed)
    n = int(r.integers(200, 20000))
    tg = r.random(n) < r.uniform(0.02, 0.5)
    s = (r.normal(1.0, 0.3, n) - 0.5 * tg).astype(np.float32)
    got = _check_dcf(s, tg, 0.0, 3.0)
    # the (0.5, 1, 1) point is the balanced accuracy: same threshold, same rates, cost = FAR + FRR = 2 (1 - accuracy) -- up to the
    # one rounding of 1 - (FAR + FRR) / 2 in best_balanced_accuracy itself (at most 2^-54 there, 2^-53 after the doubling)
    d = got["dcf"][0]
    assert d["min_dcf_threshold"] == got["best_threshold"]
    assert (d["far_at_min_dcf"], d["frr_at_min_dcf"]) == (got["far_at_best"], got["frr_at_best"])
    assert d["min_dcf"] == got["far_at_best"] + got["frr_at_best"]
    assert abs(d["min_dcf"] - 2 * (1 - got["best_balanced_accuracy"])) <= 2.0 ** -53


def test_sweep_dcf_on_a_lattice_with_infinities_and_an_empty_class():
    r = np.random.default_rng(21)
    for trial in range(4):
        n = 3000
        tg = r.random(n) < 0.3
        s = (r.integers(0, 12, n) - 3 * tg).astype(np.float32)   # a dozen distinct values: many ties
        if trial >= 2:
            s[r.random(n) < 0.05] = np.inf
            s[r.random(n) < 0.02] = np.nan
        _check_dcf(s, tg, -5.0, 12.0)
    _check_dcf(np.full(10, np.inf, np.float32), np.arange(10) % 2 == 0, 0.0, 1.0)
    got = _sweep(np.ones(5, np.float32), np.ones(5, bool), 0.0, 2.0)
    assert len(got["dcf"]) == 4 and all(np.isnan(d["min_dcf"]) and d["p_target"] == p[0] for d, p in zip(got["dcf"], POINTS))
    assert all(np.isnan(d["min_dcf"]) for d in V.sorted_dcf(np.ones(5, np.float32), np.ones(5, bool), POINTS))


def test_without_points_the_sweep_is_what_it_was():
    r = np.random.default_rng(8)
    tg = r.random(6000) < 0.2
    s = (r.normal(1.0, 0.3, 6000) - 0.5 * tg).astype(np.float32)
    calls = []

    def hist(wins, bins):
        calls.append((tuple(wins), bins))
        return V.bin_scores(s, tg, wins, bins)
    old = V.exact_sweep(hist, V.pass1_window(0.0, 3.0))   # the old call signature
    old_calls, calls = calls, []
    new = V.exact_sweep(hist, V.pass1_window(0.0, 3.0), dcf_points=())
    assert list(old) == list(new) and "dcf" not in new and old["passes"] == new["passes"] and calls == old_calls
    for k in old:
        if k != "roc":
            assert old[k] == new[k]
    with_pts = V.exact_sweep(hist, V.pass1_window(0.0, 3.0), dcf_points=[0.01])   # a bare P is (P, 1, 1)
    assert list(with_pts) == list(old) + ["dcf"] and with_pts["dcf"][0]["c_miss"] == 1.0
    for bad in ([(0.0, 1, 1)], [(1.0, 1, 1)], [(0.5, 0, 1)], [(0.5, 1)]):
        with pytest.raises(ValueError):
            V.exact_sweep(hist, V.pass1_window(0.0, 3.0), dcf_points=bad)


def test_bayes_threshold_and_its_refusal():
    cal = C.Calibration(-2.0, 3.0, 0.5, "euclidean", False, 3, True, 0.4, 0.6)
    t = V.bayes_threshold(cal, (0.01, 1, 1))
    assert t == float(np.float32(t)) and abs(t - (math.log(99.0) - 3.0) / -2.0) < 1e-6   # an fp32 value: it is compared with fp32 scores
    assert V.bayes_threshold(cal, (0.5, 1, 1)) == 1.5
    assert V.bayes_threshold(cal, (0.5, 10, 1)) > 1.5   # misses cost more: accept more
    for a in (0.0, 1.0):
        with pytest.raises(ValueError, match="not negative"):
            V.bayes_threshold(C.Calibration(a, 0.0, 0.5, "euclidean", False, 0, False, 0.7, 1.0), (0.5, 1, 1))


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_exported_and_check_their_arguments():
    names = ("vm_pair_calib_sums", "vm_pair_calib_sums_workspace_bytes", "vm_pair_calib_sums_splits")
    declared = _lib.header_functions()
    lib = _lib.lib()
    for n in names:
        assert n in declared and n in _lib.SIGNATURES and hasattr(lib.cdll, n)
    P, I, L, D = _lib.P, _lib.I, _lib.L, _lib.D
    assert _lib.SIGNATURES["vm_pair_calib_sums"] == (I, [P, P, L, I, I, P, L, L, P, P, D, D, D, P, P, P])
    assert "vm_pair_calib_sums" in _lib.program_table()[0]
    assert lib.query("vm_pair_calib_sums_workspace_bytes", 104014, 64) >= lib.query("vm_pair_score_hist_workspace_bytes", 104014, 64) + 16 * 8 * 4096
    assert lib.query("vm_pair_calib_sums_splits", 8192, 8192) == 32 and lib.query("vm_pair_calib_sums_splits", 64, 300) == 3
    ok = (16, 16, 10, 64, 0, None, 0, 10, None, None, 0.0, 0.0, 0.0, 16, 16, None)
    for k, v, msg in ((0, None, "null pointer"), (13, None, "null pointer"), (14, None, "null pointer"), (8, 16, "mu and rsig"),
                      (9, 16, "mu and rsig"), (3, 257, "bad sizes"), (4, 5, "unknown score_kind"), (4, 3, "needs weights"),
                      (7, 11, "bad row range"), (6, 11, "bad row range"), (0, 8, "16-byte aligned"), (13, 20, "8-byte"),
                      (10, math.inf, "finite"), (12, math.nan, "finite")):
        args = list(ok)
        args[k] = v
        with pytest.raises(_lib.VoicemapHipError, match=msg):
            lib.call("vm_pair_calib_sums", *args)


def test_script_flags_parse():
    import importlib
    ex = importlib.import_module("experiments.verification_accuracy")
    a = ex.parse_args(["--synthetic", "--dcf", "0.01", "--dcf", "0.05,10,1", "--calibrate", "--calib-prior", "0.1"])
    assert a.dcf == [(0.01, 1.0, 1.0), (0.05, 10.0, 1.0)] and a.calibrate and a.calib_prior == 0.1
    a = ex.parse_args(["--synthetic"])
    assert a.dcf == [] and not a.calibrate
