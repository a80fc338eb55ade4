"""CPU checks of cohort score normalisation (voicemap_amd/verification.py): the numpy twins of vm_cohort_topk_stats' selection and
statistics and of vm_pair_score_hist_norm's normalised score, against brute force; the new C-ABI symbols; the experiment script's flags."""
import math
import os
import sys

import numpy as np
import pytest

from voicemap_amd import _lib
from voicemap_amd import verification as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute_select(row, K, skip=None):
    """Sorted (key, index) list of the non-NaN, non-skipped entries of a row, cut at K: plain Python."""
    keys = V.score_keys(row)
    cand = sorted((int(keys[c]), c) for c in range(len(row)) if not np.isnan(row[c]) and c != skip)
    return [c for _, c in cand[:K]]


def _check_selection(s, K, self_row0=None):
    idx, cnt = V.cohort_select_numpy(s, K, self_row0)
    for m in range(len(s)):
        skip = self_row0 + m if self_row0 is not None else None
        ref = _brute_select(s[m], K, skip)
        assert cnt[m] == len(ref)
        assert list(idx[m, :cnt[m]]) == ref
        assert (idx[m, cnt[m]:] == -1).all()
    return idx, cnt


@pytest.mark.parametrize("seed", range(4))
def test_selection_with_heavy_ties_on_an_integer_lattice(seed):
    r = np.random.default_rng(seed)
    s = r.integers(-3, 4, (20, 300)).astype(np.float32)   # 7 distinct values: the K-th key is tied almost always
    for K in (1, 2, 7, 50, 299, 300, 301, 1000):
        idx, cnt = _check_selection(s, K)
        assert (cnt == min(K, 300)).all()
    _check_selection(np.sqrt(r.integers(0, 9, (10, 200))).astype(np.float32), 40)


def test_selection_with_signed_zeros_nan_and_infinities():
    r = np.random.default_rng(7)
    s = r.normal(0, 1, (30, 120)).astype(np.float32)
    for v, frac in ((-0.0, 0.1), (0.0, 0.1), (np.nan, 0.2), (np.inf, 0.05), (-np.inf, 0.05)):
        s[r.random(s.shape) < frac] = v
    s[3] = np.nan   # a row without scores
    for K in (1, 10, 60, 120, 500):
        idx, cnt = _check_selection(s, K)
        assert cnt[3] == 0 and (idx[3] == -1).all()
    # -0.0 and +0.0 are one key: the lower index comes first
    idx, _ = V.cohort_select_numpy(np.array([[0.0, -0.0, -1.0, 0.0]], np.float32), 3)
    assert list(idx[0]) == [2, 0, 1]


def test_selection_with_self_exclusion():
    r = np.random.default_rng(1)
    s = r.normal(0, 1, (40, 100)).astype(np.float32)
    for row0 in (0, 30, 80):
        for K in (1, 5, 100):
            idx, cnt = _check_selection(s, K, self_row0=row0)
            for m in range(40):
                if row0 + m < 100:
                    assert row0 + m not in idx[m] and cnt[m] == min(K, 99)


def test_statistics_against_fsum():
    r = np.random.default_rng(3)
    s = (r.normal(5, 2, (50, 400)) * 10.0 ** r.integers(-3, 4, (50, 1))).astype(np.float32)
    s[7, :] = 2.5   # sigma = 0: rsig = +inf
    for K in (1, 2, 17, 400):
        st = V.cohort_stats_numpy(s, K)
        for m in range(len(s)):
            v = [float(x) for x in s[m, st["topk_idx"][m, :K]]]
            mean = math.fsum(v) / len(v)
            sd = math.sqrt(math.fsum((x - mean) ** 2 for x in v) / len(v))
            assert abs(float(st["mu"][m]) - mean) <= np.spacing(np.float32(abs(mean)))
            assert abs(float(st["sigma"][m]) - sd) <= np.spacing(np.float32(sd)) + 1e-300
            assert st["rsig"][m] == np.float32(1.0 / np.float64(st["sigma"][m])) if st["sigma"][m] else np.isposinf(st["rsig"][m])
        assert np.isposinf(st["rsig"][7]) and st["sigma"][7] == 0 and st["mu"][7] == np.float32(2.5)
    st = V.cohort_stats_numpy(np.full((2, 5), np.nan, np.float32), 3)
    assert np.isnan(st["mu"]).all() and np.isnan(st["sigma"]).all() and np.isnan(st["rsig"]).all() and (st["count"] == 0).all()


def test_normalised_score_twin_is_elementwise_fp32():
    r = np.random.default_rng(5)
    n = 2000
    s = r.normal(10, 3, n).astype(np.float32)
    mu = r.normal(10, 1, 50).astype(np.float32)
    rsig = (1.0 / r.uniform(0.5, 4, 50)).astype(np.float32)
    mu[3], rsig[4] = np.nan, np.inf
    i, j = r.integers(0, 50, n), r.integers(0, 50, n)
    got = V.normalise_scores_numpy(s, i, j, mu, rsig)
    f = np.float32
    for k in range(n):
        a = f(s[k] - mu[i[k]])
        b = f(s[k] - mu[j[k]])
        with np.errstate(invalid="ignore"):
            ref = f(f(0.5) * f(f(a * rsig[i[k]]) + f(b * rsig[j[k]])))
        assert got[k].view(np.uint32) == ref.view(np.uint32) or (np.isnan(got[k]) and np.isnan(ref))
    assert got.dtype == np.float32


def test_new_entry_points_are_declared_bound_and_exported():
    names = ("vm_cohort_topk_stats", "vm_cohort_stats_workspace_bytes", "vm_pair_score_hist_norm")
    for n in names:
        assert n in _lib.header_functions() and n in _lib.SIGNATURES
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib.cdll, n)
    assert lib.query("vm_cohort_stats_workspace_bytes", 104014, 20000, 64) >= 20000 * 64 * 4
    assert lib.query("vm_cohort_stats_workspace_bytes", 104014, 20000, 64) < 400 << 20
    win = np.array([0, 20], np.int64)
    with pytest.raises(_lib.VoicemapHipError, match="null pointer"):
        lib.call("vm_cohort_topk_stats", None, 10, None, 10, 64, 0, None, -1, 5, None, None, None, None, None, None, None)
    with pytest.raises(_lib.VoicemapHipError, match="K must be"):
        lib.call("vm_cohort_topk_stats", 16, 10, 16, 10, 64, 0, None, -1, 0, 16, 16, 16, 16, None, 16, None)
    with pytest.raises(_lib.VoicemapHipError, match="null pointer"):
        lib.call("vm_pair_score_hist_norm", 16, 16, 10, 64, 0, None, 0, 10, win.ctypes.data, 1, 4096, None, None, 16, 16, None)


def test_experiment_script_flags_and_file_names():
    sys.path.insert(0, ROOT)
    from experiments import verification_accuracy as ex
    a = ex.parse_args([])
    assert (a.score_norm, a.cohort_set, a.cohort_size, a.top_k) == ("none", "train-clean-100", 5000, 300)
    assert ex.result_name(a) == "verification_accuracy_dev-clean_test-clean_euclidean.csv"
    assert ex.result_name(ex.parse_args(["--synthetic"])) == "verification_accuracy_synthetic_synthetic_euclidean.csv"
    a = ex.parse_args(["--synthetic", "--score-norm", "as-norm", "--top-k", "50"])
    assert ex.result_name(a) == "verification_accuracy_synthetic_synthetic_euclidean_asnorm_k50_c5000.csv"
    a = ex.parse_args(["--score-norm", "s-norm", "--score", "cosine", "--cohort-size", "100"])
    assert ex.result_name(a) == "verification_accuracy_dev-clean_test-clean_cosine_snorm_c100.csv"
    with pytest.raises(SystemExit):
        ex.parse_args(["--score-norm", "z-norm"])

    class _DS:
        fragment_length, pad = 10, False
        _code = np.arange(50) % 7

        def __len__(self):
            return 50

        def _load(self, i):
            return np.full(12, i)

    sub = ex.cohort_subset(_DS(), 20)
    assert len(sub) == 20 and np.all(np.diff(sub.index) > 0) and sub._load(3)[0] == sub.index[3]
    assert np.array_equal(sub._code, _DS._code[sub.index]) and np.array_equal(ex.cohort_subset(_DS(), 20).index, sub.index)
    assert len(ex.cohort_subset(_DS(), 500)) == 50
