"""CPU checks of the all-pairs verification host logic (voicemap_amd/verification.py): the zoom over integer-key histograms -- fed by
``bin_scores``, numpy's bit-for-bit twin of vm_pair_score_hist -- gives exactly what a full sort of the fp32 scores gives; row shards
of the triangle; the AUC bound; the new C-ABI symbols."""
import numpy as np
import pytest

from voicemap_amd import _lib
from voicemap_amd import verification as V

EXACT = ("eer", "eer_threshold", "far_at_eer", "frr_at_eer", "best_balanced_accuracy", "best_threshold", "far_at_best", "frr_at_best",
         "n_target", "n_nontarget", "n_nan")


def _sweep(s, tg, lo, hi):
    return V.exact_sweep(lambda wins, bins: V.bin_scores(s, tg, wins, bins), V.pass1_window(lo, hi))


def _check(s, tg, lo, hi):
    got, ref = _sweep(s, tg, lo, hi), V.sorted_metrics(s, tg)
    for k in EXACT:
        assert got[k] == ref[k] or (np.isnan(got[k]) and np.isnan(ref[k])), (k, got[k], ref[k])
    return got


def _informative(r, n, p_target=0.2):
    tg = r.random(n) < p_target
    s = (r.normal(1.0, 0.3, n) - 0.5 * tg).astype(np.float32)
    return s, tg


@pytest.mark.parametrize("seed", range(6))
def test_sweep_equals_sort_on_random_scores(seed):
    r = np.random.default_rng(seed)
    s, tg = _informative(r, int(r.integers(50, 20000)), r.uniform(0.02, 0.5))
    got = _check(s, tg, 0.0, 3.0)
    assert got["passes"] >= 2   # pass-1 bins hold several keys: the result needed a zoom


def test_sweep_converges_on_uninformative_scores():
    """Scores that do not separate the classes: many bins could hold the best threshold; the zoom still ends, exact, in a few passes."""
    r = np.random.default_rng(11)
    for _ in range(3):
        n = 5000
        s = (np.exp(r.normal(0, 10, n)) * np.sign(r.normal(size=n))).astype(np.float32)
        got = _check(s, r.random(n) < 0.3, -1.0, 1.0)
        assert got["passes"] <= 12


@pytest.mark.parametrize("seed", range(4))
def test_sweep_equals_sort_with_heavy_ties(seed):
    r = np.random.default_rng(100 + seed)
    n = int(r.integers(100, 5000))
    tg = r.random(n) < 0.3
    s = (r.integers(0, 12, n) - 3 * tg).astype(np.float32)            # a dozen distinct values
    _check(s, tg, -5.0, 12.0)
    _check(np.sqrt(r.integers(0, 40, n)).astype(np.float32), tg, 0.0, 8.0)   # sqrt of integers: euclidean on a lattice


def test_sweep_equals_sort_with_signed_zero_nan_and_infinities():
    r = np.random.default_rng(7)
    for trial in range(8):
        n = 3000
        s, tg = _informative(r, n, 0.3)
        s -= 1.0
        for v, frac in ((-0.0, 0.1), (0.0, 0.05), (np.nan, 0.03), (np.inf, 0.02 * (trial % 2)), (-np.inf, 0.02 * (trial % 3 == 0))):
            s[r.random(n) < frac] = v
        got = _check(s, tg, -1.0, 1.0)   # the infinities and part of the scores fall under / over the pass-1 window
        assert got["n_nan"] == int(np.isnan(s).sum())
    # -0.0 and +0.0 are one threshold
    s = np.array([-0.0, 0.0, 1.0, 1.0, -0.0, 2.0], np.float32)
    tg = np.array([1, 0, 1, 0, 0, 0], bool)
    _check(s, tg, 0.0, 4.0)
    # every score +inf (the only threshold is +inf), and a set with one class only
    _check(np.full(10, np.inf, np.float32), np.arange(10) % 2 == 0, 0.0, 1.0)
    got = _sweep(np.ones(5, np.float32), np.ones(5, bool), 0.0, 2.0)
    assert np.isnan(got["eer"]) and got["n_nontarget"] == 0


def test_bin_scores_window_slots():
    s = np.array([-1.0, -0.0, 0.0, 0.5, 1.0, np.inf, np.nan], np.float32)
    tg = np.array([1, 1, 0, 0, 1, 0, 1], bool)
    k0 = V.key_of(0.0)
    h = V.bin_scores(s, tg, [(k0, 23)], 256)[0]   # 2^23 keys per bin: one binade per bin from +0.0
    assert V.key_of(-0.0) == k0 and V.key_of(-1.0) < k0 < V.key_of(0.5) < V.key_of(1.0) < V.KEY_POS_INF
    assert h[0, 256] == 1 and h[0, 258] == 1          # target -1.0 under, target NaN in the NaN slot
    assert h[0, 0] == 1 and h[1, 0] == 1              # -0.0 and +0.0 share bin 0
    assert h[1, 256 + 1] == 0 and h.sum() == 7
    assert V.key_value(V.key_of(0.75)) == 0.75 and V.key_value(V.KEY_POS_INF) == np.inf


def test_auc_bound_holds():
    r = np.random.default_rng(3)
    for _ in range(5):
        s, tg = _informative(r, 4000, 0.25)
        s = np.round(s * 50) / 50   # ties too
        got = _sweep(s.astype(np.float32), tg, 0.0, 3.0)
        st, sn = np.sort(s[tg]), s[~tg]
        below = np.searchsorted(st, sn, side="left")
        ties = np.searchsorted(st, sn, side="right") - below
        true = (below.sum() + 0.5 * ties.sum()) / (len(st) * len(sn))
        assert abs(got["auc"] - true) <= got["auc_bound"] + 1e-12
        assert got["auc_bound"] < 0.01
        roc = got["roc"]
        assert np.all(np.diff(roc["far"]) >= 0) and np.all(np.diff(roc["frr"]) <= 0) and len(roc["threshold"]) > 100


@pytest.mark.parametrize("N", [1, 2, 3, 10, 63, 64, 65, 1000, 4099, 104014])
def test_triangle_shards_cover_every_pair_once_and_balance(N):
    total = N * (N - 1) // 2
    for world in range(1, 9):
        sh = V.triangle_shards(N, world)
        assert len(sh) == world and sh[0][0] == 0 and sh[-1][1] == N
        assert all(a[1] == b[0] for a, b in zip(sh[:-1], sh[1:])) and all(lo <= hi for lo, hi in sh)
        counts = [V.pairs_before(hi, N) - V.pairs_before(lo, N) for lo, hi in sh]
        assert sum(counts) == total
        assert max(counts) - min(counts) <= N, (world, counts)
        if N < 100:   # brute force: every pair {i < j} in exactly one shard
            owner = np.full((N, N), -1)
            for k, (lo, hi) in enumerate(sh):
                for i in range(lo, hi):
                    owner[i, i + 1:] = k
            assert (owner[np.triu_indices(N, 1)] >= 0).all()


def test_new_entry_points_are_declared_bound_and_exported():
    names = ("vm_pair_score_hist", "vm_pair_score_hist_workspace_bytes")
    for n in names:
        assert n in _lib.header_functions() and n in _lib.SIGNATURES
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib.cdll, n)
    assert lib.query("vm_pair_score_hist_workspace_bytes", 104014, 64) >= 104014 * 64 * 4
    # argument errors are reported without a GPU
    win = np.array([0, 20], np.int64)
    with pytest.raises(_lib.VoicemapHipError, match="null pointer"):
        lib.call("vm_pair_score_hist", None, None, 10, 64, 0, None, 0, 10, win.ctypes.data, 1, 4096, None, None, None)
    with pytest.raises(_lib.VoicemapHipError, match="LDS"):
        lib.call("vm_pair_score_hist", 16, 16, 10, 64, 0, None, 0, 10, win.ctypes.data, 1, 8192, 16, 16, None)
