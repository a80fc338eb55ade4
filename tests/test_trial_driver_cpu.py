"""The host driver the trial evaluators share (voicemap_amd/verification.py: ``place_window``, ``sample_scores``, ``counts_at_threshold``,
``triangle_sum``; ``parallel.sum_ranks``), on CPU tensors.  The pass-1 windows below were recorded from the per-evaluator code this
driver replaced (torch 2.10, numpy 2.2): the windows decide every later pass, so the refactor had to leave them bit for bit.  The
two-rank checks of the same pieces run in the gloo worker of tests/test_parallel_cpu.py."""
import numpy as np
import pytest
import torch

from voicemap_amd import enrolment as EN
from voicemap_amd import verification as V
from voicemap_amd.retrieval import EmbeddingCache

NEG_EUCLIDEAN = V.VM_SCORE_NEG_EUCLIDEAN


def _inputs():
    g = torch.Generator().manual_seed(1)
    emb = torch.randn(300, 16, generator=g)
    w = torch.rand(16, generator=g)
    mu = torch.randn(300, generator=g).float() * 0.1 + 5.0
    rsig = (torch.rand(300, generator=g) + 0.5).float()
    return emb, w, mu, rsig, np.repeat(np.arange(30), 10)


@pytest.mark.parametrize("score, window", [("euclidean", (3220791296, 13)), ("cosine", (3188490240, 13)),
                                           ("dot_product", (1046478848, 20)), (NEG_EUCLIDEAN, (1054973952, 13))])
def test_pair_windows_are_the_recorded_ones(score, window):
    emb, _, _, _, spk = _inputs()
    cache = EmbeddingCache(emb, spk)
    kind = V.SCORES.get(score, score)
    lo, hi = V.bounds(cache, kind)
    assert V.sampled_window(cache, kind, None, lo, hi) == window


def test_weighted_l1_and_normalised_pair_windows_are_the_recorded_ones():
    emb, w, mu, rsig, spk = _inputs()
    cache = EmbeddingCache(emb, spk)
    assert V.sampled_window(cache, V.SCORES["weighted_l1"], w, -50.0, 50.0) == (3226763264, 13)
    norm = V.ScoreNorm(mu, 1 / rsig, rsig, torch.full((300,), 300, dtype=torch.int32), "euclidean", None, 300)
    lo, hi = V.norm_bounds(norm, *V.bounds(cache, V.SCORES["euclidean"]))
    assert V.sampled_window(cache, V.SCORES["euclidean"], None, lo, hi, norm=norm) == (1067450368, 20)


def test_pair_windows_of_degenerate_caches_are_the_recorded_ones():
    emb, _, _, _, spk = _inputs()
    euc = V.SCORES["euclidean"]
    # fewer than two rows: no pair, the bounds' window; two rows: one score, 65 536 times
    for rows, window in ((0, (2147483648, 16)), (1, (2147483648, 19)), (2, (3232216681, 0))):
        cache = EmbeddingCache(emb[:rows], spk[:rows])
        lo, hi = V.bounds(cache, euc)
        assert V.sampled_window(cache, euc, None, lo, hi) == window
    ones = EmbeddingCache(torch.ones(50, 16), np.zeros(50, dtype=np.int64))   # every score 0
    lo, hi = V.bounds(ones, euc)
    assert V.sampled_window(ones, euc, None, lo, hi) == (2147483648, 16)
    nans = EmbeddingCache(torch.full((300, 16), float("nan")), spk)           # no finite score in the sample
    assert V.sampled_window(nans, euc, None, 0.0, 10.0) == (2147483648, 19) == V.pass1_window(0.0, 10.0)


@pytest.mark.parametrize("distance, window", [("euclidean", (3219292160, 12)), ("cosine", (3185688576, 14)),
                                              ("dot_product", (1038090240, 20))])
def test_model_trial_windows_are_the_recorded_ones(distance, window):
    emb, _, _, _, spk = _inputs()
    label = torch.as_tensor(spk)
    sums = torch.zeros(30, 16, dtype=torch.float64).index_add_(0, label, emb.double())
    msum = torch.zeros(30, dtype=torch.float64).index_add_(0, label, torch.linalg.vector_norm(emb.double(), dim=1))
    count = torch.full((30,), 10, dtype=torch.int32)
    models = EN.SpeakerModels(sums, msum, count, distance, np.arange(30), spk.astype(np.int32), EmbeddingCache(emb, spk), None)
    assert EN._pass1(models, emb) == window


def test_place_window_runs_the_sample_once_and_applies_the_100_score_rule():
    calls = []
    ramp = lambda n: torch.linspace(1.0, 2.0, n, dtype=torch.float64)

    def sample(n):
        calls.append(n)
        return 0.0, 8.0, ramp(n)
    assert V.place_window(lambda: sample(100)) == V.pass1_window(0.0, 8.0)          # 100 finite scores are not enough
    got = V.place_window(lambda: sample(101))
    q0, q1 = np.quantile(ramp(101).numpy(), [1e-4, 1 - 1e-4])
    pad = 0.05 * (q1 - q0) + 1e-6 * q1 + 1e-30
    assert got == V.pass1_window(float(q0 - pad), float(q1 + pad)) != V.pass1_window(0.0, 8.0)
    assert calls == [100, 101]
    many = torch.cat([ramp(101), torch.full((50,), np.inf, dtype=torch.float64), torch.full((50,), np.nan, dtype=torch.float64)])
    assert V.place_window(lambda: (0.0, 8.0, many)) == got                           # only the finite scores count
    assert V.place_window(lambda: (1.5, 1.6, ramp(101))) == V.pass1_window(1.5, 1.6)   # clipped to the bounds
    assert V.place_window(lambda: (0.0, 8.0, None)) == V.pass1_window(0.0, 8.0)


def test_sample_scores_are_the_float64_definitions():
    g = torch.Generator().manual_seed(3)
    a, b, w = torch.randn(40, 8, generator=g), torch.randn(40, 8, generator=g), torch.rand(8, generator=g)
    A, B, W = a.double().numpy(), b.double().numpy(), w.double().numpy()
    d = np.sqrt(((A - B) ** 2).sum(1))
    want = {V.SCORES["euclidean"]: d, NEG_EUCLIDEAN: -d, V.SCORES["dot_product"]: -(A * B).sum(1),
            V.SCORES["cosine"]: 1 - (A * B).sum(1) / (np.linalg.norm(A, axis=1) * np.linalg.norm(B, axis=1)),
            V.SCORES["weighted_l1"]: (np.abs(A - B) * W).sum(1)}
    for kind, ref in want.items():
        got = V.sample_scores(a, b, kind, w)
        assert got.dtype == torch.float64
        np.testing.assert_allclose(got.numpy(), ref, rtol=1e-13, atol=1e-13)   # float64 sums of 8 terms in another order


def test_counts_at_threshold_equal_the_direct_counts():
    rng = np.random.default_rng(5)
    s = rng.standard_normal(1000).astype(np.float32)
    s[::97] = np.nan
    tg = rng.random(1000) < 0.3
    ok = ~np.isnan(s)
    nT, nN = int((ok & tg).sum()), int((ok & ~tg).sum())
    hist_fn = lambda w, b: V.bin_scores(s, tg, w, b)
    for t in (0.25, float(s[501]), np.inf, -np.inf):
        got = V.counts_at_threshold(hist_fn, t)
        with np.errstate(invalid="ignore"):
            below = s < np.float32(t)
        far, frr = int((ok & ~tg & below).sum()) / nN, int((ok & tg & ~below).sum()) / nT
        assert (got["far"], got["frr"], got["n_target"], got["n_nontarget"]) == (far, frr, nT, nN)
        assert got["balanced_accuracy"] == 1.0 - (far + frr) / 2
        assert got["n_nan"] == int((~ok).sum()) == 11
    assert 0 < V.counts_at_threshold(hist_fn, float(s[501]))["far"] < 1
    got = V.counts_at_threshold(hist_fn, float("nan"))   # the recorded answer: key 2^32 - 1, every number below it
    assert (got["far"], got["frr"], got["n_target"], got["n_nontarget"], got["n_nan"]) == (1.0, 0.0, nT, nN, 11)


def test_window_limits_are_one_check():
    V.check_windows([(0, 20)] * V.MAX_WINDOWS, 1024)
    V.check_windows([(0, 20)], V.PASS1_BINS)
    for wins, bins in (([(0, 20)] * (V.MAX_WINDOWS + 1), 16), ([(0, 20)] * 2, V.PASS1_BINS)):
        with pytest.raises(ValueError, match="windows and"):
            V.check_windows(wins, bins)
        with pytest.raises(ValueError, match="windows and"):   # both histogram wrappers refuse before they touch the device
            V.histogram(None, 0, None, wins, bins)
        with pytest.raises(ValueError, match="windows and"):
            EN.speaker_trial_hist(None, None, None, None, None, "euclidean", True, wins, bins)


def test_triangle_sum_with_rows_is_one_device_call():
    seen = []

    def device_fn(rows):
        seen.append(rows)
        return torch.tensor([rows[0], rows[1]], dtype=torch.int64)
    assert V.triangle_sum(device_fn, 37, rows=(3, 9)).tolist() == [3, 9] and seen == [(3, 9)]
    assert V.triangle_sum(device_fn, 37).tolist() == [0, 37] and seen == [(3, 9), (0, 37)]   # one rank: the whole triangle


def test_distance_table_is_one_object_built_from_the_header():
    from voicemap_amd import _lib, mining, retrieval
    assert _lib.DIST == {"euclidean": _lib.VM_DIST_EUCLIDEAN, "cosine": _lib.VM_DIST_COSINE, "dot_product": _lib.VM_DIST_DOT}
    assert retrieval._DIST is _lib.DIST and mining._DIST is _lib.DIST and EN.KINDS is _lib.DIST
    assert V.SCORES == {**_lib.DIST, "weighted_l1": _lib.VM_SCORE_WEIGHTED_L1}
    assert V.VM_SCORE_NEG_EUCLIDEAN == _lib.VM_SCORE_NEG_EUCLIDEAN
