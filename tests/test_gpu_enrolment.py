"""-m gpu checks of speaker models (csrc/enrol.hip, voicemap_amd/enrolment.py) against the float64 numpy twins: an exact case bit for
bit, the general case within one fp32 ulp plus the float64 rounding of the sums (derived below, not measured), ranks within the interval
that tolerance allows, the trial histograms as integers against numpy's binning of the device's own score matrix, the exact metrics
against the sort-based definition, determinism, two ranks, and the cross-tile merge at a size beyond one tile in every direction."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from voicemap_amd import enrolment as EN
from voicemap_amd import retrieval
from voicemap_amd import verification as V
from voicemap_amd.retrieval import EmbeddingCache

pytestmark = pytest.mark.gpu
KINDS = ["euclidean", "cosine", "dot_product"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _corpus(N, S, E, seed, noise=1.0, scale=1.0):
    """Speaker centre + noise; unequal speaker sizes with a one-file speaker (index 0) and one un-enrolled row (label -1)."""
    r = np.random.default_rng(seed)
    w = r.uniform(0.3, 3.0, S - 1)
    cnt = np.floor(w / w.sum() * (N - 2 - 2 * (S - 1))).astype(int) + 2
    label = np.concatenate([[0], np.repeat(np.arange(1, S), cnt)])
    label = np.concatenate([label, r.integers(1, S, N - 1 - len(label)), [-1]])
    r.shuffle(label)
    cent = r.normal(0, 1, (S, E)) * scale
    emb = (cent[np.maximum(label, 0)] + r.normal(0, noise, (N, E)) * scale).astype(np.float32)
    return emb, label.astype(np.int32)


def _device(emb, label, q, q_label, kind, loo, S):
    e, ql = torch.as_tensor(emb).cuda(), torch.as_tensor(q_label).cuda()
    qq = e if q is emb else torch.as_tensor(q).cuda()
    sums, msum, count = EN.speaker_sums(e, torch.as_tensor(label).cuda(), S, kind)
    out = EN.speaker_identify(qq, ql, sums, msum, count, kind, loo, return_scores=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, (sums, msum, count), (qq, ql)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.int32)


def _assert_same_bits(got, ref, what):
    assert np.array_equal(_bits(got), _bits(ref)) or np.array_equal(got, ref, equal_nan=True) and \
        np.array_equal(np.signbit(got), np.signbit(ref)), what


def _lattice(sizes, E, seed, twins=True):
    """Integer embeddings in [-8, 8]; speaker s has sizes[s] rows; with ``twins`` the last speaker holds copies of the rows of the one
    before it (the same multiset: every other query ties between the two)."""
    r = np.random.default_rng(seed)
    label = np.repeat(np.arange(len(sizes)), sizes)
    emb = r.integers(-8, 9, (len(label), E)).astype(np.float32)
    if twins:
        assert sizes[-1] == sizes[-2]
        emb[label == len(sizes) - 1] = emb[label == len(sizes) - 2][::-1]
    p = r.permutation(len(label))
    return emb[p], label[p].astype(np.int32)


@pytest.mark.parametrize("E", [1, 3, 4, 31, 32, 33, 50, 64, 65, 100, 255, 256])
def test_exact_case_equals_the_twin_bit_for_bit(E):
    """Every mean is dyadic (divisors 1, 2, 4, 8), so every squared distance is exact in float64 in any order, with or without fma, and
    the square root is correctly rounded: scores, true_score, rank, best_idx and best_val are the twin's bits.  Without leave-one-out the
    sizes are 1, 2, 4, 8; with it 2, 3, 5, 9 for the OWN speaker's model (divisors 1, 2, 4, 8) -- the other speakers' models then
    divide by 3, 5 and 9, which is not dyadic, so under leave-one-out the whole matrix is compared on a corpus of two-file speakers
    (divisors 1 and 2) and on the 2, 3, 5, 9 corpus the bit-for-bit claim covers true_score and every cell whose divisor is a power of
    two; its other cells are held to one fp32 ulp and its ranks to the order of the device's own matrix.  None of it depends on E: the
    widths lie on both sides of the 4-wide vector load (1, 3, 4), of the 32-component stage (31, 32, 33) and of the later stages (64,
    65, 100), up to EN_MAX_E (255, 256)."""
    sizes = [1, 2, 4, 8] * 6 + [4, 4]
    emb, label = _lattice(sizes, E, 1)
    S = len(sizes)
    got, _, _ = _device(emb, label, emb, label, "euclidean", False, S)
    sc, trial = EN.trial_scores_numpy(emb, label, emb, label, "euclidean", False)
    ref = EN.ranks_numpy(sc, trial, label)
    assert trial.all()
    _assert_same_bits(got["scores"], sc.astype(np.float32), "scores")
    for k in ("true_score", "rank", "best_idx", "best_val"):
        _assert_same_bits(got[k], ref[k], k)
    # the planted twins: a query of another speaker scores both alike and the lower index comes first.  Properties of this corpus only
    # where the twin has them: from E = 32 on (checked with trial_scores_numpy / ranks_numpy); narrower random integer rows carry no
    # speaker structure, and there the equality with the twin above is the whole claim.
    if E >= 32:
        other = label < S - 2
        assert np.array_equal(got["scores"][other, S - 2], got["scores"][other, S - 1])
        assert not np.any(got["best_idx"] == S - 1)
        assert np.all(got["rank"][label == S - 1] >= 1) and np.all(got["rank"][label == S - 2] == 0)   # an own row scores 0 against both

    sizes = [2] * 30
    emb, label = _lattice(sizes, E, 2)
    S = len(sizes)
    got, _, _ = _device(emb, label, emb, label, "euclidean", True, S)
    sc, trial = EN.trial_scores_numpy(emb, label, emb, label, "euclidean", True)
    ref = EN.ranks_numpy(sc, trial, label)
    _assert_same_bits(got["scores"], sc.astype(np.float32), "scores, leave-one-out")
    for k in ("true_score", "rank", "best_idx", "best_val"):
        _assert_same_bits(got[k], ref[k], k)

    sizes = [2, 3, 5, 9] * 6 + [5, 5]
    emb, label = _lattice(sizes, E, 3)
    S = len(sizes)
    got, _, _ = _device(emb, label, emb, label, "euclidean", True, S)
    sc, trial = EN.trial_scores_numpy(emb, label, emb, label, "euclidean", True)
    ref = EN.ranks_numpy(sc, trial, label)
    assert trial.all()
    _assert_same_bits(got["true_score"], ref["true_score"], "true_score, leave-one-out")
    own = label[:, None] == np.arange(S)[None, :]
    dyadic = own | (np.asarray(sizes) == 2)[None, :]
    _assert_same_bits(got["scores"][dyadic], sc.astype(np.float32)[dyadic], "dyadic cells, leave-one-out")
    r32 = sc.astype(np.float32)
    assert np.all(np.abs(got["scores"].astype(np.float64) - sc) <= np.spacing(np.abs(r32)).astype(np.float64))
    dev = EN.ranks_numpy(got["scores"], trial, label)
    for k in ("rank", "best_idx", "best_val"):
        _assert_same_bits(got[k], dev[k], k)


def _tolerance(emb, label, q, q_label, sc, kind, S, loo, sums=None):
    """The tolerance of a device score against the float64 twin ``sc``: one fp32 ulp of fp32(sc) plus an absolute floor for the float64
    rounding of the sums, which the two sides add in different orders.  With u = 2^-53, n the largest speaker size and E components, a
    model component carries at most ~n u of relative rounding from its sum (plus a few u from the divisions), the E-term score sum
    another ~E u, so with g = 8 (n + E) u (a factor 8 for the few operations per term and the leave-one-out subtraction, which can
    cancel one of n like terms):
      euclidean   |d sqrt(sum (q - p)^2)| <= g (|q| + |p|) <= g 2 R                       (R = the largest row norm; |p| <= R)
      dot_product |d q.p| <= g |q| |p| <= g R^2
      cosine      the models are means of unit vectors: |d p| <= g against |p| >= p_min (the smallest model norm, shared or
                  leave-one-out, from the twin's sums), so |d cos| <= 2 g / p_min
    A leave-one-out near-duplicate under cosine is ~1e-16 of such noise, not a number to compare in ulps."""
    n = int(np.bincount(label[label >= 0], minlength=S).max())
    g = 8.0 * (n + emb.shape[1]) * U
    R = float(np.linalg.norm(np.concatenate([emb, q]).astype(np.float64), axis=1).max())
    if kind == "euclidean":
        floor = g * 2 * R
    elif kind == "dot_product":
        floor = g * R * R
    else:
        sm, _, count = sums if sums is not None else EN.speaker_sums_numpy(emb, label, S, 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            pn = [np.linalg.norm(sm[count > 0] / count[count > 0, None], axis=1)]
            if loo:
                qq = q.astype(np.float64)
                ok = (q_label >= 0) & (count[np.maximum(q_label, 0)] > 1)
                own = q_label[ok]
                c = qq[ok] / np.linalg.norm(qq[ok], axis=1)[:, None]
                pn.append(np.linalg.norm((sm[own] - c) / (count[own] - 1)[:, None], axis=1))
        pn = np.concatenate(pn)
        floor = 2 * g / float(np.nanmin(pn))
    with np.errstate(invalid="ignore"):
        return np.spacing(np.abs(sc.astype(np.float32))).astype(np.float64) + floor


def _rank_interval(sc, trial, tol, q_label):
    """[lo, hi] of the ranks the tolerance allows: lo = #{s: ref_s + tol_s < ref_true - tol_true}, hi = #{s: ref_s - tol_s <= ref_true +
    tol_true} - 1 (the own speaker is in the second count), over the trials of the row; rows whose own cell is NaN or no trial: None."""
    M, S = sc.shape
    rows = np.arange(M)
    own = np.clip(q_label, 0, S - 1)
    ranked = (q_label >= 0) & trial[rows, own] & ~np.isnan(sc[rows, own])
    t, tt = sc[rows, own][:, None], tol[rows, own][:, None]
    with np.errstate(invalid="ignore"):
        lo = ((sc + tol < t - tt) & trial).sum(1)
        hi = ((sc - tol <= t + tt) & trial).sum(1) - 1
    return lo, hi, ranked


def _check_general(emb, label, q, q_label, kind, loo, S, scores_too=True):
    got, _, _ = _device(emb, label, q, q_label, kind, loo, S)
    sc, trial = EN.trial_scores_numpy(emb, label, q, q_label, kind, loo, S=S)
    tol = _tolerance(emb, label, q, q_label, sc, kind, S, loo)
    lo, hi, ranked = _rank_interval(sc, trial, tol, q_label)
    # on the twin alone: the interval is a single value for at least 99 % of the rows
    assert (lo == hi)[ranked].mean() >= 0.99, (lo == hi)[ranked].mean()
    g = got["scores"]
    assert np.array_equal(np.isnan(g), ~trial | np.isnan(sc))
    ok = trial & ~np.isnan(sc)
    err = np.abs(g.astype(np.float64) - sc)
    assert np.all(err[ok] <= tol[ok]), float((err[ok] / tol[ok]).max())
    rk = got["rank"]
    own = np.clip(q_label, 0, S - 1)
    has_own = (q_label >= 0) & trial[np.arange(len(q_label)), own]
    assert np.array_equal(rk >= 0, has_own)
    assert np.all((rk[ranked] >= lo[ranked]) & (rk[ranked] <= hi[ranked]))   # no row is left out
    assert np.array_equal(np.isnan(got["true_score"]), ~has_own | np.isnan(sc[np.arange(len(own)), own]))
    # the device's own outputs agree with each other exactly: ranks, best and true_score are those of its score matrix
    dev = EN.ranks_numpy(g, trial, q_label)
    for k in ("rank", "best_idx", "best_val", "true_score"):
        _assert_same_bits(got[k], dev[k], k)
    return got, sc, trial


@pytest.mark.parametrize("loo", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("E", [64, 50, 33, 100])
def test_general_case_scores_within_one_ulp_and_ranks_within_the_interval(E, kind, loo):
    emb, label = _corpus(3000, 40, E, 10 + E)
    got, sc, trial = _check_general(emb, label, emb, label, kind, loo, 40)
    one = int(np.flatnonzero(label == 0)[0])
    un = int(np.flatnonzero(label == -1)[0])
    assert got["rank"][un] == -1 and got["best_idx"][un] >= 0
    assert (got["rank"][one] == -1) == loo and trial[one, 0] == (not loo)
    assert (got["rank"][label >= 0] == 0).mean() > 0.5


def _trial_mask(count, q_label, loo):
    c = count.cpu().numpy().astype(np.int64)
    S = len(c)
    n = np.tile(c, (len(q_label), 1))
    if loo:
        own = (q_label[:, None] == np.arange(S)[None, :])
        n = n - own
    return n > 0


@pytest.mark.parametrize("loo", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_trial_histogram_equals_numpy_binning_of_the_device_score_matrix(kind, loo):
    for E in (64, 50):
        emb, label = _corpus(3000, 40, E, 20 + E)
        emb[np.flatnonzero(label == -1)[0]] = 0.0    # an un-enrolled zero row: under cosine every one of its scores is NaN
        S = 40
        got, (sums, msum, count), (q, ql) = _device(emb, label, emb, label, kind, loo, S)
        trial = _trial_mask(count, label, loo)
        s = got["scores"]
        assert np.array_equal(np.isnan(s) & trial, np.isnan(s) & trial & (kind == "cosine"))
        assert np.all(np.isnan(s[~trial])) and (~trial).sum() == (1 if loo else 0)
        target = (label[:, None] == np.arange(S)[None, :])
        sv, tv = s[trial], target[trial]
        f = sv[np.isfinite(sv)]
        lo, hi = float(f.min()), float(f.max())
        one = [V.pass1_window(lo, 0.5 * (lo + hi))]
        h = EN.speaker_trial_hist(q, ql, sums, msum, count, kind, loo, one, 4096).cpu().numpy()
        assert np.array_equal(h, V.bin_scores(sv, tv, one, 4096)), (E, "one window")
        assert h.sum() == trial.sum() and h[0, :, -1].sum() == (S if kind == "cosine" else 0)
        b = int(np.argmax(h[0, 0, :4096] + h[0, 1, :4096]))
        k0, sh0 = one[0]
        four = [(k0 + (b << sh0), max(0, sh0 - 10)), (V.key_of(float(np.median(f))), 0), (V.key_of(0.5 * (lo + hi)), 31), (0, 22)]
        h4 = EN.speaker_trial_hist(q, ql, sums, msum, count, kind, loo, four, 1024).cpu().numpy()
        assert np.array_equal(h4, V.bin_scores(sv, tv, four, 1024)), (E, "four windows")
        # two row ranges accumulated into one histogram = one call over both
        acc = EN.speaker_trial_hist(q[:1237], ql[:1237], sums, msum, count, kind, loo, one, 4096)
        acc = EN.speaker_trial_hist(q[1237:], ql[1237:], sums, msum, count, kind, loo, one, 4096, hist=acc)
        assert np.array_equal(acc.cpu().numpy(), h), (E, "row ranges")


def _cache(emb, codes):
    return EmbeddingCache(torch.as_tensor(np.ascontiguousarray(emb, np.float32)).cuda(), np.asarray(codes))


def _assert_metrics_equal(got, ref):
    for k in ("eer", "eer_threshold", "far_at_eer", "frr_at_eer", "best_balanced_accuracy", "best_threshold", "n_target", "n_nontarget",
              "n_nan"):
        assert got[k] == ref[k], (k, got[k], ref[k])


@pytest.mark.parametrize("kind", KINDS)
def test_model_trial_metrics_equal_the_sorted_definition_on_the_device_scores(kind):
    emb, label = _corpus(3000, 40, 64, 31, noise=1.6)
    label = np.where(label < 0, 5, label)
    codes = (label * 7 + 100).astype(np.int64)          # speaker codes are not dense
    cache = _cache(emb, codes)
    S = 40
    for loo in (True, False):
        models = EN.enrol(cache, kind)
        assert np.array_equal(models.speakers, np.arange(S) * 7 + 100)
        got, (sums, msum, count), _ = _device(emb, label, emb, label, kind, loo, S)
        assert torch.equal(sums, models.sums) and torch.equal(count, models.count) and torch.equal(msum, models.msum)
        trial = _trial_mask(count, label, loo)
        target = label[:, None] == np.arange(S)[None, :]
        sv, tv = got["scores"][trial], target[trial]
        m = EN.model_trial_metrics(models, cache, leave_one_out=loo)
        _assert_metrics_equal(m, V.sorted_metrics(sv, tv))
        assert m["n_target"] == len(label) - (1 if loo else 0) and 0.0 < m["eer"] < 0.5
        for t in (m["best_threshold"], m["eer_threshold"], float(np.median(sv))):
            at = EN.model_trial_accuracy_at_threshold(models, cache, t, leave_one_out=loo)
            far, frr = float((sv[~tv] < t).mean()), float((sv[tv] >= t).mean())
            assert (at["far"], at["frr"], at["balanced_accuracy"]) == (far, frr, 1.0 - (far + frr) / 2)
        at = EN.model_trial_accuracy_at_threshold(models, cache, m["best_threshold"], leave_one_out=loo)
        assert at["balanced_accuracy"] == m["best_balanced_accuracy"]


@pytest.mark.parametrize("kind", KINDS)
def test_identify_and_cmc_against_the_twin(kind):
    emb, label = _corpus(3000, 40, 64, 41, noise=1.8)
    label = np.where(label < 0, 7, label)
    cache = _cache(emb, label)
    models = EN.enrol(cache, kind)
    res = EN.identify(models, cache)
    assert res["leave_one_out"] is True and res["n_queries"] == 3000 and res["n_unranked"] == 1
    got, sc, trial = _check_general(emb, label, emb, label, kind, True, 40)
    assert np.array_equal(res["rank"], got["rank"]) and np.array_equal(res["pred"], got["best_idx"])
    _assert_same_bits(res["true_score"], got["true_score"], "true_score")
    rk = got["rank"][got["rank"] >= 0]
    cmc = np.array([(rk < k).mean() for k in range(1, 41)])
    assert np.array_equal(res["cmc"], cmc) and res["rank1_accuracy"] == cmc[0] and res["cmc"][-1] == 1.0
    assert abs(res["mean_reciprocal_rank"] - (1.0 / (rk + 1)).mean()) < 1e-12
    assert 0.3 < res["rank1_accuracy"] <= 1.0
    # the rows of a shard, by hand
    part = EN.identify(models, cache, rows=(1000, 1500))
    assert np.array_equal(part["rank"], got["rank"][1000:1500]) and part["n_queries"] == 500


@pytest.mark.parametrize("kind", KINDS)
def test_per_speaker_mode_is_the_exhaustive_n_shot_task_of_vm_nshot_indexed(kind):
    """per_speaker = n: for a few queries the same task drawn by hand (the query's speaker first, then every other speaker, each with its
    n enrolled rows) through vm_nshot_indexed gives the same best speaker and the same scores to fp32 rounding."""
    r = np.random.default_rng(51)
    S, n, E = 12, 3, 64
    label = np.repeat(np.arange(S), r.integers(n + 1, 30, S)).astype(np.int32)
    r.shuffle(label)
    emb = (r.normal(0, 1, (S, E))[label] + r.normal(0, 1.5, (len(label), E))).astype(np.float32)
    cache = _cache(emb, label)
    models = EN.enrol(cache, kind, per_speaker=n, seed=3)
    assert np.all(models.count.cpu().numpy() == n) and (models.label >= 0).sum() == S * n
    res = EN.identify(models, cache)
    assert res["leave_one_out"] is False and res["n_queries"] == len(label) - S * n and res["n_unranked"] == 0
    assert np.array_equal(res["query_index"], np.flatnonzero(models.label < 0))
    enrolled = [np.flatnonzero(models.label == s) for s in range(S)]
    pick = r.choice(len(res["query_index"]), 40, replace=False)
    qi, sup, order = [], [], []
    for j in pick:
        row = int(res["query_index"][j])
        cls = [int(label[row])] + [s for s in range(S) if s != label[row]]
        qi.append(row)
        sup.append(np.concatenate([enrolled[s] for s in cls]))
        order.append(cls)
    _, pred = retrieval.evaluate_tasks(cache, np.array(qi), np.stack(sup), S, n, kind, return_pred=True)
    pred = pred.cpu().numpy()
    q = torch.as_tensor(emb[qi]).cuda()
    out = EN.speaker_identify(q, torch.as_tensor(label[qi]).cuda(), models.sums, models.msum, models.count, kind, False, return_scores=True)
    sc = out["scores"].cpu().numpy()
    for t in range(len(qi)):
        mine = sc[t, order[t]]
        assert np.all(np.abs(mine - pred[t]) <= 2 * np.spacing(np.abs(pred[t])) + 1e-12)
        assert order[t][int(np.argmin(pred[t]))] == res["pred"][pick[t]] or np.sort(pred[t])[1] - np.sort(pred[t])[0] <= 4 * np.spacing(
            np.abs(pred[t]).max())
        assert (int(np.argmin(pred[t])) == 0) == (res["rank"][pick[t]] == 0) or np.sort(pred[t])[1] - np.sort(pred[t])[0] <= 4 * np.spacing(
            np.abs(pred[t]).max())


def test_two_runs_give_identical_bytes():
    emb, label = _corpus(3000, 40, 50, 61)
    for kind in KINDS:
        runs = []
        for _ in range(2):
            got, (sums, msum, count), (q, ql) = _device(emb, label, emb, label, kind, True, 40)
            h = EN.speaker_trial_hist(q, ql, sums, msum, count, kind, True, [V.pass1_window(0.0, 2.0)], 4096).cpu().numpy()
            runs.append([got[k].tobytes() for k in sorted(got)] + [sums.cpu().numpy().tobytes(), msum.cpu().numpy().tobytes(),
                                                                    count.cpu().numpy().tobytes(), h.tobytes()])
        assert runs[0] == runs[1], kind


@pytest.mark.parametrize("kind", KINDS)
def test_beyond_one_tile_in_every_direction_ranks_stay_in_the_interval(kind):
    """M = 20 000 rows (313 workgroups), S = 1 000 models (16 model tiles), E = 100 (4 component chunks, the last one partial)."""
    N, S, E = 20000, 1000, 100
    r = np.random.default_rng(71)
    label = np.concatenate([np.arange(S), r.integers(0, S, N - S)]).astype(np.int32)
    r.shuffle(label)
    emb = (r.normal(0, 1, (S, E))[label] + r.normal(0, 0.9, (N, E))).astype(np.float32)
    got, _, _ = _device(emb, label, emb, label, kind, True, S)
    # the twin in blocks of rows (a leave-one-out model differs from the shared one only in the own cell)
    sums, msum, count = EN.speaker_sums_numpy(emb, label, S, kind)
    unit_sums = (sums, msum, count) if kind != "euclidean" else None   # cosine and dot_product sum the same unit vectors
    lo_all, hi_all, ranked_all = [], [], []
    kk = EN.KINDS[kind]
    for b0 in range(0, N, 2000):
        q, ql = emb[b0:b0 + 2000], label[b0:b0 + 2000]
        sc, trial = _twin_from_sums(sums, msum, count, q, ql, kk)
        tol = _tolerance(emb, label, q, ql, sc, kind, S, True, sums=unit_sums)
        lo, hi, ranked = _rank_interval(sc, trial, tol, ql)
        lo_all.append(lo), hi_all.append(hi), ranked_all.append(ranked)
    lo, hi, ranked = np.concatenate(lo_all), np.concatenate(hi_all), np.concatenate(ranked_all)
    assert (lo == hi)[ranked].mean() >= 0.99
    rk = got["rank"]
    assert np.array_equal(rk >= 0, ranked)
    assert np.all((rk[ranked] >= lo[ranked]) & (rk[ranked] <= hi[ranked]))
    dev = EN.ranks_numpy(got["scores"], ~np.isnan(got["scores"]), label)
    for k in ("rank", "best_idx", "best_val", "true_score"):
        _assert_same_bits(got[k], dev[k], k)


def _twin_from_sums(sums, msum, count, q, q_label, kind):
    """``trial_scores_numpy`` with leave-one-out for a block of query rows, vectorised: the shared models for every cell, the own cell
    from sums - c_m (the same float64 definition; the (M, S) loop of the twin is too slow at 20 000 x 1 000)."""
    q = q.astype(np.float64)
    M, S = len(q), len(count)
    qmag = np.sqrt((q * q).sum(1))
    cq = q if kind == 0 else q / qmag[:, None]

    def score(p):   # q (M, E) against p (M or 1, K, E) -> (M, K)
        if kind == 0:
            if p.shape[0] == 1:   # direct form (no norm expansion), row blocks in parallel
                return torch.cdist(torch.as_tensor(q), torch.as_tensor(p[0]), compute_mode="donot_use_mm_for_euclid_dist").numpy()
            return np.sqrt(((q[:, None, :] - p) ** 2).sum(-1))
        if kind == 1:
            return 1.0 - (q[:, None, :] * p).sum(-1) / (qmag[:, None] * np.sqrt((p * p).sum(-1)))
        return -(q[:, None, :] * p).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = count.astype(np.float64)
        P = sums / n[:, None]
        if kind == 2:
            P = (msum / n)[:, None] * P
        sc = np.concatenate([score(P[None, s0:s0 + 100]) for s0 in range(0, S, 100)], axis=1)
        trial = np.tile(count > 0, (M, 1))
        n1 = n[q_label] - 1
        p1 = (sums[q_label] - cq) / n1[:, None]
        if kind == 2:
            p1 = ((msum[q_label] - qmag) / n1)[:, None] * p1
        own = score(p1[:, None, :])[:, 0]
    rows = np.arange(M)
    sc[rows, q_label] = np.where(n1 > 0, own, np.nan)
    trial[rows, q_label] = n1 > 0
    return sc, trial


_TWO_RANK = r"""
import json, sys
sys.path.insert(0, {root!r})
import numpy as np, torch
from voicemap_amd import parallel, enrolment as EN
from voicemap_amd.retrieval import EmbeddingCache
rank, world, _ = parallel.init_distributed(timeout_s=120)
torch.cuda.set_device(0)
r = np.random.default_rng(4)
spk = r.integers(0, 13, 2001)
emb = (r.normal(0, 1, (13, 64))[spk] + r.normal(0, 1.5, (2001, 64))).astype(np.float32)
cache = EmbeddingCache(torch.as_tensor(emb).cuda(), spk)
models = EN.enrol(cache, "cosine")
res = EN.identify(models, cache)
m = EN.model_trial_metrics(models, cache)
m.pop("roc")
out = dict(m, rank1=res["rank1_accuracy"], mrr=res["mean_reciprocal_rank"], cmc=res["cmc"].tolist(), n_queries=res["n_queries"],
           rows=list(res["rows"]), n_local=len(res["rank"]))
if rank == 0:
    print("RESULT " + json.dumps(out))
"""


def test_two_rank_gloo_run_gives_the_same_results(tmp_path):
    script = tmp_path / "two_rank.py"
    script.write_text(_TWO_RANK.format(root=ROOT))
    env = dict(os.environ, VOICEMAP_DIST_BACKEND="gloo", MASTER_PORT="29741")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", str(script)], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    two = json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    r = np.random.default_rng(4)
    spk = r.integers(0, 13, 2001)
    emb = (r.normal(0, 1, (13, 64))[spk] + r.normal(0, 1.5, (2001, 64))).astype(np.float32)
    cache = _cache(emb, spk)
    models = EN.enrol(cache, "cosine")
    res = EN.identify(models, cache)
    one = EN.model_trial_metrics(models, cache)
    assert two.pop("rows") == [0, 1001] and two.pop("n_local") == 1001
    assert two.pop("rank1") == res["rank1_accuracy"] and two.pop("mrr") == res["mean_reciprocal_rank"]
    assert two.pop("cmc") == res["cmc"].tolist() and two.pop("n_queries") == 2001
    for k, v in two.items():
        assert v == one[k], k


def test_experiment_script_synthetic_prints_a_parsable_line():
    out = subprocess.run([sys.executable, "-m", "experiments.speaker_identification", "--synthetic", "--n-seconds", "1"], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    row = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert row["speakers"] == 20 and row["queries"] == 160 and row["leave_one_out"] is True
    assert 0.0 <= row["rank1_accuracy"] <= row["rank5_accuracy"] <= 1.0 and 0.0 <= row["trial_eer"] <= 1.0
    assert row["target_trials"] == 160 and row["nontarget_trials"] == 160 * 19
    out = subprocess.run([sys.executable, "-m", "experiments.speaker_identification", "--synthetic", "--n-seconds", "1", "--per-speaker", "3",
                          "--distance", "cosine"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    row = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert row["queries"] == 100 and row["leave_one_out"] is False and row["per_speaker"] == 3
