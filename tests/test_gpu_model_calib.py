"""-m gpu checks of the calibration of speaker-model trials: vm_speaker_trial_calib_sums / vm_plda_speaker_trial_calib_sums (the CALIB
mode of csrc/enrol_tile.hpp's tile kernel) and fit_model_calibration / model_cllr / model_detection_costs on top of them.

The numpy side takes its scores from the device's own ``scores`` matrix of vm_[plda_]speaker_identify (tests/model_calib_cases.py), so
only the new epilogue and reduction are under test: the counts are exact, the sums that are exact in float64 (integer scores at
a = b = tau = 0) equal numpy bit for bit, and every other sum lies within the rounding count of tests/calib_refs.py around an
extended-precision reference -- the per-trial arithmetic is the pair path's cal_terms.  Every device call runs with guard words around
its result and its workspace."""
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import calib_refs as R
from tests import model_calib_cases as MC
from tests.gpu_util import L
from voicemap_amd import calibration as C
from voicemap_amd import enrolment as EN
from voicemap_amd import verification as V
from voicemap_amd.retrieval import EmbeddingCache

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64 here")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUC, COS, DOT = MC.EUC, MC.COS, MC.DOT
POINTS = [(0.5, 1, 1), (0.01, 1, 1), (0.05, 10, 1)]


def _speaker_sums(emb, label, S, kind):
    return EN.speaker_sums(MC.cuda(emb, torch.float32), MC.cuda(label, torch.int32), S, kind)


def _cache(emb, spk):
    return EmbeddingCache(MC.cuda(emb, torch.float32), np.asarray(spk))


# ---- 1. the exact plant ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 63, 64, 65, 130])
def test_integer_scores_at_zero_give_the_exact_sums(M):
    """MC.plant: every score a small integer, a = b = tau = 0, so p = 1/2 and w = 1/4 exactly: the counts and P0, P1, W0, W1, W2 equal
    numpy bit for bit in any order, and L (n log1p(1)) lies within the rounding bound.  Every case holds a query labelled -1 and one
    labelled past S (M >= 3), a speaker without rows (S >= 3) and a one-row speaker (no own trial under leave-one-out)."""
    for S in (1, 63, 64, 65, 129):
        for E in (1, 3, 4, 64, 67, 256):
            for one_speaker in (False, True) if E in (3, 64) else (False,):
                emb, label, q, q_label = MC.plant(M, S, E, M * 1000 + S * 10 + E, one_speaker)
                sums, msum, count = _speaker_sums(emb, label, S, EUC)
                for loo in (False, True):
                    what = "plant M=%d S=%d E=%d one=%d loo=%d" % (M, S, E, one_speaker, loo)
                    s, trial = MC.device_scores(q, q_label, sums, msum, count, EUC, loo)
                    assert np.array_equal(trial, MC.trial_mask(q_label, count.cpu().numpy(), loo)), what
                    assert np.array_equal(s[trial], np.round(s[trial])) and np.all(np.abs(s[trial]) <= 480), what
                    got = MC.geo_sums(q, q_label, sums, msum, count, EUC, loo)
                    ref = EN.model_calib_sums_numpy(s, trial, q_label, 0.0, 0.0, 0.0)
                    assert np.array_equal(got[:, MC.EXACT], ref[:, MC.EXACT]), (what, got, ref)
                    assert got[0, 0] + got[1, 0] == trial.sum() and not got[:, 1].any(), what
                    tg = MC.target_mask(q_label, S)
                    if one_speaker:   # only speaker 0 has a model: one trial per row, a target iff the row is labelled 0
                        assert got[0, 0] == (q_label == 0).sum() and got[1, 0] == (q_label != 0).sum(), what
                    R.assert_sums_close(got, s[trial], tg[trial], 0.0, 0.0, 0.0, what=what)


# ---- 2. accumulators carried across tiles --------------------------------------------------------------------------------------------
def test_a_grid_whose_splits_hold_two_tiles_each():
    """M = 2048 against S = 8192 one-row models: 32 query tiles x 64 splits, and the 128 model tiles make two per split -- the smallest
    such grid in which a workgroup carries its accumulators from one tile to the next (M = 1024: 128 splits of one tile)."""
    M, S, E = 2048, 8192, 4
    assert L().query("vm_speaker_trial_calib_sums_splits", M, S) == 64
    assert L().query("vm_speaker_trial_calib_sums_splits", 1024, S) == 128
    r = np.random.default_rng(2)
    emb = np.zeros((S, E), np.float32)
    emb[:, 1] = 12 * r.integers(-5, 6, S)
    label = np.arange(S, dtype=np.int32)
    q = np.zeros((M, E), np.float32)
    q[:, 1] = 12 * r.integers(-5, 6, M)
    q_label = r.integers(0, S, M).astype(np.int32)
    sums, msum, count = _speaker_sums(emb, label, S, EUC)
    d, trial = MC.device_scores(q, q_label, sums, msum, count, EUC, False)
    assert trial.all()
    got = MC.geo_sums(q, q_label, sums, msum, count, EUC, False)
    cnt, s1, s2 = np.zeros(2), np.zeros(2), np.zeros(2)
    for lo in range(0, M, 256):   # integer sums by class: exact in float64
        blk = d[lo:lo + 256].astype(np.float64)
        own = MC.target_mask(q_label[lo:lo + 256], S)
        for c, m in enumerate((own, ~own)):
            cnt[c] += m.sum()
            s1[c] += blk[m].sum()
            s2[c] += (blk[m] ** 2).sum()
    assert cnt.tolist() == [M, M * (S - 1)]
    for c in range(2):
        assert got[c, :2].tolist() == [cnt[c], 0.0]
        assert got[c, 3:].tolist() == [cnt[c] / 2, s1[c] / 2, cnt[c] / 4, s1[c] / 4, s2[c] / 4], (c, got)
        ref = cnt[c] * np.log1p(np.longdouble(1))   # L = n log1p(1)
        assert abs(float(np.longdouble(got[c, 2]) - ref)) <= (cnt[c] + R.K["L"]) * R.U * float(ref)


# ---- 3. general scores -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _backend(name):
    """(rows, labels, S, (sums, msum, count, kind, tables), call(q, q_label, loo, abt, stats), n_max)."""
    if name in ("euclidean", "cosine", "dot_product"):
        kind = EN.KINDS[name]
        emb, spk = MC.clusters(300, 64, 37, 40 + kind)
        sums, msum, count = _speaker_sums(emb, spk, 37, kind)
        return emb, spk, 37, (sums, msum, count, kind, None), (
            lambda q, ql, loo, abt, stats: MC.geo_sums(q, ql, sums, msum, count, kind, loo, abt, stats)), None
    D = int(name[4:])
    model, rows, spk = MC.plda_case(D, 100 + D)
    assert rows.shape[1] == {63: 64, 65: 68}[D]
    sums, msum, count = _speaker_sums(rows, spk, 37, EUC)
    n_max = int(count.max().item())
    tables = EN.plda_tables_to(model.model_tables(n_max), "cuda")
    return rows, spk, 37, (sums, msum, count, EUC, tables), (
        lambda q, ql, loo, abt, stats: MC.plda_sums(q, ql, sums, count, tables, loo, abt, stats)), n_max


@pytest.mark.parametrize("loo", [False, True])
@pytest.mark.parametrize("normalised", [False, True])
@pytest.mark.parametrize("backend", ["euclidean", "cosine", "dot_product", "plda63", "plda65"])
def test_sums_of_every_back_end_lie_within_the_rounding_bound(backend, normalised, loo):
    rows, spk, S, (sums, msum, count, kind, tables), call, n_max = _backend(backend)
    s, trial = MC.device_scores(rows, spk, sums, msum, count, kind, loo, tables)
    tg = MC.target_mask(spk, S)
    # every cell is a trial but, under leave-one-out, the own cell of a row whose speaker has no other row
    assert np.array_equal(trial, MC.trial_mask(spk, count.cpu().numpy(), loo, n_max)) and (~tg | trial).sum() >= 300 * 36 + 290
    stats = None
    if normalised:
        stats = MC.synthetic_stats(s, trial, loo, 7)
        s = EN.normalise_trials_numpy(s, spk, *stats)
    s, tg = s[trial], tg[trial]
    assert np.isfinite(s).all()
    for abt in MC.ABT:
        z = abt[0] * s.astype(np.float64) + abt[1] + abt[2]
        assert np.abs(z).max() < 700 or np.abs(z).min() > 750   # no term in the denormal range of exp
        got = call(rows, spk, loo, abt, stats)
        R.assert_sums_close(got, s, tg, *abt, what="%s norm %d loo %d abt %r" % (backend, normalised, loo, abt))
        assert got[:, 0].tolist() == [tg.sum(), 300 * 36] and not got[:, 1].any()


# ---- 4. non-finite scores ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loo", [False, True])
def test_non_finite_scores_are_skipped_and_counted(loo):
    N, E, S = 200, 64, 11
    emb, spk = MC.clusters(N, E, S, 3)
    sums, msum, count = _speaker_sums(emb, spk, S, EUC)     # the models are enrolled from the clean rows
    q = emb.copy()
    q[37] = np.nan                                           # a NaN query row: S NaN scores (its own, under leave-one-out, too)
    abt = MC.ABT[0]
    s, seen = MC.device_scores(q, spk, sums, msum, count, EUC, loo)
    trial = MC.trial_mask(spk, count.cpu().numpy(), loo)
    tg = MC.target_mask(spk, S)
    assert trial.all() and np.array_equal(~seen, np.broadcast_to(np.arange(N)[:, None] == 37, seen.shape))
    got = MC.geo_sums(q, spk, sums, msum, count, EUC, loo, abt)
    assert got[:, 1].tolist() == [1.0, S - 1.0]
    R.assert_sums_close(got, s[trial], tg[trial], *abt, what="NaN row")
    # normalised: a row with rsig_q = +inf, a model with rsig_s = +inf and, under leave-one-out, a row with rsig_own = +inf
    stats = [np.array(t) if t is not None else None for t in MC.synthetic_stats(s, seen, loo, 5)]
    stats[1][50] = np.inf
    stats[3][4] = np.inf
    bad_rows, own_row = [37, 50], 60
    if loo:
        stats[5][own_row] = np.inf
    sn = EN.normalise_trials_numpy(s, spk, *stats)
    bad = ~np.isfinite(sn)
    expect = np.isin(np.arange(N), bad_rows)[:, None] | (np.arange(S) == 4)[None, :]
    if loo:   # the own cell takes the own pair: model 4's +inf does not reach its own rows' target trials, row 60's own cell is lost
        expect &= ~(tg & (np.arange(S) == 4)[None, :]) | np.isin(np.arange(N), bad_rows)[:, None]
        expect |= tg & (np.arange(N) == own_row)[:, None]
    assert np.array_equal(bad, expect) and np.isinf(sn[50]).any()
    got = MC.geo_sums(q, spk, sums, msum, count, EUC, loo, abt, stats)
    assert got[0, 1] == (bad & tg).sum() and got[1, 1] == (bad & ~tg).sum() and got[:, :2].sum() == N * S
    R.assert_sums_close(got, sn, tg, *abt, what="non-finite normalised loo %d" % loo)
    # the remaining sums are those of the trials left
    rest = got.copy()
    rest[:, 1] = 0
    R.assert_sums_close(rest, sn[~bad], tg[~bad], *abt, what="the trials left")


# ---- 5. determinism and shards -------------------------------------------------------------------------------------------------------------
def test_runs_are_bit_identical_and_shards_sum_to_the_single_call():
    emb, spk = MC.clusters(300, 64, 37, 5)
    S, abt, loo = 37, MC.ABT[0], True
    sums, msum, count = _speaker_sums(emb, spk, S, COS)
    s, trial = MC.device_scores(emb, spk, sums, msum, count, COS, loo)
    stats = MC.synthetic_stats(s, trial, loo, 9)
    sn = EN.normalise_trials_numpy(s, spk, *stats)
    tg = MC.target_mask(spk, S)
    for st, sc in ((None, s), (stats, sn)):
        cut = lambda lo, hi: None if st is None else tuple(t if k in (2, 3) else t[lo:hi] for k, t in enumerate(st))
        one = MC.geo_sums(emb, spk, sums, msum, count, COS, loo, abt, st)
        again = MC.geo_sums(emb, spk, sums, msum, count, COS, loo, abt, st)
        assert np.array_equal(one.view(np.uint64), again.view(np.uint64))
        tot, bound = np.zeros((2, 8)), np.zeros((2, 8))
        for lo, hi in ((0, 100), (100, 163), (163, 300)):
            part = MC.geo_sums(emb[lo:hi], spk[lo:hi], sums, msum, count, COS, loo, abt, cut(lo, hi))
            bound += R.assert_sums_close(part, sc[lo:hi][trial[lo:hi]], tg[lo:hi][trial[lo:hi]], *abt, what="shard %d:%d" % (lo, hi))[1]
            tot += part
        ref, full = R.assert_sums_close(one, sc[trial], tg[trial], *abt, what="single call")
        assert np.array_equal(tot[:, :2], one[:, :2])
        # each shard is within its own bound, and adding three numbers rounds twice
        assert np.all(np.abs(tot - ref) <= bound + 2 * R.U * np.abs(ref)) and np.all(bound[:, 2:] <= full[:, 2:])
    # the API's rows= is such a shard, and the default is all of them
    cache = _cache(emb, spk)
    models = EN.enrol(cache, "cosine")
    lab = models.labels_of(spk)
    direct = lambda lo, hi: MC.geo_sums(emb[lo:hi], lab[lo:hi], models.sums, models.msum, models.count, COS, True, abt)
    assert np.array_equal(EN.model_calib_sums(models, cache, *abt).view(np.uint64), direct(0, 300).view(np.uint64))
    assert np.array_equal(EN.model_calib_sums(models, cache, *abt, rows=(100, 163)).view(np.uint64), direct(100, 163).view(np.uint64))
    with pytest.raises(Exception, match="must be finite"):
        MC.geo_sums(emb, spk, sums, msum, count, COS, loo, (float("nan"), 0.0, 0.0))
    zero = MC.geo_sums(emb, spk, sums, msum, count, COS, loo, abt, M=0)   # M == 0 writes zeros
    assert not zero.any()


# ---- 6. the fit and the costs ------------------------------------------------------------------------------------------------------------
def _fit_case(name):
    """(models of the enrolled half, the test half's cache, its device scores, trial mask and target mask)."""
    if name == "plda":
        model, rows, spk = MC.plda_case(63, 11, N=600, speakers=24, noise=3.0)   # wide within-speaker noise: the classes overlap
        enrolled, test = _cache(rows[:300], spk[:300]), _cache(rows[300:], spk[300:])
        models = EN.enrol(enrolled, plda=model)
    else:
        emb, spk = MC.clusters(600, 64, 24, 13, noise=2.0)
        enrolled, test = _cache(emb[:300], spk[:300]), _cache(emb[300:], spk[300:])
        models = EN.enrol(enrolled, name)
    return models, enrolled, test


def _api_scores(models, cache, loo):
    q, q_label, loo, _, _, _ = EN._shard(models, cache, loo, (0, cache.n))
    s = EN._identify(q, q_label, *models.backend, loo, return_scores=True)["scores"].cpu().numpy()
    ql = q_label.cpu().numpy()
    return s, ~np.isnan(s), MC.target_mask(ql, models.S), ql


@pytest.mark.parametrize("name", ["euclidean", "cosine", "plda"])
def test_fit_cllr_and_costs_equal_numpy_on_the_device_scores(name):
    models, enrolled, test = _fit_case(name)
    s, trial, tg, _ = _api_scores(models, enrolled, None)     # the enrolled set's own leave-one-out trials
    for prior in (0.5, 0.05):
        cal = EN.fit_model_calibration(models, enrolled, prior=prior)
        ref = C.fit_calibration_numpy(s[trial], tg[trial], prior=prior)
        print("%s prior %g: a %.6f b %.6f, %d iterations, %d passes; numpy a %.6f b %.6f" % (name, prior, cal.a, cal.b, cal.iterations,
                                                                                            cal.passes, ref.a, ref.b))
        assert cal.converged and cal.a < 0 and 0 < cal.cllr_train < 1
        assert (cal.trials, cal.score, cal.normalised) == ("model", models.distance, False)
        assert abs(ref.a - cal.a) < 1e-6 and abs(ref.b - cal.b) < 1e-6
    st, tt, tgt, tql = _api_scores(models, test, None)        # judged on other data: the test half against the same models
    want = C.cllr_of(EN.model_calib_sums_numpy(st, tt, tql, cal.a, cal.b, 0.0))
    assert abs(EN.model_cllr(models, test, cal) - want) < 1e-12
    costs = EN.model_detection_costs(models, test, cal, POINTS)
    sv, tv = st[tt], tgt[tt]
    for g, r_ in zip([{k: v for k, v in d.items() if "act" not in k} for d in costs], V.sorted_dcf(sv, tv, POINTS)):
        for k in r_:
            assert g[k] == r_[k], (k, g, r_)
    for pt, d in zip(POINTS, costs):
        t = d["act_threshold"]
        assert t == V.bayes_threshold(cal, pt) == float(np.float32(t))
        far, frr = float((sv[~tv] < t).sum()) / (~tv).sum(), float((sv[tv] >= t).sum()) / tv.sum()
        assert (d["far_at_act"], d["frr_at_act"]) == (far, frr)
        assert d["act_dcf"] == V.dcf_value(pt, far, frr) and d["act_dcf"] >= d["min_dcf"]
    flat = C.Calibration(0.0, 0.0, 0.05, models.distance, False, 0, True, 0.0, 0.0, trials="model")
    with pytest.raises(ValueError, match="not negative"):
        EN.model_detection_costs(models, test, flat, POINTS)
    with pytest.raises(ValueError, match="pair trials, not model trials"):
        EN.model_cllr(models, test, C.Calibration(-1.0, 0.0, 0.05, models.distance, False, 0, True, 0.0, 0.0))


def test_the_normalised_fit_uses_the_normalised_scores():
    emb, spk = MC.clusters(700, 64, 24, 17, noise=2.0)
    enrolled, cohort = _cache(emb[:400], spk[:400]), _cache(emb[400:], spk[400:] + 100)
    models = EN.enrol(enrolled, "cosine")
    norm = EN.model_score_norm(models, enrolled, cohort, top_k=40)
    s, trial, tg, ql = _api_scores(models, enrolled, None)
    sn = EN.normalise_trials_numpy(s, ql, *[t.cpu().numpy() for t in norm.stats()])
    cal = EN.fit_model_calibration(models, enrolled, prior=0.05, norm=norm)
    ref = C.fit_calibration_numpy(sn[trial], tg[trial], prior=0.05)
    assert cal.normalised and cal.converged and abs(ref.a - cal.a) < 1e-6 and abs(ref.b - cal.b) < 1e-6
    with pytest.raises(ValueError, match="fitted on normalised scores"):
        EN.model_cllr(models, enrolled, cal)
    assert abs(EN.model_cllr(models, enrolled, cal, norm=norm) - cal.cllr_train) < 1e-12


# ---- 7. two ranks --------------------------------------------------------------------------------------------------------------------------
_TWO_RANK = r"""
import json, sys
sys.path.insert(0, {root!r})
import numpy as np, torch
from voicemap_amd import parallel, enrolment as EN
from voicemap_amd.retrieval import EmbeddingCache
rank, world, _ = parallel.init_distributed(timeout_s=120)
torch.cuda.set_device(0)
r = np.random.default_rng(4)
spk = r.integers(0, 13, 1001)
emb = (r.normal(0, 1, (13, 32))[spk] + r.normal(0, 1.5, (1001, 32))).astype(np.float32)
cache = EmbeddingCache(torch.as_tensor(emb).cuda(), spk)
models = EN.enrol(cache, "cosine")
cal = EN.fit_model_calibration(models, cache, prior=0.05)
costs = EN.model_detection_costs(models, cache, cal, [(0.01, 1, 1)])
sums = EN.model_calib_sums(models, cache, cal.a, cal.b, 0.0)   # a collective: every rank calls it
if rank == 0:
    print("RESULT " + json.dumps({{"a": cal.a, "b": cal.b, "converged": cal.converged, "passes": cal.passes,
                                  "sums": sums.tolist(), "costs": costs}}))
"""


def test_two_rank_gloo_run_fits_the_same_calibration(tmp_path):
    script = tmp_path / "two_rank.py"
    script.write_text(_TWO_RANK.format(root=ROOT))
    env = dict(os.environ, VOICEMAP_DIST_BACKEND="gloo", MASTER_PORT="29753")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", str(script)], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    two = json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    r = np.random.default_rng(4)
    spk = r.integers(0, 13, 1001)
    emb = (r.normal(0, 1, (13, 32))[spk] + r.normal(0, 1.5, (1001, 32))).astype(np.float32)
    cache = _cache(emb, spk)
    models = EN.enrol(cache, "cosine")
    cal = EN.fit_model_calibration(models, cache, prior=0.05)
    # the two ranks' sums add in another order than one call's: the same minimiser within the stopping rule, the same exact costs
    assert two["converged"] and cal.converged and abs(two["a"] - cal.a) < 1e-6 and abs(two["b"] - cal.b) < 1e-6
    s, trial, tg, _ = _api_scores(models, cache, None)
    R.assert_sums_close(np.array(two["sums"]), s[trial], tg[trial], two["a"], two["b"], 0.0, what="two ranks")
    R.assert_sums_close(EN.model_calib_sums(models, cache, two["a"], two["b"], 0.0), s[trial], tg[trial], two["a"], two["b"], 0.0, what="one rank")
    cal2 = C.Calibration(two["a"], two["b"], 0.05, "cosine", False, 0, True, 0.0, 0.0, trials="model")
    assert two["costs"] == EN.model_detection_costs(models, cache, cal2, [(0.01, 1, 1)])


# ---- 8. the script -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [(), ("--backend", "plda", "--lda-dim", "8", "--score-norm", "as-norm", "--top-k", "50")])
def test_experiment_script_calibrates_and_reports_act_dcf(extra):
    """--test-set synthetic-test --calibrate --dcf 0.01 end to end in a process of its own; then the same evaluation by hand: the row's
    actDCF is model_trial_accuracy_at_threshold's cost at the Bayes threshold of the printed (a, b)."""
    out = subprocess.run([sys.executable, "-m", "experiments.speaker_identification", "--synthetic", "--n-seconds", "1", "--test-set",
                          "synthetic-test", "--calibrate", "--dcf", "0.01", *extra], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    row = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    new = ["calib_a", "calib_b", "calib_prior", "calib_converged", "calib_iterations", "calib_passes", "enrol_cllr", "test_cllr",
           "trial_min_dcf_p0.01", "trial_min_dcf_threshold_p0.01", "test_act_dcf_p0.01", "test_act_threshold_p0.01", "test_far_at_act_p0.01",
           "test_frr_at_act_p0.01"]
    keys = list(row)
    assert keys[keys.index("test_frr") + 1:keys.index("test_frr") + 1 + len(new)] == new
    assert row["calib_prior"] == 0.5 and row["calib_passes"] >= 2 and row["enrol_cllr"] > 0 and row["test_cllr"] > 0
    assert (row["distance"] == "plda") == bool(extra) and ("score_norm" in row) == bool(extra)
    if not row["calib_a"] < 0:   # the script said so and the minimum cost stands alone
        assert "no actDCF" in out.stdout and row["test_act_dcf_p0.01"] != row["test_act_dcf_p0.01"]
        return
    assert 0 <= row["trial_min_dcf_p0.01"] <= row["test_act_dcf_p0.01"]
    # by hand: the script's own seeded model and generated sets, in the script's order
    from experiments._common import setup
    from experiments.verification_accuracy import cohort_subset
    from voicemap_amd import models as VM, retrieval
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    from voicemap_amd.utils import BatchPreProcessor, preprocess_instances
    setup()
    mk = lambda seed, name: SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=1.0, stochastic=False, seed=seed, subset=name)
    enrol_set, test_set = mk(1, "synthetic-enrol"), mk(1, "synthetic-test")
    enc = VM.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    net = VM.build_siamese_net(enc, (16000 // 4, 1), distance_metric="uniform_euclidean")
    pre = BatchPreProcessor("siamese", preprocess_instances(4))
    kw = {}
    if extra:
        kw = dict(backend="plda", plda_train=mk(4, "synthetic-train"), lda_dim=8, score_norm="as-norm", top_k=50,
                  cohort=cohort_subset(mk(3, "synthetic-cohort"), 5000))
    ce, ct = (retrieval.embed_corpus(net, d, pre, "siamese") for d in (enrol_set, test_set))
    nt = None
    if extra:
        from voicemap_amd import plda
        back = plda.fit_plda(retrieval.embed_corpus(net, kw["plda_train"], pre, "siamese"), lda_dim=8)
        ce, ct = back.project(ce), back.project(ct)
        models = EN.enrol(ce, plda=back)
        nt = EN.model_score_norm(models, ct, back.project(retrieval.embed_corpus(net, kw["cohort"], pre, "siamese")), top_k=50)
    else:
        models = EN.enrol(ce, "euclidean")
    cal = types.SimpleNamespace(a=row["calib_a"], b=row["calib_b"])
    t = V.bayes_threshold(cal, (0.01, 1, 1))
    at = EN.model_trial_accuracy_at_threshold(models, ct, t, norm=nt)
    assert row["test_act_threshold_p0.01"] == t
    assert row["test_act_dcf_p0.01"] == V.dcf_value((0.01, 1.0, 1.0), at["far"], at["frr"])
    assert (row["test_far_at_act_p0.01"], row["test_frr_at_act_p0.01"]) == (at["far"], at["frr"])
