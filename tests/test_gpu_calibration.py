"""-m gpu checks of score calibration and detection costs (vm_pair_calib_sums, voicemap_amd/calibration.py, the dcf_points of
verification.py).  The numpy side takes its scores from vm_pairdist_argmin on the device, as test_gpu_verification.py does, so only the
new epilogue and reduction are under test: the counts are exact, the sums that are exact in float64 (integer scores at a = b = tau = 0)
equal numpy bit for bit, and every other sum lies within the rounding count of tests/calib_refs.py around an extended-precision
reference.  Every device call here runs with guard words around its result and its workspace."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import calib_refs as R
from tests.gpu_util import L, p, stream
from voicemap_amd import calibration as C
from voicemap_amd import verification as V
from voicemap_amd.retrieval import EmbeddingCache

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64 here")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUC, COS, DOT, WL1, NEG = 0, 1, 2, 3, 4
POINTS = [(0.5, 1, 1), (0.01, 1, 1), (0.001, 1, 1), (0.05, 10, 1)]
# moderate; a = 0; saturating (|z| > 750: exp underflows); |z| about 40
ABT = [(-0.3, 1.0, -0.5), (0.0, 0.3, 0.7), (-0.25, 1000.0, 0.0), (-0.01, 40.0, 1.5)]
GUARD_D, GUARD_F = -1.2345e300, -7.75e30


def _sums(emb, spk, kind, rows, abt=(0.0, 0.0, 0.0), weights=None, mu=None, rsig=None):
    """vm_pair_calib_sums on host arrays, with guard words before and after ``sums`` and the workspace (of exactly the queried size)."""
    N, E = emb.shape
    x = torch.as_tensor(np.ascontiguousarray(emb, np.float32)).cuda()
    lab = torch.as_tensor(np.asarray(spk, np.int32)).cuda()
    dv = lambda v: None if v is None else torch.as_tensor(np.asarray(v, np.float32)).cuda()
    w, m, rs = dv(weights), dv(mu), dv(rsig)
    out = torch.full((4 + 16 + 4,), GUARD_D, dtype=torch.float64, device="cuda")
    words = (L().query("vm_pair_calib_sums_workspace_bytes", N, E) + 3) // 4
    ws = torch.full((8 + words + 8,), GUARD_F, dtype=torch.float32, device="cuda")
    L().call("vm_pair_calib_sums", p(x), p(lab), N, E, kind, p(w), rows[0], rows[1], p(m), p(rs), float(abt[0]), float(abt[1]),
             float(abt[2]), out.data_ptr() + 32, ws.data_ptr() + 32, stream())
    o, g = out.cpu().numpy(), ws.cpu().numpy()
    assert np.all(o[:4] == GUARD_D) and np.all(o[20:] == GUARD_D), "words around sums were written"
    assert np.all(g[:8] == np.float32(GUARD_F)) and np.all(g[8 + words:] == np.float32(GUARD_F)), "words around the workspace were written"
    return o[4:20].reshape(2, 8).copy()


_DIST = {}


def _dist(emb, kind):
    """vm_pairdist_argmin's (N, N) fp32 matrix of an embedding matrix (computed once per matrix and kind, never modified)."""
    key = (kind, emb.shape, hash(emb.tobytes()))
    if key not in _DIST:
        N, E = emb.shape
        x = torch.as_tensor(np.ascontiguousarray(emb, np.float32)).cuda()
        ws = torch.empty(L().query("vm_pairdist_workspace_bytes", N, N) // 4 + 16, device="cuda")
        d = torch.empty(N, N, device="cuda")
        bv = torch.empty(N, device="cuda")
        bi = torch.empty(N, dtype=torch.int32, device="cuda")
        L().call("vm_pairdist_argmin", p(x), p(x), N, N, E, kind, 0, p(d), p(bv), p(bi), p(ws), stream())
        torch.cuda.synchronize()
        d = d.cpu().numpy()
        d.setflags(write=False)
        _DIST.clear()   # one matrix at a time is kept
        _DIST[key] = d
    return _DIST[key]


def _trials(emb, spk, kind, rows, weights=None):
    """(scores, target mask, i, j) of the trials of the row range, from the device's own score matrix (NEG: its negation; WL1, on grid
    inputs whose fmaf chain is exact: float64 numpy rounded once)."""
    N = len(spk)
    i, j = np.triu_indices(N, 1)
    keep = (i >= rows[0]) & (i < rows[1])
    i, j = i[keep], j[keep]
    if kind == WL1:
        s = (np.abs(emb[i].astype(np.float64) - emb[j]) * np.asarray(weights, np.float64)).sum(1).astype(np.float32)
    elif kind == NEG:
        s = -_dist(emb, EUC)[i, j]
    else:
        s = _dist(emb, kind)[i, j]
    return s, spk[i] == spk[j], i, j


def _clusters(N, E, seed, speakers=7, grid=None):
    r = np.random.default_rng(seed)
    spk = r.integers(0, speakers, N)
    emb = r.normal(0, 1, (speakers, E))[spk] + r.normal(0, 1.0, (N, E))
    if grid:
        emb = np.round(emb * grid) / grid
    return emb.astype(np.float32), spk


def _cache(emb, spk):
    return EmbeddingCache(torch.as_tensor(np.ascontiguousarray(emb, np.float32)).cuda(), np.asarray(spk))


# ---- the exact plant -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 64, 65, 129, 300])
def test_integer_scores_at_zero_give_the_exact_sums(N):
    """Components in {-2 .. 2}, dot product, a = b = tau = 0: p = 1/2 and w = 1/4 exactly and every score is a small integer, so every
    sum but L is exact in float64 in any order and must equal numpy's bit for bit; L (n log1p(1)) lies within the rounding bound."""
    for E in (1, 3, 4, 64, 67, 256):
        r = np.random.default_rng(N * 1000 + E)
        emb = r.integers(-2, 3, (N, E)).astype(np.float32)
        some = r.integers(1, 6, N)
        some[0] = 0                                      # a singleton speaker
        for spk in (some, np.zeros(N, np.int64)):        # ... and one speaker holding every row: no non-targets
            for rows in ((0, N), (0, 1), (N - 1, N), (min(37, N - 1), min(101, N))):
                s, tg, _, _ = _trials(emb, spk, DOT, rows)
                got = _sums(emb, spk, DOT, rows)
                ref = C.calib_sums_numpy(s, tg, 0.0, 0.0, 0.0)
                assert np.array_equal(got[:, [0, 1, 3, 4, 5, 6, 7]], ref[:, [0, 1, 3, 4, 5, 6, 7]]), (E, rows, got, ref)
                assert got[:, 0].sum() == len(s) and (rows != (N - 1, N) or not got.any())
                R.assert_sums_close(got, s, tg, 0.0, 0.0, 0.0, what="plant N=%d E=%d rows=%r" % (N, E, rows))


def test_a_grid_whose_splits_hold_two_tiles_each():
    """N = 8192, E = 8: 128 query blocks x 32 splits = 4096 workgroups, and block 0's 64 reference tiles make two per split -- the
    smallest triangle in which a workgroup carries its accumulators from one tile to the next."""
    N, E = 8192, 8
    blocks, splits, most = C.plan_splits(N, (0, N))
    assert (blocks, splits) == (128, 32) and most >= 2
    assert C.plan_splits(4096, (0, 4096))[2] == 1   # the next smaller power of two: one tile per split
    r = np.random.default_rng(1)
    emb = r.integers(-2, 3, (N, E)).astype(np.float32)
    spk = r.integers(0, 40, N)
    got = _sums(emb, spk, DOT, (0, N))
    d = _dist(emb, DOT)
    cnt = np.zeros(2)
    s1, s2 = np.zeros(2), np.zeros(2)
    for lo in range(0, N, 1024):   # integer sums over the upper triangle by class: exact in float64
        blk = d[lo:lo + 1024].astype(np.float64)
        up = np.arange(N)[None, :] > np.arange(lo, lo + 1024)[:, None]
        same = spk[lo:lo + 1024, None] == spk[None, :]
        for c, m in enumerate((up & same, up & ~same)):
            cnt[c] += m.sum()
            s1[c] += blk[m].sum()
            s2[c] += (blk[m] ** 2).sum()
    assert cnt.sum() == N * (N - 1) // 2
    for c in range(2):
        assert got[c, :2].tolist() == [cnt[c], 0.0]
        assert got[c, 3:].tolist() == [cnt[c] / 2, s1[c] / 2, cnt[c] / 4, s1[c] / 4, s2[c] / 4], (c, got)
        ref = cnt[c] * np.log1p(np.longdouble(1))   # L = n log1p(1)
        assert abs(float(np.longdouble(got[c, 2]) - ref)) <= (cnt[c] + R.K["L"]) * R.U * float(ref)


# ---- general scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalised", [False, True])
@pytest.mark.parametrize("kind", [EUC, COS, DOT, WL1, NEG])
def test_sums_of_every_score_kind_lie_within_the_rounding_bound(kind, normalised):
    N, E = 300, 64
    emb, spk = _clusters(N, E, 40 + kind, grid=8 if kind == WL1 else None)   # weighted L1: a dyadic grid, so that numpy's sum is the kernel's
    r = np.random.default_rng(kind)
    w = (2.0 ** r.integers(-3, 2, E)).astype(np.float32) if kind == WL1 else None
    mu = rsig = None
    s, tg, i, j = _trials(emb, spk, kind, (0, N), w)
    if normalised:
        mu = (np.median(s) + r.normal(0, 0.1 * s.std(), N)).astype(np.float32)
        rsig = (1.0 / (s.std() * r.uniform(0.5, 2.0, N))).astype(np.float32)
        s = V.normalise_scores_numpy(s, i, j, mu, rsig)
    assert np.isfinite(s).all()
    for abt in ABT:
        z = abt[0] * s.astype(np.float64) + abt[1] + abt[2]
        assert abt != ABT[2] or np.abs(z).min() > 750
        assert np.abs(z).max() < 700 or np.abs(z).min() > 750   # no term in the denormal range of exp
        got = _sums(emb, spk, kind, (0, N), abt, w, mu, rsig)
        R.assert_sums_close(got, s, tg, *abt, what="kind %d norm %d abt %r" % (kind, normalised, abt))
        assert got[:, 0].sum() == N * (N - 1) // 2 and not got[:, 1].any()


def test_non_finite_scores_are_skipped_and_counted():
    N, E = 200, 64
    emb, spk = _clusters(N, E, 3)
    emb[37] = np.nan                                     # a NaN row: 199 NaN scores
    abt = ABT[0]
    s, tg, i, j = _trials(emb, spk, EUC, (0, N))
    got = _sums(emb, spk, EUC, (0, N), abt)
    assert got[:, 1].sum() == 199 == np.isnan(s).sum()
    R.assert_sums_close(got, s, tg, *abt, what="NaN row")
    # normalised: a row with rsig = +inf (its scores are +-inf), and a row whose normalised scores overflow
    r = np.random.default_rng(0)
    mu = r.normal(8, 1, N).astype(np.float32)
    rsig = r.uniform(0.5, 2, N).astype(np.float32)
    rsig[50] = np.inf
    mu[60], rsig[60] = -3e38, 3e38
    sn = V.normalise_scores_numpy(s, i, j, mu, rsig)
    bad = ~np.isfinite(sn)
    assert np.isinf(sn[(i == 60) | (j == 60)]).any() and bad.sum() >= 199 + 198 + 197
    got = _sums(emb, spk, EUC, (0, N), abt, None, mu, rsig)
    assert got[0, 1] == (bad & tg).sum() and got[1, 1] == (bad & ~tg).sum()
    R.assert_sums_close(got, sn, tg, *abt, what="non-finite normalised")
    # the remaining sums are those of the same call without the three rows' trials
    clean = ~np.isin(i, (37, 50, 60)) & ~np.isin(j, (37, 50, 60))
    assert np.array_equal(bad, ~clean)
    rest = got.copy()
    rest[:, 1] = 0
    R.assert_sums_close(rest, sn[clean], tg[clean], *abt, what="without the rows")


def test_runs_are_bit_identical_and_shards_sum_to_the_single_call():
    N, E = 300, 64
    emb, spk = _clusters(N, E, 5)
    abt = ABT[0]
    one = _sums(emb, spk, COS, (0, N), abt)
    assert np.array_equal(one.view(np.uint64), _sums(emb, spk, COS, (0, N), abt).view(np.uint64))
    tot, bound = np.zeros((2, 8)), np.zeros((2, 8))
    for rows in V.triangle_shards(N, 3):
        s, tg, _, _ = _trials(emb, spk, COS, rows)
        part = _sums(emb, spk, COS, rows, abt)
        bound += R.assert_sums_close(part, s, tg, *abt, what="shard %r" % (rows,))[1]
        tot += part
    s, tg, _, _ = _trials(emb, spk, COS, (0, N))
    ref, full = R.assert_sums_close(one, s, tg, *abt, what="single call")
    assert np.array_equal(tot[:, :2], one[:, :2])
    # each shard is within its own bound, and adding three numbers rounds twice
    assert np.all(np.abs(tot - ref) <= bound + 2 * R.U * np.abs(ref)) and np.all(bound[:, 2:] <= full[:, 2:])
    with pytest.raises(Exception, match="bad row range"):
        _sums(emb, spk, COS, (10, N + 1), abt)


# ---- the fit, the costs, the script --------------------------------------------------------------------------------------------------
def test_fit_reaches_a_point_where_the_numpy_gradient_vanishes():
    emb, spk = _clusters(300, 64, 6)
    cache = _cache(emb, spk)
    s, tg, _, _ = _trials(emb, spk, EUC, (0, 300))
    for prior in (0.5, 0.05):
        cal = C.fit_calibration(cache, prior=prior)
        assert cal.converged and cal.a < 0 and cal.iterations <= 50 and 0 < cal.cllr_train < 1 and not cal.normalised
        Cv, g, H = C.objective_terms(C.calib_sums_numpy(s, tg, cal.a, cal.b, C.logit(prior)), prior)
        lam = math.sqrt(C.newton_decrement2(g, H))   # the gradient in the norm of the stopping rule (test_calibration_cpu.py)
        print("fit prior %g: a %.6f b %.6f, %d iterations, %d passes, numpy decrement %.3g" % (prior, cal.a, cal.b, cal.iterations, cal.passes, lam))
        assert lam < 10 * cal.stop
        assert abs(Cv - cal.objective) < 1e-12
        ref = C.fit_calibration_numpy(s, tg, prior=prior)
        assert abs(ref.a - cal.a) < 1e-6 and abs(ref.b - cal.b) < 1e-6
        assert abs(C.cllr(cache, cal) - C.cllr_of(C.calib_sums_numpy(s, tg, cal.a, cal.b, 0.0))) < 1e-12


_TWO_RANK = r"""
import json, sys
sys.path.insert(0, {root!r})
import numpy as np, torch
from voicemap_amd import calibration as C, parallel, verification as V
from voicemap_amd.retrieval import EmbeddingCache
rank, world, _ = parallel.init_distributed(timeout_s=120)
torch.cuda.set_device(0)
r = np.random.default_rng(4)
spk = r.integers(0, 13, 1000)
emb = (r.normal(0, 1, (13, 64))[spk] + r.normal(0, 1, (1000, 64))).astype(np.float32)
cache = EmbeddingCache(torch.as_tensor(emb).cuda(), spk)
cal = C.fit_calibration(cache, prior=0.05)
costs = V.detection_costs(cache, cal, [(0.01, 1, 1)])
sums = C.calib_sums(cache, cal.a, cal.b, 0.0)   # a collective: every rank calls it
if rank == 0:
    print("RESULT " + json.dumps({{"a": cal.a, "b": cal.b, "converged": cal.converged, "passes": cal.passes,
                                  "sums": sums.tolist(), "costs": costs}}))
"""


def test_two_rank_gloo_run_fits_the_same_calibration(tmp_path):
    import json
    import subprocess
    script = tmp_path / "two_rank.py"
    script.write_text(_TWO_RANK.format(root=ROOT))
    env = dict(os.environ, VOICEMAP_DIST_BACKEND="gloo", MASTER_PORT="29741")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", str(script)], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    two = json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    r = np.random.default_rng(4)
    spk = r.integers(0, 13, 1000)
    emb = (r.normal(0, 1, (13, 64))[spk] + r.normal(0, 1, (1000, 64))).astype(np.float32)
    cache = _cache(emb, spk)
    cal = C.fit_calibration(cache, prior=0.05)
    # the two ranks' sums add in another order than one call's: the same minimiser within the stopping rule, the same exact costs
    assert two["converged"] and cal.converged and abs(two["a"] - cal.a) < 1e-6 and abs(two["b"] - cal.b) < 1e-6
    one = C.calib_sums(cache, two["a"], two["b"], 0.0)
    s, tg, _, _ = _trials(emb, spk, EUC, (0, 1000))
    R.assert_sums_close(np.array(two["sums"]), s, tg, two["a"], two["b"], 0.0, what="two ranks")
    R.assert_sums_close(one, s, tg, two["a"], two["b"], 0.0, what="one rank")
    cal2 = types.SimpleNamespace(a=two["a"], b=two["b"], score="euclidean", normalised=False)
    assert two["costs"] == V.detection_costs(cache, cal2, [(0.01, 1, 1)])


def _assert_dcf_equal(got, ref):
    assert len(got) == len(ref)
    for g, r_ in zip(got, ref):
        for k in r_:
            assert g[k] == r_[k], (k, g, r_)


def test_minimum_costs_equal_the_sort_of_pairdist_scores():
    r = np.random.default_rng(5)   # the lattice of test_gpu_verification.py's ties test
    spk = r.integers(0, 6, 800)
    emb = (r.integers(-1, 2, (800, 64)) + 2 * (spk[:, None] == np.arange(64)[None, :] % 6)).astype(np.float32)
    for dist, kind in (("euclidean", EUC), ("dot_product", DOT)):
        s, tg, _, _ = _trials(emb, spk, kind, (0, 800))
        _assert_dcf_equal(V.verification_metrics(_cache(emb, spk), dist, dcf_points=POINTS)["dcf"], V.sorted_dcf(s, tg, POINTS))
    emb, spk = _clusters(700, 64, 12, speakers=20)
    s, tg, _, _ = _trials(emb, spk, COS, (0, 700))
    m = V.verification_metrics(_cache(emb, spk), "cosine", dcf_points=POINTS)
    _assert_dcf_equal(m["dcf"], V.sorted_dcf(s, tg, POINTS))
    ref = V.sorted_metrics(s, tg)
    assert (m["eer"], m["best_threshold"]) == (ref["eer"], ref["best_threshold"]) and m["dcf"][0]["min_dcf_threshold"] == m["best_threshold"]


def test_act_dcf_is_the_cost_counted_at_the_bayes_threshold():
    emb, spk = _clusters(600, 64, 13, speakers=12)
    valid, test = _cache(emb[:300], spk[:300]), _cache(emb[300:], spk[300:])
    cal = C.fit_calibration(valid, prior=0.05, score="cosine")
    s, tg, _, _ = _trials(emb[300:], spk[300:], COS, (0, 300))
    costs = V.detection_costs(test, cal, POINTS)
    _assert_dcf_equal([{k: v for k, v in d.items() if "act" not in k} for d in costs], V.sorted_dcf(s, tg, POINTS))
    for pt, d in zip(POINTS, costs):
        t = d["act_threshold"]
        assert t == V.bayes_threshold(cal, pt) == float(np.float32(t))
        far, frr = float((s[~tg] < t).sum()) / (~tg).sum(), float((s[tg] >= t).sum()) / tg.sum()
        assert (d["far_at_act"], d["frr_at_act"]) == (far, frr)
        assert d["act_dcf"] == V.dcf_value(pt, far, frr) and d["act_dcf"] >= d["min_dcf"]
    flat = types.SimpleNamespace(a=0.0, b=0.0, score="cosine", normalised=False)
    with pytest.raises(ValueError, match="not negative"):
        V.detection_costs(test, flat, POINTS)


def test_experiment_script_calibrates_and_reports_act_dcf():
    import importlib
    sys.path.insert(0, ROOT)
    ex = importlib.import_module("experiments.verification_accuracy")
    res = ex.main(["--synthetic", "--n-seconds", "1", "--calibrate", "--dcf", "0.01"]).iloc[0]   # end to end: arguments, both sets, the CSV
    assert os.path.exists(os.path.join(ROOT, "logs", "verification_accuracy_synthetic_synthetic_euclidean_dcf_calib.csv"))
    assert res["calib_a"] < 0 and 0 < res["test_cllr"] and 0 <= res["test_min_dcf_p0.01"] <= res["test_act_dcf_p0.01"]
    # its actDCF is accuracy_at_threshold's cost at the Bayes threshold of the validation set's calibration
    from voicemap_amd import models, retrieval
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    from voicemap_amd.utils import BatchPreProcessor, preprocess_instances
    valid = SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=1, stochastic=False, seed=1)
    test = SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=1, stochastic=False, seed=2)
    enc = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (4000, 1), distance_metric="uniform_euclidean")
    pre = BatchPreProcessor("siamese", preprocess_instances(4))
    res = ex.evaluate(net, valid, test, pre, "euclidean", dcf=[0.01], calibrate=True, calib_prior=0.5)
    assert res["calib_a"] < 0 and res["calib_converged"]
    ct = retrieval.embed_corpus(net, test, pre)
    cal = types.SimpleNamespace(a=float(res["calib_a"]), b=float(res["calib_b"]), score="euclidean", normalised=False)
    t = V.bayes_threshold(cal, (0.01, 1, 1))
    at = V.accuracy_at_threshold(ct, t)
    assert res["test_act_threshold_p0.01"] == t
    assert res["test_act_dcf_p0.01"] == V.dcf_value((0.01, 1.0, 1.0), at["far"], at["frr"])
