"""-m gpu checks of cohort score normalisation (vm_cohort_topk_stats, vm_pair_score_hist_norm, verification.score_norm / norm=): the
selection equals numpy's lexsort of the keys of vm_pairdist_argmin's own scores, the statistics are float64 statistics of the selected
scores rounded once, the normalised histogram equals numpy's binning of the twin-normalised scores AS INTEGERS, the exact metrics equal
the sort-based definition on those scores, and the two-rank run and the experiment script agree."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import L, p, stream
from voicemap_amd import verification as V
from voicemap_amd.retrieval import EmbeddingCache

pytestmark = pytest.mark.gpu
DIST = {"euclidean": 0, "cosine": 1, "dot_product": 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cache(emb, spk):
    return EmbeddingCache(torch.as_tensor(np.ascontiguousarray(emb, np.float32)).cuda(), np.asarray(spk))


def _pairdist(q, ref, dist):
    """vm_pairdist_argmin's (M, N) fp32 score matrix."""
    M, E = q.shape
    N = ref.shape[0]
    x, y = torch.as_tensor(q).cuda(), torch.as_tensor(ref).cuda()
    ws = torch.empty(L().query("vm_pairdist_workspace_bytes", M, N) // 4 + 16, device="cuda")
    d = torch.empty(M, N, device="cuda")
    bv = torch.empty(M, device="cuda")
    bi = torch.empty(M, dtype=torch.int32, device="cuda")
    L().call("vm_pairdist_argmin", p(x), p(y), M, N, E, DIST[dist], -1, p(d), p(bv), p(bi), p(ws), stream())
    return d.cpu().numpy()


def _stats(q, cohort, kind, K, self_row0=-1, weights=None):
    mu, sig, rsig, cnt, topk = V.cohort_topk_stats(torch.as_tensor(q).cuda(), torch.as_tensor(cohort).cuda(), kind,
                                                   None if weights is None else torch.as_tensor(weights).cuda(), K, self_row0,
                                                   return_topk=True)
    return mu.cpu().numpy(), sig.cpu().numpy(), rsig.cpu().numpy(), cnt.cpu().numpy(), topk.cpu().numpy()


def _ulp_close(got, ref64):
    """|got - fp32(ref64)| <= 1 fp32 ulp at every finite entry; NaN where the reference is NaN."""
    ref = ref64.astype(np.float32)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    sp = np.spacing(np.abs(ref[~nan])).astype(np.float64)
    assert np.all(np.abs(got[~nan].astype(np.float64) - ref64[~nan]) <= sp), np.max(np.abs(got[~nan] - ref[~nan]) / sp)


def _check_rows(s, mu, sig, rsig, cnt, topk, K, self_row0=None):
    idx, c = V.cohort_select_numpy(s, K, self_row0)
    assert np.array_equal(cnt, c)
    assert np.array_equal(topk, idx)
    m64, s64 = np.full(len(s), np.nan), np.full(len(s), np.nan)
    for m in range(len(s)):
        if c[m]:
            v = s[m, idx[m, :c[m]]].astype(np.float64)
            m64[m] = v.mean()
            s64[m] = np.sqrt(((v - v.mean()) ** 2).mean())
    _ulp_close(mu, m64)
    _ulp_close(sig, s64)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal((1.0 / sig.astype(np.float64)).astype(np.float32), rsig, equal_nan=True)


def _rand(n, E, seed):
    r = np.random.default_rng(seed)
    return (r.normal(0, 1, (4, E))[r.integers(0, 4, n)] + r.normal(0, 1, (n, E))).astype(np.float32)


@pytest.mark.parametrize("dist", ["euclidean", "cosine", "dot_product"])
@pytest.mark.parametrize("M,C", [(1, 1), (63, 2), (64, 63), (65, 64), (1000, 65), (64, 4099), (65, 32768)])
def test_selection_and_statistics_equal_numpy_on_pairdist_scores(M, C, dist):
    for E in (64, 100, 256):
        if C >= 4099 and E != 100:
            continue
        q, co = _rand(M, E, M + C + E), _rand(C, E, 7 * C + E)
        s = _pairdist(q, co, dist)
        for K in sorted({1, 7, 300, C}):
            if K > C or (C == 32768 and K == C):
                continue
            _check_rows(s, *_stats(q, co, DIST[dist], K), K)


def test_selection_on_a_lattice_with_massive_ties_nan_rows_and_self_exclusion():
    r = np.random.default_rng(3)
    co = r.integers(-1, 2, (500, 64)).astype(np.float32)
    co[[5, 77]] = np.nan
    for dist in ("euclidean", "dot_product"):
        s = _pairdist(co[:200], co, dist)
        assert len(np.unique(s[np.isfinite(s)])) < 100
        for K in (1, 7, 300, 500):
            _check_rows(s, *_stats(co[:200], co, DIST[dist], K, self_row0=0), K, self_row0=0)
            _check_rows(s[50:], *_stats(co[50:200], co, DIST[dist], K, self_row0=50), K, self_row0=50)
    # a query row of NaN: nothing selected
    q = co[:3].copy()
    q[1] = np.nan
    mu, sig, rsig, cnt, topk = _stats(q, co, 0, 10)
    assert cnt[1] == 0 and np.isnan([mu[1], sig[1], rsig[1]]).all() and (topk[1] == -1).all() and cnt[0] == 10


def test_large_cohort_on_the_global_memory_path():
    q, co = _rand(70, 64, 1), _rand(40000, 64, 2)
    s = _pairdist(q, co, "euclidean")
    for K in (300, 5000):
        _check_rows(s, *_stats(q, co, 0, K), K)
    _check_rows(s, *_stats(q, co, 0, 300, self_row0=39950), 300, self_row0=39950)


def test_zero_sigma_gives_infinite_rsig():
    co = np.ones((50, 64), np.float32)
    mu, sig, rsig, cnt, _ = _stats(np.ones((3, 64), np.float32), co, 0, 20)
    assert (mu == 0).all() and (sig == 0).all() and np.isposinf(rsig).all() and (cnt == 20).all()


def test_head_kinds_on_an_exact_lattice():
    r = np.random.default_rng(9)
    E = 100
    q, co = r.integers(-4, 5, (130, E)).astype(np.float32), r.integers(-4, 5, (700, E)).astype(np.float32)
    w = (2.0 ** r.integers(-3, 3, E) * np.where(r.random(E) < 0.2, -1, 1)).astype(np.float32)
    d = q[:, None, :].astype(np.float64) - co[None, :, :]
    wl1 = (np.abs(d) * w).sum(2).astype(np.float32)                         # every partial sum exact in fp32
    neg = (-np.sqrt((d * d).sum(2))).astype(np.float32)                     # an exact integer sum, then one sqrt
    for kind, s, wt in ((V.SCORES["weighted_l1"], wl1, w), (V.VM_SCORE_NEG_EUCLIDEAN, neg, None)):
        for K in (1, 30, 700):
            _check_rows(s, *_stats(q, co, kind, K, weights=wt), K)


def _norm_scores(emb, spk, dist, norm):
    s = _pairdist(emb, emb, dist)
    iu = np.triu_indices(len(emb), 1)
    sn = V.normalise_scores_numpy(s[iu], iu[0], iu[1], norm.mu.cpu().numpy(), norm.rsig.cpu().numpy())
    return sn, spk[iu[0]] == spk[iu[1]]


@pytest.mark.parametrize("dist", ["euclidean", "cosine", "dot_product"])
def test_normalised_histogram_equals_numpy_binning(dist):
    emb, spk = _rand(1100, 64, 4), np.random.default_rng(4).integers(0, 9, 1100)
    cache = _cache(emb, spk)
    norm = V.score_norm(cache, _rand(900, 64, 5), dist, top_k=50)
    sn, tg = _norm_scores(emb, spk, dist, norm)
    f = sn[np.isfinite(sn)]
    lo, hi = float(f.min()), float(f.max())
    coarse = [V.pass1_window(lo, 0.5 * (lo + hi))]
    got = V.score_histogram(cache, dist, coarse, 4096, norm=norm)
    assert np.array_equal(got, V.bin_scores(sn, tg, coarse, 4096))
    b = int(np.argmax(got[0, 0, :4096] + got[0, 1, :4096]))
    k0, sh0 = coarse[0]
    zoom = [(k0 + (b << sh0), max(0, sh0 - 10)), (V.key_of(float(np.median(sn))), 0), (V.key_of(0.5 * (lo + hi)), 31)]
    got = V.score_histogram(cache, dist, zoom, 1024, norm=norm)
    assert np.array_equal(got, V.bin_scores(sn, tg, zoom, 1024))
    # determinism: statistics and histogram bit-identical from run to run
    again = V.score_norm(cache, _rand(900, 64, 5), dist, top_k=50)
    for a, b2 in ((norm.mu, again.mu), (norm.sigma, again.sigma), (norm.rsig, again.rsig), (norm.count, again.count)):
        assert torch.equal(a, b2)
    assert np.array_equal(V.score_histogram(cache, dist, zoom, 1024, norm=again), got)


def _assert_metrics_equal(got, ref):
    for k in ("eer", "eer_threshold", "far_at_eer", "frr_at_eer", "best_balanced_accuracy", "best_threshold", "n_target", "n_nontarget",
              "n_nan"):
        assert got[k] == ref[k], (k, got[k], ref[k])


@pytest.mark.parametrize("dist", ["euclidean", "cosine", "dot_product"])
def test_metrics_equal_sort_of_normalised_scores(dist):
    r = np.random.default_rng(11)
    spk = r.integers(0, 30, 1500)
    emb = (r.normal(0, 1, (30, 64))[spk] + r.normal(0, 1, (1500, 64))).astype(np.float32)
    cache = _cache(emb, spk)
    for top_k, cohort in ((None, _rand(600, 64, 12)), (100, _rand(600, 64, 12)), (100, cache)):
        norm = V.score_norm(cache, cohort, dist, top_k=top_k)
        sn, tg = _norm_scores(emb, spk, dist, norm)
        got = V.verification_metrics(cache, dist, norm=norm)
        _assert_metrics_equal(got, V.sorted_metrics(sn, tg))
        at = V.accuracy_at_threshold(cache, got["best_threshold"], dist, norm=norm)
        assert at["balanced_accuracy"] == got["best_balanced_accuracy"]
    with pytest.raises(ValueError):
        V.verification_metrics(cache, "cosine" if dist != "cosine" else "euclidean", norm=norm)


def test_as_norm_lowers_the_eer_of_miscalibrated_rows():
    """Rows with a random gain and offset: raw euclidean scores are badly calibrated across rows and AS-norm recovers most of it."""
    r = np.random.default_rng(2024)
    S, E = 60, 64
    cent = r.normal(0, 1, (S, E))

    def make(n, seed):
        g = np.random.default_rng(seed)
        spk = g.integers(0, S, n)
        x = cent[spk] + 0.6 * g.normal(0, 1, (n, E))
        x = x * g.uniform(0.3, 3.0, (n, 1)) + g.normal(0, 1.5, (n, 1))
        return x.astype(np.float32), spk

    emb, spk = make(2000, 1)
    cohort, _ = make(3000, 2)
    cache = _cache(emb, spk)
    raw = V.verification_metrics(cache, "euclidean")
    asn = V.verification_metrics(cache, "euclidean", norm=V.score_norm(cache, cohort, "euclidean", top_k=200))
    assert asn["eer"] < raw["eer"] - 0.01, (raw["eer"], asn["eer"])   # seeded and bit-reproducible: 0.323 -> 0.306


_TWO_RANK = r"""
import json, sys
sys.path.insert(0, {root!r})
import numpy as np, torch
from voicemap_amd import parallel, verification as V
from voicemap_amd.retrieval import EmbeddingCache
rank, world, _ = parallel.init_distributed(timeout_s=120)
torch.cuda.set_device(0)
r = np.random.default_rng(4)
spk = r.integers(0, 13, 2001)
emb = (r.normal(0, 1, (13, 64))[spk] + r.normal(0, 1, (2001, 64))).astype(np.float32)
cache = EmbeddingCache(torch.as_tensor(emb).cuda(), spk)
norm = V.score_norm(cache, cache, "euclidean", top_k=100)
m = V.verification_metrics(cache, "euclidean", norm=norm)
m.pop("roc")
if rank == 0:
    print("RESULT " + json.dumps(m))
"""


def test_two_rank_gloo_run_gives_the_same_normalised_metrics(tmp_path):
    script = tmp_path / "two_rank.py"
    script.write_text(_TWO_RANK.format(root=ROOT))
    env = dict(os.environ, VOICEMAP_DIST_BACKEND="gloo", MASTER_PORT="29733")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", str(script)], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    two = json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    r = np.random.default_rng(4)
    spk = r.integers(0, 13, 2001)
    emb = (r.normal(0, 1, (13, 64))[spk] + r.normal(0, 1, (2001, 64))).astype(np.float32)
    cache = _cache(emb, spk)
    one = V.verification_metrics(cache, "euclidean", norm=V.score_norm(cache, cache, "euclidean", top_k=100))
    for k, v in two.items():
        assert v == one[k], k


def test_experiment_script_with_as_norm_matches_accuracy_at_threshold():
    import importlib
    sys.path.insert(0, ROOT)
    ex = importlib.import_module("experiments.verification_accuracy")
    res = ex.main(["--synthetic", "--n-seconds", "1", "--score-norm", "as-norm", "--top-k", "50"]).iloc[0]
    assert res["score_norm"] == "as-norm" and res["top_k"] == 50 and res["cohort_size"] == 160
    assert os.path.exists(os.path.join(ROOT, "logs", "verification_accuracy_synthetic_synthetic_euclidean_asnorm_k50_c5000.csv"))
    from voicemap_amd import models, retrieval
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    from voicemap_amd.utils import BatchPreProcessor, preprocess_instances
    mk = lambda seed: SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=1, stochastic=False, seed=seed)
    enc = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (4000, 1), distance_metric="uniform_euclidean")
    pre = BatchPreProcessor("siamese", preprocess_instances(4))
    row = ex.evaluate(net, mk(1), mk(2), pre, "euclidean", "as-norm", mk(3), 50)
    cv, ct, cc = (retrieval.embed_corpus(net, d, pre) for d in (mk(1), mk(2), mk(3)))
    mv = V.verification_metrics(cv, "euclidean", norm=V.score_norm(cv, cc, "euclidean", top_k=50))
    nt = V.score_norm(ct, cc, "euclidean", top_k=50)
    at = V.accuracy_at_threshold(ct, mv["best_threshold"], "euclidean", norm=nt)
    assert row["threshold"] == mv["best_threshold"]
    assert (row["test_balanced_accuracy"], row["test_far"], row["test_frr"]) == (at["balanced_accuracy"], at["far"], at["frr"])
