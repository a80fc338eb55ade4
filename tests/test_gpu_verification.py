"""-m gpu checks of all-pairs verification (vm_pair_score_hist, voicemap_amd/verification.py): the device histograms equal numpy's
binning of vm_pairdist_argmin's own fp32 scores AS INTEGERS, the metrics equal the sort-based definition on those scores, and the
triangle shards, the u64 counts, NaN rows, the head scores and the experiment script."""
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


def _pair_scores(emb, dist):
    """Upper triangle of vm_pairdist_argmin's (N, N) matrix (row i, column j > i) and the target mask."""
    N, E = emb.shape
    x = torch.as_tensor(emb).cuda()
    ws = torch.empty(L().query("vm_pairdist_workspace_bytes", N, N) // 4 + 16, device="cuda")
    d = torch.empty(N, N, device="cuda")
    bv = torch.empty(N, device="cuda")
    bi = torch.empty(N, dtype=torch.int32, device="cuda")
    L().call("vm_pairdist_argmin", p(x), p(x), N, N, E, DIST[dist], 0, p(d), p(bv), p(bi), p(ws), stream())
    iu = np.triu_indices(N, 1)
    return d.cpu().numpy()[iu], iu


def _emb(N, E, seed, speakers=7):
    r = np.random.default_rng(seed)
    spk = r.integers(0, speakers, N)
    cent = r.normal(0, 1, (speakers, E))
    return (cent[spk] + r.normal(0, 1.0, (N, E))).astype(np.float32), spk


@pytest.mark.parametrize("dist", ["euclidean", "cosine", "dot_product"])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1000, 4099])
def test_histogram_counts_equal_numpy_binning_of_pairdist_scores(N, dist):
    for E in (64, 100, 256):
        emb, spk = _emb(N, E, N * 7 + E)
        cache = _cache(emb, spk)
        if N > 1:
            s, iu = _pair_scores(emb, dist)
            tg = spk[iu[0]] == spk[iu[1]]
        else:
            s, tg = np.zeros(0, np.float32), np.zeros(0, bool)
        f = s[np.isfinite(s)]
        lo, hi = (float(f.min()), float(f.max())) if len(f) else (0.0, 1.0)
        coarse = [V.pass1_window(lo, 0.5 * (lo + hi))]   # the top half of the scores lands in the over slot
        got = V.score_histogram(cache, dist, coarse, 4096)
        assert np.array_equal(got, V.bin_scores(s, tg, coarse, 4096)), (N, E)
        if N > 1:
            assert got.sum() == N * (N - 1) // 2
            # zoomed: into the fullest coarse bin, single keys at the median, everything below a threshold
            b = int(np.argmax(got[0, 0, :4096] + got[0, 1, :4096]))
            k0, sh0 = coarse[0]
            zoom = [(k0 + (b << sh0), max(0, sh0 - 10)), (V.key_of(float(np.median(s))), 0), (V.key_of(0.5 * (lo + hi)), 31)]
            got = V.score_histogram(cache, dist, zoom, 1024)
            assert np.array_equal(got, V.bin_scores(s, tg, zoom, 1024)), (N, E)


def _assert_metrics_equal(got, ref):
    for k in ("eer", "eer_threshold", "far_at_eer", "frr_at_eer", "best_balanced_accuracy", "best_threshold", "n_target", "n_nontarget",
              "n_nan"):
        assert got[k] == ref[k], (k, got[k], ref[k])


@pytest.mark.parametrize("dist", ["euclidean", "cosine", "dot_product"])
def test_metrics_equal_sort_of_pairdist_scores(dist):
    emb, spk = _emb(1500, 64, 11, speakers=30)
    s, iu = _pair_scores(emb, dist)
    got = V.verification_metrics(_cache(emb, spk), dist)
    _assert_metrics_equal(got, V.sorted_metrics(s, spk[iu[0]] == spk[iu[1]]))
    assert got["passes"] >= 2 and 0.5 < got["best_balanced_accuracy"] <= 1.0
    assert abs(got["auc"] - (1 - got["eer"])) < 0.2 and got["auc_bound"] < 0.01


def test_metrics_on_an_integer_lattice_with_many_exact_ties():
    r = np.random.default_rng(5)
    spk = r.integers(0, 6, 800)
    emb = (r.integers(-1, 2, (800, 64)) + 2 * (spk[:, None] == np.arange(64)[None, :] % 6)).astype(np.float32)
    for dist in ("euclidean", "dot_product"):
        s, iu = _pair_scores(emb, dist)
        assert len(np.unique(s)) < 400   # 319 600 pairs
        _assert_metrics_equal(V.verification_metrics(_cache(emb, spk), dist), V.sorted_metrics(s, spk[iu[0]] == spk[iu[1]]))


def test_weighted_l1_on_a_lattice_is_exact():
    r = np.random.default_rng(9)
    N, E = 700, 100
    emb = r.integers(-4, 5, (N, E)).astype(np.float32)
    spk = r.integers(0, 9, N)
    w = (2.0 ** r.integers(-3, 3, E) * np.where(r.random(E) < 0.2, -1, 1)).astype(np.float32)
    iu = np.triu_indices(N, 1)
    s = (np.abs(emb[iu[0]].astype(np.float64) - emb[iu[1]]) * w).sum(1).astype(np.float32)   # every partial sum exact in fp32
    tg = spk[iu[0]] == spk[iu[1]]
    cache = _cache(emb, spk)
    wins = [V.pass1_window(float(s.min()), float(s.max()))]
    got = V.histogram(cache, V.SCORES["weighted_l1"], torch.as_tensor(w).cuda(), wins, 4096)
    assert np.array_equal(got, V.bin_scores(s, tg, wins, 4096))
    wins = [(V.key_of(float(v)), 0) for v in np.unique(s)[:4]]
    got = V.histogram(cache, V.SCORES["weighted_l1"], torch.as_tensor(w).cuda(), wins, 1024)
    assert np.array_equal(got, V.bin_scores(s, tg, wins, 1024))


@pytest.mark.parametrize("head", ["uniform_euclidean", "weighted_l1"])
def test_head_score_ranks_pairs_like_the_siamese_head(head):
    from voicemap_amd import models
    from voicemap_amd.engine import HEADS, _p
    enc = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (2400, 1), distance_metric=head)
    eng = net._ensure_engine()
    if head == "uniform_euclidean":   # both signs of the head kernel
        signs = (1.0, -1.0)
    else:
        signs = (1.0,)
    N, E = 64, 32
    emb, spk = _emb(N, E, 3, speakers=5)
    cache = _cache(emb, spk)
    iu = np.triu_indices(N, 1)
    pairs = len(iu[0])
    both = torch.as_tensor(np.concatenate([emb[iu[0]], emb[iu[1]]])).cuda()
    for sg in signs:
        with torch.no_grad():
            if head == "uniform_euclidean":   # a head that does not saturate on these distances
                eng.view("head.kernel").fill_(0.05 * sg)
        pred = torch.empty(pairs, device="cuda")
        L().call("vm_siamese_head_loss", p(both), _p(eng.view("head.kernel")), _p(eng.view("head.bias")), None, pairs, E, HEADS[head], 0,
                 1.0, p(pred), None, None, None, None, None, stream())
        pr = pred.cpu().numpy().astype(np.float64)
        m = V.verification_metrics(cache, "head", model=net)
        # the head's accept set at the head's own threshold is the score's accept set (up to fp32 ties of the sigmoid)
        t = m["best_threshold"]
        acc = V.accuracy_at_threshold(cache, t, "head", model=net)
        assert acc["balanced_accuracy"] == m["best_balanced_accuracy"]
        tg = spk[iu[0]] == spk[iu[1]]
        if head == "uniform_euclidean":
            tp = m["best_threshold_p"]
            acc_p = 1 - 0.5 * ((pr[~tg] < tp).mean() + (pr[tg] >= tp).mean())
            assert abs(acc_p - acc["balanced_accuracy"]) < 0.02
        # ranking: the kernel's score and the head output agree on the order of almost every pair of pairs
        order_p = np.argsort(pr, kind="stable")
        rank_p = np.empty(pairs)
        rank_p[order_p] = np.arange(pairs)
        if head == "uniform_euclidean":
            sc = np.sqrt(((emb[iu[0]].astype(np.float64) - emb[iu[1]]) ** 2).sum(1)) * sg
        else:
            sc = (np.abs(emb[iu[0]].astype(np.float64) - emb[iu[1]]) * eng.view("head.kernel").cpu().numpy().reshape(-1)).sum(1)
        rank_s = np.empty(pairs)
        rank_s[np.argsort(sc, kind="stable")] = np.arange(pairs)
        assert np.corrcoef(rank_p, rank_s)[0, 1] > 0.99
        # the kernel's histogram of the head score is numpy's binning of it, up to the last-bit difference of the fp32 sum order
        h = V.score_histogram(cache, "head", [V.pass1_window(float(sc.min()), float(sc.max()))], 4096, model=net)
        assert h.sum() == pairs


@pytest.mark.parametrize("dist", ["euclidean", "cosine"])
def test_triangle_shards_sum_to_the_single_call(dist):
    emb, spk = _emb(1111, 64, 21)
    cache = _cache(emb, spk)
    wins = [V.pass1_window(0.0, 2.0 if dist == "cosine" else 30.0)]
    one = V.score_histogram(cache, dist, wins, 4096)
    for world in range(1, 9):
        tot = sum(V.score_histogram(cache, dist, wins, 4096, rows=r) for r in V.triangle_shards(cache.n, world))
        assert np.array_equal(tot, one), world


_TWO_RANK = r"""
import json, sys
sys.path.insert(0, {root!r})
import numpy as np, torch
from voicemap_amd import parallel, verification as V
from voicemap_amd.retrieval import EmbeddingCache
rank, world, _ = parallel.init_distributed(timeout_s=120)
torch.cuda.set_device(0)
r = np.random.default_rng(4)
spk = r.integers(0, 13, 2000)
emb = (r.normal(0, 1, (13, 64))[spk] + r.normal(0, 1, (2000, 64))).astype(np.float32)
m = V.verification_metrics(EmbeddingCache(torch.as_tensor(emb).cuda(), spk), "euclidean")
m.pop("roc")
if rank == 0:
    print("RESULT " + json.dumps(m))
"""


def test_two_rank_gloo_run_gives_the_same_metrics(tmp_path):
    script = tmp_path / "two_rank.py"
    script.write_text(_TWO_RANK.format(root=ROOT))
    env = dict(os.environ, VOICEMAP_DIST_BACKEND="gloo", MASTER_PORT="29731")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", str(script)], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    two = json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    r = np.random.default_rng(4)
    spk = r.integers(0, 13, 2000)
    emb = (r.normal(0, 1, (13, 64))[spk] + r.normal(0, 1, (2000, 64))).astype(np.float32)
    one = V.verification_metrics(_cache(emb, spk), "euclidean")
    for k, v in two.items():
        assert v == one[k], k


def test_nan_row_lands_only_in_the_nan_slots():
    emb, spk = _emb(500, 64, 8)
    emb[37] = np.nan
    s, iu = _pair_scores(emb, "euclidean")
    tg = spk[iu[0]] == spk[iu[1]]
    wins = [V.pass1_window(0.0, 40.0)]
    got = V.score_histogram(_cache(emb, spk), "euclidean", wins, 4096)
    assert got[0, :, -1].sum() == 499
    clean = (iu[0] != 37) & (iu[1] != 37)
    ref = V.bin_scores(s[clean], tg[clean], wins, 4096)
    assert np.array_equal(got[..., :-1], ref[..., :-1])
    m = V.verification_metrics(_cache(emb, spk), "euclidean")
    assert m["n_nan"] == 499
    _assert_metrics_equal(m, V.sorted_metrics(s, tg))


def test_u64_counts_of_five_billion_identical_pairs():
    N, E = 100000, 64
    r = np.random.default_rng(0)
    spk = r.integers(0, 921, N)
    emb = np.tile(r.normal(0, 1, (1, E)).astype(np.float32), (N, 1))
    cache = _cache(emb, spk)
    k0 = V.key_of(0.0)
    h = V.score_histogram(cache, "euclidean", [(k0, 20)], 4096)
    c = np.bincount(spk)
    n_t = int((c.astype(np.int64) * (c - 1) // 2).sum())
    total = N * (N - 1) // 2
    assert total == 4999950000
    assert h[0, 0, 0] == n_t and h[0, 1, 0] == total - n_t
    assert h[0, 0].sum() == n_t and h[0, 1].sum() == total - n_t


def test_experiment_script_synthetic_matches_accuracy_at_threshold():
    import importlib
    sys.path.insert(0, ROOT)
    ex = importlib.import_module("experiments.verification_accuracy")
    res = ex.main(["--synthetic", "--n-seconds", "1"]).iloc[0]       # end to end: argument parsing, both sets, the CSV
    assert 0.0 <= res["test_balanced_accuracy"] <= 1.0 and res["valid_pairs"] == res["test_pairs"] == 160 * 159 // 2
    assert os.path.exists(os.path.join(ROOT, "logs", "verification_accuracy_synthetic_synthetic_euclidean.csv"))
    # its test-set figures are accuracy_at_threshold's at the validation threshold
    from voicemap_amd import models, retrieval
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    from voicemap_amd.utils import BatchPreProcessor, preprocess_instances
    valid = SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=1, stochastic=False, seed=1)
    test = SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=1, stochastic=False, seed=2)
    enc = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (4000, 1), distance_metric="uniform_euclidean")
    pre = BatchPreProcessor("siamese", preprocess_instances(4))
    for score in ("euclidean", "head"):
        row = ex.evaluate(net, valid, test, pre, score)
        mv = V.verification_metrics(retrieval.embed_corpus(net, valid, pre), score, model=net if score == "head" else None)
        at = V.accuracy_at_threshold(retrieval.embed_corpus(net, test, pre), mv["best_threshold"], score,
                                     model=net if score == "head" else None)
        assert row["threshold"] == mv["best_threshold"]
        assert (row["test_balanced_accuracy"], row["test_far"], row["test_frr"]) == (at["balanced_accuracy"], at["far"], at["frr"])
