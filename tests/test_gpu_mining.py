"""-m gpu checks of hard-pair mining (vm_mine_pairs, voicemap_amd/mining.py).  Every comparison is exact: the lists equal
mine_pairs_numpy applied to the score matrix vm_pairdist_argmin returns for the same rows -- indices and score BITS -- over the three
distances, embedding widths around the vector and stage sizes, ragged N, K = 1 / 8 / 64, a shard in the middle, floors, a lattice with
massive ties / NaN rows / unlabelled rows, and a corpus large enough for several candidate splits and the merge; K = 1 with distinct
labels is vm_pairdist_argmin's own argmin; runs and row cuts are bit-identical; then the host layers: semi-hard mining, two ranks, the
sampler + callback in fit_generator on the host and the device path, and the script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import L, p, stream
from voicemap_amd import mining as MN
from voicemap_amd.retrieval import EmbeddingCache
from voicemap_amd.verification import score_keys

pytestmark = pytest.mark.gpu
DIST = {"euclidean": 0, "cosine": 1, "dot_product": 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairdist(q, ref, dist, q_row0=-1):
    """vm_pairdist_argmin: the (M, N) fp32 score matrix, best_val, best_idx."""
    M, E = q.shape
    N = ref.shape[0]
    x, y = torch.as_tensor(q).cuda().contiguous(), torch.as_tensor(ref).cuda().contiguous()
    ws = torch.empty(L().query("vm_pairdist_workspace_bytes", M, N) // 4 + 16, device="cuda")
    d = torch.empty(M, N, device="cuda")
    bv = torch.empty(M, device="cuda")
    bi = torch.empty(M, dtype=torch.int32, device="cuda")
    L().call("vm_pairdist_argmin", p(x), p(y), M, N, E, DIST[dist], q_row0, p(d), p(bv), p(bi), p(ws), stream())
    return d.cpu().numpy(), bv.cpu().numpy(), bi.cpu().numpy()


def _mine(emb, label, dist, rows, k_neg, k_pos, floor=None):
    out = MN.mine_rows(torch.as_tensor(emb).cuda(), torch.as_tensor(np.asarray(label, np.int32)).cuda(), DIST[dist], rows, k_neg, k_pos,
                       None if floor is None else torch.as_tensor(np.asarray(floor, np.float32)).cuda())
    return tuple(t.cpu().numpy() for t in out)


def _same(got, ref):
    """indices equal, score bits equal (NaN padding included)."""
    for g, r, name in zip(got, ref, ("neg_idx", "neg_val", "pos_idx", "pos_val")):
        assert g.shape == r.shape and g.dtype == r.dtype, name
        if g.dtype == np.float32:
            gb, rb = g.view(np.uint32), r.view(np.uint32)
            nan = np.isnan(r)
            assert np.array_equal(np.isnan(g), nan), name
            assert np.array_equal(gb[~nan], rb[~nan]), name
        else:
            assert np.array_equal(g, r), (name, np.argwhere(g != r)[:5])


def _rand(n, E, seed, S=23, unlabelled=0.03):
    r = np.random.default_rng(seed)
    spk = r.integers(0, S, n)
    emb = (r.normal(0, 1, (S, E))[spk] + r.normal(0, 1, (n, E))).astype(np.float32)
    label = np.where(r.random(n) < unlabelled, -1, spk).astype(np.int32)
    return emb, label


def _floors(s, seed):
    """One floor per row taken from the row's own scores (so the strict inequality meets equal keys), some rows without (NaN)."""
    r = np.random.default_rng(seed)
    fl = np.sort(s, axis=1)[np.arange(len(s)), r.integers(0, max(s.shape[1] // 8, 1), len(s))].astype(np.float32)
    fl[r.random(len(s)) < 0.2] = np.nan
    return fl


@pytest.mark.parametrize("E", [3, 64, 100, 256])
@pytest.mark.parametrize("dist", ["euclidean", "cosine", "dot_product"])
def test_lists_equal_numpy_on_pairdist_scores(dist, E):
    N, lo, hi = 1237, 300, 777            # N is a multiple of no tile (64 anchors, 128 candidates); a shard in the middle
    emb, label = _rand(N, E, 10 * E + DIST[dist])
    s, _, _ = _pairdist(emb[lo:hi], emb, dist)
    for rows in ((lo, hi), (0, N)) if E == 64 else ((lo, hi),):
        sr = s if rows == (lo, hi) else _pairdist(emb, emb, dist)[0]
        fl = _floors(sr, E)
        for K in (1, 8, 64):
            for floor in (None, fl):
                ref = MN.mine_pairs_numpy(sr, label, K, K, row0=rows[0], neg_floor=floor)
                _same(_mine(emb, label, dist, rows, K, K, floor), ref)
        # the two lists on their own, and different sizes
        ref = MN.mine_pairs_numpy(sr, label, 8, 4, row0=rows[0])
        _same(_mine(emb, label, dist, rows, 8, 4), ref)
        assert np.array_equal(_mine(emb, label, dist, rows, 8, 0)[0], ref[0])
        assert np.array_equal(_mine(emb, label, dist, rows, 0, 4)[2], ref[2])


def test_lattice_with_massive_ties_nan_rows_and_unlabelled_rows():
    r = np.random.default_rng(3)
    N = 700
    emb = r.integers(-1, 2, (N, 64)).astype(np.float32)
    emb[[5, 77, 300]] = np.nan
    emb[[9, 10]] = 0.0                                  # zero rows: dot_product scores of -0.0
    label = r.integers(0, 6, N).astype(np.int32)
    label[[0, 50, 77, 420]] = -1
    for dist in ("euclidean", "dot_product"):
        s, _, _ = _pairdist(emb, emb, dist)
        assert len(np.unique(s[np.isfinite(s)])) < 150
        fl = _floors(np.where(np.isnan(s), 0, s), 1)
        for K in (1, 7, 64):
            for floor in (None, fl):
                ref = MN.mine_pairs_numpy(s, label, K, K, neg_floor=floor)
                got = _mine(emb, label, dist, (0, N), K, K, floor)
                _same(got, ref)
                sub = _mine(emb, label, dist, (130, 391), K, K, None if floor is None else floor[130:391])
                _same(sub, tuple(a[130:391] for a in ref))
        if dist == "dot_product":
            assert (ref[1].view(np.uint32) == 0x80000000).any()   # a -0.0 score came back with its own bits
        assert (got[0][5] == -1).all() and (got[2][5] == -1).all() and (got[0][50] == -1).all()


@pytest.mark.parametrize("k_neg,k_pos", [(8, 4), (64, 64)])
def test_large_corpus_exercises_the_candidate_splits_and_the_merge(k_neg, k_pos):
    N, lo, hi = 40003, 19000, 21048
    emb, label = _rand(N, 64, 5, S=400, unlabelled=0.01)
    s, _, _ = _pairdist(emb[lo:hi], emb, "euclidean")
    ref = MN.mine_pairs_numpy(s, label, k_neg, k_pos, row0=lo)
    _same(_mine(emb, label, "euclidean", (lo, hi), k_neg, k_pos), ref)
    if k_neg == 8:
        fl = ref[3][:, 0]                                # semi-hard by hand: beyond the hardest positive
        _same(_mine(emb, label, "euclidean", (lo, hi), k_neg, 0, fl)[:2], MN.mine_pairs_numpy(s, label, k_neg, 0, row0=lo, neg_floor=fl)[:2])


@pytest.mark.parametrize("dist", ["euclidean", "cosine", "dot_product"])
def test_k1_with_distinct_labels_is_the_argmin_of_pairdist(dist):
    N, lo, hi = 3001, 1000, 1900
    emb, _ = _rand(N, 64, 8)
    _, bv, bi = _pairdist(emb[lo:hi], emb, dist, q_row0=lo)
    ni, nv, _, _ = _mine(emb, np.arange(N), dist, (lo, hi), 1, 0)
    assert np.array_equal(ni[:, 0], bi) and np.array_equal(nv[:, 0].view(np.uint32), bv.view(np.uint32))


def test_runs_and_row_cuts_are_bit_identical():
    N = 5000
    emb, label = _rand(N, 100, 12)
    a = _mine(emb, label, "cosine", (700, 3100), 8, 4)
    b = _mine(emb, label, "cosine", (700, 3100), 8, 4)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    pieces = [_mine(emb, label, "cosine", rows, 8, 4) for rows in ((700, 701), (701, 2047), (2047, 3100))]
    for k, x in enumerate(a):
        assert np.concatenate([pc[k] for pc in pieces]).tobytes() == x.tobytes()


def _cache(emb, spk):
    return EmbeddingCache(torch.as_tensor(np.ascontiguousarray(emb, np.float32)).cuda(), np.asarray(spk))


def test_semi_hard_negatives_lie_beyond_the_hardest_positive():
    emb, label = _rand(2500, 64, 21, S=40, unlabelled=0.0)
    spk = 1000 + 7 * label                               # speaker codes, not dense indices
    cache = _cache(emb, spk)
    plain = MN.mine_pairs(cache, "euclidean", k_neg=8, k_pos=4)
    semi = MN.mine_pairs(cache, "euclidean", k_neg=8, k_pos=4, semi_hard=True)
    assert semi.rows == (0, 2500) and np.array_equal(semi.pos_idx, plain.pos_idx)
    have = semi.neg_idx >= 0
    kneg = score_keys(semi.neg_val).astype(np.int64)
    kpos = score_keys(semi.pos_val[:, :1]).astype(np.int64)
    assert have.any() and (kneg > kpos)[have].all()
    assert not np.array_equal(semi.neg_idx, plain.neg_idx)            # on this data some nearest negatives are nearer than a positive
    assert (spk[semi.neg_idx[have]] != np.repeat(spk[:, None], 8, 1)[have]).all()
    assert semi.neg_mean > plain.neg_mean and plain.pos_fraction == 1.0 and plain.pos_mean == semi.pos_mean
    s, _, _ = _pairdist(emb, emb, "euclidean")
    _same((semi.neg_idx, semi.neg_val, semi.pos_idx, semi.pos_val),
          MN.mine_pairs_numpy(s, label, 8, 4, neg_floor=plain.pos_val[:, 0])[:2] + MN.mine_pairs_numpy(s, label, 0, 4)[2:])
    part = MN.mine_pairs(cache, "euclidean", k_neg=8, k_pos=4, rows=(100, 164))
    assert part.rows == (100, 164) and np.array_equal(part.neg_idx, plain.neg_idx[100:164])


_TWO_RANK = r"""
import json, sys
sys.path.insert(0, {root!r})
import numpy as np, torch
from voicemap_amd import parallel, mining as MN
from voicemap_amd.retrieval import EmbeddingCache
rank, world, _ = parallel.init_distributed(timeout_s=120)
torch.cuda.set_device(0)
r = np.random.default_rng(4)
spk = r.integers(0, 13, 2001)
emb = (r.normal(0, 1, (13, 64))[spk] + r.normal(0, 1, (2001, 64))).astype(np.float32)
cache = EmbeddingCache(torch.as_tensor(emb).cuda(), spk)
m = MN.mine_pairs(cache, "cosine", k_neg=8, k_pos=4, semi_hard=True)
if rank == 0:
    print("RESULT " + json.dumps([m.neg_idx.tolist(), m.neg_val.view(np.uint32).tolist(), m.pos_idx.tolist(),
                                  m.pos_val.view(np.uint32).tolist(), list(m.rows)]))
"""


def test_two_rank_gloo_run_gives_the_same_lists(tmp_path):
    script = tmp_path / "two_rank.py"
    script.write_text(_TWO_RANK.format(root=ROOT))
    env = dict(os.environ, VOICEMAP_DIST_BACKEND="gloo", MASTER_PORT="29741")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", str(script)], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    two = json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    r = np.random.default_rng(4)
    spk = r.integers(0, 13, 2001)
    emb = (r.normal(0, 1, (13, 64))[spk] + r.normal(0, 1, (2001, 64))).astype(np.float32)
    one = MN.mine_pairs(_cache(emb, spk), "cosine", k_neg=8, k_pos=4, semi_hard=True)
    assert two[4] == [0, 2001] and one.rows == (0, 2001)
    assert two[0] == one.neg_idx.tolist() and two[2] == one.pos_idx.tolist()
    assert two[1] == one.neg_val.view(np.uint32).tolist() and two[3] == one.pos_val.view(np.uint32).tolist()


def _fit_with_mining(dataset, input_len, device):
    from voicemap_amd import keras_like as K
    from voicemap_amd import models, utils
    torch.manual_seed(3)
    np.random.seed(7)
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    enc = models.get_baseline_convolutional_encoder(16, 24, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (input_len, 1), distance_metric="uniform_euclidean")
    net.compile(loss="binary_crossentropy", optimizer=K.Adam(lr=5e-3, clipnorm=1.), metrics=["accuracy"])
    sampler = MN.HardPairSampler(dataset, None, hard_fraction=0.5, seed=1)
    seen = []
    update = sampler.update
    sampler.update = lambda mined: (seen.append(mined), update(mined))[1]
    miner = MN.HardPairMiner(sampler, dataset, bp, every=1, k_neg=4, k_pos=2)
    gen = sampler.yield_verification_batches_device if device else sampler.yield_verification_batches
    hist = net.fit_generator(generator=(bp(b) for b in gen(8)), steps_per_epoch=4, epochs=3, workers=0, verbose=0, callbacks=[miner])
    h = hist.history
    assert len(h["loss"]) == 3 and all(np.isfinite(v) for v in h["loss"])
    assert len(h["mined_neg_mean"]) == 3 and len(h["mined_pos_mean"]) == 3
    assert all(np.isfinite(v) for v in h["mined_neg_mean"] + h["mined_pos_mean"])
    assert len(seen) == 4 and miner.refreshes == 4          # on_train_begin + after every epoch
    first, last = seen[0], seen[-1]
    assert first.rows == (0, len(dataset)) and first.k_neg == 4 and first.k_pos == 2
    assert (first.neg_idx[:, 0] >= 0).all() and first.pos_fraction == 1.0
    assert not np.array_equal(first.neg_val, last.neg_val, equal_nan=True)   # the model moved: so did the pools
    assert h["mined_neg_mean"][-1] == last.neg_mean
    code = np.asarray(dataset._code)
    alike, differing = sampler.verification_pairs(8)
    assert all(code[i] == code[j] for i, j in alike) and all(code[i] != code[j] for i, j in differing)
    assert all(j in last.pos_idx[i] for i, j in alike[:2]) and all(j in last.neg_idx[i] for i, j in differing[:2])


def test_fit_generator_with_sampler_and_miner_on_the_host_path():
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    train = SyntheticSpeechDataset(num_speakers=12, files_per_speaker=4, seconds=0.5, pad=True, seed=1)
    _fit_with_mining(train, 2000, device=False)


def test_fit_generator_with_sampler_and_miner_on_the_device_path(tmp_path):
    from voicemap_amd import shards
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    from voicemap_amd.shards import DeviceWindows
    src = SyntheticSpeechDataset(num_speakers=10, files_per_speaker=4, seconds=1, seed=9)
    shards.write_shards(src, str(tmp_path), shard_samples=500000)
    sd = shards.ShardedSpeechDataset(str(tmp_path), 1, stochastic=True)
    sd.to_device("cuda")
    sm = MN.HardPairSampler(sd, None, hard_fraction=0.5)
    np.random.seed(3)
    (a, b), y = sm.build_verification_batch_device(8)
    np.random.seed(3)
    (c, d), y2 = sd.build_verification_batch_device(8)
    assert isinstance(a, DeviceWindows) and a.shape == c.shape == (8, sd.fragment_length, 1)
    assert np.array_equal(a.offsets_host, c.offsets_host) and np.array_equal(b.offsets_host, d.offsets_host) and np.array_equal(y, y2)
    _fit_with_mining(sd, sd.fragment_length // 4, device=True)


@pytest.mark.parametrize("device_data", [False, True])
def test_train_siamese_script_with_hard_fraction(tmp_path, monkeypatch, device_data):
    import config
    import pandas as pd
    from experiments import _common as C
    from experiments import train_siamese
    monkeypatch.setattr(config, "PATH", str(tmp_path))
    monkeypatch.setattr(C, "PATH", str(tmp_path))
    os.makedirs(os.path.join(str(tmp_path), "logs"), exist_ok=True)
    os.makedirs(os.path.join(str(tmp_path), "models"), exist_ok=True)
    argv = ["--synthetic", "--hard-fraction", "0.5", "--mine-k-neg", "4", "--mine-k-pos", "2", "--filters", "16", "--embedding-dimension", "16",
            "--batchsize", "16", "--epochs", "2", "--steps-per-epoch", "3", "--validation-steps", "2", "--num-evaluation-tasks", "4",
            "--n-seconds", "3", "--dtype", "f32", "--workers", "0"]
    if device_data:
        argv += ["--device-data", os.path.join(str(tmp_path), "shards"), "--semi-hard"]
    hist = train_siamese.main(argv)
    assert len(hist.history["loss"]) == 2 and all(np.isfinite(v) for v in hist.history["loss"])
    assert all(np.isfinite(v) for v in hist.history["mined_neg_mean"] + hist.history["mined_pos_mean"])
    logs = [f for f in os.listdir(os.path.join(str(tmp_path), "logs")) if f.endswith(".csv")]
    df = pd.read_csv(os.path.join(str(tmp_path), "logs", logs[0]))
    assert "mined_neg_mean" in df.columns and "mined_pos_mean" in df.columns and len(df) == 2
