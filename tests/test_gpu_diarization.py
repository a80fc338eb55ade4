"""-m gpu tests of the diarization path (voicemap_amd/diarization.py) above the clustering kernel: planted blobs through ``cluster`` and
``cut``, and ``diarize`` end to end on a tiny resident corpus with the small encoder of the other GPU tests.  No DER of a trained model
is asserted anywhere: the encoder here is untrained."""
import numpy as np
import pytest
import torch

from tests import vad_cases as VC
from voicemap_amd import diarization as DZ

pytestmark = pytest.mark.gpu


def planted(seed, lens, blobs, E=8, gap=10.0, radius=0.05):
    """Per recording ``blobs[r]`` blob centres at least ``gap`` apart (distinct corners of a cube scaled by ``gap``) and points within
    ``radius`` of them per coordinate, in a random order.  -> (emb, row0, the planted labels numbered by first occurrence)."""
    rng = np.random.RandomState(seed)
    emb, want = [], []
    for n, k in zip(lens, blobs):
        corners = rng.permutation(2 ** E)[:k]
        centres = gap * ((corners[:, None] >> np.arange(E)) & 1).astype(np.float32)
        which = np.concatenate([np.arange(k), rng.randint(0, k, size=n - k)])   # every blob has a member
        rng.shuffle(which)
        emb.append(centres[which] + rng.uniform(-radius, radius, size=(n, E)).astype(np.float32))
        first = {}
        want.append(np.array([first.setdefault(int(w), len(first)) for w in which], dtype=np.int32))
    row0 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.concatenate(emb).astype(np.float32), row0, want


@pytest.mark.parametrize("linkage", DZ.LINKAGES)
def test_planted_blobs_come_back_exactly(linkage):
    """Blob diameter <= 0.1 sqrt(8) < 0.3, blob gap >= 10 - 0.1: any threshold between separates them under every linkage; the labels
    are the planted partition numbered by first occurrence -- the kernel's numbering, by lowest member.  ``cut`` of the full
    dendrogram at that threshold gives the same labels."""
    lens, blobs = [40, 25, 70, 1], [3, 2, 4, 1]
    emb, row0, want = planted(0, lens, blobs)
    emb_t = torch.from_numpy(emb).cuda()
    res = DZ.cluster(emb_t, row0, "euclidean", linkage, threshold=2.0)
    assert res.host().n_clusters.tolist() == blobs
    full = DZ.cluster(emb_t, row0, "euclidean", linkage)
    assert full.host().n_clusters.tolist() == [1, 1, 1, 1]
    for r, n in enumerate(lens):
        got, f = res.recording(r), full.recording(r)
        assert np.array_equal(got.labels, want[r]), r
        labels, c = DZ.cut(f.merge_a, f.merge_b, f.merge_h, n, threshold=2.0)
        assert c == blobs[r] and np.array_equal(labels, got.labels)
        k = int((got.merge_a >= 0).sum())
        assert k == n - blobs[r] and np.array_equal(got.merge_a[:k], f.merge_a[:k]) and np.array_equal(got.merge_h[:k], f.merge_h[:k])
    # the number of speakers given instead of a threshold
    by_count = DZ.cluster(emb_t, row0, "euclidean", linkage, n_speakers=blobs)
    assert np.array_equal(by_count.host().labels, res.host().labels)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from voicemap_amd import models, utils
    ds = VC.pause_corpus(tmp_path_factory.mktemp("diar_shards"), seconds=0.15)
    ds.to_device("cuda")
    enc = models.get_baseline_convolutional_encoder(16, 24, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (600, 1), distance_metric="uniform_euclidean")
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    conv = DZ.make_conversations(ds, 3, speakers=(2, 3), turns=(3, 5), turn_seconds=(0.2, 0.5), seed=2)
    return ds, net, bp, conv


def test_conversations_from_a_resident_corpus(setup):
    ds, _, _, conv = setup
    assert conv.audio.is_cuda and conv.audio.dtype == torch.int16 and conv.audio.numel() == int(conv.lens.sum())
    audio = conv.audio.cpu().numpy()
    for r in range(len(conv)):
        for (b, e, who), (f, s, k) in zip(conv.segments[r], conv.turns[r]):
            assert ds._code[f] == who
            assert np.array_equal(audio[conv.offsets[r] + b:conv.offsets[r] + e], np.asarray(ds._pcm(f))[s:s + k])


def test_diarize_end_to_end(setup):
    from tests.ahc_cases import pairdist
    from voicemap_amd import retrieval
    _, net, bp, conv = setup
    segments, res = DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075, n_speakers=2)
    assert res.window == 2400 and len(segments) == len(conv) == 3
    starts = DZ.sliding_windows(conv.lens, 2400, 1200)
    assert all(np.array_equal(a, b) for a, b in zip(res.starts, starts)) and min(len(s) for s in starts) >= 3
    # the embeddings are embed_from_offsets' on the same offsets
    eng = retrieval._encoder_engine(net, "siamese")
    flat = np.concatenate([o + s for o, s in zip(conv.offsets, starts)])
    direct = eng.embed_from_offsets(conv.audio, torch.as_tensor(flat), 2400, 4, True, windows_per_tower=1).clone()
    assert torch.equal(res.emb, direct) and res.emb.shape == (len(flat), 24)
    # the labels are the statement's on those embeddings' distances; the segments carry them and tile the recording
    for r in range(3):
        lo, hi = int(res.row0[r]), int(res.row0[r + 1])
        want = DZ.ahc_reference(pairdist(res.emb[lo:hi], "cosine"), "average", target=2)
        got = res.recording(r)
        assert np.array_equal(got.labels, want.labels) and got.n_clusters == want.n_clusters == 2
        assert np.array_equal(got.merge_a, want.merge_a) and np.array_equal(got.merge_h.view(np.uint32), want.merge_h.view(np.uint32))
        seg = segments[r]
        assert seg[0, 0] == 0 and seg[-1, 1] == conv.lens[r] and (seg[1:, 0] == seg[:-1, 1]).all() and (seg[:, 1] > seg[:, 0]).all()
        assert np.array_equal(seg, DZ.window_segments(starts[r], 2400, int(conv.lens[r]), got.labels))
        d = DZ.der(conv.segments[r], seg)
        assert d["total"] == conv.lens[r] and d["missed"] == d["false_alarm"] == 0 and 0.0 <= d["der"] < 1.0   # (an untrained encoder: no claim)
    # a threshold instead of a count; a recording too short for one window is named
    seg2, res2 = DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075, threshold=0.0, linkage="complete")
    assert (res2.host().n_clusters >= 1).all() and len(seg2) == 3
    with pytest.raises(ValueError, match="recording 1 holds 100 samples"):
        DZ.diarize(net, conv.audio, [0, 5000], [4000, 100], bp, 0.15, 0.075)


def test_diarize_refuses_an_engine_without_resident_input(setup, monkeypatch):
    from voicemap_amd import retrieval
    _, net, bp, conv = setup
    monkeypatch.setattr(type(retrieval._encoder_engine(net, "siamese")), "resident_input", False)
    with pytest.raises(NotImplementedError, match="raw windows"):
        DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075)


def test_the_experiment_script_prints_one_json_line():
    """experiments/diarization.py on a handful of short synthetic conversations with an untrained encoder, once per stop rule family:
    the line's fields are there and consistent.  No value of the error is asserted."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, "-m", "experiments.diarization", "--synthetic", "--conversations", "5", "--turns", "3-4", "--window-seconds", "0.5",
            "--hop-seconds", "0.25", "--linkage", "complete"]
    for extra, scored in ((["--tune-conversations", "2"], 3), (["--oracle-speakers"], 5)):
        out = subprocess.run(base + extra, cwd=root, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        row = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        assert row["conversations"] == 5 and row["scored"] == scored and row["linkage"] == "complete" and row["windows"] > 0
        assert abs(row["mean_der"] - (row["missed"] + row["false_alarm"] + row["confusion"])) < 1e-12 and row["missed"] == row["false_alarm"] == 0.0
        table = row["clusters_found_by_speakers_present"]
        assert sum(k for by in table.values() for k in by.values()) == scored and set(table) <= {"2", "3", "4"}
        if extra[0] == "--oracle-speakers":
            assert all(list(by) == [s] for s, by in table.items())   # as many clusters as speakers, every time
        else:
            assert row["tuned_on"] == 2 and isinstance(row["threshold"], float)
