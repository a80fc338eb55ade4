"""-m gpu tests of the two optional stages of ``diarize`` (voicemap_amd/diarization.py): speech gating in front of the windows and
Viterbi resegmentation behind the clustering, on a tiny resident corpus with the small untrained encoder of the other GPU tests.  What
is checked is the plumbing -- which windows are embedded, which labels enter the decode, which segments come out -- against the same
pieces called by hand.  No DER is asserted anywhere."""
import numpy as np
import pytest
import torch

from tests import vad_cases as VC
from voicemap_amd import diarization as DZ
from voicemap_amd.vad import VadPolicy

pytestmark = pytest.mark.gpu

WINDOW, HOP, FINE = 2400, 1200, 400   # 0.15 s windows every 0.075 s; the fine hop 0.025 s
FRAME = 80                            # 5 ms


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from voicemap_amd import models, utils
    ds = VC.pause_corpus(tmp_path_factory.mktemp("reseg_shards"), seconds=0.15)
    ds.to_device("cuda")
    enc = models.get_baseline_convolutional_encoder(16, 24, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (600, 1), distance_metric="uniform_euclidean")
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    kw = dict(speakers=(2, 3), turns=(4, 6), turn_seconds=(0.2, 0.5), seed=2)
    plain = DZ.make_conversations(ds, 3, **kw)
    paused = DZ.make_conversations(ds, 3, pause_seconds=(0.12, 0.2), pause_prob=0.8, **kw)
    return net, bp, plain, paused


def run(setup_, conv, **kw):
    net, bp = setup_[0], setup_[1]
    return DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075, n_speakers=2, **kw)


def test_without_the_options_diarize_is_cluster_and_window_segments(setup):
    conv = setup[2]
    segments, res = run(setup, conv)
    assert res.vad is None and res.reseg is None and res.voiced is None and res.chain_start is None
    starts = DZ.sliding_windows(conv.lens, WINDOW, HOP)
    row0 = np.concatenate([[0], np.cumsum([len(s) for s in starts])])
    assert np.array_equal(res.row0, row0) and np.array_equal(res.window_row0, row0) and all(k.all() for k in res.kept + res.clustered)
    by_hand = DZ.cluster(res.emb, row0, "cosine", "average", None, 2)
    for a, b in zip(res.host(), by_hand.host()):
        assert a.tobytes() == b.tobytes()
    for r in range(3):
        assert np.array_equal(res.starts[r], starts[r])
        assert np.array_equal(segments[r], DZ.window_segments(starts[r], WINDOW, int(conv.lens[r]), by_hand.recording(r).labels))


def test_gating_drops_the_unvoiced_windows_and_cuts_the_segments(setup):
    """hang = 0: a frame is voiced only inside a burst of active frames, and an all-zero frame is never active -- so no hypothesis
    segment may touch a frame of digital silence (with a hangover h the h frames next to speech on either side of a pause stay
    voiced: only the frames farther in are bare)."""
    conv = setup[3]
    policy = VadPolicy(frame_ms=5.0, min_run=2, hang=0)
    assert policy.frame == FRAME
    segments, res = run(setup, conv, vad=policy, min_voiced=0.5)
    mask, fb = res.vad.mask.cpu().numpy(), res.vad.frame_base_host
    assert (res.vad.info.cpu().numpy()[:, 3] == 0).all()   # no recording fell back to "all voiced"
    audio = conv.audio.cpu().numpy()
    dropped = bare = 0
    for r in range(3):
        n = int(conv.lens[r])
        m, a = mask[fb[r]:fb[r + 1]], audio[conv.offsets[r]:conv.offsets[r] + n]
        assert np.array_equal(res.voiced[r], m)
        lattice = DZ.sliding_windows([n], WINDOW, HOP)[0]
        keep = []
        for s in lattice:   # the voiced share of the frames the window overlaps, counted from the mask
            f = m[s // FRAME:(s + WINDOW - 1) // FRAME + 1]
            keep.append(f.sum() / len(f) >= 0.5)
        keep = np.array(keep)
        assert keep.any() and np.array_equal(res.kept[r], keep) and np.array_equal(res.starts[r], lattice[keep])
        dropped += int((~keep).sum())
        want_chain = [1] + [int(j - i > 1) for i, j in zip(np.flatnonzero(keep)[:-1], np.flatnonzero(keep)[1:])]
        assert res.chain_start[res.window_row0[r]:res.window_row0[r + 1]].tolist() == want_chain
        seg = segments[r]
        assert (seg[:, 1] > seg[:, 0]).all() and (seg[1:, 0] >= seg[:-1, 1]).all()
        covered = np.zeros(n, bool)
        for b, e, _ in seg:
            covered[b:e] = True
        for f in range(n // FRAME):
            if not a[f * FRAME:(f + 1) * FRAME].any():
                bare += 1
                assert m[f] == 0 and not covered[f * FRAME:(f + 1) * FRAME].any()
        assert np.array_equal(covered, np.repeat(m != 0, FRAME)[:n])   # a speaker exactly on the voiced frames
        labels = res.recording(r).labels
        assert np.array_equal(seg, DZ.cut_to_voiced(DZ.window_segments(res.starts[r], WINDOW, n, labels), m, FRAME, n))
    assert dropped > 0 and bare > 0 and res.emb.shape[0] == res.window_row0[-1] == sum(int(k.sum()) for k in res.kept)


def test_resegmentation_on_the_clustered_windows(setup):
    conv = setup[2]
    policy = DZ.ResegPolicy(0.1, iters=3)
    segments, res = run(setup, conv, reseg=policy)
    by_hand = DZ.resegment(res.emb, res.window_row0, res.labels, res.host().n_clusters, None, "cosine", 0.1, 3)
    for a, b in zip(res.reseg.host(), by_hand.host()):
        assert a.tobytes() == b.tobytes()
    assert (res.reseg.host().iters_run >= 1).all() and np.array_equal(res.reseg.n_models, [2, 2, 2])
    for r in range(3):
        assert np.array_equal(segments[r], DZ.window_segments(res.starts[r], WINDOW, int(conv.lens[r]), by_hand.recording(r).labels))
    with pytest.raises(ValueError, match="PLDA-space"):
        run(setup, conv, reseg=policy, distance="plda", plda=object())


def test_resegmentation_at_a_finer_hop_behind_gated_windows(setup):
    conv = setup[3]
    vad, policy = VadPolicy(frame_ms=5.0, min_run=2, hang=0), DZ.ResegPolicy(0.05, iters=2, hop_seconds=0.025)
    segments, res = run(setup, conv, vad=vad, reseg=policy)
    coarse_only = run(setup, conv, vad=vad)[1]
    lab_in = np.full(int(res.window_row0[-1]), -1, np.int32)
    for r in range(3):
        n = int(conv.lens[r])
        fine, coarse = DZ.sliding_windows([n], WINDOW, FINE)[0], DZ.sliding_windows([n], WINDOW, HOP)[0]
        assert np.array_equal(res.starts[r], fine[res.kept[r]]) and len(res.kept[r]) == len(fine)
        on = np.isin(res.starts[r], coarse)   # the rows on the coarse lattice (flush-end window included) are the clustered ones
        assert np.array_equal(res.clustered[r], on) and on.any() and not on.all()
        assert np.array_equal(res.starts[r][on], coarse_only.starts[r])   # ... the same windows the coarse run kept
        lo = int(res.window_row0[r])
        lab_in[lo:lo + len(on)][on] = res.recording(r).labels
    by_hand = DZ.resegment(res.emb, res.window_row0, lab_in, res.host().n_clusters, res.chain_start, "cosine", 0.05, 2)
    assert np.array_equal(by_hand.host().labels, res.reseg.host().labels) and (by_hand.host().labels >= 0).all()
    for r in range(3):
        n = int(conv.lens[r])
        whole = DZ.window_segments(res.starts[r], WINDOW, n, by_hand.recording(r).labels)
        assert np.array_equal(segments[r], DZ.cut_to_voiced(whole, res.voiced[r], FRAME, n))
    with pytest.raises(ValueError, match="multiple"):
        run(setup, conv, reseg=DZ.ResegPolicy(0.05, hop_seconds=0.05))   # 1200 is no multiple of 800


def test_the_experiment_script_with_pauses_gating_and_resegmentation():
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "experiments.diarization", "--synthetic", "--conversations", "4", "--turns", "3-4", "--window-seconds", "0.5",
           "--hop-seconds", "0.25", "--oracle-speakers", "--pause-seconds", "0.3-1.0", "--pause-prob", "0.5", "--vad", "--reseg"]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    row = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert row["conversations"] == row["scored"] == 4 and row["vad"] is True and row["reseg"] is True
    assert 0 < row["windows_kept"] <= row["windows_cut"] and row["windows_decoded"] == row["windows_kept"]
    for pre in ("", "ahc_"):
        parts = [row[pre + k] for k in ("missed", "false_alarm", "confusion")]
        assert all(p >= 0.0 for p in parts) and abs(row[pre + "mean_der"] - sum(parts)) < 1e-12
