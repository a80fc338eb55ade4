"""-m gpu tests of ``diarize(..., vbx=VbxPolicy)`` (voicemap_amd/diarization.py): VBx behind a PLDA clustering, on the tiny resident
corpus and the small untrained encoder of tests/test_gpu_diarization_reseg.py, with a PLDA model made from two random covariances.
What is checked is the plumbing -- which rows and labels enter ``vbx``, which segments come out -- against the same pieces called by
hand.  No DER is asserted anywhere."""
import numpy as np
import pytest
import torch

from tests import plda_cases as PC
from tests import vad_cases as VC
from voicemap_amd import diarization as DZ
from voicemap_amd import plda as PL
from voicemap_amd.vad import VadPolicy

pytestmark = pytest.mark.gpu

WINDOW, HOP, FINE = 2400, 1200, 400   # 0.15 s windows every 0.075 s; the fine hop 0.025 s
FRAME = 80
E = 24


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from voicemap_amd import models, utils
    ds = VC.pause_corpus(tmp_path_factory.mktemp("vbx_shards"), seconds=0.15)
    ds.to_device("cuda")
    enc = models.get_baseline_convolutional_encoder(16, E, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (600, 1), distance_metric="uniform_euclidean")
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    kw = dict(speakers=(2, 3), turns=(4, 6), turn_seconds=(0.2, 0.5), seed=2)
    plain = DZ.make_conversations(ds, 3, **kw)
    paused = DZ.make_conversations(ds, 3, pause_seconds=(0.12, 0.2), pause_prob=0.8, **kw)
    rng = np.random.default_rng(4)
    model = PL.PldaModel.from_covariances(np.zeros(E), PC.random_spd(rng, E), PC.random_spd(rng, E))
    return net, bp, plain, paused, model


def run(setup_, conv, **kw):
    net, bp, model = setup_[0], setup_[1], setup_[4]
    return DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075, n_speakers=4, distance="plda", plda=model, **kw)


POLICY = dict(loop_prob=0.9, fa=0.3, fb=17.0, init_smooth=5.0, iters=5, epsilon=1e-4)


def by_hand(res, model, lab_in):
    return DZ.vbx(res.rows, res.window_row0, lab_in, res.host().n_clusters, model, res.chain_start, **POLICY)


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a.host(), b.host()))


def test_vbx_on_the_clustered_windows_equals_its_pieces(setup):
    conv, model = setup[2], setup[4]
    segments, res = run(setup, conv, vbx=DZ.VbxPolicy(**POLICY))
    assert res.reseg is None and res.chain_start is None and np.array_equal(res.window_row0, res.row0)
    clustered = DZ.cluster(res.rows, res.row0, "plda", "average", None, 4)
    for a, b in zip(res.host(), clustered.host()):
        assert a.tobytes() == b.tobytes()
    hand = by_hand(res, model, res.labels)
    assert same(res.vbx, hand) and (hand.host().iters_run >= 1).all() and np.array_equal(res.vbx.n_models, [4, 4, 4])
    for r in range(3):
        assert np.array_equal(segments[r], DZ.window_segments(res.starts[r], WINDOW, int(conv.lens[r]), hand.recording(r).labels))


def test_vbx_behind_gated_windows_and_at_a_finer_hop(setup):
    conv, model = setup[3], setup[4]
    vad = VadPolicy(frame_ms=5.0, min_run=2, hang=0)
    for hop in (None, 0.025):
        segments, res = run(setup, conv, vad=vad, vbx=DZ.VbxPolicy(hop_seconds=hop, **POLICY))
        lab_in = np.full(int(res.window_row0[-1]), -1, np.int32)
        for r in range(3):
            n = int(conv.lens[r])
            lattice = DZ.sliding_windows([n], WINDOW, FINE if hop else HOP)[0]
            assert np.array_equal(res.starts[r], lattice[res.kept[r]])
            on = np.isin(res.starts[r], DZ.sliding_windows([n], WINDOW, HOP)[0])
            assert np.array_equal(res.clustered[r], on) and on.any() and on.all() == (hop is None)
            lo = int(res.window_row0[r])
            lab_in[lo:lo + len(on)][on] = res.recording(r).labels
        assert res.chain_start is not None and res.chain_start.sum() > 3   # gating broke chains
        hand = by_hand(res, model, lab_in)
        assert same(res.vbx, hand) and (hand.host().labels >= 0).all()
        for r in range(3):
            n = int(conv.lens[r])
            whole = DZ.window_segments(res.starts[r], WINDOW, n, hand.recording(r).labels)
            assert np.array_equal(segments[r], DZ.cut_to_voiced(whole, res.voiced[r], FRAME, n))


def test_without_vbx_nothing_changes_and_bad_combinations_raise(setup):
    conv = setup[2]
    seg_a, a = run(setup, conv)
    seg_b, b = run(setup, conv, vbx=None)
    assert a.vbx is None and b.vbx is None and all(np.array_equal(x, y) for x, y in zip(seg_a, seg_b))
    for x, y in zip(a.host(), b.host()):
        assert x.tobytes() == y.tobytes()
    net, bp = setup[0], setup[1]
    with pytest.raises(ValueError, match='vbx needs distance="plda"'):
        DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075, n_speakers=2, vbx=DZ.VbxPolicy())
    with pytest.raises(ValueError, match="one of them"):
        DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075, n_speakers=2, vbx=DZ.VbxPolicy(), reseg=DZ.ResegPolicy(0.1))
    with pytest.raises(ValueError):
        DZ.VbxPolicy(loop_prob=1.0)


def test_the_experiment_script_with_vbx():
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "experiments.diarization", "--synthetic", "--conversations", "4", "--turns", "3-4", "--window-seconds", "0.5",
           "--hop-seconds", "0.25", "--oracle-speakers", "--distance", "plda", "--vbx"]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    row = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert row["conversations"] == row["scored"] == 4 and row["vbx"] is True and row["distance"] == "plda"
    assert len(row["speakers_found"]) == len(row["ahc_speakers_found"]) == 4
    assert all(1 <= s <= a for s, a in zip(row["speakers_found"], row["ahc_speakers_found"]))
    for pre in ("", "ahc_"):
        parts = [row[pre + k] for k in ("missed", "false_alarm", "confusion")]
        assert all(p >= 0.0 for p in parts) and abs(row[pre + "mean_der"] - sum(parts)) < 1e-12
