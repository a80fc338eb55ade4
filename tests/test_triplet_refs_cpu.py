"""The triplet loss on the host: the reference helpers of tests/test_gpu_triplet_loss.py (the closed-form gradient against autograd,
the ambiguity caps of every GPU input, the derived bounds against fp32 arithmetic in two summation orders and against five wrong
variants), the P x K samplers, the C ABI's argument checks and the public surface that needs no GPU."""
import ctypes
import tempfile

import numpy as np
import pytest

from tests import triplet_refs as R

INPUTS = R.gpu_inputs()
IDS = [i[0] for i in INPUTS]
SMALL_INPUTS = [i for i in INPUTS if i[1] == "small"]


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
@pytest.mark.parametrize("inp", SMALL_INPUTS + [INPUTS[-1]], ids=[i[0] for i in SMALL_INPUTS] + [IDS[-1]])
def test_closed_form_gradient_equals_autograd(inp, variant):
    _, _, emb, lab = inp
    an = R.analyse(emb, lab, variant[0], variant[1], R.MARGIN)
    loss, g = R.autograd(emb, lab, variant[0], variant[1], R.MARGIN)
    assert abs(loss - an["loss"]) <= 1e-13 * max(1.0, abs(loss))
    assert np.abs(g - an["demb"]).max() <= 1e-13 * max(1.0, np.abs(g).max())
    assert np.abs(g).max() > 0


@pytest.mark.parametrize("inp", INPUTS, ids=IDS)
def test_every_gpu_input_is_inside_its_ambiguity_caps(inp):
    """Conditions on the inputs, not measurements: no ambiguous selection or triplet at the small shapes, at most 1 % / 1e-3 at the
    limits."""
    name, kind, emb, lab = inp
    sel, trip = R.ambiguity(emb, lab)
    print(name, "ambiguous selections %.3g, triplets %.3g" % (sel, trip))
    assert sel <= R.CAPS[kind][0] and trip <= R.CAPS[kind][1]


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
@pytest.mark.parametrize("inp", INPUTS, ids=IDS)
def test_fp32_arithmetic_stays_inside_every_bound(inp, variant, rev):
    _, _, emb, lab = inp
    out = R.triplet_f32(emb, lab, variant[0], variant[1], R.MARGIN, rev=rev)
    bad, w, an = R.check(out, emb, lab, variant[0], variant[1], R.MARGIN)
    assert not bad, bad[:3]
    assert all(v <= 1.0 for v in w.values()), w


# which (mining, soft) a wrong variant changes the mathematics of, on the class-major P x K inputs (no singleton class)
APPLIES = {"hardest_pos_min": lambda v: True,                    # (ALL reports the same selections)
           "self_positive": lambda v: v[0] == R.ALL,             # s_aa = 0 is never the farthest positive, but it adds triplets
           "pos_grad_sign": lambda v: True,
           "mean_over_n": lambda v: v[0] == R.HARD,
           "all_norm_t": lambda v: v == (R.ALL, 0)}


@pytest.mark.parametrize("wrong", R.WRONG)
def test_the_bounds_catch_a_wrong_variant(wrong):
    hit = 0
    for c in [(4, 3, 8, 0)] + R.SMALL[2:]:                        # K >= 3: the farthest positive is not the nearest
        emb, lab = R.pk_batch(*c)
        if wrong == "mean_over_n":
            lab = lab.copy()
            lab[0] = -1                                            # V < N
        for v in R.VARIANTS:
            out = R.triplet_f32(emb, lab, v[0], v[1], R.MARGIN, wrong=wrong)
            bad, w, _ = R.check(out, emb, lab, v[0], v[1], R.MARGIN)
            caught = bool(bad) or max(w.values()) > 1.0
            assert caught == APPLIES[wrong](v), (wrong, c, R.variant_id(v), bad[:2], w)
            hit += caught
    assert hit >= 3


def test_duplicate_rows_and_zero_distance_stay_finite():
    emb, lab = R.pk_batch(3, 3, 8, seed=4)
    emb[1] = emb[0]                                                # s = 0 inside class 0
    for v in R.VARIANTS:
        an = R.analyse(emb, lab, v[0], v[1], R.MARGIN)
        assert np.isfinite(an["demb"]).all() and np.isfinite(an["loss"])
        out = R.triplet_f32(emb, lab, v[0], v[1], R.MARGIN)
        assert np.isfinite(out["demb"]).all()
        bad, w, _ = R.check(out, emb, lab, v[0], v[1], R.MARGIN)
        assert not bad and all(x <= 1.0 for x in w.values()), (bad, w)


# ---- the samplers ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    return SyntheticSpeechDataset(num_speakers=7, files_per_speaker=5, seconds=0.25, min_file_seconds=0.3, max_file_seconds=0.6)


def test_speaker_batch_layout_labels_and_distinct_draws(synthetic):
    ds = synthetic
    p, k = 4, 3
    np.random.seed(3)
    files = ds._speaker_batch_files(p, k)
    assert files.shape == (p, k)
    spk = ds._code[files]
    assert (spk == spk[:, :1]).all() and len(set(spk[:, 0])) == p                 # one speaker per class, p distinct speakers
    assert all(len(set(row)) == k for row in files)                                # distinct files within a speaker
    np.random.seed(3)
    windows, labels = ds.build_speaker_batch(p, k)
    assert windows.shape == (p * k, ds.fragment_length, 1) and labels.shape == (p * k, 1)
    assert (labels[:, 0] == np.repeat(np.arange(p), k)).all()                      # class-major
    for row, f in zip(windows[:, :, 0], files.reshape(-1)):                        # every window is a fragment of its file
        rec = ds._load(int(f))
        assert any(np.array_equal(row, rec[s:s + ds.fragment_length]) for s in range(len(rec) - ds.fragment_length + 1))
    np.random.seed(3)
    assert (ds._episode_files(p, 1, k - 1) == files).all()                         # the episode rule's draws
    w2, l2 = next(ds.yield_speaker_batches(p, k))
    assert w2.shape == windows.shape and (l2 == labels).all()


def test_speaker_batch_value_errors(synthetic):
    ds = synthetic
    for p, k in ((8, 2), (3, 6), (1, 2), (3, 1)):          # 7 speakers; nobody has 6 files; one speaker; no positives
        with pytest.raises(ValueError):
            ds.build_speaker_batch(p, k)


def test_offsets_sampler_draws_what_the_host_sampler_draws(synthetic):
    from voicemap_amd import shards
    with tempfile.TemporaryDirectory() as d:
        shards.write_shards(synthetic, d)
        sh = shards.ShardedSpeechDataset(d, synthetic.fragment_seconds)
        p, k = 3, 3
        np.random.seed(11)
        offsets, labels, files = sh.build_speaker_batch_offsets(p, k, files=True)
        np.random.seed(11)
        windows, host_labels = sh.build_speaker_batch(p, k)
        np.random.seed(11)
        assert (sh._speaker_batch_files(p, k).reshape(-1) == files).all()
        assert (labels == host_labels).all() and offsets.shape == (p * k,)
        flat = np.concatenate([np.asarray(m_, dtype=np.float64) for m_ in sh._maps]) / shards.INT16_SCALE
        for row, o in zip(windows[:, :, 0], offsets):                               # the same fragments of the same files
            assert np.array_equal(row, flat[o:o + sh.fragment_length])
        with pytest.raises(ValueError):
            sh.build_speaker_batch_offsets(8, 2)


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------
def test_abi_symbols_and_argument_errors():
    from voicemap_amd import _lib
    from ctypes import c_float, c_int, c_int64, c_void_p
    P, I, L, F = c_void_p, c_int, c_int64, c_float
    assert _lib.SIGNATURES["vm_triplet_loss_supported"] == (I, [L, I])
    assert _lib.SIGNATURES["vm_triplet_loss_workspace_bytes"] == (L, [L, I, I])
    assert _lib.SIGNATURES["vm_triplet_loss"] == (I, [P, P, L, I, I, I, F, F, P, P, P, P, P, P])
    assert _lib._ENUMS["VM_TRIPLET_HARD"] == R.HARD and _lib._ENUMS["VM_TRIPLET_ALL"] == R.ALL
    lib = _lib.lib()
    assert lib.abi == 11
    buf = (ctypes.c_float * 16)()          # never read: every call below is refused before a launch
    p = ctypes.addressof(buf)
    call = lambda N, E, mining, soft, margin, emb=p: lib.call("vm_triplet_loss", emb, p, N, E, mining, soft, margin, 1.0, p, p, p, None, p,
                                                                None)
    with pytest.raises(_lib.VoicemapHipError, match=r"\(-1\).*null"):
        call(4, 4, 0, 0, 0.2, emb=None)
    with pytest.raises(_lib.VoicemapHipError, match=r"\(-1\).*N >= 2"):
        call(1, 4, 0, 0, 0.2)
    with pytest.raises(_lib.VoicemapHipError, match=r"\(-1\).*E >= 1"):
        call(4, 0, 0, 0, 0.2)
    with pytest.raises(_lib.VoicemapHipError, match=r"\(-3\)"):          # VM_ERR_UNSUPPORTED above the limits
        call(1025, 4, 0, 0, 0.2)
    with pytest.raises(_lib.VoicemapHipError, match=r"\(-3\)"):
        call(4, 257, 0, 0, 0.2)
    for margin in (-0.1, float("nan"), float("inf")):
        for mining in (R.HARD, R.ALL):
            with pytest.raises(_lib.VoicemapHipError, match=r"\(-1\).*margin"):
                call(4, 4, mining, 0, margin)
    for mining in (-1, 2):
        with pytest.raises(_lib.VoicemapHipError, match=r"\(-1\).*mining"):
            call(4, 4, mining, 0, 0.2)
    for soft in (-1, 2):
        with pytest.raises(_lib.VoicemapHipError, match=r"\(-1\).*soft"):
            call(4, 4, 0, soft, 0.2)
    for N, E, ok in ((2, 1, 1), (1024, 256, 1), (1, 8, 0), (1025, 8, 0), (8, 257, 0), (8, 0, 0)):
        assert lib.query("vm_triplet_loss_supported", N, E) == ok, (N, E)
    for mining in (R.HARD, R.ALL):
        assert lib.query("vm_triplet_loss_workspace_bytes", 1024, 64, mining) == (1024 * 1024 + 4 * 1024) * 4
    assert lib.query("vm_triplet_loss_workspace_bytes", 256, 64, 0) == (256 * 256 + 4 * 256) * 4


# ---- the public surface on the host -----------------------------------------------------------------------------------
def test_triplet_loss_compile_and_config_round_trip():
    from voicemap_amd import models, utils
    from voicemap_amd.keras_like import Adam, Dense
    loss = utils.TripletLoss(0.5, mining="all")
    assert loss.__name__ == "triplet_loss" and loss.get_config() == {"margin": 0.5, "mining": "all"}
    d = utils.TripletLoss()
    assert d.get_config() == {"margin": 0.2, "mining": "hard"} and not d.soft and d.mining_code == R.HARD
    s = utils.TripletLoss(margin="soft")
    assert s.soft and s.get_config() == {"margin": "soft", "mining": "hard"} and s.margin_value == 0.0
    for bad in ((-0.1, "hard"), (float("nan"), "hard"), ("hard", "hard"), (0.2, "semi")):
        with pytest.raises(ValueError):
            utils.TripletLoss(*bad)
    enc = models.get_baseline_convolutional_encoder(16, 32)
    enc.compile(loss=loss, optimizer=Adam(clipnorm=1.))
    assert enc._triplet_loss() is loss and enc._proto_loss() is None
    tc = enc._training_config()
    assert tc["loss"] == "triplet_loss" and tc["loss_config"] == loss.get_config()
    for cfg in (tc["loss_config"], s.get_config()):
        back = models.loss_by_name("triplet_loss", cfg)
        assert isinstance(back, utils.TripletLoss) and back.get_config() == cfg
    # the numpy statement of the loss is the reference's, in all four variants and with a row taken out
    emb, lab = R.ragged_batch()
    for mining, soft in R.VARIANTS:
        fn = utils.TripletLoss("soft" if soft else 0.7, ("hard", "all")[mining])
        assert abs(fn(emb, lab[:, None]) - R.analyse(emb, lab, mining, soft, 0.7)["loss"]) < 1e-12
    assert utils.TripletLoss()(emb, np.zeros(len(emb))) == 0.0            # one class: no valid anchor
    # a bare encoder compiled with anything else keeps its refusal; a classifier does not take the loss
    enc.compile(loss="categorical_crossentropy", optimizer=Adam())
    assert enc._triplet_loss() is None
    with pytest.raises(RuntimeError, match="the bare encoder has no loss"):
        enc._train_step(np.zeros((4, 100, 1)), np.zeros(4))
    clf = models.get_baseline_convolutional_encoder(16, 32)
    clf.add(Dense(10, activation="softmax"))
    clf.compile(loss=loss, optimizer=Adam())
    assert clf._triplet_loss() is None
    with pytest.raises(AssertionError):
        utils.BatchPreProcessor("triplet", lambda x: x)   # the preprocessor's mode list stays what it is: batches use "classifier"


def test_the_2d_variant_refuses_the_loss():
    """As for the prototypical loss: the spectrogram engine has no triplet step (its data paths are the raw-window ones).  It does
    not carry the 1-D engine's other entry points either -- it says what it serves -- and the model refuses the two losses before an
    engine is built, when training and when evaluating."""
    from voicemap_amd import models, utils
    from voicemap_amd.keras_like import Adam
    from voicemap_amd.spectro_engine import HipSpectrogramEncoderEngine as S
    for name in ("triplet_train_step", "triplet_train_step_from_offsets", "triplet_eval",
                 "prototypical_train_step", "prototypical_train_step_from_offsets", "prototypical_eval",
                 "margin_train_step", "margin_eval", "classifier_train_step",
                 "embed_from_offsets", "embed_varlen", "load_preprocessed", "preprocess", "_train_step", "_offsets_step"):
        assert not hasattr(S, name), name
    assert S.losses == {"siamese"}
    for loss in (utils.TripletLoss(), utils.PrototypicalLoss(2, 1)):
        enc = models.get_spectrogram_convolutional_encoder(8, 16)
        enc.compile(loss=loss, optimizer=Adam())
        for call in (enc.train_on_batch, enc.test_on_batch):
            with pytest.raises(NotImplementedError, match="implemented for the 1-D encoder"):
                call(np.zeros((4, 100, 1), np.float32), np.zeros(4))
        assert enc.engine is None
