"""The prototypical loss on the host: the reference helpers of tests/test_gpu_proto_loss.py (closed-form gradients against autograd,
the prototype rule against the oracle's n-shot prediction, the derived bounds against fp32 arithmetic in two summation orders and
against three wrong variants), the episode samplers, the C ABI's argument checks and the public surface that needs no GPU."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

from oracle import voicemap_oracle as O
from tests import proto_refs as R


@pytest.fixture(scope="module")
def refs():
    """(emb, labels, float64 reference, bounds) per case, computed once."""
    out = {}
    for c in R.CASES:
        k, n, m, E, alpha = c
        emb, lab = R.episode(k, n, m, E)
        ref = R.proto_ref(emb, lab, k, n, alpha)
        out[c] = (emb, lab, ref, R.proto_bounds(emb, lab, k, n, alpha, ref))
    return out


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_closed_form_gradients_equal_autograd(case, refs):
    k, n, m, E, alpha = case
    emb, lab, ref, _ = refs[case]
    g = R.proto_closed(emb, lab, k, n, alpha)
    assert np.abs(g - ref["demb"]).max() <= 1e-14 * max(1.0, np.abs(ref["demb"]).max())


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_argmax_is_the_oracles_nearest_prototype(case, refs):
    k, n, m, E, alpha = case
    emb, lab, ref, _ = refs[case]
    for j in range(m):
        pred = O.n_shot_prediction(emb[k * n + j], emb[:k * n], n, k, "euclidean")
        assert int(np.argmin(pred)) == int(ref["pred"][j]), j
        np.testing.assert_allclose(-alpha * pred ** 2, ref["logits"][j], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fp32_arithmetic_stays_inside_every_bound(case, rev, refs):
    k, n, m, E, alpha = case
    emb, lab, ref, bnd = refs[case]
    w = R.ratios(R.proto_f32(emb, lab, k, n, alpha, rev=rev), ref, bnd)
    assert all(v <= 1.0 for v in w.values()), w


WRONG = {"proto_n_plus_1": lambda c: True,            # which cases the variant changes the mathematics of
         "grad_no_alpha": lambda c: c[4] != 1.0,
         "support_no_n": lambda c: c[1] > 1}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_the_bounds_catch_a_wrong_variant(wrong, refs):
    hit = 0
    for case in R.CASES:
        k, n, m, E, alpha = case
        emb, lab, ref, bnd = refs[case]
        w = R.ratios(R.proto_f32(emb, lab, k, n, alpha, wrong=wrong), ref, bnd)
        if WRONG[wrong](case):
            assert max(w.values()) > 1.0, (case, w)
            hit += 1
        else:
            assert max(w.values()) <= 1.0, (case, w)
    assert hit >= 3


def test_scaled_embeddings_stay_finite_and_inside_the_bounds():
    """Embeddings x 12: logit gaps in the thousands, exp underflows."""
    k, n, m, E, alpha = 5, 2, 9, 64, 1.0
    emb, lab = R.episode(k, n, m, E, scale=12.0)
    ref = R.proto_ref(emb, lab, k, n, alpha)
    assert np.ptp(ref["logits"], axis=1).max() > 1000
    out = R.proto_f32(emb, lab, k, n, alpha)
    assert np.isfinite(out["demb"]).all() and np.isfinite(out["loss"])
    w = R.ratios(out, ref, R.proto_bounds(emb, lab, k, n, alpha, ref))
    assert all(v <= 1.0 for v in w.values()), w


# ---- the samplers ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    return SyntheticSpeechDataset(num_speakers=7, files_per_speaker=5, seconds=0.25, min_file_seconds=0.3, max_file_seconds=0.6)


def test_episode_layout_labels_and_distinct_draws(synthetic):
    ds = synthetic
    k, n, q = 4, 2, 3
    np.random.seed(3)
    files = ds._episode_files(k, n, q)
    assert files.shape == (k, n + q)
    spk = ds._code[files]
    assert (spk == spk[:, :1]).all() and len(set(spk[:, 0])) == k                 # one speaker per class, k distinct speakers
    assert all(len(set(row)) == n + q for row in files)                             # distinct files within a class
    np.random.seed(3)
    windows, labels = ds.build_episode(k, n, q)
    assert windows.shape == (k * n + k * q, ds.fragment_length, 1) and labels.shape == (k * q, 1)
    assert (labels[:, 0] == np.repeat(np.arange(k), q)).all()                       # queries class-major
    order = ds._episode_order(files, n)
    assert (ds._code[order[:k * n]] == np.repeat(spk[:, 0], n)).all()               # class c owns support rows c n .. c n + n - 1
    assert (ds._code[order[k * n:]] == np.repeat(spk[:, 0], q)).all()
    for row, f in zip(windows[:, :, 0], order):                                     # every window is a fragment of its file
        rec = ds._load(int(f))
        assert any(np.array_equal(row, rec[s:s + ds.fragment_length]) for s in range(len(rec) - ds.fragment_length + 1))
    w2, l2 = next(ds.yield_episodes(k, n, q))
    assert w2.shape == windows.shape and (l2 == labels).all()


def test_episode_value_errors(synthetic):
    ds = synthetic
    with pytest.raises(ValueError):
        ds.build_episode(8, 1, 1)        # 7 speakers
    with pytest.raises(ValueError):
        ds.build_episode(3, 3, 3)        # nobody has 6 files
    with pytest.raises(ValueError):
        ds.build_episode(1, 1, 1)
    with pytest.raises(ValueError):
        ds.build_episode(3, 0, 1)
    with pytest.raises(ValueError):
        ds.build_episode(3, 1, 0)


def test_offsets_sampler_draws_what_the_host_sampler_draws(synthetic):
    from voicemap_amd import shards
    with tempfile.TemporaryDirectory() as d:
        shards.write_shards(synthetic, d)
        sh = shards.ShardedSpeechDataset(d, synthetic.fragment_seconds)
        k, n, q = 3, 2, 2
        np.random.seed(11)
        offsets, labels, files = sh.build_episode_offsets(k, n, q, files=True)
        np.random.seed(11)
        windows, host_labels = sh.build_episode(k, n, q)
        np.random.seed(11)
        assert (sh._episode_order(sh._episode_files(k, n, q), n) == files).all()
        assert (labels == host_labels).all() and offsets.shape == (k * n + k * q,)
        flat = np.concatenate([np.asarray(m_, dtype=np.float64) for m_ in sh._maps]) / shards.INT16_SCALE
        for row, o in zip(windows[:, :, 0], offsets):                               # the same fragments of the same files
            assert np.array_equal(row, flat[o:o + sh.fragment_length])


def test_verification_batches_do_not_see_the_new_methods(synthetic):
    """The new samplers are never called by the existing ones: a seeded build_verification_batch is what it is without them."""
    from voicemap_amd.librispeech import LibriSpeechDataset
    np.random.seed(5)
    (a1, a2), ya = synthetic.build_verification_batch(8)
    saved = {nm: getattr(LibriSpeechDataset, nm) for nm in ("build_episode", "yield_episodes", "_episode_files", "_episode_order")}
    try:
        for nm in saved:
            delattr(LibriSpeechDataset, nm)
        np.random.seed(5)
        (b1, b2), yb = synthetic.build_verification_batch(8)
    finally:
        for nm, fn in saved.items():
            setattr(LibriSpeechDataset, nm, fn)
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2) and np.array_equal(ya, yb)


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------
def test_abi_symbols_and_argument_errors():
    from voicemap_amd import _lib
    from ctypes import c_float, c_int, c_int64, c_void_p
    P, I, L, F = c_void_p, c_int, c_int64, c_float
    assert _lib.SIGNATURES["vm_proto_loss_supported"] == (I, [I, I, L, I])
    assert _lib.SIGNATURES["vm_proto_loss"] == (I, [P, P, I, I, L, I, F, F, P, P, P, P, P])
    assert _lib.SIGNATURES["vm_proto_loss_workspace_bytes"] == (L, [I, I, L, I])
    lib = _lib.lib()
    assert lib.abi == 11
    buf = (ctypes.c_float * 16)()          # never read: every call below is refused before a launch
    p = ctypes.addressof(buf)
    for args, what in (((None, None, 2, 1, 1, 4), "null"), ((p, None, 1, 1, 1, 4), "k >= 2"), ((p, None, 2, 0, 1, 4), "n >= 1"),
                       ((p, None, 2, 1, 1, 0), "E >= 1"), ((p, None, 2, 1, 0, 4), "m >= 1")):
        with pytest.raises(_lib.VoicemapHipError, match=r"\(-1\).*" + what):
            lib.call("vm_proto_loss", *args, 1.0, 1.0, p, None, None, None, None)
    with pytest.raises(_lib.VoicemapHipError, match="alpha"):
        lib.call("vm_proto_loss", p, None, 2, 1, 1, 4, 0.0, 1.0, p, None, None, None, None)
    with pytest.raises(_lib.VoicemapHipError, match="loss_acc and ws"):
        lib.call("vm_proto_loss", p, p, 2, 1, 1, 4, 1.0, 1.0, p, None, None, None, None)
    # the support bound: 2 <= k <= 128, n <= 16, E <= 256, k E <= 16384 (the prototypes' 64 KiB of LDS)
    for k, n, m, E, ok in ((2, 1, 1, 1, 1), (128, 1, 130, 128, 1), (16, 16, 16, 256, 1), (64, 2, 128, 256, 1), (65, 1, 1, 256, 0),
                           (129, 1, 1, 64, 0), (128, 1, 1, 129, 0), (2, 17, 1, 8, 0), (2, 1, 1, 257, 0), (1, 1, 1, 8, 0), (2, 1, 1 << 31, 8, 0)):
        assert lib.query("vm_proto_loss_supported", k, n, m, E) == ok, (k, n, m, E)
    with pytest.raises(_lib.VoicemapHipError, match=r"\(-3\)"):     # VM_ERR_UNSUPPORTED outside
        lib.call("vm_proto_loss", p, None, 65, 1, 1, 256, 1.0, 1.0, p, None, None, None, None)
    assert lib.query("vm_proto_loss_workspace_bytes", 64, 2, 128, 64) == (128 * 64 + 2 * 128) * 4


# ---- the public surface on the host -----------------------------------------------------------------------------------
def test_prototypical_loss_compile_and_config_round_trip():
    from voicemap_amd import models, utils
    from voicemap_amd.keras_like import Adam
    loss = utils.PrototypicalLoss(5, 2, alpha=0.5)
    assert loss.__name__ == "prototypical_loss" and loss.get_config() == {"k_way": 5, "n_shot": 2, "alpha": 0.5}
    assert utils.PrototypicalLoss(3, 1).alpha == 1.0
    for bad in ((1, 1, 1.0), (2, 0, 1.0), (2, 1, 0.0)):
        with pytest.raises(ValueError):
            utils.PrototypicalLoss(*bad)
    enc = models.get_baseline_convolutional_encoder(16, 32)
    enc.compile(loss=loss, optimizer=Adam(clipnorm=1.))
    assert enc._proto_loss() is loss
    tc = enc._training_config()
    assert tc["loss"] == "prototypical_loss" and tc["loss_config"] == loss.get_config()
    back = models.loss_by_name(tc["loss"], tc["loss_config"])
    assert isinstance(back, utils.PrototypicalLoss) and back.get_config() == loss.get_config()
    assert models.loss_by_name("binary_crossentropy") == "binary_crossentropy"
    # the numpy statement of the loss is the reference's
    emb, lab = R.episode(5, 2, 9, 16)
    assert abs(loss(emb, lab) - R.proto_ref(emb, lab, 5, 2, 0.5)["loss"]) < 1e-12
    # a bare encoder compiled with anything else keeps its refusal (raised before an engine is asked for)
    enc.compile(loss="categorical_crossentropy", optimizer=Adam())
    assert enc._proto_loss() is None
    with pytest.raises(RuntimeError, match="the bare encoder has no loss"):
        enc._train_step(np.zeros((4, 100, 1)), np.zeros(2))
    # a classifier does not take it
    from voicemap_amd.keras_like import Dense
    clf = models.get_baseline_convolutional_encoder(16, 32)
    clf.add(Dense(10, activation="softmax"))
    clf.compile(loss=loss, optimizer=Adam())
    assert clf._proto_loss() is None


def test_mode_encoder_is_accepted_and_an_unknown_mode_is_refused():
    from voicemap_amd import utils
    for mode in ("siamese", "classifier", "encoder"):
        assert utils.NShotEvaluationCallback(1, 1, 2, None, mode=mode).mode == mode
    with pytest.raises(AssertionError):
        utils.NShotEvaluationCallback(1, 1, 2, None, mode="prototypical")
    with pytest.raises(ValueError, match="mode must be one of"):
        utils.n_shot_task_evaluation(None, None, None, 1, 1, 2, network_type="prototypical")
    assert utils.n_shot_task_evaluation(None, None, lambda x: x, 0, 1, 2, network_type="encoder") == 0   # accepted: no task, no model use
    with pytest.raises(AssertionError):
        utils.BatchPreProcessor("encoder", lambda x: x)   # the preprocessor's mode list stays what it is: episodes use "classifier"
