"""-m gpu: the triplet training step (engine.triplet_train_step: the whole P x K batch one encoder call, the triplets mined inside it
by vm_triplet_loss, no head parameters) against the float64 oracle, its replayed form against the eager one, the offsets path against
the raw-window path, and the public surface (compile(loss=TripletLoss) on the bare encoder, checkpoints, fit_generator over
yield_speaker_batches).  Sizes and thresholds are those of tests/test_gpu_proto_step.py."""
import numpy as np
import pytest
import torch

from oracle import voicemap_oracle as O
from tests import triplet_refs as R
from tests.gpu_util import cosine, grad_close, max_err, rel_err, report

pytestmark = pytest.mark.gpu

BLOCKS = [(32, 16, 4), (3, 32, 2), (3, 48, 2), (3, 64, 2)]
P_SPK, K_UTT = 4, 3
N_WIN = P_SPK * K_UTT
LABELS = np.repeat(np.arange(P_SPK), K_UTT).astype(np.int32)
MARGIN_FRACTION = 0.5        # margin = this fraction of the mean float64 pair distance
# The relative embedding error each storage mode is held to against float64: f32 as in tests/test_gpu_proto_step.py; f16 as in
# tests/test_gpu_e2e.py, where it is relative to the embeddings as the last layer's product leaves them -- here the bias (added in
# fp32, exactly) centres them, which takes nothing off the absolute error, so f16's 4e-3 is taken of the norm WITHOUT the bias.
EMB_THRESHOLD = {"f32": 1e-4, "f16": 4e-3}


def _emb_norm(e, p, dtype):
    e = np.asarray(e, dtype=np.float64)
    return float(np.linalg.norm(e if dtype == "f32" else e - p["dense.bias"].numpy()[None]))


def _tiny_batch(seed=0, l0=1200, dropout=0.0):
    """The tiny case of tests/test_gpu_proto_step.py for a 4 x 3 batch: non-trivial BatchNorm parameters (some negative gammas), 12
    whitened windows.  The last layer is then rescaled and shifted so that the float64 training-mode embeddings are centred with a
    mean pair distance of 1: the distances, the margin and the loss are O(1), the regime the project's absolute thresholds (loss
    1e-4 / 5e-3) were set in -- an untrained encoder puts its embeddings ~10 apart."""
    arch = O.EncoderArch.baseline(16, 32, dropout=dropout)
    p = O.init_params(arch, head=None, seed=seed)
    r = np.random.default_rng(seed)
    for i in range(1, 5):
        c = p[f"bn{i}.gamma"].shape[0]
        p[f"bn{i}.gamma"] = torch.tensor(r.normal(1.0, 0.2, c) * np.where(r.random(c) < 0.15, -1, 1))
        p[f"bn{i}.beta"] = torch.tensor(r.normal(0.0, 0.2, c))
        p[f"conv{i}.bias"] = torch.tensor(r.normal(0.0, 0.05, c))
    x = O.whiten(r.normal(0, 0.05, (N_WIN, l0, 1)) + r.uniform(-0.01, 0.01, (N_WIN, 1, 1))).astype(np.float32).astype(np.float64)
    masks = None
    if dropout > 0:
        masks = [torch.tensor((r.random((N_WIN, 1, c)) >= dropout).astype(np.float64)) for (_, c, _) in arch.blocks]
    e = O.encoder_forward(arch, p, torch.tensor(x), True, masks)
    scale = 1.0 / _mean_pair_distance(e.numpy())
    p["dense.kernel"] = p["dense.kernel"] * scale
    p["dense.bias"] = -(e.mean(0) * scale)
    return arch, p, x, masks


def _mean_pair_distance(e):
    d = np.sqrt(R.sq_dists(np.asarray(e, dtype=np.float64)))
    return float(d[np.triu_indices(len(d), 1)].mean())


def _clearance(e, mining, soft, margin, abs_err):
    """How far the float64 embeddings ``e`` are from a discontinuity of the loss, in units of what an embedding error of Frobenius
    norm ``abs_err`` (threshold x norm, as rel_err measures it) can move a distance by: |dd_ij| <= |de_i| + |de_j| <= 2 abs_err.  HARD: the gap
    between every selection and its runner-up, and (hinge) every |x_a|; ALL hinge: every |x|; ALL soft is smooth.  A selection gap
    or x compares two distances: it must exceed 2 tol, i.e. the returned ratio must exceed 1."""
    e = np.asarray(e, dtype=np.float64)
    tol = 2 * abs_err
    d = np.sqrt(R.sq_dists(e))
    pos, neg = R.masks(LABELS)
    worst = np.inf
    if mining == R.HARD:
        hp, hn, _ = R.select(d * d, pos, neg)
        for a in range(len(e)):
            dp, dn = np.sort(d[a, pos[a]])[::-1], np.sort(d[a, neg[a]])
            worst = min(worst, dp[0] - dp[1], dn[1] - dn[0])
            if not soft:
                worst = min(worst, abs(margin + dp[0] - dn[0]))
    elif not soft:
        for a in range(len(e)):
            worst = min(worst, np.abs(margin + d[a, pos[a]][:, None] - d[a, neg[a]][None, :]).min())
    return worst / (2 * tol)


def _engine(arch, p, dtype):
    from voicemap_amd.engine import HipEncoderEngine
    eng = HipEncoderEngine(arch.blocks, arch.embedding_dimension, dropout=arch.dropout, head=None, dtype=dtype)
    eng.set_params({k: v.numpy() for k, v in p.items()})
    return eng


def _check_params_after_adam(newp, ref_params, ref_grads, atol, steps=1, lr=1e-3):
    """The rule of tests/test_gpu_e2e.py: moving statistics and live parameters within atol; a parameter whose gradient is ~0 is moved
    by Adam by up to lr in a direction rounding decides."""
    for k, v in ref_params.items():
        got, want = np.asarray(newp[k], dtype=np.float64), v.numpy()
        if "moving" in k:
            assert max_err(got, want) < max(atol, (2.0 * (steps - 1) * lr)) * max(1.0, np.abs(want).max()), k
            continue
        if k not in ref_grads:
            assert max_err(got, want) < max(atol, 1e-5), k
            continue
        live = np.abs(ref_grads[k].numpy()) > 1e-4
        if live.any():
            assert np.abs(got - want)[live].max() < atol, k
        if (~live).any():
            assert np.abs(got - want)[~live].max() < 1.01 * steps * lr, k


def _oracle_with_validated_indices(arch, p, x, masks, pl, mining, soft, margin, dtype):
    """The kernel's selections against the float64 embeddings: the inputs are clear of every tie and kink by more than the storage
    mode's embedding error can bridge (asserted), so the selections must be the float64 reference's; the oracle step then uses them."""
    e64 = O.encoder_forward(arch, p, torch.tensor(x), True, masks).numpy()
    clear = _clearance(e64, mining, soft, margin, EMB_THRESHOLD[dtype] * _emb_norm(e64, p, dtype))
    print("clearance", clear)
    assert clear > 1.0
    hp, hn = pl["triplet"]["hard_pos"].cpu().numpy(), pl["triplet"]["hard_neg"].cpu().numpy()
    an = R.analyse(e64, LABELS, mining, soft, margin)
    if mining == R.HARD:
        assert np.array_equal(hp, an["hp_ref"]) and np.array_equal(hn, an["hn_ref"])
    else:   # ALL: the loss does not depend on the selections; they are checked on the embeddings the engine holds
        emb = pl["emb"].cpu().numpy()
        assert not R.admissible(hp, hn, R.analyse(emb, LABELS, mining, soft, margin))
        hp = hn = None
    ref = R.triplet_step_oracle(arch, p, O.AdamState(), torch.tensor(x), LABELS, mining, soft, margin, hp, hn, drop_masks=masks)
    assert abs(ref["loss"] - an["loss"]) < 1e-12
    return ref, an


# seeds at which the float64 embeddings of _tiny_batch are clear of every tie and kink (_clearance > 1, asserted in the test)
# (found on the host with the oracle alone: f32 seed 1 clears all four variants by 3.8x or more; with f16's 4e-3 and the given dropout
# masks no seed of 0..23 clears batch hard -- twelve anchors' runner-up gaps -- and seed 5 clears batch all's hinge, by 1.09x)
F32_SEED = 1
F16_SEED, F16_VARIANT = 5, (R.ALL, 0)


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_tiny_step_matches_the_oracle_in_f32(variant):
    mining, soft = variant
    arch, p, x, _ = _tiny_batch(seed=F32_SEED)
    e64 = O.encoder_forward(arch, p, torch.tensor(x), True, None).numpy()
    margin = MARGIN_FRACTION * _mean_pair_distance(e64)
    eng = _engine(arch, p, "f32")
    assert eng.head is None and not any(nm.startswith("head.") for nm in eng.get_params())
    pl = eng.triplet_train_step(x, LABELS, mining, soft, margin, drop_masks=None)
    ref, an = _oracle_with_validated_indices(arch, p, x, None, pl, mining, soft, margin, "f32")
    tag = "triplet_step[f32-%s]" % R.variant_id(variant)
    la = pl["loss_acc"].cpu().numpy()
    report(tag, "emb_rel_err_vs_fp64", rel_err(pl["emb"].cpu().numpy(), ref["e"].numpy()))
    report(tag, "loss_abs_err_vs_fp64", abs(la[0] - ref["loss"]))
    print(tag, "margin", margin, "loss", la[0], ref["loss"], "share", la[1], an["share"])
    assert rel_err(pl["emb"].cpu().numpy(), ref["e"].numpy()) < 1e-4
    assert abs(la[0] - ref["loss"]) < 1e-4
    assert abs(la[1] - an["share"]) < 1e-6
    grads = eng.get_grads()
    assert set(grads) == set(ref["grads"])
    for k, g in ref["grads"].items():
        report(tag, "grad_rel_err[%s]" % k, rel_err(grads[k], g.numpy()))
        assert grad_close(grads[k], g.numpy(), 2e-3), k
    _check_params_after_adam(eng.get_params(), ref["params"], ref["grads"], 1e-5)
    assert eng.iterations == 1


def test_f16_step_with_given_dropout_masks():
    rate = 0.05
    mining, soft = F16_VARIANT
    arch, p, x, masks = _tiny_batch(seed=F16_SEED, dropout=rate)
    e64 = O.encoder_forward(arch, p, torch.tensor(x), True, masks).numpy()
    margin = MARGIN_FRACTION * _mean_pair_distance(e64)
    eng = _engine(arch, p, "f16")
    dm = [(m[:, 0, :] / (1.0 - rate)).to("cuda", torch.float32).contiguous() for m in masks]
    # one step from a cold start: the loss scale is searched first, as a training loop's polls would (engine.calibrate_loss_scale)
    eng.calibrate_loss_scale(lambda: eng.triplet_train_step(x, LABELS, mining, soft, margin, drop_masks=dm, apply_update=False))
    pl = eng.triplet_train_step(x, LABELS, mining, soft, margin, drop_masks=dm)
    ref, an = _oracle_with_validated_indices(arch, p, x, masks, pl, mining, soft, margin, "f16")
    grads = eng.get_grads()
    assert torch.isfinite(eng.G).all() and eng.skipped_steps() == 0
    g_all = np.concatenate([np.asarray(grads[k], dtype=np.float64).ravel() for k in ref["grads"]])
    r_all = np.concatenate([g.numpy().ravel() for g in ref["grads"].values()])
    loss = pl["loss_acc"][0].item()
    tag = "triplet_step[f16]"
    report(tag, "loss_abs_err", abs(loss - ref["loss"]))
    report(tag, "emb_rel_err_vs_fp64", rel_err(pl["emb"].cpu().numpy(), ref["e"].numpy()))
    report(tag, "grad_rel_err", rel_err(g_all, r_all))
    report(tag, "grad_cosine", cosine(g_all, r_all))
    print(tag, "margin", margin, "loss scale", eng.loss_scale, "loss", loss, ref["loss"], "emb", rel_err(pl["emb"].cpu().numpy(), ref["e"].numpy()),
          "grad rel", rel_err(g_all, r_all), "cos", cosine(g_all, r_all))
    assert np.linalg.norm(pl["emb"].cpu().numpy() - ref["e"].numpy()) < EMB_THRESHOLD["f16"] * _emb_norm(ref["e"].numpy(), p, "f16")
    assert abs(loss - ref["loss"]) < 5e-3
    assert cosine(g_all, r_all) > 0.99


def _same_state(a, b, what):
    for nm in ("P", "M", "V", "NT", "ZD", "G"):
        u, v = getattr(a, nm), getattr(b, nm)
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (what, nm)
    assert a.iterations == b.iterations and a.bn_steps == b.bn_steps and a.loss_scale == b.loss_scale, what


def _pair_of_engines(dtype, dropout):
    from voicemap_amd.engine import HipEncoderEngine
    a = HipEncoderEngine(BLOCKS, 32, dropout=dropout, head=None, dtype=dtype, seed=5)
    b = HipEncoderEngine(BLOCKS, 32, dropout=dropout, head=None, dtype=dtype, seed=5)
    return a, b


@pytest.mark.parametrize("dtype,dropout", [("f16", 0.05), ("f32", 0.0)])
def test_replayed_steps_are_the_eager_steps(dtype, dropout):
    a, b = _pair_of_engines(dtype, dropout)
    b.replay = False
    r = np.random.default_rng(3)
    for step in range(5):
        x = r.normal(0, 0.05, (N_WIN, 4800, 1)).astype(np.float32)
        labels = r.permutation(LABELS) + 100 * step          # any values, any order: they are patched in, not recorded
        out = []
        for eng in (a, b):
            pl = eng.triplet_train_step(x, labels, R.HARD, 0, 3.0, preprocessed=False, downsampling=4)
            torch.cuda.synchronize()
            out.append((pl["loss_acc"].clone(), pl["emb"].clone(), pl["triplet"]["hard_pos"].clone(), pl["triplet"]["hard_neg"].clone()))
        for u, v in zip(*out):
            assert torch.equal(u, v), step
        assert (out[0][2] >= 0).all()
        _same_state(a, b, step)
    progs = a._programs.recorded()
    assert len(progs) == 1 and not b._programs.recorded()       # recorded at the second sighting, replayed from the third
    names = {k if not isinstance(k, tuple) else k[0] for _, _, k in progs[0].patches}
    assert "y" in names and names <= {"raw", "y", "loss_scale", "zc", "lr_t", "gpre", "drop", "dropb"}
    # (mining, soft, margin) are part of the key: another margin, mining or the soft margin is another program, never a stale replay
    x = r.normal(0, 0.05, (N_WIN, 4800, 1)).astype(np.float32)
    for kw in (dict(mining=R.HARD, soft=0, margin=1.5), dict(mining=R.ALL, soft=0, margin=3.0), dict(mining=R.HARD, soft=1, margin=3.0)):
        for step in range(3):
            for eng in (a, b):
                eng.triplet_train_step(x, LABELS, preprocessed=False, downsampling=4, **kw)
            torch.cuda.synchronize()
            _same_state(a, b, (kw, step))
    assert len(a._programs.recorded()) == 4
    # the soft margin ignores ``margin``: no new program for another value
    for step in range(2):
        for eng in (a, b):
            eng.triplet_train_step(x, LABELS, R.HARD, 1, 9.0, preprocessed=False, downsampling=4)
        _same_state(a, b, ("soft", step))
    assert len(a._programs.recorded()) == 4


def test_the_offsets_path_is_the_raw_window_path():
    a, b = _pair_of_engines("f16", 0.05)
    g = torch.Generator(device="cuda").manual_seed(1)
    audio = (torch.randn(200000, device="cuda", generator=g) * 0.05 * 32767).clamp(-32767, 32767).to(torch.int16)
    r = np.random.default_rng(6)
    T = 4800
    for step in range(4):
        off = r.integers(0, 200000 - T, N_WIN).astype(np.int64)
        labels = LABELS[:, None]
        windows = audio[torch.as_tensor(off, device="cuda")[:, None] + torch.arange(T, device="cuda")[None, :]]
        pa = a.triplet_train_step_from_offsets(audio, off, labels, T, R.ALL, 0, 3.0)
        pb = b.triplet_train_step(windows, labels, R.ALL, 0, 3.0, preprocessed=False, downsampling=4)
        torch.cuda.synchronize()
        assert torch.equal(pa["loss_acc"], pb["loss_acc"]) and torch.equal(pa["emb"], pb["emb"]), step
        _same_state(a, b, step)
    # device tensors are taken as they are
    pa = a.triplet_train_step_from_offsets(audio, torch.as_tensor(off, device="cuda"), torch.as_tensor(labels, device="cuda"), T, R.ALL, 0, 3.0)
    pb = b.triplet_train_step(windows, labels, R.ALL, 0, 3.0, preprocessed=False, downsampling=4)
    torch.cuda.synchronize()
    assert torch.equal(pa["loss_acc"], pb["loss_acc"])
    _same_state(a, b, "tensors")


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_evaluation_uses_the_moving_statistics_and_the_same_loss(variant):
    mining, soft = variant
    arch, p, x, _ = _tiny_batch(seed=2)
    eng = _engine(arch, p, "f32")
    lab = LABELS.copy()
    lab[5] = -1                                              # a window that takes no part
    pl = eng.triplet_eval(x, lab, mining, soft, 0.5)
    emb = pl["emb"].cpu().numpy()
    e_ref = O.encoder_forward(arch, p, torch.tensor(x), False).numpy()
    assert rel_err(emb, e_ref) < 1e-4
    out = {"hp": pl["triplet"]["hard_pos"].cpu().numpy(), "hn": pl["triplet"]["hard_neg"].cpu().numpy(),
           "loss": float(pl["loss_acc"][0]), "share": float(pl["loss_acc"][1])}
    bad, w, an = R.check(out, emb, lab, mining, soft, 0.5)   # the loss of the embeddings the engine holds
    assert not bad and all(v <= 1.0 for v in w.values()), (bad, w)
    assert out["hp"][5] == -1 and an["V"] == N_WIN - 1
    assert "demb" not in pl and eng.iterations == 0


def test_public_surface_on_synthetic_speech(tmp_path):
    from voicemap_amd import keras_like as K, models, utils
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    np.random.seed(0)
    train = SyntheticSpeechDataset(num_speakers=10, files_per_speaker=5, seconds=0.5, seed=1)
    valid = SyntheticSpeechDataset(num_speakers=8, files_per_speaker=4, seconds=0.5, stochastic=False, seed=9)
    pp, kk = 4, 3
    bp = utils.BatchPreProcessor("classifier", utils.preprocess_instances(4))
    enc = models.get_baseline_convolutional_encoder(16, 32, dropout=0.05, dtype="f32")
    with pytest.raises(RuntimeError, match="the bare encoder has no loss"):
        enc.train_on_batch(*bp(train.build_speaker_batch(pp, kk)))
    cfg = {"margin": 0.5, "mining": "all"}
    enc.compile(loss=utils.TripletLoss(**cfg), optimizer=K.Adam(clipnorm=1.))
    x, y = bp(train.build_speaker_batch(pp, kk))
    loss, share = enc.train_on_batch(x, y)
    assert np.isfinite(loss) and 0.0 <= share <= 1.0 and enc.engine.iterations == 1 and enc.engine.head is None
    l1, a1 = enc.test_on_batch(x, y)
    l2, a2 = enc.test_on_batch(np.asarray(x), y)             # the host-preprocessed windows: the same batch
    assert np.isfinite(l1) and abs(l1 - l2) < 1e-4 * max(1.0, abs(l1)) and abs(a1 - a2) < 0.02
    emb = enc.predict(x)
    assert abs(utils.TripletLoss(**cfg)(emb, y) - l1) < 1e-4 * max(1.0, abs(l1))
    gen = (bp(b) for b in train.yield_speaker_batches(pp, kk))
    vgen = (bp(b) for b in valid.yield_speaker_batches(pp, kk))
    hist = enc.fit_generator(gen, steps_per_epoch=2, epochs=1, verbose=0, workers=0, validation_data=vgen, validation_steps=1,
                             callbacks=[utils.NShotEvaluationCallback(4, 1, 3, valid, preprocessor=bp, mode="encoder")])
    assert enc.engine.iterations == 3 and np.isfinite(hist.history["loss"]).all()
    assert set(hist.history) >= {"loss", "acc", "val_loss", "val_acc", "val_1-shot_acc"}
    assert np.isfinite(enc.evaluate_generator((bp(b) for b in valid.yield_speaker_batches(pp, kk)), steps=2, workers=0)).all()
    # a saved model reloads as a bare encoder with the loss and its parameters, and embeds alike
    want = enc.predict(x)
    for ext in ("npz", "hdf5"):
        path = str(tmp_path / ("triplet." + ext))
        enc.save(path)
        back = models.load_model(path)
        assert isinstance(back, models.ConvolutionalEncoder) and not back.classifier_units
        assert isinstance(back.loss, utils.TripletLoss) and back.loss.get_config() == cfg
        be = back._ensure_engine()
        assert be.head is None and be.iterations == 3 and torch.equal(be.P, enc.engine.P)
        assert np.array_equal(back.predict(x), want)
    # the soft margin and batch hard through the same surface
    soft = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    soft.compile(loss=utils.TripletLoss("soft", "hard"), optimizer=K.Adam(clipnorm=1.))
    ls, _ = soft.train_on_batch(x, y)
    assert np.isfinite(ls) and ls > 0
    path = str(tmp_path / "soft.npz")
    soft.save(path)
    assert models.load_model(path).loss.get_config() == {"margin": "soft", "mining": "hard"}


def test_device_windows_go_to_the_offsets_path(tmp_path):
    """LazyWindows over shards.DeviceWindows (the resident corpus): train_on_batch crops on the device from one pinned upload of
    offsets and labels, and is the step on the gathered windows bit for bit."""
    from voicemap_amd import keras_like as K, models, shards, utils
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    src = SyntheticSpeechDataset(num_speakers=6, files_per_speaker=4, seconds=0.5, seed=1)
    shards.write_shards(src, str(tmp_path))
    ds = shards.ShardedSpeechDataset(str(tmp_path), 0.5)
    ds.to_device("cuda")
    pp, kk = 3, 3
    bp = utils.BatchPreProcessor("classifier", utils.preprocess_instances(4))
    a = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    b = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    for enc in (a, b):
        enc.compile(loss=utils.TripletLoss(0.3), optimizer=K.Adam(clipnorm=1.))
    b.set_weights(a.get_weights())
    np.random.seed(2)
    for step in range(4):
        x, y = bp(ds.build_speaker_batch_device(pp, kk))
        assert isinstance(x.raw, shards.DeviceWindows) and x.shape == (pp * kk, 2000, 1)
        pa = a._train_step(x, y)
        assert ("h2d_episode", pp * kk) in pa                                # the offsets path's staging ring
        pb = b.engine.triplet_train_step(x.raw.gather(), y, R.HARD, 0, 0.3, preprocessed=False, downsampling=4)
        torch.cuda.synchronize()
        assert torch.equal(pa["loss_acc"], pb["loss_acc"]) and torch.equal(a.engine.P, b.engine.P), step
    la = a.test_on_batch(x, y)
    assert np.isfinite(la).all()
