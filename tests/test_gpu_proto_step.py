"""-m gpu: the prototypical training step (engine.prototypical_train_step: the whole k-way n-shot episode one encoder call, the loss
by vm_proto_loss, no head parameters) against the float64 oracle, its replayed form against the eager one, the offsets path against
the raw-window path, and the public surface (compile(loss=PrototypicalLoss) on the bare encoder, mode="encoder" n-shot evaluation,
checkpoints)."""
import numpy as np
import pytest
import torch

from oracle import voicemap_oracle as O
from tests import proto_refs as R
from tests.gpu_util import cosine, grad_close, max_err, rel_err, report

pytestmark = pytest.mark.gpu

BLOCKS = [(32, 16, 4), (3, 32, 2), (3, 48, 2), (3, 64, 2)]
K_WAY, N_SHOT, M_QUERY = 4, 2, 8


def _tiny_episode(seed=0, l0=1200, dropout=0.0):
    """The tiny case of tests/test_gpu_e2e.py for a bare encoder: non-trivial BatchNorm parameters (some negative gammas), 16 whitened
    windows as one 4-way 2-shot episode with 8 unbalanced queries."""
    arch = O.EncoderArch.baseline(16, 32, dropout=dropout)
    p = O.init_params(arch, head=None, seed=seed)
    r = np.random.default_rng(seed)
    for i in range(1, 5):
        c = p[f"bn{i}.gamma"].shape[0]
        p[f"bn{i}.gamma"] = torch.tensor(r.normal(1.0, 0.2, c) * np.where(r.random(c) < 0.15, -1, 1))
        p[f"bn{i}.beta"] = torch.tensor(r.normal(0.0, 0.2, c))
        p[f"conv{i}.bias"] = torch.tensor(r.normal(0.0, 0.05, c))
    N = K_WAY * N_SHOT + M_QUERY
    x = O.whiten(r.normal(0, 0.05, (N, l0, 1)) + r.uniform(-0.01, 0.01, (N, 1, 1))).astype(np.float32).astype(np.float64)
    labels = np.array([0, 3, 3, 1, 2, 3, 0, 3], dtype=np.int32)
    masks = None
    if dropout > 0:
        masks = [torch.tensor((r.random((N, 1, c)) >= dropout).astype(np.float64)) for (_, c, _) in arch.blocks]
    return arch, p, x, labels, masks


def _alpha(arch, p, x, masks, scale=1.0):
    """alpha = scale / (mean squared query-prototype distance of the float64 embeddings): the logits are then O(1), the softmax is
    neither uniform nor one-hot and the loss is O(1) -- what a user tunes alpha for, and the regime the project's absolute thresholds
    (loss 1e-4 / 5e-3, grad_close's atol of 1e-7 for gradients that are analytically zero: here bn4.beta and dense.bias, the loss only
    sees differences of embeddings) were set in.  An untrained encoder puts its embeddings ~10 apart: with alpha = 1 the loss is
    14 .. 100 and its gradient norm ~2000, three orders of magnitude above the pair losses'."""
    e = O.encoder_forward(arch, p, torch.tensor(x), True, masks)
    proto = e[:K_WAY * N_SHOT].reshape(K_WAY, N_SHOT, -1).mean(1)
    return scale / float(((e[K_WAY * N_SHOT:, None] - proto[None]) ** 2).sum(-1).mean())


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


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_tiny_step_matches_the_oracle_in_f32(scale):
    arch, p, x, labels, _ = _tiny_episode()
    alpha = _alpha(arch, p, x, None, scale)
    eng = _engine(arch, p, "f32")
    assert eng.head is None and not any(nm.startswith("head.") for nm in eng.get_params())
    pl = eng.prototypical_train_step(x, labels, K_WAY, N_SHOT, alpha, drop_masks=None)
    ref = R.proto_step_oracle(arch, p, O.AdamState(), torch.tensor(x), labels, K_WAY, N_SHOT, alpha)
    tag = "proto_step[f32-scale%g]" % scale
    la = pl["loss_acc"].cpu().numpy()
    report(tag, "emb_rel_err_vs_fp64", rel_err(pl["emb"].cpu().numpy(), ref["e"].numpy()))
    report(tag, "loss_abs_err_vs_fp64", abs(la[0] - ref["loss"]))
    print(tag, "alpha", alpha, "loss", la[0], ref["loss"], "acc", la[1], ref["acc"])
    assert rel_err(pl["emb"].cpu().numpy(), ref["e"].numpy()) < 1e-4
    assert abs(la[0] - ref["loss"]) < 1e-4
    assert rel_err(pl[("proto", K_WAY, N_SHOT)]["logits"].cpu().numpy(), ref["logits"]) < 1e-4
    assert abs(la[1] - ref["acc"]) < 1e-6
    grads = eng.get_grads()
    assert set(grads) == set(ref["grads"])
    for k, g in ref["grads"].items():
        report(tag, "grad_rel_err[%s]" % k, rel_err(grads[k], g.numpy()))
        assert grad_close(grads[k], g.numpy(), 2e-3), k
    _check_params_after_adam(eng.get_params(), ref["params"], ref["grads"], 1e-5)
    assert eng.iterations == 1


def test_f16_step_with_given_dropout_masks():
    rate = 0.05
    arch, p, x, labels, masks = _tiny_episode(seed=1, dropout=rate)
    alpha = _alpha(arch, p, x, masks)
    eng = _engine(arch, p, "f16")
    dm = [(m[:, 0, :] / (1.0 - rate)).to("cuda", torch.float32).contiguous() for m in masks]
    # one step from a cold start: the loss scale is searched first, as a training loop's polls would (engine.calibrate_loss_scale)
    eng.calibrate_loss_scale(lambda: eng.prototypical_train_step(x, labels, K_WAY, N_SHOT, alpha, drop_masks=dm, apply_update=False))
    pl = eng.prototypical_train_step(x, labels, K_WAY, N_SHOT, alpha, drop_masks=dm)
    ref = R.proto_step_oracle(arch, p, O.AdamState(), torch.tensor(x), labels, K_WAY, N_SHOT, alpha, drop_masks=masks)
    grads = eng.get_grads()
    assert torch.isfinite(eng.G).all() and eng.skipped_steps() == 0
    g_all = np.concatenate([np.asarray(grads[k], dtype=np.float64).ravel() for k in ref["grads"]])
    r_all = np.concatenate([g.numpy().ravel() for g in ref["grads"].values()])
    loss = pl["loss_acc"][0].item()
    tag = "proto_step[f16]"
    report(tag, "loss_abs_err", abs(loss - ref["loss"]))
    report(tag, "emb_rel_err_vs_fp64", rel_err(pl["emb"].cpu().numpy(), ref["e"].numpy()))
    report(tag, "grad_rel_err", rel_err(g_all, r_all))
    report(tag, "grad_cosine", cosine(g_all, r_all))
    print(tag, "alpha", alpha, "loss scale", eng.loss_scale, "loss", loss, ref["loss"], "emb", rel_err(pl["emb"].cpu().numpy(), ref["e"].numpy()), "grad rel", rel_err(g_all, r_all),
          "cos", cosine(g_all, r_all))
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
    N = K_WAY * N_SHOT + M_QUERY
    for step in range(5):
        x = r.normal(0, 0.05, (N, 4800, 1)).astype(np.float32)
        labels = r.integers(0, K_WAY, M_QUERY)
        out = []
        for eng in (a, b):
            pl = eng.prototypical_train_step(x, labels, K_WAY, N_SHOT, 1.0, preprocessed=False, downsampling=4)
            torch.cuda.synchronize()
            out.append((pl["loss_acc"].clone(), pl["emb"].clone(), pl[("proto", K_WAY, N_SHOT)]["logits"].clone()))
        for u, v in zip(*out):
            assert torch.equal(u, v), step
        _same_state(a, b, step)
    progs = a._programs.recorded()
    assert len(progs) == 1 and not b._programs.recorded()
    names = {k if not isinstance(k, tuple) else k[0] for _, _, k in progs[0].patches}
    assert "y" in names and names <= {"raw", "y", "loss_scale", "zc", "lr_t", "gpre", "drop", "dropb"}
    # (k, n, alpha) are part of the key: another alpha or another split of the same 16 windows is another program, never a stale replay
    x = r.normal(0, 0.05, (N, 4800, 1)).astype(np.float32)
    for kw in (dict(k=K_WAY, n=N_SHOT, alpha=0.5), dict(k=2, n=4, alpha=1.0)):
        labels = r.integers(0, kw["k"], M_QUERY)
        for step in range(3):
            for eng in (a, b):
                eng.prototypical_train_step(x, labels, kw["k"], kw["n"], kw["alpha"], preprocessed=False, downsampling=4)
            torch.cuda.synchronize()
            _same_state(a, b, (kw, step))
    assert len(a._programs.recorded()) == 3


def test_the_offsets_path_is_the_raw_window_path():
    a, b = _pair_of_engines("f16", 0.05)
    g = torch.Generator(device="cuda").manual_seed(1)
    audio = (torch.randn(200000, device="cuda", generator=g) * 0.05 * 32767).clamp(-32767, 32767).to(torch.int16)
    r = np.random.default_rng(6)
    N, T = K_WAY * N_SHOT + M_QUERY, 4800
    for step in range(4):
        off = r.integers(0, 200000 - T, N).astype(np.int64)
        labels = r.integers(0, K_WAY, (M_QUERY, 1))
        windows = audio[torch.as_tensor(off, device="cuda")[:, None] + torch.arange(T, device="cuda")[None, :]]
        pa = a.prototypical_train_step_from_offsets(audio, off, labels, T, K_WAY, N_SHOT)
        pb = b.prototypical_train_step(windows, labels, K_WAY, N_SHOT, preprocessed=False, downsampling=4)
        torch.cuda.synchronize()
        assert torch.equal(pa["loss_acc"], pb["loss_acc"]) and torch.equal(pa["emb"], pb["emb"]), step
        _same_state(a, b, step)
    # device tensors are taken as they are
    pa = a.prototypical_train_step_from_offsets(audio, torch.as_tensor(off, device="cuda"), torch.as_tensor(labels, device="cuda"), T, K_WAY, N_SHOT)
    pb = b.prototypical_train_step(windows, labels, K_WAY, N_SHOT, preprocessed=False, downsampling=4)
    torch.cuda.synchronize()
    assert torch.equal(pa["loss_acc"], pb["loss_acc"])
    _same_state(a, b, "tensors")


def test_evaluation_uses_the_moving_statistics_and_the_same_loss():
    arch, p, x, labels, _ = _tiny_episode(seed=2)
    eng = _engine(arch, p, "f32")
    pl = eng.prototypical_eval(x, labels, K_WAY, N_SHOT, 0.5)
    emb = pl["emb"].cpu().numpy()
    e_ref = O.encoder_forward(arch, p, torch.tensor(x), False).numpy()
    assert rel_err(emb, e_ref) < 1e-4
    ref = R.proto_ref(emb, labels, K_WAY, N_SHOT, 0.5)       # the loss of the embeddings the engine holds
    bnd = R.proto_bounds(emb, labels, K_WAY, N_SHOT, 0.5, ref)
    la = pl["loss_acc"].cpu().numpy()
    assert abs(la[0] - ref["loss"]) <= bnd["loss"] and abs(la[1] - ref["acc"]) <= bnd["acc"]
    assert (np.abs(pl["proto_logits"].cpu().numpy() - ref["logits"]) <= bnd["logits"]).all()
    assert "demb" not in pl and eng.iterations == 0


def test_public_surface_on_synthetic_speech(tmp_path):
    from voicemap_amd import keras_like as K, models, utils
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    np.random.seed(0)
    train = SyntheticSpeechDataset(num_speakers=10, files_per_speaker=5, seconds=0.5, seed=1)
    valid = SyntheticSpeechDataset(num_speakers=8, files_per_speaker=4, seconds=0.5, stochastic=False, seed=9)
    k, n, q = 4, 2, 2
    bp = utils.BatchPreProcessor("classifier", utils.preprocess_instances(4))
    enc = models.get_baseline_convolutional_encoder(16, 32, dropout=0.05, dtype="f32")
    with pytest.raises(RuntimeError, match="the bare encoder has no loss"):
        enc.train_on_batch(*bp(train.build_episode(k, n, q)))
    enc.compile(loss=utils.PrototypicalLoss(k, n, alpha=0.5), optimizer=K.Adam(clipnorm=1.))
    x, y = bp(train.build_episode(k, n, q))
    loss, acc = enc.train_on_batch(x, y)
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0 and enc.engine.iterations == 1 and enc.engine.head is None
    l1, a1 = enc.test_on_batch(x, y)
    l2, a2 = enc.test_on_batch(np.asarray(x), y)             # the host-preprocessed windows: the same batch
    assert np.isfinite(l1) and abs(l1 - l2) < 1e-4 * max(1.0, abs(l1)) and a1 == a2
    emb = enc.predict(x)
    assert abs(utils.PrototypicalLoss(k, n, alpha=0.5)(emb, y) - l1) < 1e-4 * max(1.0, abs(l1))
    gen = (bp(b) for b in train.yield_episodes(k, n, q))
    vgen = (bp(b) for b in valid.yield_episodes(k, n, q))
    hist = enc.fit_generator(gen, steps_per_epoch=2, epochs=1, verbose=0, workers=0, validation_data=vgen, validation_steps=1,
                             callbacks=[utils.NShotEvaluationCallback(4, 1, 3, valid, preprocessor=bp, mode="encoder")])
    assert enc.engine.iterations == 3 and np.isfinite(hist.history["loss"]).all()
    assert set(hist.history) >= {"loss", "acc", "val_loss", "val_acc", "val_1-shot_acc"}
    assert np.isfinite(enc.evaluate_generator((bp(b) for b in valid.yield_episodes(k, n, q)), steps=2, workers=0)).all()
    # a saved model reloads as a bare encoder with the loss and its parameters, and embeds alike
    want = enc.predict(x)
    for ext in ("npz", "hdf5"):
        path = str(tmp_path / ("proto." + ext))
        enc.save(path)
        back = models.load_model(path)
        assert isinstance(back, models.ConvolutionalEncoder) and not back.classifier_units
        assert isinstance(back.loss, utils.PrototypicalLoss) and back.loss.get_config() == {"k_way": k, "n_shot": n, "alpha": 0.5}
        be = back._ensure_engine()
        assert be.head is None and be.iterations == 3 and torch.equal(be.P, enc.engine.P)
        assert np.array_equal(back.predict(x), want)
        assert [w.shape for w in back.get_weights()] == [w.shape for w in enc.get_weights()] and len(back.get_weights()) == 26


def test_device_windows_go_to_the_offsets_path(tmp_path):
    """LazyWindows over shards.DeviceWindows (the resident corpus): train_on_batch crops on the device from one pinned upload of
    offsets and labels, and is the step on the gathered windows bit for bit."""
    from voicemap_amd import keras_like as K, models, shards, utils
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    src = SyntheticSpeechDataset(num_speakers=6, files_per_speaker=4, seconds=0.5, seed=1)
    shards.write_shards(src, str(tmp_path))
    ds = shards.ShardedSpeechDataset(str(tmp_path), 0.5)
    ds.to_device("cuda")
    k, n, q = 3, 2, 2
    bp = utils.BatchPreProcessor("classifier", utils.preprocess_instances(4))
    a = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    b = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    for enc in (a, b):
        enc.compile(loss=utils.PrototypicalLoss(k, n), optimizer=K.Adam(clipnorm=1.))
    b.set_weights(a.get_weights())
    np.random.seed(2)
    for step in range(4):
        x, y = bp(ds.build_episode_device(k, n, q))
        assert isinstance(x.raw, shards.DeviceWindows) and x.shape == (k * (n + q), 2000, 1)
        pa = a._train_step(x, y)
        assert ("h2d_episode", k * q) in pa                                  # the offsets path's staging ring
        pb = b.engine.prototypical_train_step(x.raw.gather(), y, k, n, 1.0, preprocessed=False, downsampling=4)
        torch.cuda.synchronize()
        assert torch.equal(pa["loss_acc"], pb["loss_acc"]) and torch.equal(a.engine.P, b.engine.P), step
    la = a.test_on_batch(x, y)
    assert np.isfinite(la).all()
