"""-m gpu tests of vm_resample_i16 (voicemap_amd/csrc/speed.hip) against ``resample_reference`` (tests/speed_cases.py holds the cases and
their references), and of speed perturbation through the public surface.  Every comparison is equality; guard words lie before and
after the output buffer and between the utterances' outputs, which are laid out in another order than the inputs."""
import numpy as np
import pytest
import torch

from tests import speed_cases as SC
from voicemap_amd import speed as S

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, 12345


def run(buf, offsets, lens, U, D, taps, shift, seed=0):
    """One vm_resample_i16 call with the outputs in a shuffled order, one to nine guard words between them and GUARD around them ->
    the list of per-utterance outputs on the host (every guard word checked)."""
    from voicemap_amd import _lib
    rng = np.random.RandomState(seed)
    n, T = len(lens), len(taps) // U
    n_out = S.output_length(np.asarray(lens, dtype=np.int64), U, D)
    base = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
    new_offsets, cur = np.zeros(n, dtype=np.int64), GUARD
    for u in rng.permutation(n):
        new_offsets[u] = cur
        cur += int(n_out[u]) + int(rng.randint(1, 10))
    out = torch.full((cur + GUARD,), SENT, dtype=torch.int16, device="cuda")
    audio = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    tab = torch.from_numpy(np.concatenate([offsets, lens, base, new_offsets]).astype(np.int64)).cuda()
    taps_dev = torch.from_numpy(np.asarray(taps).astype(np.int32)).cuda()
    e = tab.element_size()
    _lib.lib().call("vm_resample_i16", audio.data_ptr(), tab.data_ptr(), tab.data_ptr() + n * e, tab.data_ptr() + 2 * n * e, n, U, D,
                    taps_dev.data_ptr(), T, shift, S.phase_abs_max(taps, U), tab.data_ptr() + (3 * n + 1) * e, out.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    written = np.zeros(len(h), dtype=bool)
    for u in range(n):
        written[new_offsets[u]:new_offsets[u] + n_out[u]] = True
    assert (h[~written] == SENT).all(), ("a guard word was overwritten", np.flatnonzero(~written & (h != SENT))[:8])
    return [h[new_offsets[u]:new_offsets[u] + n_out[u]] for u in range(n)]


def check(name, got, ref, lens, U, D, T):
    """Equality, reported by utterance, output index, phase and tile of the flat output list."""
    base = np.concatenate([[0], np.cumsum([len(r) for r in ref])])
    tile, c = S.tile_outputs(U, D, T), (U * T) // 2
    for u, (g, r) in enumerate(zip(got, ref)):
        assert len(g) == len(r)
        bad = np.flatnonzero(g != r)
        if bad.size:
            m = int(bad[0])
            pytest.fail("%s: utterance %d (len %d), output %d of %d, phase %d, tile %d (offset %d in it): got %d, want %d; %d outputs differ"
                        % (name, u, lens[u], m, len(r), (m * D + c) % U, (base[u] + m) // tile, (base[u] + m) % tile, g[m], r[m], bad.size))


GRID = [(U, D, T) for (U, D) in SC.RATIOS for T in SC.TAPS_PER_PHASE]


@pytest.mark.parametrize("U,D,T", GRID, ids=["%d-%d-T%d" % g for g in GRID])
def test_case_grid(U, D, T):
    """Utterance lengths around one thread's and one tile's outputs, the filter length, 0 and 1, back to back with poison between, under
    taps the 32-bit accumulator takes and taps only the 64-bit one can."""
    case = SC.grid_case(U, D, T)
    for k, (taps, shift) in enumerate(case["tables"]):
        assert (S.phase_abs_max(taps, U) <= S.NARROW_MAX) == (k == 0)
        got = run(case["buf"], case["offsets"], case["lens"], U, D, taps, shift, seed=k)
        check("%s table %d" % (case["name"], k), got, SC.reference(case, k), case["lens"], U, D, T)


@pytest.mark.parametrize("U,D", ((10, 9), (10, 11)))
def test_default_design_on_full_scale_noise_clips(U, D):
    """Random full-scale int16 and square waves at the filter's worst case under the default design: the clip occurs (and at 10/9 a
    32-bit accumulator would wrap)."""
    rng = np.random.RandomState(U + D)
    taps = S.design_taps(U, D)
    utts = [rng.randint(-32768, 32768, n).astype(np.int16) for n in (5000, 1, 2049, 333)]
    # full scale with the signs of one phase's taps, reversed in time: that output's accumulator is phase_abs_max * 2^15
    worst = np.where(taps[0::U][::-1] >= 0, 32767, -32768).astype(np.int16)
    utts += [np.tile(worst, 8), np.tile(~worst, 8), rng.choice(np.array([-32768, 32767], dtype=np.int16), 4000)]
    buf, offsets, lens = SC.pack(utts, rng, prefix=5)
    ref = [S.resample_reference(u, U, D, taps, 15) for u in utts]
    assert any((r == 32767).any() for r in ref) and any((r == -32768).any() for r in ref), "no sample clips"
    check("default %d/%d" % (U, D), run(buf, offsets, lens, U, D, taps, 15), ref, lens, U, D, 32)


@pytest.mark.parametrize("plant", SC.plants(), ids=[p[0] for p in SC.plants()])
def test_plants(plant):
    name, x, U, D, taps, shift, want = plant
    buf, offsets, lens = SC.pack([x, x[:3], x], np.random.RandomState(1), prefix=1)
    got = run(buf, offsets, lens, U, D, taps, shift)
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want), (name, got[0], want)
    check(name, got, [S.resample_reference(buf[o:o + n], U, D, taps, shift) for o, n in zip(offsets, lens)], lens, U, D, len(taps) // U)


def test_accumulator_edges():
    """phase_abs_max on either side of the switch between the two accumulators, on the input that drives the sum to its bound."""
    for mag in (S.NARROW_MAX, S.NARROW_MAX + 1):
        for sign in (1, -1):
            taps = np.array([sign * (mag - 3), 0, sign * 3, 0], dtype=np.int64)   # U = 2: phase 0 sums to mag, phase 1 to nothing
            x = np.full(50, -32768, dtype=np.int16)
            x[20:30] = 32767
            buf, offsets, lens = SC.pack([x, x[::-1].copy()], np.random.RandomState(2), prefix=2)
            for shift in (0, 15, 30):
                ref = [S.resample_reference(buf[o:o + n], 2, 1, taps, shift) for o, n in zip(offsets, lens)]
                check("edge %d %d %d" % (mag, sign, shift), run(buf, offsets, lens, 2, 1, taps, shift), ref, lens, 2, 1, 2)


def test_no_utterances_and_empty_files():
    from voicemap_amd import _lib
    _lib.lib().call("vm_resample_i16", None, None, None, None, 0, 10, 9, None, 32, 15, 71012, None, None, None)
    audio = torch.full((100,), 32767, dtype=torch.int16, device="cuda")
    taps = S.design_taps(10, 9)
    out, offs, lens = S.resample(audio, [], [], 10, 9, taps, 15)
    assert out.numel() == 0 and out.dtype == torch.int16 and len(offs) == 0 and len(lens) == 0
    out, offs, lens = S.resample(audio, [3, 50, 7], [0, 0, 0], 10, 9, taps, 15)
    assert out.numel() == 0 and list(lens) == [0, 0, 0]
    got = run(audio.cpu().numpy(), np.array([3, 50, 7, 9]), np.array([0, 0, 1, 0]), 10, 9, taps, 15)
    assert [len(g) for g in got] == [0, 0, 2, 0]
    assert np.array_equal(got[2], S.resample_reference(np.array([32767], dtype=np.int16), 10, 9, taps, 15))


def test_many_utterances():
    """70 000 utterances of 0 to 9 samples: more than a grid's second dimension holds, hundreds of utterances in every tile."""
    rng = np.random.RandomState(7)
    lens = rng.randint(0, 10, 70000).astype(np.int64)
    offsets = 3 + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    buf = np.concatenate([[32767, -32768, 32767], rng.randint(-32768, 32768, int(lens.sum())), np.resize([-32768, 32767], 24)]).astype(np.int16)
    U, D, T = 3, 2, 4
    taps = SC.random_taps(rng, U, T, S.NARROW_MAX)
    audio = torch.from_numpy(buf).cuda()
    out, new_offsets, new_lens = S.resample(audio, offsets, lens, U, D, taps, 15)
    h = out.cpu().numpy()
    assert np.array_equal(new_lens, (lens * U + D - 1) // D) and len(h) == new_lens.sum()
    for u in list(range(400)) + list(range(69990, 70000)):
        want = S.resample_reference(buf[offsets[u]:offsets[u] + lens[u]], U, D, taps, 15)
        assert np.array_equal(h[new_offsets[u]:new_offsets[u] + new_lens[u]], want), u
    # ... and all of them at once: three outputs per two samples, each a sum over the samples of its own utterance only
    again, _, _ = S.resample(audio, offsets, lens, U, D, taps, 15)
    assert torch.equal(out, again)
    flat = np.concatenate([S.resample_reference(buf[o:o + n], U, D, taps, 15) for o, n in zip(offsets[400:3000], lens[400:3000])])
    assert np.array_equal(h[new_offsets[400]:new_offsets[3000]], flat)


def test_resample_through_the_wrapper():
    case = SC.grid_case(7, 5, 31)
    taps, shift = case["tables"][0]
    audio = torch.from_numpy(case["buf"]).cuda()
    out, offs, lens = S.resample(audio, torch.from_numpy(case["offsets"]), case["lens"], 7, 5, taps, shift)
    ref = SC.reference(case, 0)
    assert np.array_equal(lens, [len(r) for r in ref]) and np.array_equal(offs, np.concatenate([[0], np.cumsum(lens)[:-1]]))
    assert np.array_equal(out.cpu().numpy(), np.concatenate(ref))
    big = torch.full((out.numel() + 9,), SENT, dtype=torch.int16, device="cuda")
    got, _, _ = S.resample(audio, case["offsets"], case["lens"], 7, 5, taps, shift, out=big[5:5 + out.numel()])
    assert got.data_ptr() == big.data_ptr() + 10 and torch.equal(got, out) and (big[:5] == SENT).all() and (big[-4:] == SENT).all()
    with pytest.raises(TypeError, match="int16 PCM"):
        S.resample(audio.float(), case["offsets"], case["lens"], 7, 5, taps, shift)
    with pytest.raises(ValueError, match="outside"):
        S.resample(audio, [audio.numel() - 5], [6], 7, 5, taps, shift)
    with pytest.raises(ValueError, match="out must be"):
        S.resample(audio, case["offsets"], case["lens"], 7, 5, taps, shift, out=big)


# ---- through the dataset ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """(the resident dataset, its speed_perturbed() form)"""
    ds = SC.corpus(tmp_path_factory.mktemp("speed_shards"))
    ds.to_device("cuda")
    return ds, ds.speed_perturbed(S.SpeedPolicy())


def test_speed_perturbed_resident_corpus(corpus):
    ds, sp = corpus
    n = len(ds)
    assert type(sp) is type(ds) and len(sp) == 3 * n - 1 and sp.num_classes() == 3 * ds.num_classes()
    h = sp.device_audio.cpu().numpy()
    old = ds.device_audio.cpu().numpy()
    assert h[:len(old)].tobytes() == old.tobytes() and len(h) == len(old) + int(sp.file_length[n:].sum())
    for i in range(len(sp)):
        assert np.array_equal(h[sp.global_offset[i]:sp.global_offset[i] + sp.file_length[i]], sp._pcm(i)), i
    # the host-only route gives the same dataset and uploads the same buffer
    from voicemap_amd import shards
    host = shards.ShardedSpeechDataset(ds.shard_dir, SC.FRAGMENT_SECONDS, pad=False).speed_perturbed(S.SpeedPolicy())
    assert np.array_equal(host.global_offset, sp.global_offset) and host.df.equals(sp.df)
    assert torch.equal(host.to_device("cuda"), sp.device_audio)
    # trimmed first, then perturbed; and a speaker shard's own layout
    from voicemap_amd.vad import VadPolicy
    for base in (ds.voiced(VadPolicy(frame_ms=2.0, min_run=2, hang=3)),
                 shards.ShardedSpeechDataset(ds.shard_dir, SC.FRAGMENT_SECONDS, pad=False, speaker_shard=(0, 2))):
        base.to_device("cuda")
        vs = base.speed_perturbed(S.SpeedPolicy(factors=(1.1,), new_speakers=False))
        assert np.array_equal(vs.device_audio.cpu().numpy(), np.concatenate([vs._pcm(i) for i in range(len(vs))]))
    # the original is untouched
    assert ds._speed is None and ds.device_audio.numel() == len(old) and len(ds) == n


def test_device_crops_of_copies_are_the_hosts(corpus):
    _, sp = corpus
    T = sp.fragment_length
    np.random.seed(3)
    o1, o2, y, f1, f2 = sp.build_verification_batch_offsets(16, files=True)
    np.random.seed(3)
    (w1, w2), y2 = sp.build_verification_batch_device(16)
    assert np.array_equal(w1.offsets_host, o1) and np.array_equal(w2.offsets_host, o2) and (np.concatenate([f1, f2]) >= len(sp) // 3).any()
    for w, o, f in ((w1, o1, f1), (w2, o2, f2)):
        crops = np.stack([sp._pcm(k)[s:s + T] for k, s in zip(f, o - sp.global_offset[f])]).astype(np.float64) / 32768.0
        assert np.array_equal(np.asarray(w)[:, :, 0], crops)


def test_two_training_steps_on_perturbed_batches(corpus):
    """A pair batch through the siamese net and a P x K batch through the triplet encoder: preprocess and train, twice each."""
    from voicemap_amd import keras_like as K
    from voicemap_amd import models, utils
    _, sp = corpus
    np.random.seed(1)
    enc = models.get_baseline_convolutional_encoder(16, 24, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (400, 1), distance_metric="uniform_euclidean")
    net.compile(loss="binary_crossentropy", optimizer=K.Adam(clipnorm=1.), metrics=["accuracy"])
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    for _ in range(2):
        loss = np.asarray(net.train_on_batch(*bp(sp.build_verification_batch_device(8))), dtype=np.float64).reshape(-1)[0]
        assert np.isfinite(loss)
    enc2 = models.get_baseline_convolutional_encoder(16, 24, input_shape=(400, 1), dropout=0.0, dtype="f32")
    enc2.compile(loss=utils.TripletLoss(0.2, "hard"), optimizer=K.Adam(clipnorm=1.), metrics=["accuracy"])
    pre = utils.BatchPreProcessor("classifier", utils.preprocess_instances(4))
    for _ in range(2):
        loss = np.asarray(enc2.train_on_batch(*pre(sp.build_speaker_batch_device(6, 2))), dtype=np.float64).reshape(-1)[0]
        assert np.isfinite(loss)
