"""Host side of the waveform augmentation (voicemap_amd/augment.py): the policy's draws, the synthetic RIR bank, the float64 statement of
the semantics against hand-computed cases, and the script flags.  No GPU."""
import numpy as np
import pytest

from voicemap_amd import augment as A
from voicemap_amd.librispeech import SyntheticSpeechDataset
from voicemap_amd.shards import ShardedSpeechDataset, write_shards


@pytest.fixture(scope="module")
def resident(tmp_path_factory):
    """A small synthetic shard directory, 'resident' on the CPU (to_device('cpu')): 5 speakers x 3 files, 0.25 s fragments."""
    d = str(tmp_path_factory.mktemp("shards"))
    src = SyntheticSpeechDataset(num_speakers=5, files_per_speaker=3, seconds=0.25, min_file_seconds=0.3, max_file_seconds=0.6, seed=3)
    write_shards(src, d)
    ds = ShardedSpeechDataset(d, 0.25, stochastic=True, pad=False)
    ds.to_device("cpu")
    return ds


def _policy(**kw):
    base = dict(p_noise=0.7, snr_db=(0.0, 15.0), babble=(1, 3), p_reverb=0.5, gain_db=(-6.0, 6.0), seed=11,
                rirs=A.synth_rir_bank(4, max_taps=64, seed=1), downsampling=4)
    base.update(kw)
    return A.AugmentPolicy(**base)


def test_same_seed_same_parameters(resident):
    recs = []
    for _ in range(2):
        pol = _policy()
        np.random.seed(5)
        (w1, w2), _ = resident.build_verification_batch_device(8, pol)
        recs.append((w1.aug, w2.aug))
    for a, b in zip(recs[0], recs[1]):
        for name in ("noise_offsets", "snr_lin", "gain", "rir_id"):
            np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    other = _policy(seed=12)
    np.random.seed(5)
    (v1, _), _ = resident.build_verification_batch_device(8, other)
    assert not np.array_equal(v1.aug.gain, recs[0][0].gain)
    # the record has the documented kinds and both towers share one K
    a1, a2 = recs[0]
    assert a1.K == a2.K and 1 <= a1.K <= 3 and a1.noise_offsets.dtype == np.int64 and a1.noise_offsets.shape == (8, a1.K)
    assert a1.snr_lin.dtype == a1.gain.dtype == np.float32 and a1.rir_id.dtype == np.int32
    assert np.all((a1.snr_lin == 0) | ((a1.snr_lin >= 1.0 - 1e-6) & (a1.snr_lin <= 10 ** 1.5 * (1 + 1e-6))))
    assert np.all((a1.gain >= 10 ** (-6 / 20) * (1 - 1e-6)) & (a1.gain <= 10 ** (6 / 20) * (1 + 1e-6)))
    assert np.all((a1.rir_id >= -1) & (a1.rir_id < 4))


def test_rir_bank_is_reproducible_causal_and_unit_energy():
    b1 = A.synth_rir_bank(6, rt60=(0.1, 0.4), max_taps=2000, seed=4)
    b2 = A.synth_rir_bank(6, rt60=(0.1, 0.4), max_taps=2000, seed=4)
    assert b1.dtype == np.float32 and b1.shape == (6, 2000)
    np.testing.assert_array_equal(b1, b2)
    assert not np.array_equal(b1, A.synth_rir_bank(6, rt60=(0.1, 0.4), max_taps=2000, seed=5))
    # unit energy per row (float32 storage: a few ulp of the sum)
    np.testing.assert_allclose(np.sum(b1.astype(np.float64) ** 2, axis=1), 1.0, atol=1e-6)
    # the direct path is tap 0: positive, a UNIT tap in units of itself (the row is the response [1, tail...] scaled to unit energy),
    # nothing precedes it (the array starts there) and it carries half the row's energy (the tail is drawn at 0 dB against it)
    assert np.all(b1[:, 0] > 0)
    np.testing.assert_allclose(b1[:, 0].astype(np.float64) ** 2, 0.5, atol=1e-6)
    # the tail decays: 60 dB in at most 0.4 s = 6400 taps -> over the last quarter of 2000 taps the energy is far below the first quarter's
    e = b1.astype(np.float64) ** 2
    assert np.all(e[:, 1500:].sum(axis=1) < 0.2 * e[:, 1:500].sum(axis=1))
    with pytest.raises(ValueError):
        A.synth_rir_bank(1, max_taps=8193)


def test_pair_and_offset_draws_are_unchanged_by_a_policy(resident):
    np.random.seed(21)
    o1, o2, y = resident.build_verification_batch_offsets(8)
    after_plain = np.random.random_sample()
    np.random.seed(21)
    (w1, w2), y2 = resident.build_verification_batch_device(8, _policy())
    after_aug = np.random.random_sample()
    np.testing.assert_array_equal(w1.offsets_host, o1)
    np.testing.assert_array_equal(w2.offsets_host, o2)
    np.testing.assert_array_equal(y, y2)
    assert after_plain == after_aug      # the global stream stands where it stood: the policy drew from its own
    np.random.seed(21)
    (c1, c2), _ = resident.build_verification_batch_device(8)
    assert c1.aug is None and c2.aug is None
    np.testing.assert_array_equal(c1.offsets_host, o1)
    # and the file ids reported for the babble exclusion are the files the offsets lie in
    np.random.seed(21)
    _, _, _, f1, f2 = resident.build_verification_batch_offsets(8, files=True)
    for o, f in ((o1, f1), (o2, f2)):
        assert np.all((o >= resident.global_offset[f]) & (o + resident.fragment_length <= resident.global_offset[f] + resident.file_length[f]))


def test_noise_crops_lie_inside_one_file_of_another_speaker(resident):
    pol = _policy(p_noise=1.0, babble=(3, 3))
    T = resident.fragment_length
    spk = resident.df['speaker_id'].values
    for seed in range(4):
        np.random.seed(seed)
        _, _, _, f1, f2 = resident.build_verification_batch_offsets(8, files=True)
        files = np.concatenate([f1, f2])
        rec = pol.draw(resident, files, T)
        assert rec.K == 3 and rec.noise is resident.device_audio
        for w in range(len(files)):
            for o in rec.noise_offsets[w]:
                inside = np.flatnonzero((resident.global_offset <= o) & (o + T <= resident.global_offset + resident.file_length))
                assert inside.size == 1, "a noise crop straddles files"
                assert spk[inside[0]] != spk[files[w]], "babble from the window's own speaker"


def test_mining_sampler_attaches_the_record(resident):
    from voicemap_amd.mining import HardPairSampler
    sampler = HardPairSampler(resident, None, hard_fraction=0.0)
    np.random.seed(9)
    o1, o2, _ = resident.build_verification_batch_offsets(8)
    np.random.seed(9)
    (w1, w2), _ = sampler.build_verification_batch_device(8, _policy())
    np.testing.assert_array_equal(w1.offsets_host, o1)
    np.testing.assert_array_equal(w2.offsets_host, o2)
    assert w1.aug is not None and len(w1.aug) == 8 and w1.aug.K == w2.aug.K
    np.random.seed(9)
    (c1, _), _ = sampler.build_verification_batch_device(8)
    assert c1.aug is None


# ---- augment_reference against hand-computed cases -------------------------------------------------------------------------------
def _case(seed=0, n=3, T=41, total=400):
    r = np.random.RandomState(seed)
    audio = r.normal(0, 0.1, total).astype(np.float32)
    noise = r.normal(0, 0.3, total).astype(np.float32)
    off = np.array([0, 17, total - T][:n], dtype=np.int64)
    return audio, noise, off, T


def test_reference_by_hand_small():
    audio = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.float32)
    noise = np.array([1, -1, 1, -1, 1, -1, 1, -1, 1], dtype=np.float32)
    rirs = np.array([[1.0, 0.5, 0.25]], dtype=np.float32)
    d = A.augment_reference(audio, [1], 5, 2, noise=noise, noise_offsets=[[0, 2]], snr_lin=[4.0], gain=[2.0], rirs=rirs, rir_id=[0],
                            whitening=False, details=True)
    # s = [2,3,4,5,6]; positions t = 0,2,4:  a = [2, 4 + 1.5 + 0.5, 6 + 2.5 + 1]
    np.testing.assert_allclose(d["a"], [[2.0, 6.0, 9.5]], rtol=0, atol=1e-15)
    # two voices, both +1 at even samples: v = [2, 2, 2];  Pa = (4 + 36 + 90.25) / 3, Pv = 4
    np.testing.assert_allclose(d["v"], [[2.0, 2.0, 2.0]])
    g = np.sqrt(((4 + 36 + 90.25) / 3) / (4 * 4.0))
    np.testing.assert_allclose(d["g"], [g], rtol=1e-15)
    np.testing.assert_allclose(d["y"], 2.0 * (np.array([[2.0, 6.0, 9.5]]) + g * 2.0), rtol=1e-15)
    assert d["x"].shape == (1, 3 + 31) and np.all(d["x"][:, :15] == 0) and np.all(d["x"][:, -16:] == 0)
    np.testing.assert_array_equal(d["x"][:, 15:18], d["y"])            # whitening off
    np.testing.assert_allclose(d["fir_abs"], [[2.0, 6.0, 9.5]])
    # int16 is read as v / 32768
    d16 = A.augment_reference(np.array([16384, -32768, 8192], dtype=np.int16), [0], 3, 1, whitening=False, details=True)
    np.testing.assert_array_equal(d16["y"], [[0.5, -1.0, 0.25]])


def test_reference_realised_snr_equals_the_request():
    audio, noise, off, T = _case()
    rirs = A.synth_rir_bank(2, max_taps=16, seed=2)
    for snr_db in (-5.0, 0.0, 12.5):
        snr = np.full(3, 10 ** (snr_db / 10), dtype=np.float32)
        d = A.augment_reference(audio, off, T, 3, noise=noise, noise_offsets=[[3, 50], [90, 7], [200, 300]], snr_lin=snr, gain=[1, 2, 0.5],
                                rirs=rirs, rir_id=[-1, 0, 1], details=True)
        Pa, Pv = np.mean(d["a"] ** 2, axis=1), np.mean(d["v"] ** 2, axis=1)
        realised = 10 * np.log10(Pa / (d["g"] ** 2 * Pv))
        np.testing.assert_allclose(realised, 10 * np.log10(snr.astype(np.float64)), rtol=0, atol=1e-10)


def test_reference_unit_rir_gain_linearity_and_whitening():
    audio, noise, off, T = _case(1)
    kw = dict(noise=noise, noise_offsets=[[5], [60], [111]], snr_lin=[2.0, 3.0, 4.0])
    plain = A.augment_reference(audio, off, T, 4, whitening=False, details=True, **kw)
    unit = A.augment_reference(audio, off, T, 4, whitening=False, details=True, rirs=np.ones((1, 1), np.float32), rir_id=[0, 0, 0], **kw)
    np.testing.assert_array_equal(unit["y"], plain["y"])      # r = [1] changes nothing
    padded = A.augment_reference(audio, off, T, 4, whitening=False, details=True, rirs=np.array([[1, 0, 0, 0, 0]], np.float32),
                                 rir_id=[0, -1, 0], **kw)
    np.testing.assert_allclose(padded["y"], plain["y"], rtol=0, atol=1e-17)
    # gain scales the un-whitened y linearly
    for G in (0.25, 3.0):
        scaled = A.augment_reference(audio, off, T, 4, whitening=False, details=True, gain=[G, 1.0, G], **kw)
        np.testing.assert_allclose(scaled["y"][0], G * plain["y"][0], rtol=1e-15)
        np.testing.assert_array_equal(scaled["y"][1], plain["y"][1])
    # no augmentation at all: the plain host preprocessing (decimate, whiten the tower as one batch)
    from voicemap_amd.utils import whiten
    clean = A.augment_reference(audio, off, T, 4)
    win = np.stack([audio[o:o + T] for o in off]).astype(np.float64)[:, ::4, None]
    np.testing.assert_allclose(clean[:, 15:-16], whiten(win)[:, :, 0], rtol=1e-13, atol=1e-15)
    # one scale per tower of windows_per_tower windows
    two = A.augment_reference(np.concatenate([audio, audio]), np.concatenate([off, off + 400]), T, 4, windows_per_tower=3)
    np.testing.assert_allclose(two[:3], clean, rtol=1e-13)
    np.testing.assert_allclose(two[3:], clean, rtol=1e-13)


def test_reference_zero_gain_rules():
    audio, noise, off, T = _case(2)
    noff = [[5, 9], [60, 61], [111, 200]]
    base = dict(noise=noise, noise_offsets=noff, details=True, whitening=False)
    # snr_lin <= 0: no noise for that window only
    d = A.augment_reference(audio, off, T, 2, snr_lin=[0.0, -1.0, 2.0], **base)
    assert d["g"][0] == 0 and d["g"][1] == 0 and d["g"][2] > 0
    np.testing.assert_array_equal(d["y"][:2], d["a"][:2])
    # K == 0
    d = A.augment_reference(audio, off, T, 2, snr_lin=[1.0, 1.0, 1.0], details=True, whitening=False)
    assert np.all(d["g"] == 0)
    # Pv == 0: an all-zero noise crop
    d = A.augment_reference(audio, off, T, 2, snr_lin=[1.0, 1.0, 1.0], noise=np.zeros_like(noise), noise_offsets=noff, details=True,
                            whitening=False)
    assert np.all(d["g"] == 0) and np.all(np.isfinite(d["x"]))
    # Pa == 0: silent speech -> g = 0, the output is silent and finite (the whitening is off here: a silent tower has no scale)
    silent = audio.copy()
    silent[off[1]:off[1] + T] = 0
    d = A.augment_reference(silent, off[1:2], T, 2, snr_lin=[1.0], noise=noise, noise_offsets=noff[1:2], details=True, whitening=False)
    assert d["g"][0] == 0 and np.all(d["y"] == 0)


def test_device_windows_materialise_the_mixture_at_the_decimated_positions(resident):
    """The chosen np.asarray behaviour: the clean crop with every downsampling-th sample replaced by augment_reference's y."""
    pol = _policy(p_noise=1.0, p_reverb=1.0)
    np.random.seed(2)
    (w1, _), _ = resident.build_verification_batch_device(6, pol)
    np.random.seed(2)
    (c1, _), _ = resident.build_verification_batch_device(6)
    x, clean = np.asarray(w1), np.asarray(c1)
    assert x.shape == clean.shape == (6, resident.fragment_length, 1) and x.dtype == np.float64
    a = w1.aug
    host = resident.device_audio.numpy()
    d = A.augment_reference(host, w1.offsets_host, w1.length, 4, noise=host, noise_offsets=a.noise_offsets, snr_lin=a.snr_lin, gain=a.gain,
                            rirs=a.rirs_host, rir_id=a.rir_id, whitening=False, details=True)
    np.testing.assert_array_equal(x[:, ::4, 0], d["y"])
    keep = np.ones(resident.fragment_length, bool)
    keep[::4] = False
    np.testing.assert_array_equal(x[:, keep], clean[:, keep])
    assert not np.array_equal(x[:, ::4], clean[:, ::4])
    # through the host preprocessor it is the reference's network input
    from voicemap_amd.utils import preprocess_instances
    lazy = np.asarray(preprocess_instances(4)(w1))
    full = A.augment_reference(host, w1.offsets_host, w1.length, 4, noise=host, noise_offsets=a.noise_offsets, snr_lin=a.snr_lin,
                               gain=a.gain, rirs=a.rirs_host, rir_id=a.rir_id)
    np.testing.assert_allclose(lazy[:, :, 0], full[:, 15:-16], rtol=1e-12, atol=1e-15)
    with pytest.raises(TypeError, match="augmented"):
        w1.gather()


# ---- script flags ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", ["train_siamese", "siamese_contrastive_loss"])
def test_script_flags(module, monkeypatch):
    import argparse
    import importlib
    mod = importlib.import_module("experiments." + module)
    from experiments import _common as C
    seen = {}

    class Stop(Exception):
        pass

    def setup(*a, **k):
        raise Stop()
    monkeypatch.setattr(C, "setup", setup)
    orig = argparse.ArgumentParser.parse_args

    def spy(self, argv=None, ns=None):
        seen["a"] = orig(self, argv, ns)
        return seen["a"]
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", spy)
    # off by default
    with pytest.raises(Stop):
        mod.main(["--synthetic"])
    a = seen["a"]
    assert a.augment is False and a.aug_snr is None and a.aug_babble is None and a.aug_reverb is None and a.aug_seed is None
    assert A.policy_from_args(a, 4) is None
    # they parse, and make the policy they describe
    argv = ["--synthetic", "--device-data", "/nonexistent", "--augment", "--aug-snr", "0", "10", "--aug-babble", "2", "4", "--aug-reverb", "0.3",
            "--aug-rt60", "0.1", "0.2", "--aug-gain-db", "-3", "3", "--aug-seed", "5"]
    with pytest.raises(Stop):
        mod.main(argv)
    pol = A.policy_from_args(seen["a"], 4)
    assert (pol.snr_db, pol.babble, pol.p_reverb, pol.gain_db, pol.seed, pol.downsampling) == ((0.0, 10.0), (2, 4), 0.3, (-3.0, 3.0), 5, 4)
    assert pol.rirs_host is not None and pol.rirs_host.shape[1] <= A.MAX_RIR_TAPS
    # --augment without --device-data is an error that says so; so is a parameter without --augment
    with pytest.raises(SystemExit, match="--device-data"):
        mod.main(["--synthetic", "--augment"])
    with pytest.raises(SystemExit, match="--augment"):
        mod.main(["--synthetic", "--aug-seed", "3"])
