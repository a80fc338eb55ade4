"""CPU tests of voicemap_amd/speed.py: the numpy statement of the resampler against the literal double loop, the planted rounding /
clipping / overflow inputs, the default filter design, ``ShardedSpeechDataset.speed_perturbed`` on a host-only shard directory, the
flags, and the argument refusals of vm_resample_i16 (no launch)."""
import argparse

import numpy as np
import pytest

from tests import speed_cases as SC
from voicemap_amd import speed as S
from voicemap_amd.vad import VadPolicy, vad_reference


@pytest.mark.parametrize("U,D", SC.RATIOS, ids=["%d-%d" % r for r in SC.RATIOS])
def test_reference_is_the_literal_double_loop(U, D):
    rng = np.random.RandomState(31 * U + D)
    T = 6
    for n in (0, 1, 2, T - 1, T, T + 1, 257):
        x = rng.randint(-32768, 32768, n).astype(np.int16)
        for taps, shift in ((rng.randint(-40000, 40001, U * T), 15), (rng.randint(-3, 4, U * T), 0), (rng.randint(-2 ** 31, 2 ** 31, U * T), 30)):
            got = S.resample_reference(x, U, D, taps, shift)
            assert got.dtype == np.int16 and len(got) == (n * U + D - 1) // D == S.output_length(n, U, D)
            assert np.array_equal(got, SC.literal(x, U, D, taps, shift)), (U, D, n, shift)


def test_unit_tap_is_the_identity():
    x = np.random.RandomState(0).randint(-32768, 32768, 300).astype(np.int16)
    for T in (1, 2, 31, 32, 64):
        taps = np.zeros(T, dtype=np.int64)
        taps[T // 2] = 1
        assert np.array_equal(S.resample_reference(x, 1, 1, taps, 0), x)
        assert np.array_equal(S.resample_reference(x, 1, 1, taps << 7, 7), x)


@pytest.mark.parametrize("plant", SC.plants(), ids=[p[0] for p in SC.plants()])
def test_plants(plant):
    name, x, U, D, taps, shift, want = plant
    got = S.resample_reference(x, U, D, taps, shift)
    if name == "overflow":   # the outputs that see all four taps: acc = -2^32 (0 to a wrapped int32)
        assert (got[1:len(x) - 2] == -32768).all() and S.phase_abs_max(taps, U) == 1 << 17 > S.NARROW_MAX
    else:
        assert np.array_equal(got, want), (name, got)
    assert np.array_equal(got, SC.literal(x, U, D, taps, shift))


@pytest.mark.parametrize("U,D", ((10, 9), (10, 11)))
def test_default_design(U, D):
    taps = S.design_taps(U, D)
    assert taps.shape == (U * 32,) and np.issubdtype(taps.dtype, np.integer)
    dc = taps.reshape(-1, U).sum(axis=0)
    assert np.abs(dc - (1 << 15)).max() <= 8, dc
    brute = max(sum(abs(int(taps[p + i * U])) for i in range(32)) for p in range(U))
    assert S.phase_abs_max(taps, U) == brute
    if (U, D) == (10, 9):
        assert brute == 71012 > S.NARROW_MAX   # a 32-bit accumulator can wrap on full-scale input
    # a 1 kHz tone of amplitude 12000 against the ideal resampled sine (the filter has no delay: output m sits at input time m D / U)
    n = 16000
    y = S.resample_reference(SC.tone(1000.0, 12000.0, n), U, D, taps, 15).astype(np.float64)
    ideal = 12000.0 * np.sin(2 * np.pi * 1000.0 * (np.arange(len(y)) * D / U) / 16000.0)
    mid = slice(64, len(y) - 64)
    snr = 10 * np.log10((ideal[mid] ** 2).sum() / ((y - ideal)[mid] ** 2).sum())
    print("U/D = %d/%d: phase_abs_max %d, 1 kHz tone SNR %.1f dB" % (U, D, brute, snr))
    assert snr >= 75.0, snr
    if (U, D) == (10, 11):   # 7.9 kHz is above the new Nyquist rate (7.27 kHz): it must not fold back
        x = SC.tone(7900.0, 12000.0, n)
        y = S.resample_reference(x, U, D, taps, 15).astype(np.float64)
        down = 10 * np.log10((y[mid] ** 2).mean() / (x.astype(np.float64) ** 2).mean())
        print("7.9 kHz tone at 10/11: %.1f dB" % down)
        assert down <= -30.0, down


def test_policy_and_ratio():
    assert S.ratio(0.9) == (10, 9) and S.ratio(1.1) == (10, 11) and S.ratio(1.5) == (2, 3) and S.ratio(1.0) == (1, 1)
    p = S.SpeedPolicy()
    assert p.factors == (0.9, 1.1) and p.ratios == ((10, 9), (10, 11)) and p.new_speakers and p.shift == 15
    assert np.array_equal(p.taps(1), S.design_taps(10, 11, 32, 0.95, 9.0, 15))
    for bad in (dict(factors=()), dict(factors=(1.0,)), dict(factors=(0.9, 0.9)), dict(factors=(-1.0,)), dict(factors=(100.0,)),
                dict(taps_per_phase=0), dict(taps_per_phase=65), dict(shift=31), dict(rolloff=0.0)):
        with pytest.raises(ValueError):
            S.SpeedPolicy(**bad)
    assert S.tile_outputs(10, 9, 32) == S.TILE_OUTPUTS and S.tile_outputs(1, 64, 64) == 56 and S.tile_outputs(1, 64, 1) == 56
    for U, D in SC.RATIOS + ((1, 64), (64, 1)):
        for T in SC.TAPS_PER_PHASE:   # a tile's input span fits the staging buffer
            t = S.tile_outputs(U, D, T)
            assert 1 <= t <= S.TILE_OUTPUTS and ((t - 1) * D + U - 1) // U + 1 + T <= S.SPAN


def test_flags():
    def parse(*argv):
        ap = argparse.ArgumentParser()
        ap.add_argument("--device-data", default="")
        return S.add_speed_args(ap).parse_args(list(argv))
    assert S.policy_from_args(parse(), need_device_data=True) is None
    p = S.policy_from_args(parse("--speed-perturb", "0.9,1.1", "--device-data", "d"), need_device_data=True)
    assert p.factors == (0.9, 1.1) and p.new_speakers
    assert not S.policy_from_args(parse("--speed-perturb", "0.9", "--speed-same-speaker")).new_speakers
    for argv in (("--speed-perturb", "0.9"), ("--speed-same-speaker",), ("--speed-perturb", "1.0", "--device-data", "d")):
        with pytest.raises(SystemExit):
            S.policy_from_args(parse(*argv), need_device_data=True)
    from experiments import _common as C
    a = C.add_speed_args(C.base_parser("x")).parse_args(["--speed-perturb", "1.1"])
    with pytest.raises(SystemExit, match="--device-data"):
        C.speed_policy(a)


# ---- the dataset ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return SC.corpus(tmp_path_factory.mktemp("speed_shards"))


def _check_layout(base, sp, policy):
    """Rows, lengths, offsets and host audio of ``sp = base.speed_perturbed(policy)``; returns the kept source rows per factor."""
    n = len(base)
    assert type(sp) is type(base) and sp._speed is policy and base._speed is None
    assert np.array_equal(sp.df["id"].values, np.arange(len(sp)))
    assert np.array_equal(sp.file_length[:n], base.file_length) and np.array_equal(sp.global_offset[:n], base.global_offset)
    assert (sp.df["speed"].values[:n] == 1.0).all() and np.array_equal(sp.df["speaker_id"].values[:n], base.df["speaker_id"].values)
    at, row, kept = base._buffer_samples(), n, []
    for k, (f, (U, D)) in enumerate(zip(policy.factors, policy.ratios), start=1):
        lens = S.output_length(base.file_length, U, D)
        keep = np.flatnonzero(lens / 16000.0 > base.fragment_seconds)
        kept.append(keep)
        rows = slice(row, row + len(keep))
        assert np.array_equal(sp.file_length[rows], lens[keep]) and (sp.df["speed"].values[rows] == f).all()
        assert np.array_equal(sp.global_offset[rows], at + np.cumsum(lens[keep]) - lens[keep])
        assert list(sp.df["filepath"].values[rows]) == list(base.df["filepath"].values[keep])
        at, row = at + int(lens[keep].sum()), row + len(keep)
    assert row == len(sp) and np.array_equal(sp.df["length"].values, sp.file_length)
    assert np.array_equal(sp.df["seconds"].values, sp.file_length / 16000.0) and (sp.file_length >= sp.fragment_length).all()
    # the buffer to_device() would upload is the base's, then the copies: every row's slice is its _pcm
    cat = np.concatenate(sp._host_parts())
    assert len(cat) == at and np.array_equal(cat[:base._buffer_samples()], np.concatenate(base._host_parts()))
    for i in range(len(sp)):
        assert np.array_equal(cat[sp.global_offset[i]:sp.global_offset[i] + sp.file_length[i]], sp._pcm(i)), i
    return kept


def test_speed_perturbed_rows_ids_and_drop_rule(corpus):
    ds = corpus
    n, policy = len(ds), S.SpeedPolicy()
    assert n == 15 and ds.file_length[-1] == ds.fragment_length + 1 == 1601 and ds.device_audio is None
    sp = ds.speed_perturbed(policy)
    kept = _check_layout(ds, sp, policy)
    # a file of fragment_length + 1 samples: its 0.9 copy (1779 samples) stays, its 1.1 copy (1456) cannot give a fragment
    assert list(kept[0]) == list(range(n)) and list(kept[1]) == list(range(n - 1)) and len(sp) == 3 * n - 1
    assert S.output_length(1601, 10, 9) == 1779 and S.output_length(1601, 10, 11) == 1456
    # a copy is the statement of its source, new speakers are k B + id with B = 1000 above the largest id 104
    taps = policy.taps(0)
    assert np.array_equal(sp._pcm(n + 3), S.resample_reference(np.asarray(ds._pcm(3)), 10, 9, taps, 15))
    assert np.array_equal(sp._load(n + 3), sp._pcm(n + 3) / 32768.0)
    ids = ds.df["speaker_id"].values
    assert np.array_equal(sp.df["speaker_id"].values, np.concatenate([ids, 1000 + ids, 2000 + ids[:-1]]))
    assert sp.unique_speakers == sp.num_classes() == 15 and ds.unique_speakers == 5
    assert sp._label(n) == 1100 and sp.datasetid_to_speaker_id[2 * n] == 2100 and sp.datasetid_to_filepath[n] == ds.datasetid_to_filepath[0]
    # the same speakers
    same = ds.speed_perturbed(S.SpeedPolicy(new_speakers=False))
    assert same.unique_speakers == same.num_classes() == 5 and len(same) == 3 * n - 1
    assert np.array_equal(same.df["speaker_id"].values, np.concatenate([ids, ids, ids[:-1]]))
    # one factor, padded datasets keep every copy
    from voicemap_amd import shards
    padded = shards.ShardedSpeechDataset(ds.shard_dir, SC.FRAGMENT_SECONDS, pad=True).speed_perturbed(S.SpeedPolicy(factors=(1.1,)))
    assert len(padded) == 2 * n and padded.file_length[-1] == 1456
    # the refusals
    with pytest.raises(ValueError, match="already speed-perturbed"):
        sp.speed_perturbed(policy)
    with pytest.raises(ValueError, match="trim first"):
        sp.voiced(VadPolicy())


def test_speed_perturbed_samplers_draw_inside_every_file(corpus):
    sp = corpus.speed_perturbed(S.SpeedPolicy())
    T, seen = sp.fragment_length, set()
    np.random.seed(4)
    for _ in range(40):
        o1, o2, y, f1, f2 = sp.build_verification_batch_offsets(16, files=True)
        for o, f in ((o1, f1), (o2, f2)):
            assert (o >= sp.global_offset[f]).all() and (o + T <= sp.global_offset[f] + sp.file_length[f]).all()
            seen.update(f.tolist())
        spk = sp.df["speaker_id"].values
        assert (spk[f1[:8]] == spk[f2[:8]]).all() and (spk[f1[8:]] != spk[f2[8:]]).all()
    assert len(seen) == len(sp)   # originals and copies of both factors are all drawn
    o, lab, f = sp.build_speaker_batch_offsets(12, 2, files=True)
    assert (o >= sp.global_offset[f]).all() and (o + T <= sp.global_offset[f] + sp.file_length[f]).all()


def test_speed_perturbed_of_a_voiced_dataset_and_of_a_speaker_shard(corpus):
    from voicemap_amd import shards
    ds = corpus
    vp = VadPolicy(frame_ms=2.0, min_run=2, hang=3)
    vo = ds.voiced(vp)
    assert (vo.file_length < ds.file_length).any()
    policy = S.SpeedPolicy()
    sp = vo.speed_perturbed(policy)
    kept = _check_layout(vo, sp, policy)
    src = int(kept[1][2])
    trimmed = vad_reference(np.asarray(ds._pcm(src)), vo._vad)["pcm"]
    assert np.array_equal(sp._pcm(len(vo) + len(kept[0]) + 2), S.resample_reference(trimmed, 10, 11, policy.taps(1), 15))
    with pytest.raises(ValueError):
        sp.voiced(vp)
    sh = shards.ShardedSpeechDataset(ds.shard_dir, SC.FRAGMENT_SECONDS, pad=False, speaker_shard=(1, 2))
    shp = sh.speed_perturbed(policy)
    _check_layout(sh, shp, policy)
    assert shp.speaker_shard == (1, 2) and shp.unique_speakers == 3 * sh.unique_speakers


# ---- the entry point ----------------------------------------------------------------------------------------------------------------------
def test_the_library_refuses_bad_arguments_without_a_launch():
    from voicemap_amd import _lib
    lib = _lib.lib()
    good = dict(U=10, D=9, T=32, shift=15, pam=71012, n=0)

    def call(**kw):
        k = dict(good, **kw)
        lib.call("vm_resample_i16", None, None, None, None, k["n"], k["U"], k["D"], None, k["T"], k["shift"], k["pam"], None, None, None)
    for bad, word in ((dict(U=0), "U and D"), (dict(U=65), "U and D"), (dict(D=0), "U and D"), (dict(D=65), "U and D"), (dict(T=0), "T "),
                      (dict(T=65), "T "), (dict(shift=-1), "shift"), (dict(shift=31), "shift"), (dict(pam=-1), "phase_abs_max"),
                      (dict(pam=1 << 47), "phase_abs_max"), (dict(n=-1), "n_utts"), (dict(n=1), "null pointer")):
        with pytest.raises(_lib.VoicemapHipError, match=word):
            call(**bad)
    call()   # no utterances: nothing to do, whatever the pointers
    for U, D, taps, shift in ((0, 1, [1], 0), (1, 65, [1], 0), (1, 1, [1], 31), (2, 1, [1, 2, 3], 0), (1, 1, [1.0], 0), (1, 1, [1 << 31], 0),
                              (1, 1, [(1 << 31) - 1] * 65, 0)):
        with pytest.raises(ValueError):
            S.resample_reference(np.zeros(4, dtype=np.int16), U, D, np.array(taps), shift)
    with pytest.raises(TypeError, match="int16 PCM"):
        S.resample_reference(np.zeros(4, dtype=np.float32), 1, 1, np.array([1]), 0)
    with pytest.raises(TypeError, match="int16 PCM"):
        S.resample(np.zeros(4, dtype=np.int16), [0], [4], 1, 1, np.array([1]), 0)
