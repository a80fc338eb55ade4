"""CPU checks of the host side of voicemap_amd/diarization.py: sliding windows, window labels -> segments, the diarization error rate
and its assignment solver, and the synthetic conversations."""
import itertools

import numpy as np
import pytest

from voicemap_amd import diarization as DZ


# ---- sliding_windows -------------------------------------------------------------------------------------------------------------------
def test_sliding_windows_exact_fit_tail_and_too_short():
    exact, tail, one = DZ.sliding_windows([100, 107, 40], 40, 20)
    assert exact.tolist() == [0, 20, 40, 60] and exact.dtype == np.int64            # the last window ends at 100
    assert tail.tolist() == [0, 20, 40, 60, 67]                                     # 60 + 40 = 100 < 107: one more, flush with the end
    assert one.tolist() == [0]
    assert DZ.sliding_windows([41], 40, 20)[0].tolist() == [0, 1]
    assert DZ.sliding_windows([], 40, 20) == []
    with pytest.raises(ValueError, match="recording 1 holds 39 samples"):
        DZ.sliding_windows([50, 39], 40, 20)
    with pytest.raises(ValueError):
        DZ.sliding_windows([50], 40, 0)


# ---- window_segments -------------------------------------------------------------------------------------------------------------------
def test_window_segments_midpoints_and_ties():
    # centres at 20, 40, 60, 87: boundaries at the midpoints 30, 50, 73.5; sample 30 is as near to 20 as to 40 -> the earlier window
    seg = DZ.window_segments([0, 20, 40, 67], 40, 107, [0, 1, 1, 0])
    assert seg.tolist() == [[0, 31, 0], [31, 74, 1], [74, 107, 0]] and seg.dtype == np.int64
    # brute force: every sample takes the nearest centre, ties to the earlier window
    starts, window, length, labels = np.array([0, 7, 14, 21, 23]), 10, 33, np.array([2, 2, 0, 1, 0])
    seg = DZ.window_segments(starts, window, length, labels)
    per_sample = np.empty(length, np.int64)
    for b, e, lab in seg:
        per_sample[b:e] = lab
    centres2 = 2 * starts + window
    want = [labels[int(np.argmin(np.abs(2 * s - centres2)))] for s in range(length)]    # argmin: the first minimum
    assert per_sample.tolist() == want
    assert seg[0, 0] == 0 and seg[-1, 1] == length and (seg[1:, 0] == seg[:-1, 1]).all()  # tiles
    assert (seg[1:, 2] != seg[:-1, 2]).all()                                              # neighbours with one label are joined
    assert DZ.window_segments([0], 10, 10, [4]).tolist() == [[0, 10, 4]]
    with pytest.raises(ValueError):
        DZ.window_segments([0, 5], 10, 20, [1])


# ---- der ---------------------------------------------------------------------------------------------------------------------------------
def test_der_perfect_under_a_permuted_labelling():
    ref = [[0, 100, 7], [100, 250, 3], [250, 300, 7], [300, 420, 9]]
    hyp = [[0, 100, 1], [100, 250, 0], [250, 300, 1], [300, 420, 5]]
    d = DZ.der(ref, hyp)
    assert d == {"missed": 0, "false_alarm": 0, "confusion": 0, "total": 420, "der": 0.0, "mapping": {3: 0, 7: 1, 9: 5}}


def test_der_hand_computed_miss_false_alarm_confusion():
    # reference: A on [0, 100), B on [100, 200), silence on [200, 250)
    ref = [[0, 100, 0], [100, 200, 1]]
    # hypothesis: x on [10, 120) -- 10 missed, 20 of B called x; y on [120, 180); nothing on [180, 200) -- 20 missed; y on [200, 230): false alarm
    hyp = [[10, 120, 0], [120, 180, 1], [200, 230, 1]]
    d = DZ.der(ref, hyp)
    assert (d["missed"], d["false_alarm"], d["confusion"], d["total"]) == (30, 30, 20, 200)
    assert d["der"] == 80 / 200 and d["mapping"] == {0: 0, 1: 1}
    # overlapping reference speakers: both active on [50, 100), one hypothesis cluster there
    d = DZ.der([[0, 100, 0], [50, 150, 1]], [[0, 150, 0]])
    assert (d["missed"], d["false_alarm"], d["confusion"], d["total"]) == (50, 0, 50, 200)
    # an empty reference: every hypothesis sample is a false alarm and the rate is undefined
    d = DZ.der(np.zeros((0, 3)), [[0, 10, 0]])
    assert d["false_alarm"] == 10 and d["total"] == 0 and np.isnan(d["der"])


def test_der_more_clusters_than_speakers_and_fewer():
    ref = [[0, 100, 0], [100, 200, 1]]
    # three clusters: the unmapped one (30 samples inside speaker 1) is confusion
    d = DZ.der(ref, [[0, 100, 5], [100, 170, 6], [170, 200, 7]])
    assert (d["missed"], d["false_alarm"], d["confusion"], d["total"]) == (0, 0, 30, 200) and d["mapping"] == {0: 5, 1: 6}
    # one cluster for everything: the shorter speaker is confusion
    d = DZ.der([[0, 120, 0], [120, 200, 1]], [[0, 200, 3]])
    assert (d["missed"], d["false_alarm"], d["confusion"], d["total"]) == (0, 0, 80, 200) and d["mapping"] == {0: 3}


# ---- the assignment solver -----------------------------------------------------------------------------------------------------------
def _brute(W):
    n, m = W.shape
    if n <= m:
        return max(sum(W[i, p[i]] for i in range(n)) for p in itertools.permutations(range(m), n))
    return _brute(W.T)


def _value(W, col):
    used = col[col >= 0]
    assert len(set(used.tolist())) == len(used) and len(used) == min(W.shape)   # one-to-one, nobody left out needlessly
    return sum(W[i, j] for i, j in enumerate(col) if j >= 0)


def test_assignment_against_brute_force_and_scipy():
    rng = np.random.RandomState(0)
    shapes = [(n, m) for n in range(1, 7) for m in range(1, 7)]
    for n, m in shapes:
        for trial in range(4):
            W = rng.randint(0, 6 if trial % 2 else 1000, size=(n, m)).astype(np.int64)   # small range: many ties
            assert _value(W, DZ.assign_max(W)) == _brute(W), (n, m, W)
    W = rng.rand(5, 6)
    assert np.isclose(_value(W, DZ.assign_max(W)), _brute(W))
    assert DZ.assign_max(np.zeros((0, 3))).size == 0 and DZ.assign_max(np.zeros((2, 0))).tolist() == [-1, -1]
    optimize = pytest.importorskip("scipy.optimize")
    for n, m in ((6, 6), (4, 9), (9, 4), (12, 12)):
        W = rng.randint(0, 50, size=(n, m)).astype(np.int64)
        r, c = optimize.linear_sum_assignment(W, maximize=True)
        assert _value(W, DZ.assign_max(W)) == W[r, c].sum()


# ---- make_conversations --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset():
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    return SyntheticSpeechDataset(num_speakers=5, files_per_speaker=2, seconds=0.05, min_file_seconds=0.2, max_file_seconds=0.4, seed=3)


def test_make_conversations(dataset):
    from voicemap_amd.shards import to_int16
    np.random.seed(11)
    state = np.random.get_state()
    conv = DZ.make_conversations(dataset, 6, speakers=(2, 4), turns=(3, 7), turn_seconds=(0.05, 0.5), seed=4)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]   # the dataset's stream is untouched
    assert len(conv) == 6 and conv.audio.dtype.is_floating_point is False and conv.audio.numel() == int(conv.lens.sum())
    assert np.array_equal(conv.offsets, np.concatenate([[0], np.cumsum(conv.lens)[:-1]]))
    audio = conv.audio.cpu().numpy()
    length = dataset.df["length"].values
    clamped = 0
    for r in range(6):
        seg, turns = conv.segments[r], conv.turns[r]
        assert 3 <= len(seg) <= 7 and 2 <= conv.speakers[r] <= 4
        assert (seg[1:, 2] != seg[:-1, 2]).all()                                              # no speaker twice in a row
        assert seg[0, 0] == 0 and seg[-1, 1] == conv.lens[r] and (seg[1:, 0] == seg[:-1, 1]).all()   # the segments tile it
        for (b, e, who), (f, s, k) in zip(seg, turns):
            assert dataset._code[f] == who and e - b == k and 0 <= s and s + k <= length[f]
            assert 1 <= k <= int(round(0.5 * 16000))
            clamped += k == length[f]
            assert np.array_equal(audio[conv.offsets[r] + b:conv.offsets[r] + e], to_int16(dataset._load(f))[s:s + k])
    assert clamped > 0   # files of 0.2 .. 0.4 s against turns of up to 0.5 s: some turns are whole files
    again = DZ.make_conversations(dataset, 6, speakers=(2, 4), turns=(3, 7), turn_seconds=(0.05, 0.5), seed=4)
    assert np.array_equal(again.audio.cpu().numpy(), audio) and all(np.array_equal(a, b) for a, b in zip(again.segments, conv.segments))
    other = DZ.make_conversations(dataset, 6, speakers=(2, 4), turns=(3, 7), turn_seconds=(0.05, 0.5), seed=5)
    assert not (len(other.audio) == len(audio) and np.array_equal(other.audio.cpu().numpy(), audio))
    with pytest.raises(ValueError):
        DZ.make_conversations(dataset, 1, speakers=(2, 6))
    with pytest.raises(ValueError):
        DZ.make_conversations(dataset, 1, speakers=(1, 2))


def test_alias_package_exposes_the_module():
    import voicemap
    from voicemap.diarization import ahc_reference, der, diarize  # noqa: F401
    assert voicemap.diarization is DZ
