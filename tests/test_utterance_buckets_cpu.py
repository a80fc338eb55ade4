"""CPU tests of the whole-utterance bucket planner (voicemap_amd/utterances.py): every recording in exactly one bucket, the inverse
permutation, the bucket length quantum, the row budget, the padding bound and the bound on distinct bucket shapes, on random and
adversarial length lists."""
import numpy as np
import pytest

from voicemap_amd.utterances import (DEFAULT_MAX_PAD_FRAC, DEFAULT_ROW_BUDGET, ladder, plan_buckets, pool_quantum,
                                     valid_lengths)

BASELINE = [(32, 128, 4), (3, 128, 2), (3, 128, 2), (3, 128, 2)]
Q = 32


def _librispeech_like(n, seed):
    """Decimated lengths (16 kHz / 4) of n recordings: 0.8 x Normal(14 s, 2.5 s) + 0.2 x Uniform(1 s, 35 s), clipped to 1 .. 35 s."""
    r = np.random.default_rng(seed)
    s = np.where(r.random(n) < 0.8, r.normal(14.0, 2.5, n), r.uniform(1.0, 35.0, n))
    return (np.clip(s, 1.0, 35.0) * 4000).astype(np.int64)


def _check(l0s, bp, row_budget=DEFAULT_ROW_BUDGET, f=DEFAULT_MAX_PAD_FRAC):
    l0s = np.asarray(l0s)
    seen = np.concatenate([idx for _, idx in bp.buckets])
    assert len(seen) == len(l0s) and np.array_equal(np.sort(seen), np.arange(len(l0s)))   # each recording exactly once
    assert np.array_equal(bp.order[bp.inverse], np.arange(len(l0s)))                      # the inverse restores input order
    assert np.array_equal(np.arange(len(l0s))[bp.order][bp.inverse], np.arange(len(l0s)))
    for L0, idx in bp.buckets:
        assert L0 % Q == 0
        assert len(idx) * L0 <= row_budget
        assert (l0s[idx] <= L0).all()
        pad = int((L0 - l0s[idx]).sum())
        if L0 >= Q / f:
            assert pad <= f * len(idx) * L0, (L0, pad)
        else:   # the short rungs: one quantum apart, a recording pads less than one quantum
            assert (L0 - l0s[idx] < Q).all()
        assert np.all(np.diff(l0s[idx]) >= 0)                                                # length-sorted inside a bucket


def test_quantum_is_the_product_of_the_pools():
    assert pool_quantum(BASELINE) == 32
    v = valid_lengths([32, 33, 100, 12000], BASELINE)
    assert v.dtype == np.int32 and v.shape == (5, 4)
    assert v[:, 1].tolist() == [33, 8, 4, 2, 1] and v[:, 2].tolist() == [100, 25, 12, 6, 3]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_lengths(seed):
    l0s = _librispeech_like(5000, seed)
    bp = plan_buckets(l0s)
    _check(l0s, bp)
    assert bp.pad_overhead < DEFAULT_MAX_PAD_FRAC / (1 - DEFAULT_MAX_PAD_FRAC)


def test_uniform_random_lengths_with_small_budget():
    r = np.random.default_rng(5)
    l0s = r.integers(32, 40000, 3000)
    bp = plan_buckets(l0s, row_budget=200000, max_pad_frac=0.25)
    _check(l0s, bp, 200000, 0.25)


@pytest.mark.parametrize("case", ["all_equal", "one_huge", "many_at_minimum", "primes", "single"])
def test_adversarial_lengths(case):
    if case == "all_equal":
        l0s = np.full(4000, 12000)
    elif case == "one_huge":
        l0s = np.r_[np.full(500, 4000), [140000]]
    elif case == "many_at_minimum":
        l0s = np.r_[np.full(10000, 32), np.arange(33, 300)]
    elif case == "primes":
        l0s = np.array([p for p in range(33, 20000) if all(p % d for d in range(2, int(p ** 0.5) + 1))])
    else:
        l0s = np.array([777])
    bp = plan_buckets(l0s)
    _check(l0s, bp)
    if case == "all_equal":
        (L0,) = bp.shapes   # one rung: the first at or above 12 000
        assert L0 >= 12000 and L0 == min(r for r in ladder(Q, DEFAULT_MAX_PAD_FRAC, 12000) if r >= 12000)
        assert len(bp.buckets) == -(-4000 // (DEFAULT_ROW_BUDGET // L0))
    if case == "one_huge":
        assert bp.buckets[-1][1].tolist() == [500]


def test_distinct_shapes_bounded_for_100k_lengths():
    l0s = _librispeech_like(100000, 7)
    bp = plan_buckets(l0s)
    _check(l0s, bp)
    rungs = ladder(Q, DEFAULT_MAX_PAD_FRAC, int(l0s.max()))
    assert set(bp.shapes) <= set(rungs)
    # the ladder, not the corpus, bounds the shapes: 8 rungs up to 256, then ratio 8/7 up to 35 s (140 000 decimated samples)
    assert len(rungs) <= 60 and len(bp.shapes) <= len(rungs)
    # doubling the corpus adds no shape
    assert set(plan_buckets(np.r_[l0s, _librispeech_like(100000, 8)]).shapes) <= set(rungs)


def test_ladder_spacing_bounds_padding():
    rungs = ladder(Q, 1 / 8, 200000)
    assert rungs[:8] == [32 * k for k in range(1, 9)] and rungs[-1] >= 200000
    for a, b in zip(rungs, rungs[1:]):
        assert b % Q == 0 and b > a and (b <= 256 or a >= b * (1 - 1 / 8))


def test_too_short_recordings_raise():
    with pytest.raises(ValueError, match="recording 2 is too short.*31 decimated samples, the minimum is 32"):
        plan_buckets([100, 32, 31, 5000])
    with pytest.raises(ValueError, match="recording b.flac"):
        plan_buckets([100, 7], names=["a.flac", "b.flac"])


def test_recording_larger_than_the_budget_raises():
    with pytest.raises(ValueError, match="row budget"):
        plan_buckets([40000], row_budget=30000)


def test_empty():
    bp = plan_buckets([])
    assert bp.buckets == [] and len(bp.order) == 0


def test_file_names_for_error_messages():
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    from voicemap_amd.retrieval import file_names

    d = SyntheticSpeechDataset(num_speakers=3, files_per_speaker=2, seconds=1, stochastic=False, seed=1)
    names = file_names(d, 1, 4)
    assert names == [str(v) for v in d.df["filepath"].values[1:4]] and all(n.startswith("synthetic://") for n in names)

    class Subset:   # a subset of a dataset's files (experiments/verification_accuracy.CohortSubset)
        base, index = d, np.array([5, 0, 2])
    assert file_names(Subset(), 0, 2) == [str(d.df["filepath"].values[5]), str(d.df["filepath"].values[0])]

    class Bare:
        pass
    assert file_names(Bare(), 7, 9) == ["file 7", "file 8"]
    with pytest.raises(ValueError, match="recording synthetic://"):
        plan_buckets([100, 5], names=file_names(d, 0, 2))
