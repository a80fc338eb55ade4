"""The byte layout of a training step's single host-to-device copy (voicemap_amd/staging.py), on plain numpy buffers: the segment lists
are the ones staging.step_segments builds for the engine's offsets path -- [offsets | labels] of a siamese step, + [snr_lin | gain | rir_id | noise offsets] of an
augmented one, [offsets | labels] of an episode -- at the smallest sizes that can go wrong (an odd number of 4-byte labels ends off an
8-byte boundary)."""
import numpy as np
import pytest

from voicemap_amd import staging
from voicemap_amd.augment import AugmentRecord


def _siamese(pairs, K=None):
    """The segments of a siamese step of ``pairs`` pairs; K: augmented, with K noise recordings per window."""
    rng = np.random.default_rng(pairs * 10 + (K or 0))
    towers = [rng.integers(0, 2 ** 40, pairs) for _ in range(2)]
    aug = None
    if K is not None:
        aug = [AugmentRecord(rng.integers(0, 2 ** 40, (pairs, K)), rng.random(pairs), rng.random(pairs), rng.integers(-1, 5, pairs), None,
                             None, None, 4) for _ in range(2)]
    return staging.step_segments(towers, rng.integers(0, 2, (pairs, 1)).astype(np.float64), pairs, np.float32, aug)


def _episode(N, m):
    rng = np.random.default_rng(N * 10 + m)
    return staging.step_segments((rng.integers(0, 2 ** 40, N),), rng.integers(0, 3, m), m, np.int32)


def test_the_segments_of_a_step_have_the_dtypes_the_kernels_read():
    seg = dict(_siamese(3, 2))
    assert [(k, v.dtype, v.size) for k, v in seg.items()] == [
        ("offsets", np.int64, 6), ("labels", np.float32, 3), ("snr_lin", np.float32, 6), ("gain", np.float32, 6), ("rir_id", np.int32, 6),
        ("noise_offsets", np.int64, 12)]
    seg = dict(_episode(3, 1))
    assert [(k, v.dtype, v.size) for k, v in seg.items()] == [("offsets", np.int64, 3), ("labels", np.int32, 1)]


CASES = [_siamese(p, K) for p in (1, 3) for K in (None, 0, 1, 2)] + [_episode(3, 1)]


@pytest.mark.parametrize("segments", CASES, ids=lambda s: "-".join("%s%d" % (n[0], a.size) for n, a in s))
def test_segments_are_aligned_disjoint_and_come_back_exactly(segments):
    offsets, total = staging.layout(segments)
    assert list(offsets) == [name for name, _ in segments]
    end = 0
    for name, a in segments:
        assert offsets[name] >= end, "segment %s overlaps its predecessor" % name
        if a.dtype == np.int64:
            assert offsets[name] % 8 == 0
        end = offsets[name] + a.nbytes
    assert total == sum((a.nbytes + 7) // 8 * 8 for _, a in segments) and total >= end
    buf = np.full(total, 0xA5, dtype=np.uint8)
    assert staging.pack(buf, segments) == offsets
    for name, a in segments:
        back = buf[offsets[name]:offsets[name] + a.nbytes].view(a.dtype)
        assert back.dtype == a.dtype and np.array_equal(back, a.reshape(-1))


def test_no_noise_recordings_no_noise_offset_segment():
    assert "noise_offsets" not in staging.layout(_siamese(3, 0))[0]
    assert "noise_offsets" in staging.layout(_siamese(3, 1))[0]
    # ... and an odd number of labels is what moves the segment behind them onto the next 8-byte boundary
    assert staging.layout(_siamese(3))[0]["labels"] == 48 and staging.layout(_siamese(3, 0))[0]["snr_lin"] == 64
