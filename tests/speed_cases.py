"""Cases shared by tests/test_speed_cpu.py and tests/test_gpu_speed.py: the literal double loop over the resampler's formula, int16
buffers whose utterances lie at odd sample offsets between runs of full-scale poison (an over-read at either end of a file meets the
largest sample there is), the planted rounding / clipping / overflow inputs, and a tiny shard directory.  ``reference(case, k)`` is
``resample_reference`` over the case's utterances under its k-th tap table; it is computed once and shared."""
import functools

import numpy as np

from voicemap_amd import speed as S

RATIOS = ((1, 1), (10, 9), (10, 11), (3, 2), (2, 3), (7, 5), (64, 63))   # (U, D)
TAPS_PER_PHASE = (1, 2, 31, 32, 64)
POISON = (-32768, 32767)


def literal(x, U, D, taps, shift):
    """The statement as a double loop over Python integers (no index algebra: every (m, k) pair is tried)."""
    x, taps = [int(v) for v in x], [int(v) for v in taps]
    n, c = len(taps), len(taps) // 2
    out = []
    for m in range((len(x) * U + D - 1) // D):
        acc = 0
        for k in range(len(x)):
            j = m * D + c - k * U
            if 0 <= j < n:
                acc += taps[j] * x[k]
        if shift > 0:
            acc += 1 << (shift - 1)
        out.append(min(max(acc >> shift, -32768), 32767))
    return np.array(out, dtype=np.int16)


def random_taps(rng, U, T, per_phase):
    """U T integer taps of either sign whose per-phase sum of magnitudes is at most ``per_phase`` (and reaches it in phase 0)."""
    mag = max(per_phase // T, 1)
    taps = rng.randint(-mag, mag + 1, U * T).astype(np.int64)
    taps[0::U] = mag * (2 * rng.randint(0, 2, T) - 1)
    assert S.phase_abs_max(taps, U) == mag * T <= max(per_phase, T)
    return taps


def lengths(U, D, T):
    """Utterance lengths around every constant of the kernel: 0, 1 and the filter length; the outputs of one thread and of one tile,
    one less and one more; more than two tiles (the input span of every file's last tile crosses the file's end)."""
    tile, per = S.tile_outputs(U, D, T), S.THREAD_OUTPUTS
    lens = {0, 1, 2, max(T - 1, 0), T, T + 1}
    for n_out in (per, 2 * per, tile, 2 * tile):
        base = (n_out * D) // U
        lens.update(max(base + d, 0) for d in (-1, 0, 1, 2))
    lens.add(((2 * tile + per + 3) * D) // U + 1)
    return sorted(lens)


def pack(utts, rng, prefix):
    """``buf`` = poison prefix, then the utterances with one to three poison samples after each (the starts take either parity)."""
    parts, offsets, cur = [np.resize(np.array(POISON, dtype=np.int16), prefix)], [], prefix
    for u in utts:
        offsets.append(cur)
        gap = int(rng.randint(1, 4))
        parts += [u, np.array([POISON[(cur + i) % 2] for i in range(gap)], dtype=np.int16)]
        cur += len(u) + gap
    parts.append(np.resize(np.array(POISON, dtype=np.int16), 24))
    return np.concatenate(parts).astype(np.int16), np.array(offsets, dtype=np.int64), np.array([len(u) for u in utts], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def grid_case(U, D, T):
    """One buffer of utterances of ``lengths(U, D, T)`` (shuffled, full-scale random samples) and two tap tables: one the 32-bit
    accumulator takes (phase sum NARROW_MAX exactly) and one only the 64-bit one can (int32-sized taps)."""
    rng = np.random.RandomState(1000 * U + 10 * D + T)
    lens = lengths(U, D, T)
    rng.shuffle(lens)
    utts = [rng.randint(-32768, 32768, n).astype(np.int16) for n in lens]
    for u in utts:
        if len(u) >= 4:   # full scale where the zero padding begins
            u[0], u[1], u[-2], u[-1] = 32767, -32768, -32768, 32767
    buf, offsets, ln = pack(utts, rng, prefix=3)
    assert set((offsets % 2).tolist()) == {0, 1}
    tables = ((random_taps(rng, U, T, S.NARROW_MAX), 15), (random_taps(rng, U, T, T * ((1 << 31) - 1)), 30))
    return {"name": "%d/%d-T%d" % (U, D, T), "U": U, "D": D, "T": T, "buf": buf, "offsets": offsets, "lens": ln, "tables": tables}


_REF = {}


def reference(case, k):
    """``resample_reference`` of every utterance of the case under its k-th (taps, shift); cached by case name, read-only."""
    key = (case["name"], k)
    if key not in _REF:
        taps, shift = case["tables"][k]
        rows = [S.resample_reference(case["buf"][o:o + n], case["U"], case["D"], taps, shift) for o, n in zip(case["offsets"], case["lens"])]
        for r in rows:
            r.setflags(write=False)
        _REF[key] = rows
    return _REF[key]


def plants():
    """(name, x, U, D, taps, shift, expected) of the planted inputs: rounding half up at shift = 1 on either side of zero, the clip on
    both sides, and an accumulator of -2^32 that a wrapped int32 would turn into 0."""
    i16 = lambda *v: np.array(v, dtype=np.int16)  # noqa: E731
    return (("round+1", i16(-1, -3, 1, 3, -2, 2, 0), 1, 1, np.array([1]), 1, i16(0, -1, 1, 2, -1, 1, 0)),
            ("round-1", i16(1, 3, -1, -3, 2, -2, 0), 1, 1, np.array([-1]), 1, i16(0, -1, 1, 2, -1, 1, 0)),
            ("clip", i16(32767, -32768, 16384, -16385, 16383, -16384), 1, 1, np.array([2 << 15]), 15,
             i16(32767, -32768, 32767, -32768, 32766, -32768)),
            ("clip-neg-tap", i16(32767, -32768, 16384, -16385, 16383), 1, 1, np.array([-(2 << 15)]), 15,
             i16(-32768, 32767, -32768, 32767, -32766)),
            # c = 2: outputs 1 .. len - 3 see all four taps: acc = 4 * 2^15 * -32768 = -2^32
            ("overflow", np.full(40, -32768, dtype=np.int16), 1, 1, np.full(4, 1 << 15), 15, np.full(40, -32768, dtype=np.int16)))


def tone(freq, amplitude, n, rate=16000.0):
    return np.rint(amplitude * np.sin(2 * np.pi * freq * np.arange(n) / rate)).astype(np.int16)


FRAGMENT_SECONDS = 0.1   # 1600 samples


def corpus(tmp_path, n_speakers=5, files=3):
    """A tiny shard directory read as a ``ShardedSpeechDataset`` of 0.1 s fragments: files of 1.2 to 4 fragments of noise with a
    planted pause each, speaker ids 100 .., and one last file of ``fragment_length + 1`` samples (kept; its copy at speed 1.1 is
    shorter than a fragment, its copy at 0.9 is not)."""
    import pandas as pd
    from voicemap_amd import shards
    rng = np.random.RandomState(9)
    rows, waves = [], []
    frag = int(FRAGMENT_SECONDS * 16000)
    for s in range(n_speakers):
        for k in range(files):
            n = frag + 1 if (s, k) == (n_speakers - 1, files - 1) else int(rng.randint(int(1.2 * frag), 4 * frag))
            x = rng.randint(-30000, 30001, n).astype(np.float64)
            if n > 2 * frag:
                b = int(rng.randint(0, n - 300))
                x[b:b + int(rng.randint(100, 300))] = rng.randint(-1, 2)
            waves.append(x / 32768.0)
            rows.append(dict(filepath="spk%d/f%d.flac" % (s, k), id=100 + s, sex="F" if s % 2 else "M", minutes=1.0, subset="tiny",
                             length=n, seconds=n / 16000.0, name="s%d" % s))

    class Source:
        df = pd.DataFrame(rows).rename(columns={"id": "speaker_id", "minutes": "speaker_minutes"})

        def __len__(self):
            return len(waves)

        def _load(self, i):
            return waves[i]
    shards.write_shards(Source(), str(tmp_path))
    return shards.ShardedSpeechDataset(str(tmp_path), FRAGMENT_SECONDS, stochastic=True, pad=False)
