"""Cases shared by tests/test_vad_cpu.py and tests/test_gpu_vad.py: int16 buffers whose utterances lie back to back with no gap (an
over-read meets the neighbour) between a poisoned prefix and suffix of +-32767 (an over-read at either end of the corpus meets the
largest energy there is), with the policy each is run under.  ``reference(case)`` is ``vad_reference`` over the case's utterances, laid
out as the entry points lay their outputs out; it is computed once per case and shared.

Frames are made LOUD (magnitudes 2000..8000) or QUIET (-1, 0, 1): a quiet frame's mean energy is at most 1 against at least 4e6, so at
the default 25 dB a loud frame is active and a quiet one is not as long as one frame in ten thousand is loud, and a case plants the
activity pattern it wants."""
import functools

import numpy as np

from voicemap_amd.vad import DECIDE_CHUNK, VadPolicy, vad_reference

POISON = 32767
PAIRS = ((1, 0), (3, 10), (64, 256))   # (min_run, hang)


def _policy(frame, min_run, hang, **kw):
    # sampling_rate 1000: frame_ms is the frame in samples
    return VadPolicy(frame_ms=float(frame), sampling_rate=1000, min_run=min_run, hang=hang, **kw)


def utterance(rng, frame, pattern, last=None):
    """int16 utterance of len(pattern) frames, frame f loud where pattern[f]; the last frame holds ``last`` samples (default: full)."""
    pattern = np.asarray(pattern, dtype=bool)
    n = (len(pattern) - 1) * frame + (frame if last is None else last)
    loud = np.repeat(pattern, frame)[:n]
    x = np.where(loud, rng.randint(2000, 8001, n) * (2 * rng.randint(0, 2, n) - 1), rng.randint(-1, 2, n))
    return x.astype(np.int16)


def of_length(rng, frame, n, p_loud=0.6):
    """A random utterance of exactly n samples."""
    F = (n + frame - 1) // frame
    pat = rng.random_sample(F) < p_loud
    return utterance(rng, frame, pat, n - (F - 1) * frame)


def pack(name, policy, utts, prefix):
    """The case: ``buf`` = poison prefix + the utterances back to back + poison suffix."""
    lens = np.array([len(u) for u in utts], dtype=np.int64)
    offsets = prefix + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    sign = np.where(np.arange(prefix + 24) % 2 == 0, POISON, -POISON).astype(np.int16)
    buf = np.concatenate([sign[:prefix]] + list(utts) + [sign[:24]]).astype(np.int16)
    return {"name": name, "policy": policy, "buf": buf, "offsets": offsets, "lens": lens}


def _alignment_cases(rng):
    out = []
    for frame in (1, 7, 8, 160, 400, 4096):
        pairs = PAIRS if frame <= 8 else PAIRS[:2]
        for k, (m, h) in enumerate(pairs):
            lens = sorted({n for n in (1, frame - 1, frame, frame + 1, 2 * frame - 1, 2 * frame, 2 * frame + 1, 3 * frame + 5, 70 * frame + 3)
                           if n >= 1 and n <= 70000})
            utts = [of_length(rng, frame, n) for n in lens]
            prefix = 3 + k
            # every residue mod 8 of an utterance's first sample: a filler utterance moves the next start to it
            cur = prefix + sum(len(u) for u in utts)
            for r in range(8):
                fill = (r - cur) % 8 or 8
                utts.append(of_length(rng, frame, fill, p_loud=1.0))
                cur += fill
                assert cur % 8 == r
                utts.append(of_length(rng, frame, 2 * frame + 3))
                cur += 2 * frame + 3
            c = pack("align-f%d-m%d-h%d" % (frame, m, h), _policy(frame, m, h), utts, prefix)
            assert set((c["offsets"] % 8).tolist()) == set(range(8))
            out.append(c)
    return out


def _chunk_cases(rng):
    """frame = 1 (a frame is a sample, so the buffers stay small): frame counts on either side of the decide pass's chunk and of twice
    it; runs of min_run - 1 and min_run active frames ending and starting exactly at a chunk edge; loud frames whose hangover crosses
    an edge upwards and downwards."""
    C, out = DECIDE_CHUNK, []
    for (m, h) in PAIRS:
        utts = []
        for F in (C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1):
            utts.append(utterance(rng, 1, rng.random_sample(F) < 0.3))
        F = 2 * C + 1 + m
        # runs ending exactly at an edge: min_run frames before the first edge (kept), min_run - 1 before the second (dropped)
        pat = np.zeros(F, dtype=bool)
        pat[C - m:C] = True
        pat[2 * C - (m - 1):2 * C] = True
        utts.append(utterance(rng, 1, pat))
        # runs starting exactly at an edge: min_run - 1 after the first (dropped), min_run after the second (kept)
        pat = np.zeros(F, dtype=bool)
        pat[C:C + m - 1] = True
        pat[2 * C:2 * C + m] = True
        utts.append(utterance(rng, 1, pat))
        # a run that straddles an edge, half on either side
        pat = np.zeros(F, dtype=bool)
        pat[C - m // 2:C - m // 2 + m] = True
        utts.append(utterance(rng, 1, pat))
        # speech just below an edge (its hangover reaches up across it) and just above the next (reaches down across it)
        pat = np.zeros(F + 2 * h, dtype=bool)
        pat[C - m - h // 2:C - h // 2] = True
        pat[2 * C + h // 2:2 * C + h // 2 + m] = True
        utts.append(utterance(rng, 1, pat))
        out.append(pack("chunk-m%d-h%d" % (m, h), _policy(1, m, h), utts, prefix=5))
    # the same edges at frame = 2 with a short last frame
    utts = [utterance(rng, 2, rng.random_sample(F) < 0.3, last=1) for F in (C, C + 1, 2 * C + 1)]
    out.append(pack("chunk-f2", _policy(2, 3, 10), utts, prefix=1))
    return out


def fallback_edge(min_keep_delta):
    """One utterance of 40 frames of 8 with 9 loud frames under (min_run, hang) = (1, 0): V = 72.  min_keep = 72 + delta."""
    rng = np.random.RandomState(11)
    pat = np.zeros(40, dtype=bool)
    pat[[0, 5, 6, 7, 19, 20, 30, 38, 39]] = True
    return pack("fallback%+d" % min_keep_delta, _policy(8, 1, 0, min_keep=72 + min_keep_delta), [utterance(rng, 8, pat)], prefix=2)


def _special_cases(rng):
    out = []
    zeros = np.zeros(1000, dtype=np.int16)
    out.append(pack("all-zero", _policy(160, 3, 10), [of_length(rng, 160, 333), zeros, of_length(rng, 160, 500)], prefix=7))
    full = np.full(2 * 4096 + 17, -32768, dtype=np.int16)
    out.append(pack("all-min-f4096", _policy(4096, 1, 0), [full, of_length(rng, 4096, 5000)], prefix=6))
    out.append(pack("floor", _policy(8, 1, 0, floor_energy=1.0e6), [of_length(rng, 8, 801), np.full(64, 1000, dtype=np.int16),
                                                                    np.full(64, 999, dtype=np.int16)], prefix=0))
    out.append(fallback_edge(0))
    out.append(fallback_edge(1))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.RandomState(2024)
    return tuple(_alignment_cases(rng) + _chunk_cases(rng) + _special_cases(rng))


def many_utterances(n=70000):
    """n utterances of 3..9 samples at frame = 2: more utterances than a grid's second dimension holds."""
    rng = np.random.RandomState(7)
    lens = rng.randint(3, 10, n).astype(np.int64)
    total = int(lens.sum())
    body = np.where(rng.random_sample(total) < 0.5, rng.randint(-8000, 8001, total), rng.randint(-3, 4, total)).astype(np.int16)
    sign = np.where(np.arange(24) % 2 == 0, POISON, -POISON).astype(np.int16)
    offsets = 3 + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return {"name": "many", "policy": _policy(2, 1, 1), "buf": np.concatenate([sign[:3], body, sign]), "offsets": offsets, "lens": lens}


def reference_many(case):
    """``reference(case)`` for a case with min_run = 1 and hang = 1, in flat numpy over all utterances at once (``vad_reference`` per
    utterance takes seconds at 70 000 of them); the first 300 utterances and the last are checked against ``vad_reference`` here."""
    pol, lens, offs = case["policy"], case["lens"], case["offsets"]
    assert pol.min_run == 1 and pol.hang == 1
    Fr, n = pol.frame, len(lens)
    body = case["buf"][offs[0]:offs[-1] + lens[-1]].astype(np.int64)
    F = (lens + Fr - 1) // Fr
    fb = np.concatenate([[0], np.cumsum(F)]).astype(np.int64)
    utt = np.repeat(np.arange(n), F)                                 # the utterance of every flat frame
    f_in = np.arange(fb[-1]) - fb[utt]                               # its index in the utterance
    start = (offs - offs[0])[utt] + f_in * Fr
    n_f = np.minimum(Fr, lens[utt] - f_in * Fr)
    E = np.add.reduceat(body ** 2, start)
    T = np.add.reduceat(E, fb[:-1])
    Ed, nd = E.astype(np.float64), n_f.astype(np.float64)
    a = (E > 0) & (Ed * lens[utt].astype(np.float64) >= np.float64(pol.rel) * (T[utt].astype(np.float64) * nd)) \
        & (Ed >= np.float64(pol.floor_energy) * nd)
    first, last = f_in == 0, f_in == F[utt] - 1
    v = a | (np.concatenate([[False], a[:-1]]) & ~first) | (np.concatenate([a[1:], [False]]) & ~last)
    whole = np.add.reduceat(v * n_f, fb[:-1]) < pol.keep()
    v = v | whole[utt]
    kept = v * n_f
    new_lens = np.add.reduceat(kept, fb[:-1])
    run = np.cumsum(kept) - kept
    ref = {"energy": E, "mask": v.astype(np.uint8), "dst": run - run[fb[:-1]][utt], "active": a, "frame_base": fb, "new_lens": new_lens,
           "out": body[np.repeat(v, n_f)].astype(np.int16),
           "info": np.stack([F, np.add.reduceat(a.astype(np.int64), fb[:-1]), np.add.reduceat(v.astype(np.int64), fb[:-1]),
                             whole.astype(np.int64)], axis=1).astype(np.int32)}
    for u in list(range(min(n, 300))) + [n - 1]:
        r = vad_reference(case["buf"][offs[u]:offs[u] + lens[u]], pol)
        sl = slice(fb[u], fb[u + 1])
        assert np.array_equal(ref["energy"][sl], r["energy"]) and np.array_equal(ref["mask"][sl], r["mask"])
        assert np.array_equal(ref["dst"][sl], r["dst"]) and tuple(ref["info"][u]) == r["info"] and new_lens[u] == r["new_len"]
    return ref


_REF = {}


def reference(case):
    """``vad_reference`` of every utterance of the case in the layout of the entry points: flat ``energy`` / ``mask`` / ``dst`` /
    ``active``, ``frame_base``, ``new_lens``, ``info`` (n, 4) and ``out``, the trimmed utterances back to back.  Cached by case name;
    the arrays are read-only."""
    if case["name"] not in _REF:
        rows = [vad_reference(case["buf"][o:o + n], case["policy"]) for o, n in zip(case["offsets"], case["lens"])]
        cat = lambda k, dt: np.concatenate([np.asarray(r[k]) for r in rows]).astype(dt) if rows else np.zeros(0, dt)  # noqa: E731
        ref = {"energy": cat("energy", np.int64), "mask": cat("mask", np.uint8), "dst": cat("dst", np.int64),
               "active": cat("active", bool), "out": cat("pcm", np.int16),
               "frame_base": np.concatenate([[0], np.cumsum([r["info"][0] for r in rows])]).astype(np.int64),
               "new_lens": np.array([r["new_len"] for r in rows], dtype=np.int64),
               "info": np.array([r["info"] for r in rows], dtype=np.int32).reshape(-1, 4)}
        for v in ref.values():
            v.setflags(write=False)
        _REF[case["name"]] = ref
    return _REF[case["name"]]


def pause_corpus(tmp_path, seconds=0.05, n_speakers=6, files=3):
    """A tiny shard directory read as a ``ShardedSpeechDataset`` of ``seconds`` fragments: files of 2.5 to 5 fragments of noise with
    three planted pauses each (100 to 500 samples of -1, 0 or 1)."""
    import pandas as pd
    from voicemap_amd import shards
    rng = np.random.RandomState(5)
    rows, waves = [], []
    for s in range(n_speakers):
        for k in range(files):
            n = int(rng.randint(int(2.5 * 16000 * seconds), int(5 * 16000 * seconds)))
            x = rng.randint(-6000, 6001, n).astype(np.float64)
            for _ in range(3):
                b = int(rng.randint(0, n - 500))
                x[b:b + int(rng.randint(100, 500))] = rng.randint(-1, 2)
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
    return shards.ShardedSpeechDataset(str(tmp_path), seconds, stochastic=True, pad=False)
