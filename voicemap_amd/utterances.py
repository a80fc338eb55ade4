"""Whole-utterance embedding: the host planner behind ``HipEncoderEngine.embed_varlen``.

The reference's encoder (voicemap/models.py:6-41 with ``input_shape=None``) is fully convolutional and ends in GlobalMaxPool1D, so
``encoder.predict`` takes a recording of any length.  For a recording of n_raw samples the embedding is what the encoder computes on it
ALONE: ``r[::ds]`` (l0 = ceil(n_raw / ds) samples), ``whiten`` over those l0 samples, then every block at its own length (each pools to
floor(L / pool)) and the global max over the last block's rows.  A recording whose last pooled length would be 0 is rejected.

On the device recordings of similar length share a bucket: one padded length L0 and a per-window valid length (the *_varlen entry
points of include/voicemap_hip.h write every pooled row past a window's valid length as zero, which is exactly the next convolution's
SAME padding, so the valid rows are bit for bit what the recording alone gives).  This module decides the buckets:

* L0 is a multiple of the product of the pool sizes (32 for the baseline): every block length of the bucket is then exact and even,
  so the fused conv + pool launches serve the 16-bit modes;
* L0 comes from a FIXED ladder (``ladder``): every multiple of that quantum up to quantum / max_pad_frac, then a geometric ladder of
  ratio 1 / (1 - max_pad_frac).  A recording lands on the first rung at or above its length, so a bucket's padded rows are below
  max_pad_frac of its rows (below one quantum per recording on the short rungs), and the number of distinct bucket lengths is bounded by
  the rungs up to the longest recording, whatever the length distribution;
* n * L0 <= row_budget (default: the decimated rows of bench.py's inference batch, 256 windows x 3 s), so device memory does not grow
  with the corpus.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

DEFAULT_ROW_BUDGET = 256 * 12000      # bench.py's inference batch: 256 windows of 3 s at 16 kHz, decimated by 4
DEFAULT_MAX_PAD_FRAC = 1.0 / 8
MAX_PLANS = 16                        # what embed_varlen may leave on an engine, whatever the corpus (it leaves one arena)


def pool_quantum(blocks: Sequence[Tuple[int, int, int]]) -> int:
    """Product of the pool sizes: the bucket-length quantum and the shortest decimated length the encoder accepts (its last pooled
    length is then >= 1)."""
    q = 1
    for (_, _, p) in blocks:
        q *= int(p)
    return q


def ladder(quantum: int, max_pad_frac: float, top: int) -> List[int]:
    """The bucket lengths, ascending, up to the first rung >= ``top``."""
    if not (0.0 < max_pad_frac < 1.0):
        raise ValueError("max_pad_frac must lie in (0, 1)")
    base = quantum * int(math.ceil(1.0 / max_pad_frac))
    rungs, L = [], quantum
    while True:
        rungs.append(L)
        if L >= top:
            return rungs
        if L < base:
            L += quantum
        else:   # the next rung is at most L / (1 - f): a recording above L pads less than f of the rung
            L = max(L + quantum, int(L / (1.0 - max_pad_frac)) // quantum * quantum)


class BucketPlan:
    """``buckets``: [(L0, indices into the input, ascending length)]; ``order``: their concatenation; ``inverse``: the position of
    every input row in ``order``."""

    def __init__(self, buckets, n, l0s, row_budget, max_pad_frac, quantum):
        self.buckets = buckets
        self.order = np.concatenate([b for _, b in buckets]) if buckets else np.zeros(0, np.int64)
        self.inverse = np.empty(n, np.int64)
        self.inverse[self.order] = np.arange(n)
        self.row_budget, self.max_pad_frac, self.quantum = row_budget, max_pad_frac, quantum
        self.valid_rows = int(np.asarray(l0s, np.int64).sum())
        self.padded_rows = int(sum(L0 * len(b) for L0, b in buckets))

    @property
    def shapes(self):
        """Distinct bucket lengths."""
        return sorted({L0 for L0, _ in self.buckets})

    @property
    def pad_overhead(self) -> float:
        """padded rows / valid rows - 1."""
        return self.padded_rows / max(self.valid_rows, 1) - 1.0


def plan_buckets(l0s, row_budget: int = DEFAULT_ROW_BUDGET, max_pad_frac: float = DEFAULT_MAX_PAD_FRAC, quantum: int = 32,
                 names: Optional[Sequence] = None) -> BucketPlan:
    """Pack recordings of decimated lengths ``l0s`` into buckets (pure host code).  ``names`` (optional, per recording) label the
    error of a recording shorter than ``quantum``."""
    l0s = np.asarray(l0s, dtype=np.int64).reshape(-1)
    n = len(l0s)
    short = np.nonzero(l0s < quantum)[0]
    if short.size:
        i = int(short[0])
        raise ValueError("recording %s is too short for the encoder: %d decimated samples, the minimum is %d"
                         % (names[i] if names is not None else i, int(l0s[i]), quantum))
    if n == 0:
        return BucketPlan([], 0, l0s, row_budget, max_pad_frac, quantum)
    rungs = np.asarray(ladder(quantum, max_pad_frac, int(l0s.max())), dtype=np.int64)
    if rungs[np.searchsorted(rungs, l0s.max())] > row_budget:
        raise ValueError("a recording of %d decimated samples does not fit the row budget %d" % (int(l0s.max()), row_budget))
    rung = np.searchsorted(rungs, l0s, side="left")          # first rung >= l0
    order = np.lexsort((np.arange(n), l0s))                   # by length, ties in input order
    buckets = []
    r_sorted = rung[order]
    starts = np.flatnonzero(np.r_[True, r_sorted[1:] != r_sorted[:-1]])
    ends = np.r_[starts[1:], n]
    for s, e in zip(starts, ends):
        L0 = int(rungs[r_sorted[s]])
        cap = row_budget // L0
        for b0 in range(s, e, cap):
            buckets.append((L0, order[b0:min(b0 + cap, e)].astype(np.int64)))
    return BucketPlan(buckets, n, l0s, row_budget, max_pad_frac, quantum)


def valid_lengths(l0s, blocks) -> np.ndarray:
    """(len(blocks) + 1, n) int32: the valid length of every window at the input of each block, and of the last block's output."""
    out = [np.asarray(l0s, dtype=np.int64)]
    for (_, _, p) in blocks:
        out.append(out[-1] // int(p))
    return np.stack(out).astype(np.int32)
