"""Speed perturbation of the device-resident int16 corpus: every file resampled to other tempos by an integer polyphase filter.

Most speaker-embedding recipes train on three copies of every file -- at 0.9x, 1.0x and 1.1x speed -- and count the two resampled
copies as NEW speakers: pitch and formants move with the tempo.  This module states the resampler in numpy (``resample_reference``:
what every test compares against), runs it over the resident corpus in one launch (``resample``: ``vm_resample_i16``,
voicemap_amd/csrc/speed.hip) and designs its filter (``design_taps``).  The audio is int16 PCM, the taps are integers and the
accumulator is an integer, so the kernel and the statement agree bit for bit.

The statement.  A speed factor is a rational D / U in lowest terms: U output samples per D input samples (speed 0.9: U, D = 10, 9;
speed 1.1: 10, 11).  For one file x of ``len`` int16 samples, an integer table ``taps`` of n = U T entries and c = n // 2:

  n_out  = (len U + D - 1) // D
  acc[m] = sum over k in [0, len) with 0 <= m D + c - k U < n of taps[m D + c - k U] x[k]                     (int64)
  y[m]   = clip((acc[m] + (1 << (shift - 1))) >> shift, -32768, 32767)       (arithmetic shift: round half up, negatives included)

Samples outside the file are zero -- nothing of a neighbouring file is ever read; ``shift`` = 0 adds no rounding term; ``len`` = 0
gives no output.  Output m reads the T taps of ONE phase, p = (m D + c) % U: acc[m] = sum_{i < T} taps[p + i U] x[q - i] with
q = (m D + c) // U, so |acc| <= 2^15 max_p sum_i |taps[p + i U]| (``phase_abs_max``), which must stay below 2^62.

Limits: 1 <= U, D, T <= 64, 0 <= shift <= 30, 0 <= len < 2^31.

Whether speed perturbation lowers the EER on real data has not been measured here.
"""
from __future__ import annotations

from fractions import Fraction
from typing import Optional

import numpy as np

MAX_UD, MAX_TAPS_PER_PHASE, MAX_SHIFT, MAX_LEN = 64, 64, 30, (1 << 31) - 1
# the kernel's constants (csrc/speed.hip): the tests place utterance lengths on their edges
THREAD_OUTPUTS = 8     # SP_PER: consecutive outputs one thread computes and stores as one 16-byte word
TILE_OUTPUTS = 2048    # SP_TILE: outputs per tile at most
SPAN = 4096            # SP_SPAN: input samples a tile may read; its output count shrinks until they fit (``tile_outputs``)
NARROW_MAX = 65535     # SP_NARROW_MAX: ``phase_abs_max`` up to here runs the 32-bit accumulator, above it the 64-bit one


def tile_outputs(U: int, D: int, T: int) -> int:
    """Outputs per tile of the kernel for this ratio and filter length (sp_tile_outputs of csrc/speed.hip)."""
    t = min(TILE_OUTPUTS, ((SPAN - T - 1) * U) // D)
    return t - t % THREAD_OUTPUTS if t >= THREAD_OUTPUTS else t


def ratio(factor) -> tuple:
    """(U, D) of a speed factor: D / U = ``Fraction(factor).limit_denominator(64)`` in lowest terms."""
    f = Fraction(float(factor)).limit_denominator(MAX_UD)
    U, D = f.denominator, f.numerator
    if not (1 <= U <= MAX_UD and 1 <= D <= MAX_UD):
        raise ValueError("speed factor %r is %d/%d: numerator and denominator must be in [1, %d]" % (factor, D, U, MAX_UD))
    return U, D


def output_length(lens, U: int, D: int):
    """n_out = ceil(len U / D), for an integer or an int64 array."""
    if np.ndim(lens) == 0:
        return (int(lens) * U + D - 1) // D
    return (np.asarray(lens, dtype=np.int64) * U + D - 1) // D


def design_taps(U: int, D: int, T: int = 32, rolloff: float = 0.95, beta: float = 9.0, shift: int = 15) -> np.ndarray:
    """The Kaiser-windowed sinc low-pass of U T integer taps, cut off at ``rolloff`` of the lower of the two Nyquist rates, with a
    per-phase DC gain of 2^shift."""
    n = U * T
    j = np.arange(n) - n // 2
    fc = rolloff * 0.5 / max(U, D)
    return np.rint(2 * fc * np.sinc(2 * fc * j) * np.kaiser(n + 1, beta)[:n] * U * 2.0 ** shift).astype(np.int64)


def phase_abs_max(taps, U: int) -> int:
    """max over the U phases of sum_i |taps[p + i U]|: 2^15 times this bounds every |acc|."""
    return int(np.abs(np.asarray(taps, dtype=np.int64)).reshape(-1, U).sum(axis=0).max())


def _check(U, D, taps, shift):
    U, D, shift = int(U), int(D), int(shift)
    if not (1 <= U <= MAX_UD and 1 <= D <= MAX_UD):
        raise ValueError("U and D must be in [1, %d]" % MAX_UD)
    if not 0 <= shift <= MAX_SHIFT:
        raise ValueError("shift must be in [0, %d]" % MAX_SHIFT)
    taps = np.asarray(taps)
    if taps.ndim != 1 or taps.size == 0 or taps.size % U or not np.issubdtype(taps.dtype, np.integer):
        raise ValueError("taps must be a 1-D integer table of U * T entries")
    T = taps.size // U
    if not 1 <= T <= MAX_TAPS_PER_PHASE:
        raise ValueError("taps per phase must be in [1, %d]" % MAX_TAPS_PER_PHASE)
    taps = taps.astype(np.int64)
    if taps.size and (taps.min() < -(1 << 31) or taps.max() > (1 << 31) - 1):
        raise ValueError("a tap does not fit int32")
    pam = phase_abs_max(taps, U)
    if pam >= 1 << 47:
        raise ValueError("the taps of one phase sum to %d in magnitude: 2^15 times that must stay below 2^62" % pam)
    return U, D, taps, T, shift, pam


def _as_pcm(pcm) -> np.ndarray:
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16:
        raise TypeError("the resampler reads int16 PCM (shards.to_int16), not %s" % pcm.dtype)
    return pcm.reshape(-1)


def resample_reference(pcm, U: int, D: int, taps, shift: int) -> np.ndarray:
    """The statement of the module docstring for ONE file, numpy int64.  ``pcm``: 1-D int16; returns int16 of ceil(len U / D)."""
    x = _as_pcm(pcm).astype(np.int64)
    U, D, taps, T, shift, _ = _check(U, D, taps, shift)
    n, c = int(x.size), (U * T) // 2
    if n > MAX_LEN:
        raise ValueError("a file must hold fewer than 2^31 samples")
    n_out = output_length(n, U, D)
    y = np.empty(n_out, dtype=np.int16)
    rnd = (1 << (shift - 1)) if shift > 0 else 0
    i = np.arange(T, dtype=np.int64)
    for m0 in range(0, n_out, 1 << 16):
        v = np.arange(m0, min(m0 + (1 << 16), n_out), dtype=np.int64) * D + c
        q, p = v // U, v % U
        k = q[:, None] - i[None, :]
        inside = (k >= 0) & (k < n)
        acc = (taps[p[:, None] + i[None, :] * U] * np.where(inside, x[np.clip(k, 0, max(n - 1, 0))], 0)).sum(axis=1)
        y[m0:m0 + len(v)] = np.clip((acc + rnd) >> shift, -32768, 32767)
    return y


class SpeedPolicy:
    """Which copies ``ShardedSpeechDataset.speed_perturbed`` adds: one per entry of ``factors`` (each a rational D / U with U, D <= 64:
    ``ratio``), resampled by ``design_taps(U, D, taps_per_phase, rolloff, beta, shift)``.  ``new_speakers``: a copy counts as a new
    speaker (the recipes' default); with False it keeps its speaker, and a same-speaker pair may then be a file and its own copy."""

    def __init__(self, factors=(0.9, 1.1), taps_per_phase: int = 32, rolloff: float = 0.95, beta: float = 9.0, shift: int = 15,
                 new_speakers: bool = True):
        self.factors = tuple(float(f) for f in factors)
        self.taps_per_phase, self.rolloff, self.beta, self.shift = int(taps_per_phase), float(rolloff), float(beta), int(shift)
        self.new_speakers = bool(new_speakers)
        if not self.factors:
            raise ValueError("no speed factor given")
        if not all(np.isfinite(f) and f > 0 for f in self.factors):
            raise ValueError("speed factors must be positive numbers")
        self.ratios = tuple(ratio(f) for f in self.factors)
        if any(U == D for U, D in self.ratios) or len(set(self.ratios)) != len(self.ratios):
            raise ValueError("speed factors must differ from 1 and from each other (the originals are always kept)")
        if not 1 <= self.taps_per_phase <= MAX_TAPS_PER_PHASE:
            raise ValueError("taps_per_phase must be in [1, %d]" % MAX_TAPS_PER_PHASE)
        if not 0 <= self.shift <= MAX_SHIFT:
            raise ValueError("shift must be in [0, %d]" % MAX_SHIFT)
        if not (0.0 < self.rolloff <= 1.0 and self.beta >= 0.0):
            raise ValueError("rolloff must be in (0, 1] and beta non-negative")

    def taps(self, k: int) -> np.ndarray:
        """The filter of factor k (0-based)."""
        U, D = self.ratios[k]
        return design_taps(U, D, self.taps_per_phase, self.rolloff, self.beta, self.shift)


def resample(audio, offsets, lens, U: int, D: int, taps, shift: int, out=None):
    """(audio', offsets', lens'): every utterance ``audio[offsets[u] : offsets[u] + lens[u]]`` of a resident int16 buffer resampled by
    U / D, back to back in a new device buffer of exactly their size; ``offsets'`` / ``lens'`` are host int64 arrays.  One launch, no
    read-back and no synchronisation: the host knows every output length in closed form.  ``out`` (optional): a contiguous int16 device
    tensor of exactly that size to write into (a slice of a larger buffer), returned as ``audio'``."""
    import torch
    from . import _lib
    U, D, taps, T, shift, pam = _check(U, D, taps, shift)
    offsets = np.ascontiguousarray(np.asarray(offsets.cpu() if hasattr(offsets, "cpu") else offsets, dtype=np.int64).reshape(-1))
    lens = np.ascontiguousarray(np.asarray(lens.cpu() if hasattr(lens, "cpu") else lens, dtype=np.int64).reshape(-1))
    if offsets.size != lens.size:
        raise ValueError("offsets and lens differ in length")
    if lens.size and (lens.min() < 0 or lens.max() > MAX_LEN):
        raise ValueError("every utterance must hold 0 <= len < 2^31 samples")
    if not torch.is_tensor(audio) or audio.dtype != torch.int16:
        raise TypeError("the resampler reads the resident int16 PCM buffer (ShardedSpeechDataset.to_device), not %s"
                        % (audio.dtype if hasattr(audio, "dtype") else type(audio).__name__))
    if audio.dim() != 1 or not audio.is_cuda or not audio.is_contiguous():
        raise ValueError("audio must be a contiguous 1-D device tensor")
    if lens.size and (offsets.min() < 0 or int((offsets + lens).max()) > audio.numel()):
        raise ValueError("an utterance lies outside the audio buffer")
    n = int(lens.size)
    new_lens = output_length(lens, U, D)
    base = np.concatenate([[0], np.cumsum(new_lens)]).astype(np.int64)
    new_offsets, total = base[:-1].copy(), int(base[-1])
    if out is None:
        out = torch.empty(total, dtype=torch.int16, device=audio.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.int16 and out.dim() == 1 and out.is_contiguous() and out.numel() == total
              and out.device == audio.device):
        raise ValueError("out must be a contiguous 1-D int16 tensor of %d samples on the audio's device" % total)
    if n and total:
        tab = torch.from_numpy(np.concatenate([offsets, lens, base, new_offsets])).to(audio.device)   # one upload
        taps_dev = torch.from_numpy(taps.astype(np.int32)).to(audio.device)
        e = tab.element_size()
        _lib.lib().call("vm_resample_i16", audio.data_ptr(), tab.data_ptr(), tab.data_ptr() + n * e, tab.data_ptr() + 2 * n * e, n, U, D,
                        taps_dev.data_ptr(), T, shift, pam, tab.data_ptr() + (3 * n + 1) * e, out.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
        # (tab and taps_dev are freed on return: the allocator hands their memory out again in this stream's order, after the launch)
    return out, new_offsets, new_lens


def add_speed_args(parser):
    """``--speed-perturb`` and ``--speed-same-speaker``, off by default (``policy_from_args`` makes the policy)."""
    parser.add_argument('--speed-perturb', metavar='FACTORS', default=None,
                        help='add a resampled copy of every training file per comma-separated speed factor, e.g. 0.9,1.1, counted as '
                             'new speakers (voicemap_amd/speed.py); off by default')
    parser.add_argument('--speed-same-speaker', action='store_true',
                        help='with --speed-perturb: the copies keep their speaker (a same-speaker pair may then be a file and its own copy)')
    return parser


def policy_from_args(args, need_device_data: bool = False) -> Optional[SpeedPolicy]:
    """The policy the scripts' ``--speed-perturb`` flags ask for (None without them).  ``need_device_data``: the training scripts,
    where the resampler runs on the resident corpus of ``--device-data``."""
    spec = getattr(args, "speed_perturb", None)
    if not spec:
        if getattr(args, "speed_same_speaker", False):
            raise SystemExit("--speed-same-speaker needs --speed-perturb")
        return None
    if need_device_data and not getattr(args, "device_data", False):
        raise SystemExit("--speed-perturb needs --device-data: the resampler runs on the resident training corpus")
    try:
        return SpeedPolicy(factors=[float(s) for s in str(spec).split(",") if s.strip()],
                           new_speakers=not getattr(args, "speed_same_speaker", False))
    except ValueError as e:
        raise SystemExit("--speed-perturb: %s" % e)
