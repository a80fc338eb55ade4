"""Exact references for the waveform front end (tests/test_gpu_wave_exact.py; checked on the host by tests/test_wave_exact_cpu.py).

The 1-D path's input stage is csrc/preproc.hip (crop, x[::ds], per-window mean, one scale per tower, the 15 / 16 halo, the varlen form)
and csrc/augment.hip (the polyphase decimating FIR, the babble sums, g, the gain).  tests/test_gpu_augment.py holds the FIR to the
worst-case fp32 bound gamma_R sum |r_j| |s|, under which a tap at a loop edge is invisible at the tap counts training uses
(tests/test_wave_exact_cpu.py measures it).  This module is the anchor at tolerance zero: pure numpy, it imports neither the library
nor torch.

Method (that of gemm_exact.py / bn_exact.py / spectro_exact.py / score_exact.py).  Speech and noise are k / 32768 with k ODD and
|k| <= 255 -- the same values as int16 and as fp32, non-zero everywhere, so what lies before a crop and at or past raw_len is real data
the kernel must not use.  RIR taps are t / 16 with t in +-{1..4}: every tap non-zero, no decaying tail, every product matters.  A
product is a multiple of 2^-19 (A_UNIT); ``fir_exact`` takes the convolution in int64 and asserts max_i sum_j |t_j| |k_{i ds - j}| < 2^24,
so every fp32 partial sum IN ANY ORDER is exact (255 * 4 * 8192 < 2^23 is the ceiling at R = 8192; the table peaks near 2^21) and the FIR's
output is known bit for bit: one missing or misplaced product moves an output by at least one grid unit.

After the FIR everything on the device is float64.  The five partial-sum planes (sum a, a^2, v, v^2, a v) are exact on this grid in
any order (integers below 2^53 in units of 2^-19 / 2^-38: ``window_sums`` asserts it with Python integers), so the reference works from
the exact sums in closed form:

    g   = sqrt((A / L0) / ((V / L0) snr))              A, V the exact sums of a^2, v^2
    y_i = G (a_i + g v_i)
    m   = G (Sa + g Sv) / Ln                           Sa, Sv the exact sums of a, v
    Q   = G^2 (A + 2 g AV + g^2 V)                     the window's sum of y^2
    sc  = rms / sqrt(fsum_tower(Q) / (wpt Ln))         (whitening off: m = 0, sc = 1)
    x_i = (y_i - m) sc

The acceptance rule (``accept``).  Device and reference both round in float64 and may differ in the last bits (the contraction of
pa + g pv and y + g b into fused multiply-adds, a plain sqrt whose rounding nobody has measured, another order of the tower's sum).
With d = C 2^-53 (sc (|y| + |m|) + |x|), a sample is AMBIGUOUS if fp32(x - d) != fp32(x + d); the device must equal fp32(x) on every
other sample and lie in [fp32(x - d), fp32(x + d)] -- two neighbouring fp32 numbers, except around an x of exactly zero -- on an
ambiguous one.  C counts the float64 roundings of the longest path, each taken relative to the magnitude the formula carries:

    device     g: A / L0, V / L0, Pv snr, the quotient, and a square root that halves those four and adds one            3
               y: g b (3 + 1), the sum, the gain                                                            6 on sc |y|
               m: g pv (4), the sum, the gain; seven additions of the 8 segments; / Ln                      14 on sc |m|
               sc: 2 g av (4) | g g qv (6 + 1 + 1 = 8, the longest), two sums, G^2: 11; the tower's sum over wpt * 8 partials
                   (two per thread at most up to wpt = 33, six butterfly steps, two more) 10; / (wpt Ln) 1: 22; the square root
                   halves them and adds one: 12; rms / . : 13; then y - m and (.) sc                         15 on |x|
    reference  g 3, y 6, m = G (Sa + g Sv) / Ln 7; Q 11, fsum 1, the quotient 1: 13, the square root 7.5, rms / . 8.5, the two
               operations of x                                                                              10.5 on |x|

so C = 15 + 11 = 26 (C_ROUNDINGS).  d carries |y|, not |a| + g |v|: where a and g v cancel to a small fraction of their size the
two forms of y + g b differ by more than d in float64 (4.8 d measured on the host, at a y of 6e-7) -- which reaches the fp32 result
only if that sample also sits within that distance of an fp32 midpoint; the host test holds the contracted form to the rule itself.  At most AMBIGUOUS_CAP = 1e-4 of a case's samples may be ambiguous:
the host test asserts it from the reference alone for every input the device file uses (the expected share is a few 2^-22 per sample;
seeds are chosen so that the cases stay inside).  Two families of inputs would break the cap by construction and are kept out:
L0 = 1 with whitening (y - mean is identically zero: every sample is a zero, which the rule must call ambiguous; those cases run with
whitening off, where g and the segments are still observed), and whitening off with g = 0 and a gain that is no power of two (G k is
a 32-bit integer rounded to 24: an exact tie once in 256).

The host models (``model_fir``, ``model_plain``) restate the loop structure of fir_decimate_kernel (phase, 256-tap chunk, 2048-output
tile, causal limit, mb_end rounded up to 8) and of the whitening passes (8 statistics segments, 8 apply splits, the halo) with
switchable defects; the host test shows that each defect fails the exact comparison."""
import functools
import math
from fractions import Fraction

import numpy as np

# the kernels' constants: no ABI query returns them
FIR_TILE, FIR_MC, FIR_O = 2048, 256, 8     # voicemap_amd/csrc/augment.hip:38  FIR_T * FIR_O outputs per tile, FIR_MC taps per chunk
N_SEG = 8                                  # augment.hip:15 AUG_SEG, preproc.hip:16 WS_SEG
N_SPLIT = 8                                # augment.hip:16 AUG_SPLIT, preproc.hip:52 WA_SPLIT
HALO_L, HALO_R = 15, 16                    # preproc.hip:10, augment.hip:14
HALO = HALO_L + HALO_R
MAX_R = 8192                               # vm_crop_augment_decimate_whiten's limit

S_UNIT, T_UNIT, A_UNIT = 2.0 ** -15, 2.0 ** -4, 2.0 ** -19     # sample, tap and product grids
LIMIT = 1 << 24                            # integers below it are fp32 numbers
RMS = float(np.float32(0.038021))          # the C ABI takes rms as fp32
C_ROUNDINGS = 26                           # module docstring
AMBIGUOUS_CAP = 1e-4

DS_VALUES = (1, 2, 3, 4, 7)
L0_SMALL, L0_LARGE = (1, 7, 8, 9), (2047, 2048, 2049, 4097)
FIR_GAINS = (1.0, 0.5, 2.0)
WPT_VALUES = (1, 2, 32, 33)


# ---- grid inputs --------------------------------------------------------------------------------------------------------------------
def grid_samples(rng, total):
    """int64 k, odd, |k| <= 255: the sample is k / 32768."""
    return 2 * rng.integers(-128, 128, int(total)) + 1


def as_source(k, src):
    """The buffer the kernel reads: int16 k, or fp32 k / 32768 (the same values)."""
    k = np.asarray(k)
    return k.astype(np.int16) if src == "i16" else (k * S_UNIT).astype(np.float32)


def grid_taps(rng, n, R):
    """int64 (n, R) t in +-{1..4}: the tap is t / 16."""
    return rng.integers(1, 5, (n, R)) * rng.choice((-1, 1), (n, R))


def as_rirs(t):
    return (np.asarray(t) * T_UNIT).astype(np.float32)


def raw_len_of(L0, ds, end):
    """The two ends of the raw lengths that decimate to L0 samples."""
    return (L0 - 1) * ds + 1 if end == "lo" else L0 * ds


def n_out(raw_len, ds):
    return (raw_len + ds - 1) // ds


# ---- the FIR ------------------------------------------------------------------------------------------------------------------------
def fir_exact(k, t, ds):
    """a in units of 2^-19 (int64, (L0,)): the full convolution's first raw_len samples, decimated.  Asserts the precondition of
    exactness, max_i sum_j |t_j| |k_{i ds - j}| < 2^24: every fp32 partial sum in any order is then an fp32 number."""
    k, t = np.asarray(k, dtype=np.int64), np.asarray(t, dtype=np.int64)
    a = np.convolve(k, t)[:len(k)][::ds]
    peak = int(np.convolve(np.abs(k), np.abs(t))[:len(k)][::ds].max())
    assert peak < LIMIT, (len(k), len(t), peak)
    return a, peak


def r_values(ds):
    """The tap counts of a decimation: 1, 2, around ds (more phases than taps), around one 8-tap block per phase, phase 0's Mp across
    the 256-tap chunk, two chunks and a remainder, the limit."""
    v = {1, 2, ds - 1, ds, ds + 1, 8 * ds - 1, 8 * ds + 1, 255 * ds, 256 * ds, 256 * ds + 1, 257 * ds, 512 * ds + ds - 1, MAX_R}
    return tuple(sorted(r for r in v if 1 <= r <= MAX_R))


def fir_case_table():
    """(ds, R, L0, end, src, gain) of every FIR launch: per (ds, R) one small and one large L0, the other axes cycled.  R = 8192 takes
    L0 = 2049 as its large one: with ds = 1 that is the clipped-causal case (tile 0 clipped to 2048 taps, tile 1 nine chunks, the
    last with one tap left)."""
    out, c = [], 0
    for ds in DS_VALUES:
        for R in r_values(ds):
            large = 2049 if R == MAX_R else L0_LARGE[c % 4]
            for j, L0 in enumerate((L0_SMALL[c % 4], large)):
                q = (c // 4 + j) % 4                      # every length meets both ends of raw_len in both source types
                out.append((ds, R, L0, ("lo", "hi")[q & 1], ("i16", "f32")[q >> 1], FIR_GAINS[(c + j) % 3]))
            c += 1
    return tuple(out)


FIR_CASES = fir_case_table()
FIR_PAD = 45           # samples of the buffer outside the longest crop


def fir_id(c):
    return "ds%d-R%d-L%d-%s-%s-g%g" % c


class FirCase:
    """One launch that shows the FIR alone (whitening = 0, K = 0): three windows of one buffer -- an RIR window that ends with the
    buffer (its history is real data), a window without an RIR, an RIR window at offset 0 (real data at and past raw_len) -- two
    RIRs, one gain for all."""

    def __init__(self, ds, R, L0, end, src, gain):
        self.ds, self.R, self.L0, self.end, self.src, self.g = ds, R, L0, end, src, gain
        self.raw_len = raw_len_of(L0, ds, end)
        rng = np.random.default_rng(1000003 * ds + 101 * R + L0 + (end == "hi"))
        self.total = self.raw_len + FIR_PAD
        self.k = grid_samples(rng, self.total)
        self.t = grid_taps(rng, 2, R)
        self.offsets = np.array([self.total - self.raw_len, 3, 0], dtype=np.int64)
        self.rir_id = np.array([0, -1, 1], dtype=np.int32)
        self.gain = np.full(3, gain, dtype=np.float32)
        self.n = 3

    def window(self, w):
        return self.k[self.offsets[w]:self.offsets[w] + self.raw_len]

    def a_units(self):
        """(n, L0) int64 in units of 2^-19 and the largest sum |t| |k| of the case."""
        a, peak = np.zeros((self.n, self.L0), dtype=np.int64), 0
        for w in range(self.n):
            if self.rir_id[w] >= 0:
                a[w], pk = fir_exact(self.window(w), self.t[self.rir_id[w]], self.ds)
                peak = max(peak, pk)
            else:
                a[w] = 16 * self.window(w)[::self.ds]
        return a, peak

    def expected(self):
        """(n, L0 + 31) fp32: gain * a between the zero halos, exact."""
        a, _ = self.a_units()
        x = a.astype(np.float64) * A_UNIT * float(self.g)
        out = np.pad(x, ((0, 0), (HALO_L, HALO_R))).astype(np.float32)
        assert np.array_equal(out.astype(np.float64)[:, HALO_L:HALO_L + self.L0], x)      # nothing rounded
        return out


@functools.lru_cache(maxsize=None)
def fir_case(c):
    return FirCase(*c)


def fir_locate(w, i):
    return "window %d, output %d (tile %d, thread %d, slot %d)" % (w, i, i // FIR_TILE, (i % FIR_TILE) // FIR_O, i % FIR_O)


def fir_report(got, want, gain, what):
    """None, or the first mismatch by window, output, tile and slot with the difference in grid units of 2^-19 gain."""
    got, want = np.asarray(got), np.asarray(want)
    bad = ~(got == want)                                   # NaN (an entry never written) is a mismatch
    if not bad.any():
        return None
    w, col = (int(v) for v in np.argwhere(bad)[0])
    i = col - HALO_L
    L0 = want.shape[1] - HALO
    where = fir_locate(w, i) if 0 <= i < L0 else "window %d, halo column %d" % (w, col)
    return "%s: %d of %d samples differ; first at %s: expected %r, got %r, difference %.6g grid units" % (
        what, int(bad.sum()), bad.size, where, float(want[w, col]), float(got[w, col]),
        (float(got[w, col]) - float(want[w, col])) / (A_UNIT * float(gain)))


DEFECTS_FIR = ("drop_last_tap", "drop_chunk_edge_block", "causal_strict", "history", "phase_sign")


def model_fir(buf, off, raw_len, ds, taps, defect=None, dtype=np.int64):
    """fir_decimate_kernel's loop structure on one window (buf[off : off + raw_len], taps (R,)): phases, chunks of 256 taps with the
    TILE + 256 staged samples, tiles of 2048 outputs, mlim = min(Mp, i_end), mb_end rounded up to a multiple of 8, zero history, nothing
    at or past raw_len.  ``dtype`` int64: integers in grid units; float32: the kernel's own arithmetic on the fp32 values (products
    and sums each rounded -- on the grid nothing rounds).  ``defect``: one of DEFECTS_FIR."""
    buf, taps = np.asarray(buf), np.asarray(taps)
    R, L0 = len(taps), n_out(raw_len, ds)
    out = np.zeros(L0, dtype=dtype)
    lane = np.arange(FIR_TILE + FIR_MC, dtype=np.int64)
    for i0 in range(0, L0, FIR_TILE):
        i_end = min(i0 + FIR_TILE, L0)
        acc = np.zeros(FIR_TILE, dtype=dtype)
        for p in range(min(ds, R)):
            Mp = (R - p + ds - 1) // ds
            mlim = min(Mp, i_end - (1 if defect == "causal_strict" else 0))
            for m0 in range(0, mlim, FIR_MC):
                m = m0 + np.arange(FIR_MC)
                live = m < (Mp - 1 if defect == "drop_last_tap" else Mp)
                tp = np.where(live, taps[np.minimum(p + m * ds, R - 1)], 0).astype(dtype)
                kmin = i0 - m0 - FIR_MC
                tt = (kmin + lane) * ds + (p if defect == "phase_sign" else -p)
                ok = (tt >= 0) & (tt < raw_len)
                if defect == "history":
                    ok = (off + tt >= 0) & (tt < raw_len)
                seg = np.where(ok, buf[np.clip(off + tt, 0, len(buf) - 1)], 0).astype(dtype)
                left = mlim - m0
                mb_end = FIR_MC if left >= FIR_MC else (left + 7) & ~7
                for mm in range(mb_end):
                    if defect == "drop_chunk_edge_block" and p == min(1, ds - 1) and m0 == 0 and FIR_MC - 8 <= mm:
                        continue
                    if tp[mm] != 0:
                        acc = acc + tp[mm] * seg[FIR_MC - mm:FIR_MC - mm + FIR_TILE]
        out[i0:i_end] = acc[:i_end - i0]
    return out


def fir_f32_ascending(s, r, ds):
    """The FIR in fp32 in the other order: per output, taps j = 0, 1, ... ascending, product and sum each rounded to fp32."""
    s, r = np.asarray(s, dtype=np.float32), np.asarray(r, dtype=np.float32)
    pos = np.arange(0, len(s), ds)
    acc = np.zeros(len(pos), dtype=np.float32)
    for j in range(len(r)):
        tt = pos - j
        acc = acc + r[j] * np.where(tt >= 0, s[np.maximum(tt, 0)], np.float32(0))
    return acc


# ---- the acceptance rule ------------------------------------------------------------------------------------------------------------
def accept(x, d):
    """(lo, hi, ambiguous): fp32(x - d), fp32(x + d) and where they differ."""
    lo, hi = (x - d).astype(np.float32), (x + d).astype(np.float32)
    return lo, hi, lo != hi


def violations(got, ref):
    """Boolean (n, L0 + 31): where the device output breaks the rule against ``ref`` (a dict of ``whiten_closed_form``): outside
    [lo, hi] -- which is "differs from fp32(x)" on every sample that is not ambiguous -- or a non-zero halo / tail."""
    got = np.asarray(got)
    return ~((got >= ref["lo"]) & (got <= ref["hi"]))


def rule_report(got, ref, what):
    bad = violations(got, ref)
    if not bad.any():
        return None
    w, col = (int(v) for v in np.argwhere(bad)[0])
    i = col - HALO_L
    return ("%s: %d of %d samples break the rule; first at window %d, sample %d (segment %d of %d, apply split %d): reference %.17g "
            "-> fp32 %r, d = %.3g (%s), got %r" % (
                what, int(bad.sum()), bad.size, w, i, *_seg_of(i, ref["Ln"][w]), _split_of(col, got.shape[1]), ref["x"][w, col],
                float(np.float32(ref["x"][w, col])), ref["d"][w, col], "ambiguous" if ref["amb"][w, col] else "not ambiguous",
                float(got[w, col])))


def _seg_of(i, Ln):
    per = max(1, -(-int(Ln) // N_SEG))
    return (i // per if 0 <= i < Ln else -1), N_SEG


def _split_of(col, row):
    return col // -(-row // N_SPLIT)


def whiten_closed_form(y, Ln, S, Q, wpt, whitening, rms=RMS):
    """The whitening of rows y (n, L0) float64 (valid to Ln[w], zero after) from their exact-or-rounded sums S (sum y) and Q (sum
    y^2): x (n, L0 + 31) float64 with the halo, d, the fp32 interval [lo, hi] and the ambiguous mask (module docstring).  Halo and
    tail: x = d = 0, so the device must write exact zeros there."""
    y = np.asarray(y, dtype=np.float64)
    n, L0 = y.shape
    Ln = np.asarray(Ln, dtype=np.int64).reshape(n)
    m, sc = np.zeros(n), np.ones(n)
    if whitening:
        for t0 in range(0, n, wpt):
            assert np.all(Ln[t0:t0 + wpt] == Ln[t0])
            tot = math.fsum(float(q) for q in Q[t0:t0 + wpt])
            sc[t0:t0 + wpt] = rms / math.sqrt(tot / (float(wpt) * float(Ln[t0])))
        m = np.asarray(S, dtype=np.float64) / Ln
    valid = np.arange(L0)[None, :] < Ln[:, None]
    xc = np.where(valid, (y - m[:, None]) * sc[:, None], 0.0)
    dc = np.where(valid, C_ROUNDINGS * 2.0 ** -53 * (sc[:, None] * (np.abs(y) + np.abs(m)[:, None]) + np.abs(xc)), 0.0)
    x, d = np.pad(xc, ((0, 0), (HALO_L, HALO_R))), np.pad(dc, ((0, 0), (HALO_L, HALO_R)))
    lo, hi, amb = accept(x, d)
    return {"x": x, "d": d, "lo": lo, "hi": hi, "amb": amb, "m": m, "scale": sc, "y": y, "Ln": Ln, "samples": int(Ln.sum())}


def ambiguous_share(ref):
    return float(ref["amb"].sum()) / max(ref["samples"], 1)


def fma(a, b, c):
    """round(a * b + c) with one rounding, from exact rationals (Python 3.10 has no math.fma; Fraction -> float rounds correctly)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


# ---- the mixture: stats, g, gain, whitening -------------------------------------------------------------------------------------------
def py_sum(v):
    return sum(int(e) for e in v)


def window_sums(a, v):
    """The exact sums (Sa, A, Sv, V, AV) of one window from integers a, v in units of 2^-19, as float64 -- after asserting with Python
    integers that numpy's int64 sums are the true ones and that every sum of absolute terms is below 2^53 units (then each float64
    partial sum in any order is exact, whatever the segment split, the thread stride and the reduction tree)."""
    a, v = np.asarray(a, dtype=np.int64), np.asarray(v, dtype=np.int64)
    sums = (int(a.sum()), int((a * a).sum()), int(v.sum()), int((v * v).sum()), int((a * v).sum()))
    truth = (py_sum(a), sum(int(e) ** 2 for e in a), py_sum(v), sum(int(e) ** 2 for e in v), sum(int(e) * int(f) for e, f in zip(a, v)))
    assert sums == truth
    room = max(sum(int(e) ** 2 for e in a), sum(int(e) ** 2 for e in v), sum(abs(int(e) * int(f)) for e, f in zip(a, v)))
    assert room < 1 << 53, room
    u = (A_UNIT, A_UNIT ** 2, A_UNIT, A_UNIT ** 2, A_UNIT ** 2)
    out = tuple(float(s) * w for s, w in zip(sums, u))
    assert all(Fraction(o) == Fraction(s) * Fraction(w) for o, s, w in zip(out, sums, u))
    return out, room


# name: (kind, ds, L0, end, n, wpt, K, R, src, noise src); R = 0: no RIR bank.  plant: K = 1, noise = 2^j speech, snr = 4^m, gain 2^e.
MIX_CASES = (
    ("plant", 4, 2049, "hi", 4, 2, 1, 0, "i16", "i16"),
    ("plant", 1, 9, "lo", 3, 1, 1, 0, "f32", "f32"),
    ("plant", 3, 7, "lo", 33, 33, 1, 0, "i16", "f32"),
    ("plant", 2, 8, "hi", 64, 32, 1, 0, "f32", "i16"),
    ("plant", 7, 1, "hi", 2, 1, 1, 0, "i16", "i16"),
    ("general", 4, 2049, "lo", 4, 2, 3, 40, "i16", "i16"),
    ("general", 1, 100, "lo", 3, 1, 1, 9, "f32", "i16"),
    ("general", 3, 9, "hi", 64, 32, 3, 9, "i16", "f32"),
    ("general", 2, 8, "lo", 66, 33, 1, 5, "f32", "f32"),
    ("general", 7, 7, "hi", 4, 2, 3, 15, "i16", "i16"),
    ("general", 4, 1, "hi", 2, 1, 1, 3, "f32", "i16"),
    ("general", 2, 1500, "hi", 33, 33, 1, 40, "i16", "f32"),
    ("general", 3, 4097, "lo", 2, 1, 3, 300, "f32", "f32"),
)


# added to a case's seed where the first draw put a sample on a rounding boundary of the reference (a y equal to its window's mean, an
# x within d of an fp32 midpoint): the cap is a property of the inputs, asserted on the host from the reference alone
SEED_SALT = {"plant-ds2-L8-hi-n64-wpt32-K1-R0-f32-i16": 1}


def mix_id(c):
    return "%s-ds%d-L%d-%s-n%d-wpt%d-K%d-R%d-%s-%s" % c


def whitenings(L0):
    """L0 = 1 with whitening is identically zero (module docstring): whitening off only."""
    return (0,) if L0 == 1 else (0, 1)


class MixCase:
    def __init__(self, kind, ds, L0, end, n, wpt, K, R, src, nsrc):
        self.kind, self.ds, self.L0, self.end, self.n, self.wpt, self.K, self.R, self.src, self.nsrc = kind, ds, L0, end, n, wpt, K, R, src, nsrc
        T = self.raw_len = raw_len_of(L0, ds, end)
        rng = np.random.default_rng(7919 * ds + 31 * L0 + 1009 * n + K + R + SEED_SALT.get(mix_id((kind, ds, L0, end, n, wpt, K, R, src, nsrc)), 0))
        self.total = 3 * T + 64
        self.k = grid_samples(rng, self.total)
        self.offsets = rng.integers(0, self.total - T + 1, n).astype(np.int64)
        self.offsets[0], self.offsets[-1] = 0, self.total - T
        if kind == "plant":
            # window w's noise crop is 2^j times its own speech; the rest of the noise buffer is grid noise
            self.j = rng.integers(0, 4, n)
            self.m = rng.integers(-1, 3, n)
            self.snr = (4.0 ** self.m).astype(np.float32)
            self.gain = (2.0 ** rng.integers(-2, 3, n)).astype(np.float32)
            self.nk = grid_samples(rng, n * T + 16)
            self.noff = (np.arange(n, dtype=np.int64) * T).reshape(n, 1)
            for w in range(n):
                self.nk[w * T:(w + 1) * T] = self.k[self.offsets[w]:self.offsets[w] + T] << int(self.j[w])
            self.rir_id, self.t = np.full(n, -1, dtype=np.int32), None
        else:
            self.snr = rng.uniform(0.3, 20.0, n).astype(np.float32)
            self.gain = rng.uniform(0.5, 2.0, n).astype(np.float32)
            if n > 2:
                self.snr[1], self.gain[1] = 0.0, 0.5          # a window without noise: g = 0 (a power-of-two gain, module docstring)
            self.nk = grid_samples(rng, self.total)
            self.noff = rng.integers(0, self.total - T + 1, (n, K)).astype(np.int64)
            self.noff[0, 0], self.noff[-1, -1] = self.total - T, 0
            self.t = grid_taps(rng, 2, R)
            self.rir_id = np.array([(0, -1, 1)[w % 3] for w in range(n)], dtype=np.int32)

    def units(self):
        """a, v (n, L0) int64 in units of 2^-19."""
        T, ds = self.raw_len, self.ds
        a, v = np.zeros((self.n, self.L0), dtype=np.int64), np.zeros((self.n, self.L0), dtype=np.int64)
        for w in range(self.n):
            s = self.k[self.offsets[w]:self.offsets[w] + T]
            a[w] = fir_exact(s, self.t[self.rir_id[w]], ds)[0] if self.rir_id[w] >= 0 else 16 * s[::ds]
            for kk in range(self.K):
                v[w] += 16 * self.nk[self.noff[w, kk]:self.noff[w, kk] + T:ds]
        return a, v

    @functools.lru_cache(maxsize=None)
    def sums(self):
        a, v = self.units()
        per = [window_sums(a[w], v[w]) for w in range(self.n)]
        return a, v, [p[0] for p in per], max(p[1] for p in per)

    def g_of(self, w, A, V):
        snr = float(self.snr[w])
        if self.K == 0 or not snr > 0.0:
            return 0.0
        Pa, Pv = A / float(self.L0), V / float(self.L0)
        return math.sqrt(Pa / (Pv * snr)) if Pa > 0.0 and Pv > 0.0 else 0.0

    @functools.lru_cache(maxsize=None)
    def reference(self, whitening, contracted=False):
        """The closed form of the module docstring.  ``contracted``: y = G fma(g, v, a) and S = G fma(g, Sv, Sa), the device's
        possible contractions, from exact rationals (the host test shows both forms inside the rule)."""
        a, v, sums, _ = self.sums()
        af, vf = a.astype(np.float64) * A_UNIT, v.astype(np.float64) * A_UNIT
        y, S, Q, g = np.zeros((self.n, self.L0)), np.zeros(self.n), np.zeros(self.n), np.zeros(self.n)
        for w in range(self.n):
            Sa, A, Sv, V, AV = sums[w]
            G = float(self.gain[w])
            g[w] = gg = self.g_of(w, A, V)
            if gg == 0.0:
                y[w], S[w], Q[w] = G * af[w], G * Sa, (G * G) * A
            elif contracted:
                y[w] = [G * fma(gg, b, e) for e, b in zip(af[w], vf[w])]
                S[w], Q[w] = G * fma(gg, Sv, Sa), (G * G) * (A + 2.0 * gg * AV + (gg * gg) * V)
            else:
                y[w], S[w], Q[w] = G * (af[w] + gg * vf[w]), G * (Sa + gg * Sv), (G * G) * (A + 2.0 * gg * AV + (gg * gg) * V)
        ref = whiten_closed_form(y, np.full(self.n, self.L0), S, Q, self.wpt, whitening)
        ref["g"] = g
        return ref


@functools.lru_cache(maxsize=None)
def mix_case(c):
    return MixCase(*c)


# ---- the plain entries ----------------------------------------------------------------------------------------------------------------
# (entry, ds, L0, end, n, wpt, src): "rows" = vm_decimate_whiten (row n at n * raw_len), "crop" = vm_crop_decimate_whiten
PLAIN_CASES = (
    ("rows", 1, 9, "lo", 3, 1, "i16"), ("rows", 4, 2049, "lo", 4, 2, "f32"), ("rows", 3, 8, "hi", 64, 32, "i16"),
    ("rows", 2, 7, "lo", 66, 33, "f32"), ("rows", 7, 1, "hi", 2, 1, "f32"), ("rows", 4, 4097, "hi", 2, 1, "i16"),
    ("crop", 1, 2048, "lo", 2, 2, "f32"), ("crop", 4, 2047, "hi", 4, 2, "i16"), ("crop", 7, 9, "lo", 64, 32, "f32"),
    ("crop", 3, 100, "lo", 66, 33, "i16"), ("crop", 2, 1, "lo", 3, 1, "i16"), ("crop", 4, 7, "hi", 5, 1, "f32"),
    ("crop", 2, 8, "lo", 33, 33, "i16"),
)
VARLEN_CASES = tuple((ds, 2000, src) for ds, src in zip(DS_VALUES, ("i16", "f32", "f32", "i16", "f32")))
POISON = {"i16": 32767, "f32": 1e30}


def plain_id(c):
    return "%s-ds%d-L%d-%s-n%d-wpt%d-%s" % c


def varlen_lens(ds, L0):
    """raw_lens that give Ln in {1, L0 - 1, L0} with every raw_lens % ds, at least 8 rows: (raw_lens, Ln)."""
    lens = [1] + [(L0 - 2) * ds + 1 + r for r in range(ds)] + [(L0 - 1) * ds + 1 + r for r in range(ds)]
    while len(lens) < 8:
        lens.append(lens[1 + len(lens) % (2 * ds)])
    lens = np.array(lens, dtype=np.int64)
    return lens, (lens + ds - 1) // ds


def varlen_id(c):
    ds, L0, src = c
    return "ds%d-L%d-Ln1+%d+%d-%s" % (ds, L0, L0 - 1, L0, src)


def plain_reference(k, offsets, raw_lens, ds, L0, wpt, whitening):
    """The plain path on integer samples k (units of 2^-15): window w = k[offsets[w] : offsets[w] + raw_lens[w]] decimated to
    Ln[w] <= L0 samples, whitened over its tower of wpt windows (varlen: wpt = 1, its own Ln), zero after Ln."""
    k = np.asarray(k, dtype=np.int64)
    n = len(offsets)
    Ln = (np.asarray(raw_lens, dtype=np.int64) + ds - 1) // ds
    y, S, Q = np.zeros((n, L0)), np.zeros(n), np.zeros(n)
    for w in range(n):
        s = k[offsets[w]:offsets[w] + raw_lens[w]:ds]
        assert len(s) == Ln[w]
        (S[w], Q[w], _, _, _), _ = window_sums(16 * s, np.zeros_like(s))
        y[w, :Ln[w]] = s * S_UNIT
    return whiten_closed_form(y, Ln, S, Q, wpt, whitening)


class PlainCase:
    def __init__(self, entry, ds, L0, end, n, wpt, src):
        self.entry, self.ds, self.L0, self.end, self.n, self.wpt, self.src = entry, ds, L0, end, n, wpt, src
        T = self.raw_len = raw_len_of(L0, ds, end)
        rng = np.random.default_rng(104729 * ds + 13 * L0 + 499 * n + wpt + (entry == "crop") + SEED_SALT.get(plain_id((entry, ds, L0, end, n, wpt, src)), 0))
        if entry == "rows":
            self.total = n * T
            self.offsets = np.arange(n, dtype=np.int64) * T
        else:
            self.total = 2 * T + 50
            self.offsets = rng.integers(0, self.total - T + 1, n).astype(np.int64)
            self.offsets[0], self.offsets[-1] = 0, self.total - T
        self.k = grid_samples(rng, self.total)

    @functools.lru_cache(maxsize=None)
    def reference(self, whitening):
        return plain_reference(self.k, self.offsets, np.full(self.n, self.raw_len), self.ds, self.L0, self.wpt, whitening)


@functools.lru_cache(maxsize=None)
def plain_case(c):
    return PlainCase(*c)


class VarlenCase:
    """Rows at a stride of L0 ds + 16 in one buffer.  ``poisoned``: the same buffer with large values at every position the kernel
    must not read -- off the decimated grid inside the row, and from raw_lens[n] to the next row."""

    def __init__(self, ds, L0, src):
        self.ds, self.L0, self.src = ds, L0, src
        self.raw_lens, self.Ln = varlen_lens(ds, L0)
        self.n = len(self.raw_lens)
        stride = L0 * ds + 16
        rng = np.random.default_rng(15485863 + 7 * ds + L0 + SEED_SALT.get(varlen_id((ds, L0, src)), 0))
        self.total = self.n * stride
        self.k = grid_samples(rng, self.total)
        self.offsets = np.arange(self.n, dtype=np.int64) * stride
        self.unread = np.ones(self.total, dtype=bool)
        for w in range(self.n):
            self.unread[self.offsets[w]:self.offsets[w] + self.raw_lens[w]:ds] = False

    def source(self, poisoned):
        buf = as_source(self.k, self.src)
        if poisoned:
            buf[self.unread] = POISON[self.src]
        return buf

    @functools.lru_cache(maxsize=None)
    def reference(self, whitening):
        return plain_reference(self.k, self.offsets, self.raw_lens, self.ds, self.L0, 1, whitening)


@functools.lru_cache(maxsize=None)
def varlen_case(c):
    return VarlenCase(*c)


DEFECTS_PLAIN = ("seg_end", "scale_L0", "halo_swapped", "past_end")


def model_plain(k, offsets, raw_lens, ds, L0, wpt, whitening, defect=None, rms=RMS):
    """The two whitening passes of preproc.hip in float64 on samples k / 32768: 8 statistics segments per window (per = ceil(Ln / 8)),
    the tower's scale from wpt * 8 partials with Ln in the mean and the scale, 8 apply splits of the (L0 + 31) row with the 15 / 16
    halo.  ``defect``: one of DEFECTS_PLAIN (past_end: the length taken as floor(raw_len / ds) + 1, which reads the sample AT raw_len
    when ds divides raw_len)."""
    k = np.asarray(k, dtype=np.int64)
    n, row = len(offsets), L0 + HALO
    Ln = (np.asarray(raw_lens, dtype=np.int64) + ds - 1) // ds
    if defect == "past_end":
        Ln = np.asarray(raw_lens, dtype=np.int64) // ds + 1
    smp = lambda w, i: float(k[offsets[w] + i * ds]) * S_UNIT       # noqa: E731
    psum, psq = np.zeros((n, N_SEG)), np.zeros((n, N_SEG))
    for w in range(n):
        per = -(-int(Ln[w]) // N_SEG)
        for seg in range(N_SEG):
            i1 = min((seg + 1) * per, int(Ln[w])) - (1 if defect == "seg_end" else 0)
            vals = [smp(w, i) for i in range(seg * per, i1)]
            psum[w, seg], psq[w, seg] = math.fsum(vals), math.fsum(e * e for e in vals)
    out = np.zeros((n, row))
    left = HALO_R if defect == "halo_swapped" else HALO_L
    for w in range(n):
        m, sc = 0.0, 1.0
        if whitening:
            tw = w // wpt
            tot = math.fsum(psq[tw * wpt:(tw + 1) * wpt].ravel())
            r = math.sqrt(tot / (float(wpt) * float(L0 if defect == "scale_L0" else Ln[w])))
            sc = rms / r if r else float("inf")
            m = math.fsum(psum[w]) / float(Ln[w])
        per = -(-row // N_SPLIT)
        for b in range(N_SPLIT):
            for i in range(b * per, min((b + 1) * per, row)):
                t = i - left
                if 0 <= t < min(int(Ln[w]), L0):
                    out[w, i] = (smp(w, t) - m) * sc
    return out.astype(np.float32)
