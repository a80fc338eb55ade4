"""Exactly representable inputs for the log-mel front end and the first Conv2D of the 2-D variant (csrc/spectro.hip;
tests/test_gpu_spectro_exact.py on the device, tests/test_spectro_exact_cpu.py on the host), after tests/gemm_exact.py and
tests/bn_exact.py: seeded operands on a power-of-two grid, small enough that every product and every partial sum of every output is an
fp32 number.  A result then does not depend on summation order, on which matrix instruction formed it or on the hi / lo split of an
operand: an fp32 output equals the float64 reference bit for bit, a 16-bit output its round-to-nearest-even, and a tap, band, clip,
sample or bin taken from the wrong place moves an element by at least one grid unit.  The one inexact step of the front end is logf:
its outputs are held to K_LOG fp32 ulps of float64 log.  The references restate include/voicemap_hip.h (section "a10 / f4"), not
the kernels.  Pure numpy / torch: nothing here touches the HIP library or a GPU."""
import functools

import numpy as np

from tests.bn_exact import ulp32
from tests.gemm_exact import BITS, LAYOUTS, LIMIT, STORE, _ints, exact_in, require_exact_sums, rounding_census, store, sums_exact  # noqa: F401

DT16 = ("bf16", "f16")
# what assert_exact names a mismatch by: clip, band, position and channel
LAYOUTS.update({"bmtc": ("clip", "band", "position", "channel"), "rowc": ("statistics row (window * rows + chunk)", "channel"),
                "ksc": ("kt", "km (slot of Cs)", "channel"), "bmrc": ("clip", "band", "row (1 + pooled position)", "channel"),
                "bprs": ("clip", "band pair", "row (1 + pooled position)", "stacked channel (dm * C + c)"), "wc": ("window", "channel")})
SENTINEL = -1536.0          # what a never-written entry holds (exact in every storage type; no case produces it)


# ======================================================================================================================================
# A. the first Conv2D(3 x 3), one input channel
#   z[(b, m)][t][c] = relu(bias[c] + sum_kt sum_km W[kt][km][c] * in[(b, m + km - 1)][t + kt - 1])     bands outside the clip and
#   positions outside the window are zero (header: `in` has L + 2 rows, zero halo rows; W is (3, Cs, C), entries km >= 3 padding)
# ======================================================================================================================================
# (n_clips, M, L, C) -> what the shape reaches
MFMA_SHAPES = [
    (2, 3, 37, 32),      # CB = 1; one partial 32-tile per row; band 0 / band M - 1 masks; n_rows = 6: the second workgroup is half empty
    (1, 2, 129, 64),     # CB = 2; a second statistics row that holds ONE position (whole == false, nbytes = one row)
    (2, 5, 298, 96),     # CB = 3; three statistics rows; odd M: the last band has no pool partner
    (1, 2, 256, 128),    # CB = 4; whole tiles only
    (3, 1, 5, 32),       # M = 1: all six neighbour taps masked
]
VALU_SHAPES = [
    (2, 3, 37, 24),      # CV = 3: 64 % CV != 0 (the LDS reduction), PPB = 85, thread 255 idle
    (2, 2, 140, 40),     # CV = 5: the LDS reduction, PPB = 51, one idle thread; two statistics rows
]
VALU_F32_SHAPES = [
    (1, 2, 130, 120),    # CV = 15: the LDS reduction; a second statistics row with two positions
    (1, 3, 5, 8),        # CV = 1: the shuffle reduction over all 64 lanes
]
# weight gradient only: n_clips * M > 2048 windows, so a workgroup walks wpb = 2 of them
WPB_MFMA_SHAPES = [
    (1025, 2, 3, 32),    # 2050 windows in 1025 workgroups: every workgroup holds one whole clip
    (683, 3, 3, 32),     # 2049 windows: workgroups straddle clips (win % M changes inside), the last one holds ONE window
]
WPB_VALU_SHAPES = [(683, 3, 3, 24), (1025, 2, 3, 8)]      # the same walk in the vector-ALU kernel (LDS / shuffle reduction)
# the partial 32-position K block of the matrix-pipe gradient: the guarded scalar gather at p0 + kt + 8 > L + 2 and du read as zero past L
WGRAD_TAIL_SHAPES = [
    (2, 3, 33, 32),      # block 1 holds position 32 alone: every lane group but one gathers through the guarded path
    (1, 2, 70, 64),      # block 2 holds positions 64 .. 69: a 16-byte gather whose last du positions (70, 71) lie past L
]
CONV_REGIMES = ("small", "wide", "lo-x", "lo-w")


def conv_klass(dt, regime):
    """The operand class a case is generated for: `small` and `wide` operands are exact in every storage type; the lo operands carry
    9 extra bits for bf16 and 12 for f16."""
    return ("bf16" if dt == "bf16" else "f16") if regime in ("lo-x", "lo-w") else "any"


def halves(v, dt):
    """hi = store(v), lo = store(v - hi): the two planes of vm_stft_logmel_f16s_split / the split of the filters inside
    vm_conv2d_first_fwd_split; asserts that they carry v whole."""
    v = np.asarray(v, dtype=np.float64)
    hi = store(v, dt)
    lo = store(v - hi, dt)
    assert np.array_equal(hi + lo, v), "hi + lo must be the operand"
    return hi, lo


def conv2d_first(img, w, bias, wrong=None):
    """img (n, M, L), w (3 kt, 3 km, C), bias (C) -> the pre-activation (n, M, L, C) in float64.  `wrong`: the three defects the
    planting must expose -- "clip": the band masks at the clip edges left out (band 0 sees the previous clip's last band); "tap": the
    tap kt = 2 applied at t - 1 instead of t + 1; "swap": km and kt exchanged."""
    n, M, L = img.shape
    p = np.zeros((n * M + 2, L + 2)) if wrong == "clip" else np.zeros((n, M + 2, L + 2))
    if wrong == "clip":
        p[1:-1, 1:-1] = img.reshape(n * M, L)
    else:
        p[:, 1:-1, 1:-1] = img
    out = np.zeros((n, M, L, w.shape[2]))
    for kt in range(3):
        for km in range(3):
            kk = 0 if (wrong == "tap" and kt == 2) else kt
            src = (p[km:km + n * M, kk:kk + L].reshape(n, M, L) if wrong == "clip" else p[:, km:km + M, kk:kk + L])
            out += src[..., None] * (w[km, kt] if wrong == "swap" else w[kt, km])
    return out + bias


def conv2d_first_wgrad(img, du, cs):
    """dW (3, Cs, C): dW[kt][km][c] = sum over clips, bands, positions of in[(b, m + km - 1)][t + kt - 1] * du[(b, m)][t][c]; the
    entries km >= 3 are zero."""
    n, M, L = img.shape
    p = np.zeros((n, M + 2, L + 2))
    p[:, 1:-1, 1:-1] = img
    out = np.zeros((3, cs, du.shape[-1]))
    for kt in range(3):
        for km in range(3):
            out[kt, km] = np.einsum("nml,nmlc->c", p[:, km:km + M, kt:kt + L], du)
    return out


def _lo_values(r, shape, k):
    """a + b * 2^-k, a in {-2, -1, 1, 2} or the element is 0, |b| <= 3: more significand bits than the storage type keeps (k = 9:
    bf16, 10 .. 11 bits; k = 12: f16, 13 .. 14 bits), so the low plane carries b."""
    a = r.choice([-2.0, -1.0, 1.0, 2.0], shape)
    b = r.integers(-3, 4, shape).astype(np.float64)
    return (a + b * 2.0 ** -k) * (r.random(shape) < 0.75)


def stat_rows(v):
    """(n, M, L, C) -> the BatchNorm partial sums (n * M * rows, C) of v and v^2, one row per 128 positions (vm_conv_stat_rows)."""
    n, M, L, C = v.shape
    rows = -(-L // 128)
    pad = np.zeros((n * M, rows * 128, C))
    pad[:, :L] = v.reshape(n * M, L, C)
    pad = pad.reshape(n * M * rows, 128, C)
    return pad.sum(1), (pad * pad).sum(1)


class Conv2dCase:
    """Operands and float64 references of one (shape, regime): x (n, M, L) image, w (3, 3, C) [kt][km], b (C), du (n, M, L, C);
    pre = conv + b UNROUNDED, z = relu(pre), gw(cs) the kernel gradient of the high plane.  Regimes (tests/gemm_exact.py REGIMES):
      small  integers: nothing rounds in any type, sums of squares included;
      wide   integers large enough that z passes 256 / 2048: 16-bit storage rounds, exact ties occur (one-plane entry points);
      lo-x   the image has more significand bits than the storage type (in_lo != 0), the filters few (w_lo == 0);
      lo-w   the mirror.  In both the reference is w_hi * in + w_hi * in_lo + w_lo * in = w * in: the fourth product is zero.
    Channel `c_neg` is negative everywhere before the ReLU."""

    def __init__(self, shape, regime, klass):
        n, M, L, C = shape
        self.shape, self.regime, self.klass = shape, regime, klass
        r = np.random.default_rng([n, M, L, C, sum(map(ord, regime)), len(klass)])
        k = 9 if klass == "bf16" else 12
        self.grid = 2.0 ** -k if regime in ("lo-x", "lo-w") else 1.0
        if regime == "small":
            x, w = _ints(r, (n, M, L), 3, 0.25), _ints(r, (3, 3, C), 2, 0.25)
        elif regime == "wide":
            x, w = _ints(r, (n, M, L), 127), _ints(r, (3, 3, C), 31)
        elif regime == "lo-x":
            x, w = _lo_values(r, (n, M, L), k), _ints(r, (3, 3, C), 1, 0.25)
        elif regime == "lo-w":
            x, w = _ints(r, (n, M, L), 1, 0.25), _lo_values(r, (3, 3, C), k)
        else:
            raise ValueError(regime)
        b = _ints(r, (C,), 3)
        self.c_neg = 5 % C
        b[self.c_neg] = -(np.abs(w[:, :, self.c_neg]).sum() * np.abs(x).max() + 1.0)
        self.x, self.w, self.b = x, w, b
        self.du = _ints(r, (n, M, L, C), 1, 0.25)
        self.dts = DT16 + ("f32",) if klass == "any" else (klass,)
        # the precondition, per output: sum |product| + |bias| in grid units, the hi and lo parts of an operand as separate products
        head = None
        for dt in self.dts:
            if dt == "f32":
                ax, aw = np.abs(x), np.abs(w)
            else:
                (xh, xl), (wh, wl) = halves(x, dt), halves(w, dt)
                ax, aw = np.abs(xh) + np.abs(xl), np.abs(wh) + np.abs(wl)
                if regime in ("small", "wide"):
                    assert not xl.any() and not wl.any()
                elif regime == "lo-x":
                    assert (xl != 0).mean() > 0.25 and not wl.any()
                else:
                    assert (wl != 0).mean() > 0.25 and not xl.any()
            head = conv2d_first(ax, aw, np.abs(b))
            self.head_fwd = require_exact_sums(head, self.grid, "conv2d_first forward")
        self.pre = conv2d_first(x, w, b)
        self.z = np.maximum(self.pre, 0.0)
        assert (self.pre[..., self.c_neg] < 0).all() and (self.z > 0).mean() > 0.2
        assert exact_in(b, "f32") and exact_in(w, "f32") and exact_in(self.du, "bf16")
        if regime in ("small", "wide"):
            self.head_wgrad = require_exact_sums(conv2d_first_wgrad(np.abs(x), np.abs(self.du), 3), 1.0, "conv2d_first wgrad")
        if regime == "small":
            assert self.z.max() <= 256 and all(exact_in(self.z, dt) for dt in DT16)
        if regime == "wide":
            for dt in DT16:
                frac, ties = rounding_census(self.z, dt)
                assert frac >= 0.005 and ties >= min(100, self.z.size // 40) and self.z.max() < 60000, (dt, frac, ties)

    def planes(self, dt):
        """The image as the two planes of `dt` (n, M, L) each."""
        return (self.x, np.zeros_like(self.x)) if dt == "f32" else halves(self.x, dt)

    def one_plane(self, dt):
        """relu(pre) of the ONE-plane entry point: the high plane of the image times the filters rounded to `dt` (header: "rounded to
        `dtype` inside").  The same tensor as z in `small` and `wide`."""
        if dt == "f32" or self.regime in ("small", "wide"):
            return self.z
        return np.maximum(conv2d_first(halves(self.x, dt)[0], halves(self.w, dt)[0], self.b), 0.0)

    def forward(self, dt, split):
        """(z as stored, the low plane store(z - z_stored), the statistics rows of what the entry point sums -- the stored z, in
        split mode the two-plane value -- and whether the sums / the sums of squares meet the precondition)."""
        z = self.z if split else self.one_plane(dt)
        zs = store(z, dt)
        zl = store(z - zs, dt)
        v = zs + zl if split else zs
        ss, sq = stat_rows(v)
        ok_sum, ok_sq = sums_exact(np.abs(ss), self.grid), sums_exact(sq, self.grid * self.grid)
        ok_sq = ok_sq and exact_in(v * v, "f32")                 # (each square is itself rounded by the kernel's fmaf otherwise)
        assert ok_sum and (ok_sq or self.regime != "small")
        return zs, zl, ss, sq, ok_sq

    def gw(self, cs, dt="f32"):
        return conv2d_first_wgrad(self.planes(dt)[0], self.du, cs)

    def wrong(self, which):
        return np.maximum(conv2d_first(self.x, self.w, self.b, wrong=which), 0.0)

    def weights(self, cs):
        """The fp32 kernel (3, Cs, C) of the flat store; its padding entries km >= 3 hold 5.0: the kernels must not read them."""
        out = np.full((3, cs, self.w.shape[2]), 5.0)
        out[:, :3] = self.w
        return out


@functools.lru_cache(maxsize=4)
def _conv2d_case(shape, regime, klass):
    return Conv2dCase(shape, regime, klass)


def conv2d_case(shape, regime, dt):
    return _conv2d_case(tuple(shape), regime, conv_klass(dt, regime))


def padded_rows(a, halo=0.0):
    """(windows, L, C) -> (windows, L + 2, C) with `halo` in rows 0 and L + 1."""
    out = np.full((a.shape[0], a.shape[1] + 2) + a.shape[2:], halo, dtype=np.float64)
    out[:, 1:-1] = a
    return out


class Boundary:
    """vm_conv2d_first_bn_pool_stack on a Conv2dCase (header): y = drop * (scale * relu(conv + bias) + shift) in fp32,
    q[(b, m)][1 + t'] = store(max(y[2 t'], y[2 t' + 1])), xs[(b, mo)][1 + t'][dm * C + c] = the larger STORED q of the band pair
    mo + dm - 1 where that pair lies inside the clip's M / 2 pairs.  Never written: the halo rows of both tensors, out-of-clip slots
    and the channels [3 C, Cs2) of xs (an odd last band still gets its q).  scale in +-{0.5, 1, 2} and integer shift per
    tower, drop in {0, 1.25} per (window, channel): every product stays on the grid.  Planted: a channel with scale < 0 under a live
    drop, a channel dropped in every window, tied position pairs and tied band pairs with positive values (counted)."""

    def __init__(self, case, dt, cpt, cs2):
        n, M, L, C = case.shape
        assert n % cpt == 0 and M >= 2 and L >= 2 and cs2 >= 3 * C and cs2 % 8 == 0
        towers, Mo, Lq = n // cpt, M // 2, L // 2
        r = np.random.default_rng([n, M, L, C, cpt, 11])
        self.scale = r.choice([0.5, 1.0, 2.0], (towers, C)) * r.choice([-1.0, 1.0], (towers, C))
        self.shift = _ints(r, (towers, C), 2)
        self.drop = r.choice([0.0, 1.25], (n * M, C), p=[0.2, 0.8])
        self.c_inv, self.c_drop = 3 % C, 7 % C
        self.scale[:, self.c_inv] = -2.0
        self.drop[:, self.c_inv] = 1.25
        self.drop[:, self.c_drop] = 0.0
        sc = np.repeat(self.scale, cpt, axis=0)[:, None, None, :]
        sh = np.repeat(self.shift, cpt, axis=0)[:, None, None, :]
        aff = sc * case.z + sh
        y = self.drop.reshape(n, M, 1, C) * aff
        assert exact_in(aff, "f32") and exact_in(y, "f32"), "the affine must be exact in fp32"
        assert towers == 1 or not np.array_equal(self.scale[0], self.scale[1])
        yp = y[:, :, :2 * Lq].reshape(n, M, Lq, 2, C)
        qv = store(yp.max(3), dt)                                            # (n, M, Lq, C)
        self.tied_positions = int(((yp[:, :, :, 0] == yp[:, :, :, 1]) & (yp[:, :, :, 0] > 0)).sum())
        pooled = np.maximum(qv[:, 0:2 * Mo:2], qv[:, 1:2 * Mo:2])            # (n, Mo, Lq, C)
        self.tied_bands = int(((qv[:, 0:2 * Mo:2] == qv[:, 1:2 * Mo:2]) & (pooled > 0)).sum())
        self.rounded = float((qv != yp.max(3)).mean())
        self.q = np.full((n * M, Lq + 2, C), SENTINEL)
        self.q[:, 1:-1] = qv.reshape(n * M, Lq, C)
        self.xs = np.full((n, Mo, Lq + 2, cs2), SENTINEL)
        for dm in range(3):
            for mo in range(Mo):
                if 0 <= mo + dm - 1 < Mo:
                    self.xs[:, mo, 1:-1, dm * C:(dm + 1) * C] = pooled[:, mo + dm - 1]
        self.xs = self.xs.reshape(n * Mo, Lq + 2, cs2)
        assert SENTINEL not in qv and exact_in(SENTINEL, "bf16")
        assert (y[..., self.c_inv] < 0).any() and not y[..., self.c_drop].any()


# vm_fold_pool_windows_bwd: (n_clips, M, L, C, Cs) -> reaches
FOLD_SHAPES = [
    (2, 5, 7, 8, 24),        # odd M: the last band's dq, s0 and sa are zero and owed
    (2, 4, 149, 32, 96),     # four row lanes per channel vector walk 149 rows
    (1, 2, 5, 96, 288),      # 256 / 12 = 21 row lanes, four idle threads
    (2, 3, 4, 4, 16),        # C % 8 != 0: the one-element path of the 16-bit types
    (1, 2, 300, 8, 24),      # 256 row lanes (16-bit), 300 rows: the second trip of the row walk
]


class FoldPoolCase:
    """dxs (n * Mo, L, Cs) integers, q (n * M, L + 2, C) integers in 0 .. 3 (ties between the bands are the rule), zero halo:
    din[(b, mo)][t][c] = sum_dm dxs[(b, mo - dm + 1)][t][dm * C + c] goes to the band of the pair that holds the first maximum,
    zero to the other and to an odd last band; s0 / sa (n * M, C) = the sums of dq and of dq * q over a window."""

    def __init__(self, shape):
        n, M, L, C, Cs = shape
        Mo = M // 2
        r = np.random.default_rng([n, M, L, C, Cs, 5])
        self.dxs = _ints(r, (n, Mo, L, Cs), 2)
        self.q = r.integers(0, 4, (n, M, L, C)).astype(np.float64)
        din = np.zeros((n, Mo, L, C))
        for dm in range(3):
            for mo in range(Mo):
                if 0 <= mo - dm + 1 < Mo:
                    din[:, mo] += self.dxs[:, mo - dm + 1, :, dm * C:(dm + 1) * C]
        first = self.q[:, 0:2 * Mo:2] >= self.q[:, 1:2 * Mo:2]
        self.ties = int((self.q[:, 0:2 * Mo:2] == self.q[:, 1:2 * Mo:2]).sum())
        self.dq = np.zeros((n, M, L, C))
        self.dq[:, 0:2 * Mo:2] = np.where(first, din, 0.0)
        self.dq[:, 1:2 * Mo:2] = np.where(first, 0.0, din)
        self.s0 = self.dq.sum(2).reshape(n * M, C)
        self.sa = (self.dq * self.q).sum(2).reshape(n * M, C)
        require_exact_sums(np.abs(self.dq * self.q).sum(2), 1.0, "fold_pool sums")
        assert exact_in(din, "bf16") and self.ties > 0


# ======================================================================================================================================
# B. STFT -> power -> mel -> log
#   out[(b * n_mels + m)][1 + t] = log(sum_k melw[k][m] * (re_t[k]^2 + im_t[k]^2) + log_floor),
#   re_t[k] | im_t[k] = sum_n basis[n][k | 256 + k] * raw[b][t * hop + n],  T = 1 + (raw_len - win) / hop
# ======================================================================================================================================
# logf is the one inexact step.  AMD's table of device math accuracy is not among the files ROCm installs (no document under its
# tree states a bound for logf), so the bound is the OpenCL specification's for log: 3 ulp.  The library is built without fast-math.
K_LOG = 3
LOG_FLOOR = 2.0 ** -20
# (win, hop, T) -> reaches
STFT_GEOMETRIES = [
    (400, 160, 33),      # the shipped geometry; a second frame tile that holds one frame
    (401, 1, 65),        # odd window: the one-term last k-step of the fp32 kernel; Kp = 416; heavily overlapping frames
    (37, 5, 71),         # a window shorter than one 64-sample load; Kp = 48
    (16, 40, 32),        # hop > win; exactly one full tile; ONE f16 K step: the prefetch clamp n1 = n0 fires on the first step
    (2, 3, 1),           # the smallest window the header allows; one frame
    (496, 160, 3),       # the largest f16 window whose frame matrices fit in 64 KiB of LDS
]
STFT_LDS_GEOMETRY = (512, 160, 3)        # 65 664 (fp32 kernel) / 66 560 (f16 kernels) bytes of dynamic LDS
N_MELS = (32, 64, 96, 128)
STFT_REGIMES = ("exact", "lo-x", "lo-b")
STFT_LO_GEOMETRIES = [(400, 160, 33), (401, 1, 65)]        # (the second: Kp = 416 zero padding under non-zero low halves)


def stft_cases():
    """(win, hop, T, n_mels, is_int16, regime): every geometry with both sample types, n_mels cycling so that each of the four NMB
    instantiations of both kernels runs with both sample types; the lo regimes on two geometries."""
    out, gi = [], 0
    for g in STFT_GEOMETRIES:
        out += [g + (N_MELS[(gi + i16) % 4], bool(i16), "exact") for i16 in (0, 1)]
        gi += 1
    for g in STFT_LO_GEOMETRIES:
        for reg in ("lo-x", "lo-b"):
            out += [g + (N_MELS[(gi + i16) % 4], bool(i16), reg) for i16 in (0, 1)]
            gi += 1
    return out


def lds_bytes(win, n_mels):
    """Dynamic LDS of (the fp32 kernel, the f16 kernels): the frame matrices, or the mel partial sums where those are larger."""
    red = 4 * n_mels * 32 * 4
    return max(32 * (win + 1) * 4, red), max(2 * 32 * ((win + 15) // 16 * 16 + 8) * 2, red)


def mel_matrix(n_mels, seed=0):
    """(256, n_mels) in eighths, banded: bin k feeds mel k * n_mels / 256 and the next one (the last mel: itself twice), weights
    1/8 .. 7/8 each -- bins 0 and 255 have non-zero weight, which the shipped triangular filters do not give them."""
    r = np.random.default_rng([n_mels, seed])
    m = np.zeros((256, n_mels))
    for k in range(256):
        m0 = k * n_mels // 256
        m[k, m0] += r.integers(1, 8) / 8.0
        m[k, min(m0 + 1, n_mels - 1)] += r.integers(1, 8) / 8.0
    assert m[0].any() and m[255].any() and ((m != 0).sum(1) <= 2).all() and (m.sum(0) > 0).all()
    return m


def f16_halves(v):
    v = np.asarray(v, dtype=np.float64)
    hi = store(v, "f16")
    lo = store(v - hi, "f16")
    return hi, lo


def frames_of(raw, win, hop, T, late=0):
    """(n, raw_len) -> (n, T, win): frame t = raw[t * hop + late : t * hop + late + win] (zero past the end)."""
    raw = np.concatenate([raw, np.zeros((raw.shape[0], late))], axis=1)
    idx = (np.arange(T) * hop + late)[:, None] + np.arange(win)[None, :]
    return raw[:, idx]


def logmel(frames, basis, melw, floor):
    """float64: (S, log(S + floor)) of frames (n, T, win); (n, T, n_mels)."""
    X = frames @ basis
    P = X[..., :256] ** 2 + X[..., 256:] ** 2
    S = P @ melw
    return S, np.log(S + floor)


class StftCase:
    """Inputs and float64 reference of one (win, hop, T, n_mels, sample type, regime), two clips.
      exact   integer basis entries and int16 samples in -3 .. 3 (fp32 samples: n / 32768): re, im, the power and the mel sum are all
              fp32 numbers in any order and on either matrix pipe (asserted: < 2^24 units of 2^-15, 2^-30, 2^-33), the x 256 and
              2^-16 of the f16 kernel are exact and both low halves are zero;
      lo-x    sparse samples +-4 (4096 + b) / 32768 (13 bits: x 256 they split into f16 halves, bh * xl != 0; log S stays clear of
              zero, where a 16-bit spacing is no wider than the bound), a +-1 basis;
      lo-b    a sparse basis +-(1 + 2^-12) (its low half bl = +-2^-12, bl * xh != 0: leaving that product out divides every S by
              (1 + 2^-12)^2 exactly, far outside the bound), samples +-(16 .. 31) / 32768.
    In the lo regimes re and im stay exact; P and S round: `rounds` counts the roundings of S (all terms >= 0, proto_refs' way)."""

    def __init__(self, win, hop, T, n_mels, i16, regime, n=2):
        self.geom, self.n, self.n_mels, self.i16, self.regime = (win, hop, T), n, n_mels, i16, regime
        r = np.random.default_rng([win, hop, T, n_mels, int(i16), sum(map(ord, regime))])
        raw_len = win + hop * (T - 1) + min(hop - 1, 2)         # a tail that does not make another frame
        self.raw_len = raw_len
        assert 1 + (raw_len - win) // hop == T
        if regime == "exact":
            basis = r.integers(-3, 4, (win, 512)).astype(np.float64)
            ni = r.integers(-3, 4, (n, raw_len))
        elif regime == "lo-x":
            basis = r.choice([-1.0, 1.0], (win, 512))
            ni = r.choice([-1, 1], (n, raw_len)) * 4 * (4096 + r.integers(-15, 16, (n, raw_len))) * (r.random((n, raw_len)) < 0.125)
        elif regime == "lo-b":
            basis = r.choice([-1.0, 1.0], (win, 512)) * (1.0 + 2.0 ** -12) * (r.random((win, 512)) < 0.125)
            ni = r.choice([-1, 1], (n, raw_len)) * r.integers(16, 32, (n, raw_len))
        else:
            raise ValueError(regime)
        self.basis, self.samples_i16 = basis, ni.astype(np.int16)
        self.raw = ni.astype(np.float64) / 32768.0
        self.melw = mel_matrix(n_mels)
        self.floor = LOG_FLOOR
        assert exact_in(self.raw, "f32") and exact_in(basis, "f32") and np.array_equal(self.samples_i16, ni)
        fr = frames_of(self.raw, win, hop, T)
        self.S, self.ref = logmel(fr, basis, self.melw, self.floor)
        # what the f16 kernel multiplies: (256 x) as two halves each
        xh, xl = f16_halves(self.raw * 256.0)
        bh, bl = f16_halves(basis)
        assert np.array_equal(xh + xl, self.raw * 256.0) and np.array_equal(bh + bl, basis)
        self.bh = bh
        ub = 2.0 ** -12 if regime == "lo-b" else 1.0                        # the grid of the basis
        u_re = 2.0 ** -15 * ub
        afr = frames_of(np.abs(xh) + np.abs(xl), win, hop, T) / 256.0
        self.head_re = require_exact_sums(afr @ (np.abs(bh) + np.abs(bl)), u_re, "re / im")
        if regime == "exact":
            assert not xl.any() and not bl.any()
            X = fr @ basis
            P = X[..., :256] ** 2 + X[..., 256:] ** 2
            self.head_p = require_exact_sums(P, u_re ** 2, "power")
            self.head_s = require_exact_sums(self.S + self.floor, u_re ** 2 / 8.0, "mel sum + floor")
            self.rounds = 0
        else:
            assert ((xl != 0).mean() > 0.05) if regime == "lo-x" else ((bl != 0).mean() > 0.1 and (self.S > self.floor).all())
            assert not (bl.any() if regime == "lo-x" else xl.any())          # the fourth product is zero
            # S: re^2 and im^2 round, their sum rounds (or one of the three is fused away): <= 3 per bin; a mel sums <= nb bins, each a
            # multiply-add (<= 2 roundings if not fused), then three adds of the waves' partial sums and the floor
            nb = int((self.melw != 0).sum(0).max())
            self.rounds = 3 + 2 * nb + 3 + 1
        assert (self.S >= 0).all()

    def tol32(self, ref=None):
        """The bound of an fp32 output around float64 log(S + floor): K_LOG ulps of logf, plus -- lo regimes -- `rounds` roundings of
        non-negative terms: a relative error of S of at most (1 + 2^-24)^rounds - 1, which the logarithm turns into an absolute one."""
        ref = self.ref if ref is None else ref
        rel = (1 + 2.0 ** -24) ** self.rounds - 1                  # |log(1 + d)| <= |d| / (1 - |d|)
        return K_LOG * ulp32(ref) + rel / (1 - rel)

    def stored(self, dt):
        """(expected, alt, flagged): a 16-bit output must equal `expected` = store(ref) except where the reference lies within the
        bound of a rounding boundary (`flagged`, from the reference alone); there it may be `alt`, the neighbour across the boundary."""
        tol = self.tol32()
        lo, hi, mid = store(self.ref - tol, dt), store(self.ref + tol, dt), store(self.ref, dt)
        flagged = lo != hi
        alt = np.where(lo != mid, lo, hi)
        return mid, alt, flagged

    def wrong(self, which):
        """float64 log-mel of a deliberately wrong evaluation; see tests/test_spectro_exact_cpu.py."""
        win, hop, T = self.geom
        fr, basis, melw = frames_of(self.raw, win, hop, T), self.basis, self.melw
        if which == "odd-tail":                  # the last k-step of an odd window dropped
            assert win % 2 == 1
            fr = fr.copy()
            fr[..., win - 1] = 0.0
        elif which == "no-bl-xh":                # the product bl * xh dropped: x meets the high half of the basis alone
            basis = self.bh
        elif which == "late":                    # frames read one sample late
            fr = frames_of(self.raw, win, hop, T, late=1)
        elif which == "bins":                    # two bins exchanged in front of the mel matrix
            basis = basis.copy()
            for off in (0, 256):
                basis[:, [off + 5, off + 200]] = basis[:, [off + 200, off + 5]]
        elif which == "wave":                    # one wave's 64-bin partial sum missing
            melw = melw.copy()
            melw[64:128] = 0.0
        else:
            raise ValueError(which)
        return logmel(fr, basis, melw, self.floor)


@functools.lru_cache(maxsize=4)
def stft_case(win, hop, T, n_mels, i16, regime):
    return StftCase(win, hop, T, n_mels, i16, regime)


def ulp_of(v, dt):
    """The spacing of the storage type at |v| (normal range)."""
    _, e = np.frexp(np.abs(np.asarray(v, dtype=np.float64)))
    return np.ldexp(1.0, e - BITS[dt])


def check_log_f32(got, case, what=""):
    """|got - ref| <= the bound at every element; returns the worst error in fp32 ulps of the reference."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - case.ref)
    bad = ~(err <= case.tol32())
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements outside the bound; first at (clip %d, frame %d, mel %d): got %r, want %r (%.2f ulp)" % (
            what, int(bad.sum()), bad.size, i[0], i[1], i[2], got[i], case.ref[i], err[i] / ulp32(case.ref[i])))
    return float((err / ulp32(case.ref)).max())


def check_log_stored(got, case, dt, what=""):
    """A 16-bit output: store(ref) everywhere but at flagged elements, where the neighbour across the boundary is allowed too."""
    got = np.asarray(got, dtype=np.float64)
    want, alt, flagged = case.stored(dt)
    bad = (got != want) & ~(flagged & (got == alt))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ (%d flagged); first at (clip %d, frame %d, mel %d): got %r, want %r" % (
            what, int(bad.sum()), bad.size, int(flagged.sum()), i[0], i[1], i[2], got[i], want[i]))
    return float(flagged.mean())


def image_layout(a):
    """(n, T, n_mels) -> (n * n_mels, T): the rows 1 .. T of the block-1 input the entry points write."""
    n, T, m = a.shape
    return a.transpose(0, 2, 1).reshape(n * m, T)
