"""Exactly representable inputs for the BatchNorm / dropout / max-pool passes of csrc/bnpool.hip (tests/test_gpu_bn_exact.py on the
device, tests/test_bn_exact_cpu.py on the host).  Every kernel of the family does fp32 fma arithmetic on per-channel constants that are
inputs of the call (scale, shift, mean, invstd, c1, c2, drop); here they all sit on a power-of-two grid, z holds small integers and dp
small integers, so every product and every partial sum is an fp32 number.  The outputs then do not depend on the segment count of a
window, the pool groups a thread keeps in flight, the reduction order or FMA contraction: an fp32 output must equal the float64
reference bit for bit, a 16-bit output its round-to-nearest-even.  The references are written from the statements of
include/voicemap_hip.h ("BN apply + SpatialDropout1D + MaxPool1D" down to the pair forms), not from the kernels.  Pure numpy / torch:
nothing here touches the HIP library or a GPU."""
import functools

import numpy as np
import torch

from tests import gemm_exact as G
from tests.gemm_exact import STORE, exact_in, require_exact_sums, rounding_census, store

G.LAYOUTS.update({"nqc": ("window", "pooled row", "channel"), "nrc": ("window", "partial row", "channel")})

PART_ROWS = 8               # vm_bn_part_rows() (the device file asserts it)
VEC = {"f32": 4, "bf16": 8, "f16": 8}
EMPTY = 0x7fffffff          # the position of an empty (value, position) partial


# ---- the launch arithmetic of bnpool.hip, for the shape tables' comments and the host checks -----------------------------------------
def bn_segs(lq, c, dt):
    """Workgroups per window: 8 when pooled rows x channel vectors >= 2048, else 1."""
    return 8 if lq * (c // VEC[dt]) >= 2048 else 1


def lanes_for(cv):
    p = 1
    while p < cv and p < 256:
        p <<= 1
    return p


def launch(l, c, pool, dt):
    """(CV, P, RP, nseg, stride, remainder): channel vectors, channel lanes (next power of two >= CV, at most 256), row lanes 256 / P,
    segments, the pooled-row stride RP * nseg of a thread, L % pool."""
    cv = c // VEC[dt]
    p = lanes_for(cv)
    nseg = bn_segs(l // pool, c, dt)
    return cv, p, 256 // p, nseg, 256 // p * nseg, l % pool


# ---- the shape tables: (n, windows per tower, L, C, pool, dropout) ------------------------------------------------------------------------
# Lq = L // pool, CV = C / 4 (fp32) or C / 8 (16-bit), P = lanes_for(CV), RP = 256 / P, a thread walks pooled rows at stride RP * nseg
BN_SHAPES = [
    # Lq 300: Lq * CV = 4800 (fp32) / 2400 (16-bit) >= 2048 -> 8 segments in every type; P 16 / 8, stride 128 / 256: the two-in-flight
    # loop runs (q + stride < 300) and leaves a tail (300 % 256, 300 % 128 != 0); L % 2 = 1: one remainder row
    (4, 2, 601, 64, 2, True),
    # Lq 256: 16-bit Lq * CV = 256 * 8 = 2048, exactly the threshold -> 8 segments (fp32 4096: 8); L % 4 = 2
    (3, 3, 1026, 64, 4, False),
    # Lq 255: 16-bit 2040 < 2048 -> 1 segment, fp32 4080 -> 8; L % 4 = 2
    (3, 3, 1022, 64, 4, False),
    # CV 34 (fp32) / 17 (16-bit): P 64 / 32, so 30 / 15 idle channel lanes; Lq 16, 1 segment; L % 4 = 3
    (2, 1, 67, 136, 4, False),
    # fp32 CV 258 > 256: the second trip of the cvb channel loop (2 live lanes of 256) with its reuse of the LDS row; 16-bit CV 129 -> P
    # 256, RP 1 (no row lanes to reduce over); Lq 2; L % 4 = 2
    (2, 2, 10, 1032, 4, True),
    # three towers (windows 0-1, 2-3, 4-5 take their own constants); Lq 25, 1 segment
    (6, 2, 50, 16, 2, True),
    # L == pool: one pool group, no remainder, every row lane but the first idle
    (2, 2, 2, 8, 2, False), (2, 2, 4, 8, 4, False),
    # pool 1 (no routing choice); CV 128 / 64, Lq * CV = 8192 / 4096 -> 8 segments, stride 16 / 32: two trips of the two-in-flight loop
    (2, 2, 64, 512, 1, False),
    # the parity tests' small shapes: one tower of four windows with L % 2 = 1; CV 6 / 3 (P 8 / 4) with L % 4 = 1
    (4, 4, 31, 8, 2, True), (2, 2, 9, 24, 4, False),
]
# pair forms (16-bit, pool 2, L even): 8 segments with a tail / 8 segments, CV 16, Lq 600 (stride 128: four full trips and a tail) /
# three pairs / three towers
PAIR_SHAPES = [(4, 2, 600, 64, 2, True), (2, 1, 1200, 128, 2, False), (2, 2, 6, 8, 2, False), (6, 2, 50, 16, 2, True)]
# sparse finalize (bn_bwd_gmax_finalize_kernel: 32 lanes x U = 4 windows, TW = 2 towers per trip): one window; 33 windows per tower (lanes
# past the tower's windows in the second u); 129 and 130 windows per tower (the second trip of w0 += 128, with 1 / 2 live lanes); three
# towers (the clamped lane of TW = 2 in the second tower trip); one tower (the same clamp in the first); the training launch shape
SPARSE_SHAPES = [(1, 1, 8, 16, 2, False), (66, 33, 8, 16, 2, True), (258, 129, 8, 16, 2, False), (390, 130, 8, 16, 2, True),
                 BN_SHAPES[0]]
# vm_bn_finalize / vm_bn_bwd_finalize: (partial rows per tower, towers, C).  32 chunks of ceil(rows / 32) rows: 1 and 5 rows leave most
# chunks empty, 33 gives chunks of 2 with the last 15 empty, 520 = 32 * 16 + 8 the four-rows-in-flight loop; C 8 / 136 / 192: the 32-
# and 64-channel workgroups with a partial last block (136 = 2 * 64 + 8)
FINALIZE_SHAPES = [(1, 1, 8), (5, 2, 136), (33, 3, 192), (520, 2, 8), (520, 3, 136), (33, 1, 192), (1, 3, 136), (5, 1, 192)]
DTS = ("f32", "bf16", "f16")
DT16 = ("bf16", "f16")


# ---- float64 references, from the header's statements ------------------------------------------------------------------------------------
def per_window(a_tc, wpt):
    """(towers, C) -> (n, 1, C)."""
    return np.repeat(np.asarray(a_tc, dtype=np.float64), wpt, axis=0)[:, None, :]


def groups(z, pool):
    n, l, c = z.shape
    return z[:, :l // pool * pool].reshape(n, l // pool, pool, c)


def forward(z, scale, shift, drop, wpt, pool):
    """out[n][q][c] = max_j (z * scale + shift) * drop over the pool group q (n, L // pool, C); drop (n, C) or None."""
    d = 1.0 if drop is None else drop[:, None, :]
    return groups((z * per_window(scale, wpt) + per_window(shift, wpt)) * d, pool).max(2) + 0.0


def global_max(out, dt, lens=None):
    """GlobalMaxPool1D of the storage-rounded `out` (n, Lq, C): the values and the FIRST maximum's row (-0 == +0); lens: rows per window
    that count."""
    o = store(out, dt)
    if lens is not None:
        o = np.where(np.arange(o.shape[1])[None, :, None] < np.asarray(lens)[:, None, None], o, -np.inf)
    return o.max(1), o.argmax(1).astype(np.int32)


def reduce_partials(part_v, part_i):
    """The documented rule over the vm_bn_part_rows() (value, position) rows of a window: the best value, of equal values the smallest
    position; a row with position 0x7fffffff is empty.  (n, rows, C) each -> (n, C) each."""
    v = np.where(part_i == EMPTY, -np.inf, np.asarray(part_v, dtype=np.float64))
    best = v.max(1)
    idx = np.where(v == best[:, None, :], part_i, EMPTY).min(1)
    return best, idx.astype(np.int32)


def route(z, ka, pool):
    """The library's documented rule: the extreme of a pool group is the maximum of z where scale * drop >= 0, else the minimum, the
    first of equal values.  z (n, L, C), ka = scale * drop (n, 1, C) -> ext (n, Lq, C), arg (n, Lq, C) in [0, pool)."""
    g = groups(z, pool)
    arg = np.where((ka < 0)[:, :, None, :], -g, g).argmax(2)
    return np.take_along_axis(g, arg[:, :, None, :], 2)[:, :, 0, :], arg


def route_y(z, scale, shift, drop, wpt, pool):
    """The oracle's rule (MaxPool1D's gradient: the first maximum of y)."""
    d = 1.0 if drop is None else drop[:, None, :]
    return groups((z * per_window(scale, wpt) + per_window(shift, wpt)) * d, pool).argmax(2)


def scatter_dy(dyq, arg, l, pool):
    """dy (n, L, C): dyq (n, Lq, C) at element arg of every pool group, 0 elsewhere and on the remainder rows."""
    n, lq, c = dyq.shape
    dy = np.zeros((n, l, c))
    hot = np.arange(pool)[None, None, :, None] == arg[:, :, None, :]
    dy[:, :lq * pool] = (hot * dyq[:, :, None, :]).reshape(n, lq * pool, c)
    return dy


def backward(z, dp, scale, mean, invstd, drop, c1, c2, wpt, pool):
    """dy, zhat, du (n, L, C) UNROUNDED and the per-window sums sum dy, sum dy * zhat (n, C) of one block's backward:
    dy = drop * dp at the first extreme of every pool group, du = [z > 0] * scale * (dy - c1 - zhat * c2) on every row."""
    d = np.ones((z.shape[0], z.shape[2])) if drop is None else drop
    s = per_window(scale, wpt)
    _, arg = route(z, s * d[:, None, :], pool)
    dy = scatter_dy(d[:, None, :] * dp, arg, z.shape[1], pool)
    zhat = (z - per_window(mean, wpt)) * per_window(invstd, wpt)
    du = (z > 0) * s * (dy - per_window(c1, wpt) - zhat * per_window(c2, wpt)) + 0.0
    return dy, zhat, du, dy.sum(1), (dy * zhat).sum(1)


def finalize(sdy, sdyz, wpt, count):
    """vm_bn_bwd_finalize of per-window sums (n, C): c1 = (float)(sum / count), c2 likewise per tower; grad_gamma = sum dy * zhat and
    grad_beta = sum dy over all towers.  The quotient is taken in float64 and cast once."""
    n, c = sdy.shape
    a, b = sdy.reshape(n // wpt, wpt, c).sum(1), sdyz.reshape(n // wpt, wpt, c).sum(1)
    f = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)
    return f(a / count), f(b / count), b.sum(0), a.sum(0)


def dense_dp(dg, gidx, lq, dt):
    """GlobalMaxPool1D's backward: dp[n][q][c] = dg[n][c] (as the storage type holds it) if q == gidx[n][c] else 0."""
    return (np.arange(lq)[None, :, None] == gidx[:, None, :]) * store(dg, dt)[:, None, :]


# ---- the pair form of vm_conv_fwd_fold ---------------------------------------------------------------------------------------------------
def pair_encode(z, gamma, dt, center=None, wpt=1):
    """z (n, L even, C) >= 0 -> e PADDED (n, L/2 + 2, C) and o (n, L/2, C) as CPU tensors of the storage type: e the pair's extreme
    (gemm_exact.pair_extreme: the maximum where gamma >= 0), minus center[tower] where given; o the other element with its sign bit
    set where the extreme is the pair's second element."""
    ext, oth, second = G.pair_extreme(z, gamma)
    if center is not None:
        ext = ext - per_window(center, wpt)
    assert exact_in(ext, dt) and exact_in(oth, dt) and (oth >= 0).all()
    n, lq, c = ext.shape
    e = torch.zeros(n, lq + 2, c, dtype=STORE[dt])
    e[:, 1:-1] = torch.as_tensor(ext).to(STORE[dt])
    ob = torch.as_tensor(oth).to(STORE[dt]).contiguous().view(torch.int16) | (torch.as_tensor(second).to(torch.int16) << 15)
    return e, ob.view(STORE[dt]).contiguous()


def pair_decode(e, o, center=None, wpt=1):
    """The inverse, as the header states it: (n, L, C) float64."""
    ob = o.contiguous().view(torch.int16)
    second = (ob < 0).numpy()
    oth = (ob & 0x7fff).view(o.dtype).to(torch.float64).numpy()
    ext = e[:, 1:-1].to(torch.float64).numpy()
    if center is not None:
        ext = ext + per_window(center, wpt)
    n, lq, c = ext.shape
    return np.stack([np.where(second, oth, ext), np.where(second, ext, oth)], 2).reshape(n, 2 * lq, c)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _ints(r, shape, lo, hi):
    return r.integers(lo, hi + 1, shape).astype(np.float64)


class BnCase:
    """Inputs and float64 references of one shape (n, wpt, L, C, pool, dropout), seeded from it.  z (n, L, C): integers 0..7, about
    40 % zeros; gamma (C) in +-{0.5, 1, 2} with channel 5 exactly 0, channel 1 negative; invstd (towers, C) in {0.5, 1, 2}; scale =
    gamma * invstd; mean, shift: multiples of 1/4 in [-2, 2]; drop (n, C) in {0, 2} or None; dp (n, Lq, C): integers -4..4; c1, c2:
    multiples of 1/8 in [-1/4, 1/4]; dg (n, C) integers -4..4 with gidx of the reference forward (gidx) and a random valid one (gidx_r)."""

    def __init__(self, shape):
        n, wpt, l, c, pool, use_drop = shape
        assert n % wpt == 0 and c % 8 == 0 and l >= pool
        self.shape, self.towers, self.lq, self.count = shape, n // wpt, l // pool, float(wpt * l)
        towers, lq = self.towers, self.lq
        r = np.random.default_rng([n, wpt, l, c, pool, int(use_drop)])
        self.z = _ints(r, (n, l, c), 1, 7) * (r.random((n, l, c)) >= 0.4)
        g = r.choice([0.5, 1.0, 2.0], c) * r.choice([-1.0, 1.0], c)
        g[1], g[2], g[5] = -abs(g[1]), abs(g[2]), 0.0
        self.gamma = g
        self.invstd = r.choice([0.5, 1.0, 2.0], (towers, c))
        self.scale = g[None, :] * self.invstd
        self.mean, self.shift = _ints(r, (towers, c), -8, 8) / 4, _ints(r, (towers, c), -8, 8) / 4
        self.drop = None
        if use_drop:
            self.drop = 2.0 * (r.random((n, c)) < 0.75)
            self.drop[0, [1, 5]], self.drop[0, 2] = 2.0, 0.0        # a kept negative-gamma and gamma == 0 channel, a dropped channel
        self.dp = _ints(r, (n, lq, c), -4, 4)
        # a tie between positive extremes with a gradient on it in the first pool group of window 0, whatever the seed gives elsewhere:
        # channel 3 (gamma > 0, kept: a tied maximum) and channel 1 (gamma < 0, kept: a tied minimum)
        g[3] = abs(g[3])
        if use_drop:
            self.drop[0, 3] = 2.0
        self.z[0, :pool, 3], self.z[0, :pool, 1] = 5.0, 2.0
        self.dp[0, 0, 3], self.dp[0, 0, 1] = 3.0, -2.0
        self.c1, self.c2 = _ints(r, (towers, c), -2, 2) / 8, _ints(r, (towers, c), -2, 2) / 8
        # ... and that element's du an exact bf16 tie in every case: du = scale * (drop * 3 + 1 + 19/64) = a power of two times 275/64
        # or 467/64, nine significant bits with the last one set
        self.invstd[0, 3], self.mean[0, 3], self.c1[0, 3], self.c2[0, 3] = 0.5, 0.25, -1.0, -0.125
        self.scale = g[None, :] * self.invstd
        self.dg = _ints(r, (n, c), -4, 4)
        self.gidx_r = r.integers(0, lq, (n, c)).astype(np.int32)
        self.e_center = _ints(r, (towers, c), 0, 8) / 4             # (the pair form's centred variant)

        d = np.ones((n, c)) if self.drop is None else self.drop
        self.ka = per_window(self.scale, wpt) * d[:, None, :]
        self.out = forward(self.z, self.scale, self.shift, self.drop, wpt, pool)
        self.ext, self.arg = route(self.z, self.ka, pool)
        # where scale * drop != 0 the documented rule IS the oracle's (the first maximum of y); they differ only where y is constant
        live = np.broadcast_to(self.ka != 0, self.arg.shape)
        assert np.array_equal(self.arg[live], route_y(self.z, self.scale, self.shift, self.drop, wpt, pool)[live])
        self.dy, self.zhat, self.du, self.sdy, self.sdyz = backward(self.z, self.dp, self.scale, self.mean, self.invstd, self.drop,
                                                                    self.c1, self.c2, wpt, pool)
        self.s0 = self.dp.sum(1)
        self.sa_ext, self.sa_act = (self.dp * self.ext).sum(1), (self.dp * self.out).sum(1)
        self.gidx = global_max(self.out, "f32")[1]                  # (out is exact in every type: the same rows in all of them)

        # ---- preconditions: from the inputs and the reference only
        for dt in DTS:
            for name in ("z", "dp", "dg", "out"):
                assert exact_in(getattr(self, name), dt), "%s must be exact in %s" % (name, dt)
        for name in ("scale", "shift", "mean", "invstd", "c1", "c2", "e_center") + (("drop",) if use_drop else ()):
            assert exact_in(getattr(self, name), "f32"), name
        assert np.abs(self.du).max() < 2.0 ** 15 and np.array_equal(self.du * 2.0 ** 8, np.round(self.du * 2.0 ** 8)) and exact_in(self.du, "f32")
        self.head = {
            "part_dy": require_exact_sums(np.abs(self.dy).sum(1), 1.0, "part_dy"),
            "part_dyz": require_exact_sums(np.abs(self.dy * self.zhat).sum(1), 1.0 / 8, "part_dyz"),
            "S1": require_exact_sums((np.abs(self.dp) * (self.ext + np.abs(per_window(self.mean, wpt)))).sum(1), 1.0 / 4, "S1 - mean * S0"),
            "S0": require_exact_sums(np.abs(self.dp).sum(1), 1.0, "S0"),
            "SA": require_exact_sums(np.abs(self.dp * self.out).sum(1), 1.0 / 4, "SA"),
            "part_du": max(require_exact_sums(np.abs(store(self.du, dt)).sum(1), 2.0 ** -8, "part_du " + dt) for dt in DTS),
        }
        # ---- census: conditions on the inputs
        g_ = groups(self.z, pool)
        tied = ((g_ == self.ext[:, :, None, :]).sum(2) >= 2) & (self.ext > 0) & (self.dp != 0) & live
        self.tie_share = float(tied.mean())
        assert pool == 1 or self.tie_share >= 0.01, self.tie_share           # (a group of one element has no ties)
        assert (self.ka < 0).any(), "no channel with scale * drop < 0"
        assert not use_drop or (self.drop == 0).any()
        self.bf16_rounded, self.bf16_ties = rounding_census(self.du, "bf16")
        assert self.bf16_rounded > 0 and self.bf16_ties >= 1

    def du_stored(self, dt):
        return store(self.du, dt)

    def sparse(self, which, dt):
        """(gidx, dense dp, backward(...)) of the sparse form: which = "fwd" (the reference forward's rows) or "rand"."""
        n, wpt, l, c, pool, _ = self.shape
        gi = self.gidx if which == "fwd" else self.gidx_r
        dp = dense_dp(self.dg, gi, self.lq, dt)
        return gi, dp, backward(self.z, dp, self.scale, self.mean, self.invstd, self.drop, self.c1, self.c2, wpt, pool)


@functools.lru_cache(maxsize=32)
def bn_case(shape):
    return BnCase(tuple(shape))


def split_rows(r, total, rows):
    """`total` (n, C) of grid multiples as `rows` partial rows (n * rows, C) that add up to it: random integer multiples of the grid in
    all rows but the last."""
    n, c = total.shape
    parts = r.integers(-64, 65, (n, rows, c)).astype(np.float64) / 4
    parts[:, -1] = total - parts[:, :-1].sum(1)
    assert exact_in(parts, "f32")
    return parts.reshape(n * rows, c)


class FinalizeCase:
    """vm_bn_finalize on chosen partial rows: count = 3 * 2^10, mean m on the 1/4 grid, var + eps = 4^k exactly with eps = 2^-10 (k in
    {-1, 0, 1}: invstd 2, 1, 0.5), momentum 0.5, dyadic starting moving statistics and zero-debias accumulators, zd_correction 2 (the first
    step).  sum z = m * count and sum z^2 = (4^k - eps + m^2) * count are integers; every output but the moving variance is an fp32 number.
    center: None, "bias" (center_bias (C): the statistics stay those of z) or "tile" (tile_center (towers, C): the rows hold the sums over
    t = z - ctr)."""
    EPS, MOMENTUM, COUNT, ZD_CORRECTION = 2.0 ** -10, 0.5, 3072.0, 2.0

    def __init__(self, shape, center):
        rows, towers, c = shape
        r = np.random.default_rng([rows, towers, c, 11])
        cnt, eps = self.COUNT, self.EPS
        self.m = _ints(r, (towers, c), -8, 8) / 4
        self.istd = r.choice([0.5, 1.0, 2.0], (towers, c))
        var = 1.0 / self.istd ** 2 - eps
        ssum, ssq = self.m * cnt, (var + self.m ** 2) * cnt
        self.gamma = r.choice([0.5, 1.0, 2.0], c) * r.choice([-1.0, 1.0], c)
        self.gamma[5 % c] = 0.0
        self.beta = _ints(r, (c,), -8, 8) / 4
        self.center_bias = self.tile_center = None
        ctr = None
        if center == "bias":
            self.center_bias = _ints(r, (c,), -4, 8) / 4             # negative biases: ctr = max(bias, 0)
            ctr = np.broadcast_to(np.maximum(self.center_bias, 0.0), (towers, c))
        elif center == "tile":
            self.tile_center = ctr = _ints(r, (towers, c), 0, 8) / 4
            ssq = ssq - 2 * ctr * ssum + cnt * ctr ** 2             # the sums over t = z - ctr
            ssum = ssum - cnt * ctr
        assert np.array_equal(ssum, np.round(ssum)) and np.array_equal(ssq, np.round(ssq)) and np.abs(ssq).max() < 2.0 ** 24
        self.stat_sum, self.stat_sq = split_rows(r, ssum, rows), split_rows(r, ssq, rows)
        # starting moving mean and zero-debias mean accumulators anywhere on the 1/4 grid; the variance side starts as Keras starts it
        # (moving variance 1, accumulators 0), so that the 1 ulp of the moving variance is not spent on a cancellation of the test's making
        self.mm0, self.mv0 = _ints(r, (c,), -8, 8) / 4, np.ones(c)
        self.zd0 = _ints(r, (towers, 2, c), -8, 8) / 4
        self.zd0[:, 1] = 0.0
        # ---- references
        self.scale = self.gamma[None, :] * self.istd
        self.shift = self.beta[None, :] - self.m * self.scale
        if ctr is not None:
            self.shift_adj, self.mean_adj = self.shift + self.scale * ctr, self.m - ctr
        vv = var * (cnt / (cnt - (1.0 + eps)))                      # not dyadic: float64
        mom = self.MOMENTUM
        mm, mv = self.mm0.copy(), self.mv0.copy()
        for t in range(towers):                                     # the plain exponential average, tower by tower
            mm = mm - (mm - self.m[t]) * (1.0 - mom)
            mv = mv - (mv - vv[t]) * (1.0 - mom)
        self.mm_plain, self.mv_plain = mm, mv
        self.zd = self.zd0.copy()                                   # zero-debias: every tower its own accumulator, the last one's wins
        self.zd[:, 0] = self.zd0[:, 0] - (self.zd0[:, 0] - self.m) * (1.0 - mom)
        self.zd[:, 1] = self.zd0[:, 1] - (self.zd0[:, 1] - vv) * (1.0 - mom)
        self.mm_zd, self.mv_zd = self.zd[-1, 0] * self.ZD_CORRECTION, self.zd[-1, 1] * self.ZD_CORRECTION
        for v in (self.m, self.istd, self.scale, self.shift, self.mm_plain, self.zd[:, 0], self.mm_zd, self.gamma, self.beta, self.mm0, self.mv0):
            assert exact_in(v, "f32")
        assert not exact_in(vv, "f32")


# The moving variance carries count / (count - (1 + eps)), which is not dyadic.  One update r' = r - (r - (float)v) * 0.5 with r, v > 0
# rounds v (<= ulp(v) / 2, halved), the difference (<= ulp(max(r, v)) / 2, halved) and the result (<= ulp(r') / 2); r' >= max(r, v) / 2,
# so ulp(v), ulp(max(r, v)) <= 2 ulp(r'): at most 1.5 ulp(r') per update, and what the previous tower left is halved in value but may
# sit in a binade twice as coarse: it carries over at most whole.  Zero-debias form: one update from a zero accumulator (the difference
# and the result are exact) and an exact doubling: 1/2 ulp + the cast of the reference -- the 1 ulp the test holds it to.
PLAIN_MV_ULPS = 1.5


def ulp32(v):
    """The spacing of fp32 at |v| (float64 array)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)
