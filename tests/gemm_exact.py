"""Exactly representable inputs for the conv GEMM kernels (tests/test_gpu_conv_exact.py on the device, tests/test_gemm_exact_cpu.py on
the host): seeded operands on a power-of-two grid, small enough that every product and every partial sum of every output is an fp32
number.  The result then does not depend on summation order, tile shape, split-K plan, MFMA shape or the hi / lo split of VM_F32S: an
fp32 output must equal the float64 reference bit for bit, a 16-bit output its round-to-nearest-even (csrc/common.hpp: both conversions
are RNE, like torch.Tensor.to), and one dropped, doubled or misplaced product moves an element by at least one grid unit.  Pure
numpy / torch: nothing here touches the HIP library or a GPU."""
import functools

import numpy as np
import torch

LIMIT = 2.0 ** 24           # integers below it, and all their partial sums, are fp32 numbers
STORE = {"f32": torch.float32, "f32s": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
BITS = {"f32": 24, "f32s": 24, "bf16": 8, "f16": 11}        # significand bits
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float64: torch.int64}
REGIMES = {"f32": ("small", "wide"), "f32s": ("small", "lo-x", "lo-w"), "bf16": ("small", "wide"), "f16": ("small", "wide")}

# ---- the shape tables (n, L, c_in, c_out); the first two are the lists of tests/test_gpu_kernels.py (the device file asserts it) ------
GEMM_SHAPES = [(3, 200, 16, 24), (2, 300, 128, 256), (1, 129, 8, 136), (2, 5, 24, 8), (2, 260, 32, 64), (3, 131, 96, 32),
               (8, 140, 64, 384), (3, 520, 256, 512), (8, 300, 64, 256), (16, 1030, 256, 256)]
RESIDENT_SHAPES = [(2, 700, 128, 256), (3, 760, 256, 256), (2, 650, 64, 512), (1, 129, 32, 128), (2, 5, 128, 128),
                   (3, 131, 192, 320), (1, 62, 64, 64), (4, 3000, 128, 256), (4, 1500, 256, 384), (4, 750, 384, 512)]
FALLBACK_SHAPES = [GEMM_SHAPES[i] for i in (1, 2, 3, 5, 7, 9)]                  # test_conv_fwd_dgrad_wgrad_fallback_kernels
WGRAD_VARIANT_SHAPES = [(2, 700, 128, 256), (2, 650, 64, 512), (2, 5, 128, 128), (3, 131, 192, 320), (1, 62, 64, 64),
                        (4, 750, 384, 512)]                                     # test_conv_wgrad_kernel_variants
# n_windows * ceil(L / 128) > 512 = launch_nt's grid cap: the second trip of the persistent loops; 520 % 8 == 0 takes the XCD order
PERSISTENT_SHAPES = [(520, 100, 8, 16), (515, 100, 8, 16), (520, 100, 64, 256), (515, 100, 64, 256)]
# (n, windows per tower, L, c_in, c_out) of test_conv_wgrad_split_granularity
SPLIT_SHAPES = [(6, 3, 190, 64, 64), (10, 5, 64, 128, 128), (3, 3, 62, 64, 128), (14, 7, 1000, 128, 128), (2, 1, 3000, 128, 256),
                (9, 9, 129, 192, 64), (22, 11, 318, 64, 64)]
# the fused forwards: K side 128 / 256 / 384 / 512 (every written-out K loop of conv_nt3_kernel) and 64 / 192 (none: the packed pointer
# must fall back); lengths either side of the 254-position tile, cfg-A's block 2 with 2 windows
FUSED_SHAPES = [(2, 508, 128, 256), (2, 254, 256, 128), (2, 1016, 64, 128), (2, 254, 384, 128), (2, 254, 512, 256), (2, 254, 192, 128),
                (2, 3000, 128, 256)]
BNRED_SHAPES = [(3, 254, 128, 256, True), (2, 255, 128, 64, False), (2, 1000, 256, 384, True), (3, 509, 384, 512, True),
                (1, 130, 256, 128, False), (2, 254, 128, 192, True)]            # (n, L, c_in, c_out, red_a padded); K side = c_out


def conv_cases(shapes, dts=("f32", "f32s", "bf16", "f16"), regimes=None):
    """(dt, regime, n, L, c_in, c_out) for every regime the storage type has (or those of `regimes` it has)."""
    return [(dt, reg) + tuple(s) for s in shapes for dt in dts for reg in REGIMES[dt] if regimes is None or reg in regimes]


def case_key(dt, regime):
    """The operand class a case is generated for: `small` and lo operands do not depend on the storage type, `wide` ones on whether it
    is bf16 (8 significand bits) or not."""
    return ("bf16" if dt == "bf16" else "f16") if regime == "wide" else "f32"


# what tests/test_gpu_conv_exact.py parametrises over (tests/test_gemm_exact_cpu.py constructs every one of them on the host first)
DT16 = ("bf16", "f16")
DEFAULT_CASES = conv_cases(GEMM_SHAPES + RESIDENT_SHAPES)
FALLBACK_CASES = conv_cases(FALLBACK_SHAPES, ("f32", "bf16", "f16"))
WGRAD_VARIANT_CASES = conv_cases(WGRAD_VARIANT_SHAPES, DT16)
PERSISTENT_CASES = conv_cases(PERSISTENT_SHAPES, ("f32", "f32s", "f16"), ("small",))
SPLIT_CASES = [(dt, "small", n, l, cin, cout) for n, _, l, cin, cout in SPLIT_SHAPES for dt in DT16]
FWD_E_CASES = conv_cases(FUSED_SHAPES, DT16)
FWD_POOL_CASES = conv_cases(FUSED_SHAPES, DT16, ("small",))
BNRED_CASES = [(dt, reg) + tuple(s) for s in BNRED_SHAPES for dt in DT16 for reg in REGIMES[dt]]   # (.., red_a padded)
ALL_CONV_CASES = (DEFAULT_CASES + FALLBACK_CASES + WGRAD_VARIANT_CASES + PERSISTENT_CASES + SPLIT_CASES + FWD_E_CASES + FWD_POOL_CASES +
                  [c[:6] for c in BNRED_CASES])


# ---- number formats ------------------------------------------------------------------------------------------------------------------
def store(a, dt):
    """float64 -> the storage type (RNE) -> float64."""
    return torch.as_tensor(np.asarray(a, dtype=np.float64) + 0.0).to(STORE[dt]).to(torch.float64).numpy()     # (+ 0.0: no -0.0 in a reference)


def exact_in(a, dt):
    return bool(np.array_equal(store(a, dt), np.asarray(a, dtype=np.float64)))


def rounding_census(v, dt):
    """(fraction of v that storage rounding changes, number of exact ties) from the reference alone."""
    v = np.asarray(v, dtype=np.float64)
    st = store(v, dt)
    _, e = np.frexp(v)                                          # |v| = m * 2^e, m in [0.5, 1): spacing 2^(e - bits)
    half = np.ldexp(0.5, e - BITS[dt])
    changed = st != v
    return float(changed.mean()), int((changed & (np.abs(st - v) == half)).sum())


def bf16_halves(a):
    """hi = bf16(x), lo = bf16(x - hi): the operand split of VM_F32S (csrc/conv_common.hpp split_f32x4)."""
    t = torch.as_tensor(np.asarray(a, dtype=np.float64)).to(torch.float32)
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi.to(torch.float64).numpy(), lo.to(torch.float64).numpy()


def require_exact_sums(abs_sum, grid, what):
    """THE precondition: terms that are multiples of `grid` whose absolute values sum to less than 2^24 grid units have every partial
    sum, in any order, in fp32.  Computed from the inputs and the reference only, never from a kernel's output."""
    m = float(np.max(abs_sum)) / grid
    assert m < LIMIT, "%s: sum |term| = %.3g grid units >= 2^24" % (what, m)
    return m


def sums_exact(abs_sum, grid):
    return float(np.max(abs_sum)) / grid < LIMIT


# ---- float64 references: plain matmuls ---------------------------------------------------------------------------------------------------
def pad1(a):
    n, l, c = a.shape
    out = np.zeros((n, l + 2, c))
    out[:, 1:l + 1] = a
    return out


def conv_same(x, w):
    """x (n, L, c_in), w (3, c_in, c_out) -> (n, L, c_out): Conv1D(3, padding='same'), out[t] = sum_k x[t + k - 1] @ w[k]."""
    n, l, _ = x.shape
    xp = pad1(x)
    return sum(xp[:, k:k + l].reshape(n * l, -1) @ w[k] for k in range(3)).reshape(n, l, -1)


def conv_dgrad(du, w):
    """dx[t] = sum_k du[t + 1 - k] @ w[k]^T."""
    n, l, _ = du.shape
    dp = pad1(du)
    return sum(dp[:, 2 - k:2 - k + l].reshape(n * l, -1) @ w[k].T for k in range(3)).reshape(n, l, -1)


def conv_wgrad(x, du):
    """dW[k] = sum_{n, t} x[t + k - 1]^T du[t]."""
    n, l, _ = x.shape
    xp = pad1(x)
    return np.stack([xp[:, k:k + l].reshape(n * l, -1).T @ du.reshape(n * l, -1) for k in range(3)])


def pair_extreme(z, gamma):
    """(n, L, c) -> (n, L // 2, c): the pair maximum where gamma >= 0, else the pair minimum (what MaxPool1D(2) of the BatchNorm output
    selects); `second`: the extreme is the pair's second element (ties: the first)."""
    n, l, c = z.shape
    pr = z[:, :l // 2 * 2].reshape(n, l // 2, 2, c)
    pos = (np.asarray(gamma) >= 0)[None, None, :]
    second = np.where(pos, pr[:, :, 1] > pr[:, :, 0], pr[:, :, 1] < pr[:, :, 0])
    return np.where(second, pr[:, :, 1], pr[:, :, 0]), np.where(second, pr[:, :, 0], pr[:, :, 1]), second


# ---- input generators ------------------------------------------------------------------------------------------------------------------
def _ints(r, shape, amp, p_zero=0.0):
    v = r.integers(-amp, amp + 1, shape).astype(np.float64)
    if p_zero:
        v *= r.random(shape) >= p_zero
    return v


def _var(a):
    return a * (a + 1) / 3.0            # of a uniform integer in [-a, a]


def _wide_amplitudes(dt, cin, cout):
    """Uniform integer ranges for x, w, du whose forward / dgrad outputs have a standard deviation of about 300 (bf16: integers past 256
    are rounded) or 2400 (f16: past 2048; fp32 storage takes the same operands)."""
    target = 300.0 ** 2 if dt == "bf16" else 2400.0 ** 2
    a = 1
    while _var(-(-3 * a // 2)) * _var(a) * 3 * cin < target:
        a += 1
    ax, aw, ad = -(-3 * a // 2), a, 1
    while _var(ad) * _var(aw) * 3 * cout < target:
        ad += 1
    return ax, aw, ad


def _lo_operand(r, shape):
    """a + b * 2^-9, a in {-2, -1, 1, 2} or the element is 0, |b| <= 3: 10 .. 11 significant bits, so the bf16 `lo` half carries b."""
    a = r.choice([-2.0, -1.0, 1.0, 2.0], shape)
    b = r.integers(-3, 4, shape).astype(np.float64)
    v = (a + b * 2.0 ** -9) * (r.random(shape) < 0.5)
    hi, lo = bf16_halves(v)
    assert np.array_equal(hi + lo, v) and (lo != 0).mean() > 0.25 and exact_in(v, "f32")
    return v


class ConvCase:
    """Operands and float64 references of one (shape, regime): x (n, L, c_in), w (3, c_in, c_out), b (c_out), du_d / du_w (n, L, c_out:
    the output gradient the dgrad / the wgrad takes -- the same tensor except in the lo regimes, where each of the four cross products
    a_hi * b_lo gets an operand pair of its own), z = relu(conv + b), dx, gw; `grid`: the unit every product is a multiple of."""

    def __init__(self, shape, regime, dt):
        n, l, cin, cout = shape
        self.shape, self.regime = shape, regime
        r = np.random.default_rng([n, l, cin, cout, sum(map(ord, regime))])
        self.grid = 1.0
        if regime == "small":
            x, w = _ints(r, (n, l, cin), 1, 0.25), _ints(r, (3, cin, cout), 1, 0.25)       # about half zeros each
            du = _ints(r, (n, l, cout), 1, 0.25)
            dud, duw = du, du
        elif regime == "wide":
            ax, aw, ad = _wide_amplitudes(dt, cin, cout)
            x, w, du = _ints(r, (n, l, cin), ax), _ints(r, (3, cin, cout), aw), _ints(r, (n, l, cout), ad)
            dud, duw = du, du
        elif regime in ("lo-x", "lo-w"):
            self.grid = 2.0 ** -9
            x, w, du = _ints(r, (n, l, cin), 1, 0.25), _ints(r, (3, cin, cout), 1, 0.25), _ints(r, (n, l, cout), 1, 0.25)
            dud, duw = du, du
            if regime == "lo-x":        # forward x_lo * w_hi, wgrad x_lo * du_hi, dgrad du_lo * w_hi
                x, dud = _lo_operand(r, x.shape), _lo_operand(r, du.shape)
            else:                       # forward x_hi * w_lo, dgrad du_hi * w_lo, wgrad x_hi * du_lo
                w, duw = _lo_operand(r, w.shape), _lo_operand(r, du.shape)
            for narrow in ((w, duw) if regime == "lo-x" else (x, dud)):
                assert not bf16_halves(narrow)[1].any()                                     # at most 8 bits: lo == 0, so lo * lo == 0
        else:
            raise ValueError(regime)
        b = _ints(r, (cout,), 3)
        self.x, self.w, self.b, self.du_d, self.du_w = x, w, b, dud, duw
        # the precondition, per output element: sum |product| (+ |bias|) in grid units; VM_F32S issues the hi and lo parts of an operand
        # as separate products, so its wide operand enters as |hi| + |lo|
        a = lambda v: np.add(*map(np.abs, bf16_halves(v))) if regime in ("lo-x", "lo-w") else np.abs(v)
        self.head_fwd = require_exact_sums(conv_same(a(x), a(w)) + np.abs(b), self.grid, "forward")
        self.head_dgrad = require_exact_sums(conv_dgrad(a(dud), a(w)), self.grid, "dgrad")
        self.head_wgrad = require_exact_sums(conv_wgrad(a(x), a(duw)), self.grid, "wgrad")
        self.z = np.maximum(conv_same(x, w) + b, 0.0)
        self.dx = conv_dgrad(dud, w)
        self.gw = conv_wgrad(x, duw)
        for dt_ in (("f32", "f32s", "bf16", "f16") if regime == "small" else (dt,)):
            assert all(exact_in(v, dt_) for v in (x, w, dud, duw)), "operands must be exact in %s" % dt_
        if regime == "small":           # no storage rounding in any type: |values| <= 256
            assert max(self.z.max(), np.abs(self.dx).max()) <= 256 and exact_in(self.z, "bf16") and exact_in(self.dx, "bf16")
        if regime == "wide" and dt in ("bf16", "f16"):
            for name, v in (("z", self.z), ("dx", self.dx)):
                # at least 0.5 % of the outputs rounded and 100 exact ties; a tensor too small to hold 100 (about one output in ten
                # is a tie at these amplitudes: the first rounded binade has a spacing of 2) owes one per 40 elements instead
                frac, ties = rounding_census(v, dt)
                assert frac >= 0.005 and ties >= min(100, v.size // 40) and np.abs(v).max() < 60000, (name, frac, ties, np.abs(v).max())

    def forward(self, dt):
        """z as stored in `dt`, the BatchNorm statistics of the stored values (n, c_out) and whether their sums meet the precondition
        over the whole window (always in the `small` regime)."""
        z = store(self.z, dt)
        g = self.grid
        ok_sum, ok_sq = sums_exact(z.sum(1), g), sums_exact((z * z).sum(1), g * g)
        assert ok_sum and (ok_sq or self.regime != "small")     # the sum in every regime, the sum of squares at least in `small`
        return z, z.sum(1), (z * z).sum(1), ok_sq


@functools.lru_cache(maxsize=6)
def _conv_case(shape, regime, klass):
    return ConvCase(shape, regime, klass)


def conv_case(shape, regime, dt):
    """Cached per operand class (case_key)."""
    return _conv_case(tuple(shape), regime, case_key(dt, regime))


# ---- the folded-BatchNorm forms ----------------------------------------------------------------------------------------------------------
def signs(c, seed):
    """BatchNorm gammas of both signs, one of them zero (gamma >= 0 selects the maximum)."""
    g = np.random.default_rng(seed).choice([-1.5, -1.0, 1.0, 2.0], c)
    g[5 % c] = 0.0
    return g


def _affine(r, towers, c, scales=(0.5, 1.0, 2.0)):
    """Per-tower BatchNorm affines that keep every product on a power-of-two grid: scale in +-{0.5, 1, 2}, integer shift."""
    return r.choice(scales, (towers, c)) * r.choice([-1.0, 1.0], (towers, c)), _ints(r, (towers, c), 2)


class FoldFactors:
    """vm_conv_wgrad_fold on (x, du) of a ConvCase: dW[k][ci][co] = sum_t scale_t[ci] * G_t[k][ci][co] + shift_t[ci] * dsum[t][k][co], G_t the
    plain weight gradient over tower t's windows, dsum[t][k] = the sum of du over the positions whose tap k lies inside the window."""

    def __init__(self, shape, x, du):
        n, wpt, l, cin, cout = shape
        towers = n // wpt
        r = np.random.default_rng([n, wpt, l, cin, cout])
        self.scale, self.shift = _affine(r, towers, cin)
        dut = du.reshape(towers, wpt, l, cout)
        cs = dut.sum((1, 2))
        self.dsum = np.stack([cs - dut[:, :, 0].sum(1), cs, cs - dut[:, :, -1].sum(1)], 1)
        acs = np.abs(dut).sum((1, 2))
        self.gw, head = 0.0, 0.0
        for t in range(towers):
            sl = slice(t * wpt, (t + 1) * wpt)
            s, h = self.scale[t][None, :, None], self.shift[t][None, :, None]
            self.gw = self.gw + s * conv_wgrad(x[sl], du[sl]) + h * self.dsum[t][:, None, :]
            head = head + np.abs(s) * conv_wgrad(np.abs(x[sl]), np.abs(du[sl])) + np.abs(h) * acs[t][None, None, :]
        require_exact_sums(acs, 1.0, "dsum")
        require_exact_sums(head, 0.5, "folded wgrad")


class FoldCase:
    """vm_fold_bn_weights + vm_conv_fwd_fold: e (n, L, c_in) >= 0 (a pool extreme of a ReLU output), two towers with their own affines,
    the layer's input y = scale_t * e + shift_t inside the window and 0 in the SAME padding: z = relu(conv(y) + b).  wf (towers, c_out, 3,
    c_in) = W * scale, hb (towers, 3, c_out) = sum_ci W * shift, ctr (towers, c_out) = max(b + hb[0] + hb[1] + hb[2], 0)."""

    def __init__(self, shape, dt):
        n, l, cin, cout = shape
        towers, wpt = 2, n // 2
        r = np.random.default_rng([n, l, cin, cout, 7])
        self.e = r.integers(0, 3, (n, l, cin)).astype(np.float64) * (r.random((n, l, cin)) < 0.5)
        self.w, self.b = _ints(r, (3, cin, cout), 1, 0.25), _ints(r, (cout,), 3)
        # (scales +-{1, 2}: with halves z^2 sits on a grid of 1/4 and the sum of squares of a 512-channel window passes 2^24 units)
        self.scale, self.shift = _affine(r, towers, cin, (1.0, 2.0))
        self.gamma = signs(cout, l + cout)
        self.wf = np.stack([(self.w * self.scale[t][None, :, None]).transpose(2, 0, 1) for t in range(towers)])
        self.hb = np.einsum("kio,ti->tko", self.w, self.shift)
        self.ctr = np.maximum(self.b + self.hb.sum(1), 0.0)
        z, head = np.empty((n, l, cout)), np.empty((n, l, cout))
        for t in range(towers):
            sl = slice(t * wpt, (t + 1) * wpt)
            z[sl] = conv_same(self.e[sl] * self.scale[t] + self.shift[t], self.w) + self.b
            head[sl] = conv_same(self.e[sl], np.abs(self.w) * np.abs(self.scale[t])[None, :, None]) + (
                np.abs(self.hb[t]).sum(0) + np.abs(self.b) + self.ctr[t])
        require_exact_sums(head, 1.0, "folded forward")
        require_exact_sums(np.abs(self.w).sum(1) * np.abs(self.shift).max(), 1.0, "hb")
        self.z = np.maximum(z, 0.0)
        self.z_st = store(self.z, dt)
        assert exact_in(self.wf, dt) and exact_in(self.ctr, dt) and exact_in(self.e, dt)
        cw = np.repeat(self.ctr, wpt, axis=0)[:, None, :]
        for tile in ((self.z_st, self.z - cw) if dt == "f16" else (self.z_st,)):      # f16: also the centred tile t = relu(z) - ctr
            assert dt != "f16" or exact_in(tile, dt)                                     # (11 bits: no rounding on this grid below 1024)
            require_exact_sums(np.abs(tile).sum(1), 1.0, "statistics: sum")
            require_exact_sums((tile * tile).sum(1), 1.0, "statistics: sum of squares")


@functools.lru_cache(maxsize=2)
def fold_case(shape, dt):
    return FoldCase(tuple(shape), dt)


# ---- block 1: Conv1D(F, 32) on the waveform ------------------------------------------------------------------------------------------------
CONV1_SHAPES = [(3, 700, 16), (2, 256, 128), (1, 37, 8)]                              # (n, L, F) of test_conv1_fwd
CONV1_WGRAD_SHAPE = (3, 1500, 24)                                                     # of test_conv1_wgrad
CONV1_FUSED_SHAPES = [(4, 700, 16), (2, 1200, 128), (2, 532, 40), (2, 300, 160)]      # ragged chunks, F tails (16, 40, 160), F > 128


def pad_wave(x):
    """(n, L) -> (n, L + 31): 15 zeros before, 16 after (the SAME padding of a 32-tap filter)."""
    out = np.zeros((x.shape[0], x.shape[1] + 31))
    out[:, 15:15 + x.shape[1]] = x
    return out


def conv32(x, w):
    """x (n, L), w (32, 1, F) -> (n, L, F): out[t] = sum_k xp[t + k] * w[k]."""
    return np.lib.stride_tricks.sliding_window_view(pad_wave(x), 32, axis=1) @ w[:, 0, :]


def pool_extreme(z, gamma, pool):
    n, l, c = z.shape
    pr = z[:, :l // pool * pool].reshape(n, l // pool, pool, c)
    return np.where((np.asarray(gamma) >= 0)[None, None, :], pr.max(2), pr.min(2))


class Conv1Case:
    """x (n, L) waveform, w (32, 1, F), b (F), du (n, L, F); z = relu(conv + b) UNROUNDED, gw = the filter gradient.  Regimes: small,
    wide (as ConvCase, K = 32), lo-w: filters a + b * 2^-12, exact only as hi + lo halves (f16) or hi + lo bf16s, and lo-x: a waveform
    a + b * 2^-9 whose bf16 lo half is non-zero (the x_lo * w_hi product of bf16 storage and of f1_products = 3) and which a half holds."""

    def __init__(self, shape, regime, dt):
        n, l, f = shape
        self.regime = regime
        r = np.random.default_rng([n, l, f, sum(map(ord, regime))])
        self.grid = 1.0
        if regime == "wide":
            target, a = (300.0 ** 2 if dt == "bf16" else 2400.0 ** 2), 1
            while _var(-(-3 * a // 2)) * _var(a) * 32 < target:
                a += 1
            x, w = _ints(r, (n, l), -(-3 * a // 2)), _ints(r, (32, 1, f), a)
        else:
            x, w = _ints(r, (n, l), 1, 0.25), _ints(r, (32, 1, f), 1, 0.25)
        if regime == "lo-w":
            self.grid = 2.0 ** -12
            w = r.choice([-2.0, -1.0, 1.0, 2.0], w.shape) + r.integers(-3, 4, w.shape) * 2.0 ** -12
            wh = store(w, "f16")
            assert not exact_in(w, "f16") and exact_in(w - wh, "f16") and np.array_equal(np.add(*bf16_halves(w)), w)
        if regime == "lo-x":
            self.grid = 2.0 ** -9
            x = _lo_operand(r, x.shape)
            assert exact_in(x, "f16")
        du = _ints(r, (n, l, f), 1, 0.25)
        b = _ints(r, (f,), 3)
        self.x, self.w, self.b, self.du = x, w, b, du
        ax = np.add(*map(np.abs, bf16_halves(x)))                  # the hi and lo halves are separate products
        require_exact_sums(conv32(ax, np.add(*map(np.abs, bf16_halves(w)))) + np.abs(b), self.grid, "conv1 forward")
        self.z = np.maximum(conv32(x, w) + b, 0.0)
        if regime == "lo-w":
            self.z_hi = np.maximum(conv32(x, store(w, "f16")) + b, 0.0)     # what f1_products = 1 (x_hi * w_hi alone) computes
        xp = pad_wave(x)
        wg = lambda xx, dd: np.stack([np.einsum("nt,ntf->f", xx[:, k:k + l], dd) for k in range(32)])[:, None, :]
        require_exact_sums(wg(np.abs(xp), np.abs(du)), self.grid, "conv1 wgrad")
        self.gw = wg(xp, du)
        assert exact_in(du, "bf16") and (regime == "lo-x" or exact_in(x, "bf16")) and (regime == "lo-w" or exact_in(w, "bf16"))
        if regime == "lo-x":
            self.z_xhi = np.maximum(conv32(bf16_halves(x)[0], w) + b, 0.0)     # what leaving out x_lo * w_hi would give
        if regime == "wide" and dt in ("bf16", "f16"):
            frac, ties = rounding_census(self.z, dt)
            assert frac >= 0.005 and ties >= min(100, self.z.size // 40) and self.z.max() < 60000, (frac, ties)

    def stats(self, z):
        """The sums of z and z^2 per window and whether each meets the precondition: both in `small`, the sum in `wide` too."""
        g = self.grid
        ok_sum, ok_sq = sums_exact(z.sum(1), g), sums_exact((z * z).sum(1), g * g)
        assert (ok_sum or self.regime in ("lo-x", "lo-w")) and (ok_sq or self.regime != "small")
        return z.sum(1), (z * z).sum(1), ok_sum, ok_sq


@functools.lru_cache(maxsize=4)
def _conv1_case(shape, regime, klass):
    return Conv1Case(shape, regime, klass)


def conv1_case(shape, regime, dt):
    return _conv1_case(tuple(shape), regime, case_key(dt, regime))


# ---- block 1, fused backward: vm_conv1_fused_bwd -----------------------------------------------------------------------------------------
# ((n, L, F), windows per tower).  256-position chunks, 32-position tiles, 32-channel column tiles (CT of them per 128 channels), Lq = L //
# pool; a tile takes the fast path when all its 32 positions are pooled.
CONV1_BWD_SHAPES = [
    ((4, 701, 16), 2),      # 3 chunks, the last tile ragged (L % 2 = L % 4 = 1); one column tile shared by four waves
    ((2, 534, 40), 2),      # L % 4 = 2; CT = 2 with an 8-channel second tile
    ((3, 1283, 160), 3),    # 6 chunks, the last of 3 positions (pool 4: no pooled position in it at all); a second blockIdx.y
    ((3, 1283, 160), 1),    # ... and three towers
    ((2, 291, 96), 1),      # CT = 3 with one idle wave; L % 4 = 3
    ((1, 512, 32), 1),      # exactly two chunks, no remainder: the `more` prefetch must not read a chunk that does not exist
    ((1, 5, 8), 1),         # L just above pool: one (pool 4) or two pooled positions and a remainder row, no fast tile
]
CONV1_BWD_LO_SHAPES = [CONV1_BWD_SHAPES[1], CONV1_BWD_SHAPES[5]]      # the lo regimes: also test_conv1_fused_bwd_products' shapes
CONV1_BWD_REGIMES = ("small", "rounded", "lo-x", "lo-w")
CONV1_BWD_GRIDS = ("default", "window", "split")      # vm_set_tuning("f1_blocks", .): untouched (1024), n, 2 n


def f1_splits(n, chunks, target):
    """(workgroups per window, chunks per workgroup) of the fused block-1 backward (csrc/conv1_fused.hip f1_splits)."""
    s = min(max(-(-target // n), 1), chunks)
    cps = -(-chunks // s)
    return -(-chunks // cps), cps


def f1_grid(n, l, form):
    return f1_splits(n, -(-l // 256), {"default": 1024, "window": n, "split": 2 * n}[form])


def conv1_bwd_grids(n, l):
    """The grid forms that differ at this shape: `window` walks every chunk of a window in one workgroup (the double-buffered loop),
    `split` gives two workgroups per window -- of 2 + 1 chunks at three chunks (a short last split), 3 + 3 at six."""
    forms, seen = [], set()
    for form in CONV1_BWD_GRIDS:
        g = f1_grid(n, l, form)
        if g not in seen:
            seen.add(g)
            forms.append(form)
    return forms


def _conv1_bwd_cases():
    """(dt, regime, n, L, F, wpt, pool, drop, grid form).  Every (pool, drop) pair on the default grid; the other grid forms where they
    differ from it, on the diagonal (pool 2, no drop), (pool 4, drop).  The lo regimes at two shapes; `rounded` not at (1, 5, 8), whose
    40 elements cannot hold the census it asserts.  Ordered so that the cases of one reference are neighbours (the caches are small)."""
    out = []
    for (shape, wpt) in CONV1_BWD_SHAPES:
        for regime in CONV1_BWD_REGIMES:
            if (regime in ("lo-x", "lo-w") and (shape, wpt) not in CONV1_BWD_LO_SHAPES) or (regime == "rounded" and shape[1] < 256):
                continue
            for pool in (2, 4):
                for drop in (False, True):
                    for form in conv1_bwd_grids(shape[0], shape[1]):
                        if form == "default" or drop == (pool == 4):
                            out += [(dt, regime) + shape + (wpt, pool, drop, form) for dt in DT16]
    return out


CONV1_BWD_CASES = _conv1_bwd_cases()
CONV1_BWD_PRODUCT_CASES = [(regime,) + shape + (wpt, pool, pool == 4) for shape, wpt in CONV1_BWD_LO_SHAPES for pool in (2, 4)
                           for regime in ("small", "lo-x", "lo-w")]
# every (shape, wpt, regime, pool, drop) the device file builds a reference for: the host file walks it
ALL_CONV1_BWD_CASES = sorted({c[2:5] + (c[5], c[1], c[6], c[7]) for c in CONV1_BWD_CASES} |
                             {c[1:4] + (c[4], c[0], c[5], c[6]) for c in CONV1_BWD_PRODUCT_CASES})


def dyadic_grid(a):
    """The largest power of two that every element of `a` is a multiple of (1 for an array of integers or of zeros)."""
    a = np.asarray(a, dtype=np.float64)
    g = 1.0
    while not np.array_equal(a / g, np.round(a / g)):
        g /= 2
        assert g > 2.0 ** -40
    return g


def conv1_wgrad(xp, du):
    """xp (n, L + 31) padded waveform, du (n, L, F) -> (32, 1, F): gw[k] = sum_{n, t} xp[n][t + k] * du[n][t]."""
    win = np.lib.stride_tricks.sliding_window_view(xp, 32, axis=1)                  # (n, L, 32)
    return (win.reshape(-1, 32).T @ du.reshape(-1, du.shape[2]))[:, None, :]


class Conv1BwdCase:
    """vm_conv1_fused_bwd on the waveform, filters and bias of a Conv1Case: per-tower scale, mean, invstd, c1, c2 (towers, F), drop (n, F)
    in {0, 2} or None, dp (n, L // pool, F) small integers.  The kernel folds ga = scale * drop, gb0 = scale * (invstd * c2 * mean - c1),
    gc = -scale * invstd * c2 in fp32 and forms du = [z > 0] * (gc * z + gb0 + [first extreme] * ga * dp) by fmas; with scale in +-{1, 2}
    (one 0), invstd in {0.5, 1}, c2 = +-1 / (invstd * |scale|) (so gc = +-1) and integer mean, c1 in [-2, 2] every one of them is exact.
    References (float64): z = the UNROUNDED relu(conv + b), du_exact from bn_exact.backward, du = bf16(du_exact) under both storage types
    (the kernel hands du to the weight-gradient MFMA as bf16 whatever the storage type is), gw[k] = sum bf16(x)[t + k] * du[t], gb = sum du.

    Regimes: `small` (Conv1Case small: du exact in bf16, a census of tied and of all-non-positive pool windows), `rounded` (Conv1Case wide
    of the bf16 class for both storage types: du rounded, a census of its rounding), lo-x / lo-w (the recompute of z needs the cross
    product; dropping it must change gw).  The lo regimes take c2 = 0 (gc = 0), so that du is an integer which the lo product decides
    through the ReLU mask and the routing of near-ties.  With gc = +-1 du inherits the 2^-9 / 2^-12 grid of z and the sums miss the
    precondition at these shapes: lo-x (bf16(x) on a 2^-8 grid) sum |bf16(x)| |du| = 6.9e8 units of 2^-17 at (2, 534, 40), 41 times 2^24;
    lo-w sum |du| = 1.8e7 .. 2.9e7 units of 2^-12, 1.1 .. 1.7 times 2^24.  gc * z itself is covered by `small` and `rounded`.

    The scale signs by (tower, 32-channel tile), the unit of the kernel's wave-uniform choice: the first is all >= 0 with the zero (the
    all_max path), the second mixed (use_min), the rest as drawn.  A shape with one tower and one tile takes its one path from `drop`:
    all_max with dropout, mixed without."""

    def __init__(self, shape, regime, pool, wpt, drop):
        from tests import bn_exact as B
        n, l, f = shape
        assert n % wpt == 0 and l >= pool and f % 8 == 0
        self.shape, self.regime, self.pool, self.wpt = shape, regime, pool, wpt
        self.towers, self.lq = n // wpt, l // pool
        self.c = c = conv1_case(shape, "wide", "bf16") if regime == "rounded" else conv1_case(shape, regime, "f16")
        r = np.random.default_rng([n, l, f, pool, wpt, int(drop), sum(map(ord, regime))])
        towers, tiles = self.towers, -(-f // 32)
        scale = r.choice([1.0, 2.0], (towers, f)) * r.choice([-1.0, 1.0], (towers, f))
        units = [(t, j) for t in range(towers) for j in range(tiles)]
        plan = ["max" if drop else "min"] if len(units) == 1 else ["max", "min"]
        for (t, j), kind in zip(units, plan):
            ch = slice(32 * j, min(32 * j + 32, f))
            width = ch.stop - ch.start
            if kind == "max":
                scale[t, ch] = np.abs(scale[t, ch])
                scale[t, ch.start + 5 % width] = 0.0
            else:
                scale[t, ch.start], scale[t, ch.start + 1] = -abs(scale[t, ch.start]), abs(scale[t, ch.start + 1])
                if len(units) == 1:
                    scale[t, ch.start + 5 % width] = 0.0
        self.scale = scale
        self.invstd = r.choice([0.5, 1.0], (towers, f))
        mag = np.where(scale == 0, 1.0, 1.0 / (self.invstd * np.maximum(np.abs(scale), 1.0)))
        self.c2 = r.choice([-1.0, 1.0], (towers, f)) * mag * (0.0 if regime in ("lo-x", "lo-w") else 1.0)
        self.mean, self.c1 = _ints(r, (towers, f), 2), _ints(r, (towers, f), 2)
        self.drop = None
        if drop:
            self.drop = 2.0 * (r.random((n, f)) < 0.75)
            self.drop[0, 0], self.drop[0, 2 % f] = 2.0, 0.0
        self.dp = _ints(r, (n, self.lq, f), 3)
        self.paths = {(t, j): "min" if (scale[t, 32 * j:32 * j + 32] < 0).any() else "max" for t, j in units}
        assert (scale == 0).any() and all(self.paths[u] == k for u, k in zip(units, plan))
        assert any(k == "max" and (scale[t, 32 * j:32 * j + 32] == 0).any() for (t, j), k in self.paths.items()) or plan == ["min"]

        # ---- the constants the kernel folds and every intermediate of du: fp32 numbers, in any association
        pw = lambda a: B.per_window(a, wpt)
        sc, mu, is_, k1, k2 = pw(self.scale), pw(self.mean), pw(self.invstd), pw(self.c1), pw(self.c2)
        dr = np.ones((n, 1, f)) if self.drop is None else self.drop[:, None, :]
        self.ga, self.gb0, self.gc = sc * dr, sc * (is_ * k2 * mu - k1), -sc * is_ * k2
        for v in (self.scale, self.mean, self.invstd, self.c1, self.c2, self.ga, self.gb0, self.gc, is_ * k2, k2 * mu, is_ * k2 * mu,
                  is_ * k2 * mu - k1, sc * is_, sc * k2):
            assert exact_in(v, "f32")
        assert exact_in(self.dp, "bf16") and exact_in(self.dp, "f16") and exact_in(bf16_halves(c.x)[0], "bf16")
        assert set(np.unique(np.abs(self.gc))) <= ({0.0} if regime in ("lo-x", "lo-w") else {0.0, 1.0})
        self.xh = pad_wave(bf16_halves(c.x)[0])
        self.du_exact, self.du, self.gw, self.gb = self.reference(c.z, check=True)

        # ---- the censuses and the discriminating power, from the inputs and the references alone
        g = B.groups(c.z, pool)
        self.windows = g.shape[0] * g.shape[1] * f
        ext, _ = B.route(c.z, np.broadcast_to(sc, (n, 1, f)), pool)
        self.tied = float(((g == ext[:, :, None, :]).sum(2) >= 2).mean()) if self.windows else 0.0
        live = (ext > 0) & (self.dp != 0) & np.broadcast_to(self.ga != 0, ext.shape)
        self.tied_live = float((((g == ext[:, :, None, :]).sum(2) >= 2) & live).mean()) if self.windows else 0.0
        self.all_nonpositive = float((g.max(2) <= 0).mean()) if self.windows else 0.0
        if regime == "small":
            assert exact_in(self.du_exact, "bf16"), "small: du must be exact in bf16"
            if self.windows >= 1000:
                assert self.tied >= 0.05 and self.all_nonpositive >= 0.05 and self.tied_live >= 0.01, (
                    self.tied, self.all_nonpositive, self.tied_live)
            assert self.head >= 6.0, self.head
        if regime == "rounded":
            self.census = rounding_census(self.du_exact[self.du_exact != 0], "bf16")
            assert self.census[0] >= 0.05 and self.census[1] >= 100, self.census
        if regime == "lo-x":
            self.gw_dropped = self.reference(c.z_xhi)[2]               # x_lo * w_hi left out of the recompute
            self.gw_full_x = conv1_wgrad(pad_wave(c.x), self.du)       # the filter gradient formed from x, not bf16(x)
            assert not np.array_equal(self.gw_full_x, self.gw)
        if regime == "lo-w":
            self.du_hi, self.gw_hi, self.gb_hi = self.reference(c.z_hi, check=True)[1:]    # f1_products = 1: x_hi * w_hi alone
            self.gw_dropped = self.gw_hi
        if regime in ("lo-x", "lo-w"):
            self.dropped_share = float((self.gw_dropped != self.gw).mean())
            assert self.dropped_share >= 0.01, self.dropped_share

    def reference(self, z, check=False):
        """(du_exact, du, gw, gb) for the recomputed activations z; check: assert the preconditions of this reference (head: the
        smaller head-room of the two sums, a factor)."""
        from tests import bn_exact as B
        n, l, f = self.shape
        du_exact = B.backward(z, self.dp, self.scale, self.mean, self.invstd, self.drop, self.c1, self.c2, self.wpt, self.pool)[2]
        du = store(du_exact, "bf16")
        if check:
            # every intermediate of the three evaluation orders of the kernel: fma(gc, z, gb0 or gb1), fma(gc, z, gb0) + ga * dp
            dpr = np.zeros((n, l, f))
            dpr[:, :self.lq * self.pool] = np.repeat(self.dp, self.pool, axis=1)
            for v in (self.gc * z, self.ga * dpr, self.ga * dpr + self.gb0, self.gc * z + self.gb0, self.gc * z + self.gb0 + self.ga * dpr,
                      du_exact):
                assert exact_in(v, "f32"), "an intermediate of du is not an fp32 number"
            grid = dyadic_grid(self.xh) * dyadic_grid(du)
            heads = (require_exact_sums(conv1_wgrad(np.abs(self.xh), np.abs(du)), grid, "conv1 fused bwd: sum |bf16(x)| |du|"),
                     require_exact_sums(np.abs(du).sum((0, 1)), dyadic_grid(du), "conv1 fused bwd: sum |du|"))
            self.head = min(getattr(self, "head", np.inf), LIMIT / max(max(heads), 1.0))
        return du_exact, du, conv1_wgrad(self.xh, du), du.sum((0, 1))


@functools.lru_cache(maxsize=4)
def conv1_bwd_case(shape, regime, pool, wpt, drop):
    return Conv1BwdCase(tuple(shape), regime, pool, wpt, bool(drop))


# ---- the length-masked fused inference kernels: vm_conv_fwd_pool_varlen and vm_conv1_fused_fwd_varlen --------------------------------------
# A bucket's windows share the padded length L and carry lens[n]; pooled rows at or past lens[n] // pool are +0.  The cases zero the
# input at and past lens[n], so the unmasked reference of a window's valid rows is also the reference of that recording ALONE at its
# own length (a valid row reads at most the zero just past the length: the SAME padding) -- which the host file asserts.
TROWS = 254         # conv_gemm.hip n2r::TROWS: positions per tile of conv_nt2r_kernel / conv_nt3_kernel
F1_CHUNK = 256      # conv1_fused.hip: positions per double-buffered chunk ...
F1_TILE = 32        # ... and per MFMA row tile (the host file reads all three from the sources)
OVER = 5            # lens[n] = L + OVER: a length past the padded one behaves as L

# (n, L, c_in, c_out), all served by vm_conv_fwd_pool_supported: 254 + 254 + 192 with n * tiles = 72 (8-group swizzle), two column
# tiles, c_in 128 (conv_nt3_kernel with packed weights); 254 + 254 with n * tiles = 26 (plain division), c_in 256; three full tiles
# with n * tiles = 57 and c_in 64, which conv_nt3_kernel does not serve
POOL_VARLEN_SHAPES = [(24, 700, 128, 256), (13, 508, 256, 128), (19, 762, 64, 128)]
# (n, L, F): CONV1_FUSED_SHAPES' ragged ones with enough windows for the table of either pool
CONV1_VARLEN_SHAPES = [(32, 700, 16), (28, 532, 40), (28, 300, 160)]
CONV1_VARLEN_REGIMES = ("small", "lo-x")


def mask_rows(full, lens, pool):
    """The mask helper: full (n, L // pool, c), lens (n,) -> rows q >= lens[n] // pool are +0."""
    q = np.arange(full.shape[1])[None, :, None]
    return np.where(q < (np.asarray(lens, dtype=np.int64) // pool)[:, None, None], full, 0.0)


def zero_past(x, lens):
    """x (n, L, ...) with every position at or past lens[n] zeroed."""
    t = np.arange(x.shape[1]).reshape((1, -1) + (1,) * (x.ndim - 2))
    return np.where(t < np.asarray(lens, dtype=np.int64).reshape((-1,) + (1,) * (x.ndim - 1)), x, 0.0)


def pool_varlen_lens(l):
    """vm_conv_fwd_pool_varlen: L, L - 1 (odd: the last position is dropped), past L, every tile edge t (the start of a ragged last tile
    is one) with t - 2 .. t + 3 -- the tile before it one row short and exactly full, the tile behind it dead, and with one pooled row
    (dq == 1), each at an even and an odd length --, one pooled row (2, 3) and none (0, 1)."""
    v = {l, l - 1, l + OVER, 0, 1, 2, 3}
    for t in range(TROWS, l, TROWS):
        v |= {t + d for d in (-2, -1, 0, 1, 2, 3)}
    assert all(x <= l or x == l + OVER for x in v)
    return sorted(v)


def conv1_edges(l, pool):
    """{kind: [32-position tile edges of that kind]}: `tile` an edge inside a whole chunk, `chunk` a 256-position chunk edge,
    `last-chunk` a tile edge inside the ragged last chunk, `last-tile` the start of the ragged last tile.  An edge counts where the
    pool group behind it still lies inside the window."""
    c0, s = (l - 1) // F1_CHUNK * F1_CHUNK, (l - 1) // F1_TILE * F1_TILE
    ok = lambda e: 0 < e and e + pool <= l // pool * pool
    out = {"tile": [e for e in range(F1_TILE, c0, F1_TILE) if e % F1_CHUNK and ok(e)],
           "chunk": [e for e in range(F1_CHUNK, l, F1_CHUNK) if ok(e)],
           "last-chunk": [e for e in range(c0 + F1_TILE, l, F1_TILE) if l % F1_CHUNK and ok(e)],
           "last-tile": [s] if l % F1_TILE and ok(s) else []}
    return out


def conv1_varlen_lens(l, pool):
    """vm_conv1_fused_fwd_varlen: L, L - 1 .. L - pool + 1 (with L: every lens % pool), past L, and for one edge e of every kind of
    conv1_edges: e (Lv on the edge: a fast tile next to a dead one, no boundary tile), e + 1 .. e + pool - 1 (the same Lv, every
    remainder), e - pool and e + pool (a boundary tile with one group missing / one group valid); one pooled row (pool) and none
    (pool - 1, 0)."""
    v = {l, l + OVER, pool, pool - 1, 0} | {l - r for r in range(1, pool)}
    for kind, edges in conv1_edges(l, pool).items():
        for e in edges[len(edges) // 2:len(edges) // 2 + 1]:            # the middle one
            v |= {e - pool, e + pool} | {e + r for r in range(pool)}
    assert all(x <= l or x == l + OVER for x in v)
    return sorted(v)


def spread(table, n, seed):
    """The table's lengths over n >= len(table) windows (the rest repeats it), shuffled: neighbouring windows differ, dead and live
    tiles interleave in the launch order."""
    assert n >= len(table), (n, len(table))
    v = np.array([table[i % len(table)] for i in range(n)], dtype=np.int32)
    return np.random.default_rng(seed).permutation(v)


def pool_tile_class(l, ln, q):
    """The branch of conv_nt2r_kernel / conv_nt3_kernel (EPI_FWD_POOL) that writes pooled row q of a window of length ln."""
    t0 = 2 * q // TROWS * TROWS
    d = (ln >> 1) - (t0 >> 1)
    if d <= 0:
        return "dead"                                                   # n2_pool_dead_tile
    return "live-full" if d >= (min(l - t0, TROWS) >> 1) else "live-partial"    # n2_tile_drain: dq == vq / dq < vq


def conv1_tile_class(l, pool, ln, q):
    """The branch of conv1_fused_fwd_kernel that writes pooled row q of a window of length ln."""
    t0 = q * pool // F1_TILE * F1_TILE
    lv = min(ln // pool, l // pool) * pool
    return "dead" if t0 >= lv else "fast" if t0 + F1_TILE <= lv else "boundary"


def varlen_note(lens, klass):
    """assert_exact's note for a (window, pooled row, channel) index: the window's lens value and the tile class of the row."""
    return lambda i: "lens[%d] = %d, %s tile" % (i[0], int(lens[i[0]]), klass(int(lens[i[0]]), i[1]))


# A host model of the masking: the tiles of a window in launch form, each dead, fast (conv1 only) or drained with dq valid rows.
# MASK_DEFECTS move one comparison, or the length it reads, in the direction that changes a result; the host file shows that each
# changes the expected output of a case of the tables.  MASK_NEUTRAL move the dead-tile and the fast-tile comparison the other way:
# the slower branch they then take masks per row and gives the same bits (asserted as well), so no output can see them.
MASK_DEFECTS = ("ceil", "positions", "dead-early", "dq+1", "dq-1", "lens-prev", "lens-next", "fast-early")
MASK_NEUTRAL = ("dead-late", "fast-late")


def mask_model(full, lens, l, pool, tile, fast, defect=None):
    """full (n, L // pool, c) unmasked, lens (n,) -> what the kernel stores.  tile: 254 (the GEMM kernels, fast = False) or 32 (conv1,
    fast = True).  Defects: `ceil` valid rows = ceil(lens / pool); `positions` lens compared with pooled rows (the shift / the `* POOL`
    forgotten); `dead-early` a tile with one valid row taken as dead (`<=` in `(t0 >> 1) < (lens >> 1)` read the harmful way: `t0 / pool +
    1 >= valid`); `dq+1` / `dq-1`; `lens-prev` / `lens-next` the neighbouring window's length; `fast-early` a tile one group short of
    full taken as fast.  Neutral: `dead-late` (`>` for `>=`: the drain runs with dq = 0), `fast-late` (`<` for `<=`: a full tile takes
    the boundary branch)."""
    n, lq, _ = full.shape
    out = np.full(full.shape, np.nan)
    for i in range(n):
        ln = int(lens[(i + {"lens-prev": -1, "lens-next": 1}.get(defect, 0)) % n])
        nv = -(-ln // pool) if defect == "ceil" else ln if defect == "positions" else ln // pool
        for t0 in range(0, l, tile):
            q0, whole = t0 // pool, (t0 + tile) // pool
            q1 = min(whole, lq)                                         # the pooled rows this tile owns
            if (q0 + 1 >= nv) if defect == "dead-early" else (q0 > nv) if defect == "dead-late" else (q0 >= nv):
                out[i, q0:q1] = 0.0
                continue
            top = min(nv, lq)
            if fast and ((whole <= top + 1) if defect == "fast-early" else (whole < top) if defect == "fast-late" else (whole <= top)):
                out[i, q0:q1] = full[i, q0:q1]
                continue
            dq = min(nv - q0, q1 - q0) + {"dq+1": 1, "dq-1": -1}.get(defect, 0)
            dq = max(min(dq, q1 - q0), 0)
            out[i, q0:q0 + dq] = full[i, q0:q0 + dq]
            out[i, q0 + dq:q1] = 0.0
    assert not np.isnan(out).any(), "a pooled row no tile writes"
    return out


def pool_affine(l, c):
    """test_fwd_pool's grid: scale +-{0.5, 1, 2, 4}, integer shift."""
    r = np.random.default_rng(l + c)
    return r.choice([0.5, 1.0, 2.0, 4.0], c) * r.choice([-1.0, 1.0], c), r.integers(-3, 4, c).astype(np.float64)


def pool_forward(x, w, b, scale, shift, dt):
    """vm_conv_fwd_pool in float64: max over the pair of scale * store(relu(conv + b)) + shift, unrounded."""
    y = store(np.maximum(conv_same(x, w) + b, 0.0), dt) * scale + shift
    q = x.shape[1] // 2
    return np.maximum(y[:, 0:2 * q:2], y[:, 1:2 * q:2])


class PoolVarlenCase:
    """vm_conv_fwd_pool_varlen on `small` operands: x (n, L, c_in) zero at and past lens[n], full (n, L // 2, c_out) the unmasked pooled
    tensor before its storage rounding (outputs pass 256: bf16 rounds them), want(dt) the masked, stored one."""

    def __init__(self, shape):
        n, l, cin, cout = shape
        self.shape = shape
        r = np.random.default_rng([n, l, cin, cout, 11])
        self.lens = spread(pool_varlen_lens(l), n, l + cin)
        self.x_raw = _ints(r, (n, l, cin), 1, 0.25)
        self.x = zero_past(self.x_raw, self.lens)
        self.w, self.b = _ints(r, (3, cin, cout), 1, 0.25), _ints(r, (cout,), 3)
        self.scale, self.shift = pool_affine(l, cout)
        require_exact_sums(conv_same(np.abs(self.x_raw), np.abs(self.w)) + np.abs(self.b), 1.0, "masked forward")
        z = np.maximum(conv_same(self.x, self.w) + self.b, 0.0)
        assert exact_in(z, "bf16") and exact_in(z * self.scale + self.shift, "f32")     # z is stored unrounded; the fma is exact
        self.full = pool_forward(self.x, self.w, self.b, self.scale, self.shift, "f32")

    def want(self, dt):
        return mask_rows(store(self.full, dt), self.lens, 2)

    def alone(self, i):
        """Window i truncated to its own length and run alone: (min(lens, L) // 2, c_out)."""
        ln = min(int(self.lens[i]), self.shape[1])
        if ln == 0:
            return np.zeros((0, self.shape[3]))
        return pool_forward(self.x_raw[i:i + 1, :ln], self.w, self.b, self.scale, self.shift, "f32")[0]

    def note(self):
        return varlen_note(self.lens, lambda ln, q: pool_tile_class(self.shape[1], ln, q))


@functools.lru_cache(maxsize=3)
def pool_varlen_case(shape):
    return PoolVarlenCase(tuple(shape))


def conv1_affine(l, f, pool):
    """test_conv1_fused_fwd's mode-1 grid."""
    r = np.random.default_rng(l + f + pool)
    return r.choice([0.5, 1.0, 2.0, 4.0], f) * r.choice([-1.0, 1.0], f), r.integers(-3, 4, f).astype(np.float64)


def conv1_forward(x, w, b, scale, shift, pool):
    """Mode 1 of vm_conv1_fused_fwd in float64, unrounded: fma(pool extreme by sign(scale) of relu(conv + b), scale, shift)."""
    return pool_extreme(np.maximum(conv32(x, w) + b, 0.0), scale, pool) * scale + shift


class Conv1VarlenCase:
    """vm_conv1_fused_fwd_varlen: a waveform (n, L) zero at and past lens[n], `small` or `lo-x` (a + b * 2^-9: bf16 storage needs x_lo *
    w_hi), filters and bias as Conv1Case `small`; full (n, L // pool, F) unmasked and unrounded."""

    def __init__(self, shape, regime, pool):
        n, l, f = shape
        self.shape, self.pool = shape, pool
        r = np.random.default_rng([n, l, f, pool, sum(map(ord, regime))])
        self.lens = spread(conv1_varlen_lens(l, pool), n, l + f + pool)
        self.x_raw = _lo_operand(r, (n, l)) if regime == "lo-x" else _ints(r, (n, l), 1, 0.25)
        assert regime in CONV1_VARLEN_REGIMES and exact_in(self.x_raw, "f16")
        self.x = zero_past(self.x_raw, self.lens)
        self.w, self.b = _ints(r, (32, 1, f), 1, 0.25), _ints(r, (f,), 3)
        self.scale, self.shift = conv1_affine(l, f, pool)
        grid = 2.0 ** -9 if regime == "lo-x" else 1.0
        require_exact_sums(conv32(np.add(*map(np.abs, bf16_halves(self.x_raw))), np.abs(self.w)) + np.abs(self.b), grid, "masked conv1")
        self.full = conv1_forward(self.x, self.w, self.b, self.scale, self.shift, pool)
        assert exact_in(self.full, "f32")                               # the fma is exact: one rounding, to storage

    def want(self, dt):
        return mask_rows(store(self.full, dt), self.lens, self.pool)

    def alone(self, i):
        ln = min(int(self.lens[i]), self.shape[1])
        if ln == 0:
            return np.zeros((0, self.shape[2]))
        return conv1_forward(self.x_raw[i:i + 1, :ln], self.w, self.b, self.scale, self.shift, self.pool)[0]

    def note(self):
        return varlen_note(self.lens, lambda ln, q: conv1_tile_class(self.shape[1], self.pool, ln, q))


@functools.lru_cache(maxsize=4)
def conv1_varlen_case(shape, regime, pool):
    return Conv1VarlenCase(tuple(shape), regime, pool)


def unreached_from(ln, l, kind, pool=2):
    """The first input position no valid output's taps reach (the reference's own tap range): the k = 3 conv's last valid row 2 * (ln //
    2) - 1 reads one position further; conv1's last valid position Lv - 1 reads 16 further (pad_wave: 15 before, 16 after)."""
    ln = min(ln, l)
    return 2 * (ln // 2) + 1 if kind == "pool" else ln // pool * pool + 16


# ---- the hand-off: conv1 -> conv + pool -> global max over one masked bucket against each recording alone --------------------------------
CHAIN_SHAPE = (12, 800, 128, 128)       # (n, L, F, c_out): L / 2 = 400 = 254 + 146 and L / 4 = 200 are both served by the second layer


def chain_lens(n, l, pool):
    """Mixed lengths of one bucket: full, odd ones, one pooled row at the end (2 pool, 2 pool + 1: lens // pool // 2 == 1; 4 pool - 1: an
    odd row count at the second layer), the second layer's tile edge where the window reaches it, the rest drawn."""
    v = [l, l - 1, l - pool - 1, 2 * pool, 2 * pool + 1, 4 * pool - 1]
    e = TROWS * pool
    if e + 2 * pool + 1 <= l:
        v += [e - 1, e, e + 1, e + 2 * pool + 1]
    r = np.random.default_rng(l + pool)
    v += [int(k) for k in r.integers(2 * pool, l, n - len(v))]
    return np.array(v, dtype=np.int32)


class ChainCase:
    """vm_conv1_fused_fwd_varlen -> vm_conv_fwd_pool_varlen (lens // pool) -> vm_global_maxpool_fwd_varlen (lens // pool // 2) in `dt`
    storage.  Scales +-{0.5, 1, 2}, integer shifts; the first layer's STORED outputs are the second layer's operands, and the
    precondition is asserted on them."""

    def __init__(self, pool, dt):
        n, l, f, cout = CHAIN_SHAPE
        self.pool, self.dt = pool, dt
        r = np.random.default_rng([n, l, f, cout, pool])
        self.lens = chain_lens(n, l, pool)
        self.x_raw = _ints(r, (n, l), 1, 0.25)
        self.x = zero_past(self.x_raw, self.lens)
        self.w1, self.b1 = _ints(r, (32, 1, f), 1, 0.25), _ints(r, (f,), 3)
        self.w2, self.b2 = _ints(r, (3, f, cout), 1, 0.25), _ints(r, (cout,), 3)
        (self.s1, self.h1), (self.s2, self.h2) = _affine(r, 1, f), _affine(r, 1, cout)
        self.s1, self.h1, self.s2, self.h2 = self.s1[0], self.h1[0], self.s2[0], self.h2[0]
        # the bucket as the three launches see it, every precondition on the way
        require_exact_sums(conv32(np.abs(self.x_raw), np.abs(self.w1)) + np.abs(self.b1), 1.0, "chain: conv1")
        y1 = conv1_forward(self.x, self.w1, self.b1, self.s1, self.h1, pool)
        assert exact_in(y1, "f32")
        self.act1 = mask_rows(store(y1, dt), self.lens, pool)
        g = dyadic_grid(self.act1)
        require_exact_sums(conv_same(np.abs(self.act1), np.abs(self.w2)) + np.abs(self.b2), g, "chain: conv2 on conv1's stored outputs")
        z2 = store(np.maximum(conv_same(self.act1, self.w2) + self.b2, 0.0), dt)
        assert exact_in(z2 * self.s2 + self.h2, "f32") and np.abs(z2 * self.s2 + self.h2).max() < 60000
        self.lens1 = self.lens // pool
        self.act2 = mask_rows(store(pool_forward(self.act1, self.w2, self.b2, self.s2, self.h2, dt), dt), self.lens1, 2)
        self.lens2 = self.lens1 // 2
        assert self.lens2.min() == 1

    def alone(self, i):
        """Recording i alone in float64: truncate, k = 32 conv, floor-pool, affine, round to storage, k = 3 SAME conv over its own rows
        only, floor-pool, round, first maximum and its row.  -> (act1, act2, gmax, gidx)."""
        ln, dt = int(self.lens[i]), self.dt
        a1 = store(conv1_forward(self.x_raw[i:i + 1, :ln], self.w1, self.b1, self.s1, self.h1, self.pool), dt)
        a2 = store(pool_forward(a1, self.w2, self.b2, self.s2, self.h2, dt), dt)
        return a1[0], a2[0], a2[0].max(0), a2[0].argmax(0).astype(np.int32)


@functools.lru_cache(maxsize=4)
def chain_case(pool, dt):
    return ChainCase(pool, dt)


# ---- the comparator ------------------------------------------------------------------------------------------------------------------
LAYOUTS ={"nlc": ("window", "position", "channel"), "kio": ("tap", "c_in", "c_out"), "nc": ("window", "channel"),
           "tkc": ("tower", "tap", "channel"), "c": ("channel",), "k1f": ("filter tap", "one", "filter"), "tc": ("tower", "channel"),
           "tokc": ("tower", "c_out", "tap", "c_in")}


def _describe(idx, layout, shape):
    names = LAYOUTS[layout]
    s = ", ".join("%s %d" % (nm, i) for nm, i in zip(names, idx))
    if "position" in names:
        pos, l = int(idx[names.index("position")]), shape[names.index("position")]
        s += " [128-tile %d, 254-tile %d, %d from the window edge]" % (pos // 128, pos // 254, min(pos, l - 1 - pos))
    return s


def assert_exact(got, want, layout, neg_zero=False, what="", note=None):
    """Bit-pattern equality of `got` (torch tensor, any storage type) with the float64 reference `want`, which must itself be exact in
    got's type.  neg_zero: -0.0 and +0.0 compare equal -- the one allowed difference, for outputs of a ReLU (max(-0.0, 0) may keep the
    sign) and products with an exactly zero factor; everything else is compared as bits.  On a mismatch: the count, the first and the
    worst element by (window, position, channel), their 128- and 254-position tile indices and the distance from the window edge, and
    what `note(index)` adds about an element (the length-masked cases: the window's `lens` value and the class of the element's tile)."""
    got = torch.as_tensor(got).detach().cpu().contiguous()
    want64 = np.asarray(want, dtype=np.float64) + 0.0
    assert tuple(got.shape) == want64.shape, (tuple(got.shape), want64.shape)
    wt = torch.as_tensor(want64).to(got.dtype)
    assert np.array_equal(wt.to(torch.float64).numpy(), want64), "the reference is not exact in %s" % got.dtype
    iv = INT_VIEW[got.dtype]
    gb, wb = got.view(iv).numpy(), wt.contiguous().view(iv).numpy()
    bad = gb != wb
    if neg_zero:
        bad &= ~((got.to(torch.float64).numpy() == 0.0) & (want64 == 0.0))
    if not bad.any():
        return
    g64 = got.to(torch.float64).numpy()
    idx = np.argwhere(bad)
    diff = np.where(bad, np.abs(np.nan_to_num(g64, nan=np.inf) - want64), -1.0)
    worst = np.unravel_index(int(np.argmax(diff)), diff.shape)
    first = tuple(idx[0])
    more = (lambda i: " {%s}" % note(tuple(int(v) for v in i))) if note is not None else (lambda i: "")
    raise AssertionError("%s: %d of %d elements differ; first at (%s%s): got %r, want %r; worst at (%s%s): got %r, want %r" % (
        what or layout, len(idx), bad.size, _describe(first, layout, bad.shape), more(first), g64[first], want64[first],
        _describe(worst, layout, bad.shape), more(worst), g64[worst], want64[worst]))
