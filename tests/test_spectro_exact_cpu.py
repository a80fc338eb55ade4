"""Host-side checks of tests/spectro_exact.py (the helper of tests/test_gpu_spectro_exact.py): every generated case meets its
preconditions and census from the inputs and the float64 reference alone, fp32 arithmetic in two different summation orders reproduces
the reference bit for bit, and the deliberately wrong evaluations -- a neighbouring clip's band, a tap at t - 1 instead of t + 1, km and
kt exchanged; a dropped last k-step, a dropped bl * xh product, late frames, exchanged bins, a missing wave -- are rejected."""
import numpy as np
import pytest
import torch

from tests import spectro_exact as X
from tests.gemm_exact import assert_exact, rounding_census, store

CONV_SHAPES = X.MFMA_SHAPES + X.VALU_SHAPES + X.VALU_F32_SHAPES + X.WPB_MFMA_SHAPES + X.WPB_VALU_SHAPES + X.WGRAD_TAIL_SHAPES
CONV_CASES = [(s, reg, kl) for s in CONV_SHAPES for reg in X.CONV_REGIMES for kl in (("any",) if reg in ("small", "wide") else X.DT16)]


@pytest.mark.parametrize("shape,regime,klass", CONV_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_conv2d_cases_meet_their_preconditions(shape, regime, klass):
    """Constructing a case asserts: sum |product| + |bias| < 2^24 grid units with the hi and lo parts as separate products (27 in split
    mode), operands whole in their two planes, the fourth product zero, a channel negative everywhere.  Here: the statistics'
    preconditions, the census of rounded values, exact ties and non-zero low planes, and the three planted defects."""
    n, M, L, C = shape
    c = X.Conv2dCase(shape, regime, klass)
    assert c.head_fwd < X.LIMIT
    for dt in (X.DT16 if klass == "any" else (klass,)):
        for split in (False, True):
            zs, zl, ss, sq, ok_sq = c.forward(dt, split)              # asserts the sums' precondition; `small`: the squares' too
            assert not zs[..., c.c_neg].any() and not zl[..., c.c_neg].any() and not ss[:, c.c_neg].any()
            if regime == "small":
                assert ok_sq and np.array_equal(zs, c.z) and not zl.any()
        frac, ties = rounding_census(c.z, dt)
        if regime != "small":
            zs, zl, _, _, _ = c.forward(dt, True)
            assert ties >= 1 and frac > 0.05 and (zl != 0).mean() > 0.05 and np.array_equal(zs + zl, c.z), (frac, ties)
        if regime in ("lo-x", "lo-w"):
            assert not np.array_equal(c.one_plane(dt), c.z)           # the one-plane entry point computes something else there
    # the planted defects: every one moves the reference by at least a grid unit -- in every window, or for the clip mask in exactly
    # the windows on either side of a boundary between two clips
    diff = {w: (c.wrong(w) != c.z).reshape(n * M, -1).any(1) for w in ("clip", "tap", "swap")}
    assert diff["tap"].any() and diff["swap"].any() and (n == 1 or diff["clip"].any())
    if L >= 33:
        edge = np.zeros((n, M), bool)
        edge[1:, 0] = True
        edge[:-1, -1] = True
        assert diff["tap"].all() and diff["swap"].all() and np.array_equal(diff["clip"], edge.ravel())
    for w in ("clip", "tap", "swap"):
        if diff[w].any():
            assert np.abs(c.wrong(w) - c.z)[c.wrong(w) != c.z].min() >= c.grid


def _f32_two_orders(terms, bias):
    """The sum of `terms` (float64 arrays) + bias in fp32, forward from the bias and backward with the bias last."""
    t32 = [t.astype(np.float32) for t in terms]
    a = np.broadcast_to(bias.astype(np.float32), t32[0].shape).copy()
    for t in t32:
        a = a + t
    b = np.zeros_like(t32[0])
    for t in reversed(t32):
        b = b + t
    return a, b + bias.astype(np.float32)


@pytest.mark.parametrize("dt", X.DT16)
@pytest.mark.parametrize("regime", X.CONV_REGIMES)
@pytest.mark.parametrize("shape", [(2, 3, 37, 32), (2, 2, 140, 40)])
def test_conv2d_fp32_in_two_orders_is_the_reference(shape, regime, dt):
    """The 27 products of the split entry point (w_hi in, w_hi in_lo, w_lo in; nine where the low planes are zero), each rounded to fp32
    and summed in fp32 in two orders: both are the float64 reference bit for bit; so is the weight gradient over positions."""
    n, M, L, C = shape
    c = X.conv2d_case(shape, regime, dt)
    (xh, xl), (wh, wl) = X.halves(c.x, dt), X.halves(c.w, dt)
    zero = np.zeros(C)
    terms = []
    for xx, ww in ((xh, wh), (xl, wh), (xh, wl)):
        for kt in range(3):
            for km in range(3):
                w1 = np.zeros_like(ww)
                w1[kt, km] = ww[kt, km]
                terms.append(X.conv2d_first(xx, w1, zero))
    assert all(np.array_equal(t.astype(np.float32).astype(np.float64), t) for t in terms)      # every product is an fp32 number
    a, b = _f32_two_orders(terms, c.b)
    assert np.array_equal(a.astype(np.float64), c.pre) and np.array_equal(b.astype(np.float64), c.pre)
    assert not X.conv2d_first(xl, wl, zero).any()                                               # the fourth product
    if regime == "small":
        du32, gw = c.du.astype(np.float32), c.gw(3)
        p = np.zeros((n, M + 2, L + 2), np.float32)
        p[:, 1:-1, 1:-1] = c.x
        for order in (1, -1):
            acc = np.zeros((3, 3, C), np.float32)
            for t in range(L)[::order]:
                for kt in range(3):
                    for km in range(3):
                        acc[kt, km] += np.einsum("nm,nmc->c", p[:, km:km + M, kt + t], du32[:, :, t])
            assert np.array_equal(acc.astype(np.float64), gw)


@pytest.mark.parametrize("shape,regime,klass", [(s, reg, kl) for s, reg, kl in CONV_CASES if s in X.MFMA_SHAPES[:2]],
                         ids=lambda v: str(v).replace(" ", ""))
def test_comparator_rejects_the_wrong_convolutions(shape, regime, klass):
    for dt in (X.DT16 if klass == "any" else (klass,)):
        c = X.conv2d_case(shape, regime, dt)
        n, M, L, C = shape
        want = store(c.z, dt).reshape(n * M, L, C)
        t = lambda a: torch.as_tensor(store(a, dt).reshape(n * M, L, C)).to(X.STORE[dt])
        assert_exact(t(c.z), want, "nlc")
        for w in ("clip", "tap", "swap"):
            if w == "clip" and n == 1:
                continue
            with pytest.raises(AssertionError, match="window"):
                assert_exact(t(c.wrong(w)), want, "nlc")
        one = want.copy()
        one[n * M - 1, L - 1, C - 1] += X.ulp_of(max(one[n * M - 1, L - 1, C - 1], 1.0), dt)     # one element, one storage ulp
        with pytest.raises(AssertionError, match="1 of"):
            assert_exact(t(one), want, "nlc")


def test_shape_tables_reach_what_they_claim():
    """The loop edges the tables' comments name, recomputed from the launch arithmetic of csrc/spectro.hip."""
    for n, M, L, C in X.WPB_MFMA_SHAPES + X.WPB_VALU_SHAPES:
        nw = n * M
        blocks = min(nw, 2048)
        wpb = -(-nw // blocks)
        assert wpb == 2 and -(-nw // wpb) == 1025
    assert [n * M % 2 for n, M, _, _ in X.WPB_MFMA_SHAPES] == [0, 1] and X.WPB_MFMA_SHAPES[1][1] % 2 == 1     # a last workgroup with one window; clips straddled
    assert sorted({c // 32 for _, _, _, c in X.MFMA_SHAPES}) == [1, 2, 3, 4]
    idle = {c: 256 - (256 // (c // 8)) * (c // 8) for _, _, _, c in X.VALU_SHAPES + X.VALU_F32_SHAPES}
    assert idle == {24: 1, 40: 1, 120: 1, 8: 0}
    assert [64 % (c // 8) != 0 for c in (24, 40, 120, 8)] == [True, True, True, False]
    assert [c for c in range(8, 129, 8) if 64 % (c // 8)] == [24, 40, 48, 56, 72, 80, 88, 96, 104, 112, 120]
    n, M, L, C = X.MFMA_SHAPES[0]
    assert n * M * -(-L // 128) == 6 and L % 32 != 0
    assert X.MFMA_SHAPES[1][2] == 129 and X.MFMA_SHAPES[2][1] % 2 == 1 and X.MFMA_SHAPES[3][2] % 128 == 0 and X.MFMA_SHAPES[4][1] == 1
    for _, _, L, _ in X.WGRAD_TAIL_SHAPES:
        assert L % 32 != 0
    assert sorted({n_mels // 32 for *_, n_mels, _, reg in X.stft_cases() if reg == "exact"}) == [1, 2, 3, 4]
    assert {(n_mels, i16) for *_, n_mels, i16, reg in X.stft_cases()} == {(m, b) for m in X.N_MELS for b in (False, True)}
    assert X.lds_bytes(512, 32) == (65664, 66560) and X.lds_bytes(497, 32)[1] == 66560 and max(X.lds_bytes(496, 128)) <= 65536
    assert [(-(-w // 16) * 16) for w, _, _ in X.STFT_GEOMETRIES] == [400, 416, 48, 16, 16, 496]


@pytest.mark.parametrize("dt", X.DT16)
@pytest.mark.parametrize("regime", ("small", "lo-x", "lo-w"))
@pytest.mark.parametrize("shape,cpt", [(s, 1) for s in X.MFMA_SHAPES[:4]] + [((2, 5, 298, 96), 2)])
def test_boundary_cases_meet_their_preconditions(shape, cpt, regime, dt):
    """Constructing asserts that the affine and the dropout product are fp32 numbers.  Census: tied position pairs and tied band pairs
    with positive values, a channel with scale * drop < 0, a dropped channel; the never-written entries hold the sentinel."""
    n, M, L, C = shape
    cs2 = 3 * C + 8
    b = X.Boundary(X.conv2d_case(shape, regime, dt), dt, cpt, cs2)
    assert b.tied_positions >= 1 and b.tied_bands >= 1, (b.tied_positions, b.tied_bands)
    assert (b.scale[:, b.c_inv] * b.drop[:, b.c_inv].max() < 0).all() and not b.drop[:, b.c_drop].any()
    assert regime == "small" or b.rounded > 0.01
    Lq, Mo = L // 2, M // 2
    assert (b.q[:, 0] == X.SENTINEL).all() and (b.q[:, -1] == X.SENTINEL).all() and (b.q[:, 1:-1] != X.SENTINEL).all()
    xs = b.xs.reshape(n, Mo, Lq + 2, cs2)
    assert (xs[..., 3 * C:] == X.SENTINEL).all() and (xs[:, 0, :, :C] == X.SENTINEL).all() and (xs[:, -1, :, 2 * C:3 * C] == X.SENTINEL).all()
    assert (xs[:, :, 1:-1, C:2 * C] != X.SENTINEL).all() and (xs[:, :, 0] == X.SENTINEL).all()
    assert store(b.q, dt).tobytes() == b.q.tobytes() and store(b.xs, dt).tobytes() == b.xs.tobytes()


@pytest.mark.parametrize("shape", X.FOLD_SHAPES)
def test_fold_pool_cases_meet_their_preconditions(shape):
    c = X.FoldPoolCase(shape)
    n, M, L, C, Cs = shape
    assert c.ties > 0 and c.dq.any() and (M % 2 == 0 or not c.dq[:, -1].any())
    assert np.array_equal(c.dq.reshape(n, M, L, C).sum(2).reshape(n * M, C), c.s0)


# ---- the front end ---------------------------------------------------------------------------------------------------------------------
ALL_STFT = X.stft_cases() + [X.STFT_LDS_GEOMETRY + (128, False, "exact"), X.STFT_LDS_GEOMETRY + (64, True, "exact")]


@pytest.mark.parametrize("case", ALL_STFT, ids=lambda v: str(v).replace(" ", ""))
def test_stft_cases_meet_their_preconditions(case):
    """Constructing asserts: sum |x| |b| with the f16 halves as separate products, and in the exact regime P and S + floor, below 2^24
    units.  Here: the flagged share of both 16-bit types stays below 1 %, and every wrong evaluation leaves the bound at EVERY element
    whose mel sum it changes."""
    win, hop, T, n_mels, i16, regime = case
    c = X.StftCase(*case)
    assert c.ref.shape == (2, T, n_mels) and np.isfinite(c.ref).all()
    for dt in X.DT16:
        want, alt, flagged = c.stored(dt)
        assert flagged.mean() < 0.01, (dt, flagged.mean())
        d = np.abs(alt - want)[flagged]
        assert (d > 0).all() and (d <= X.ulp_of(np.maximum(np.abs(alt), np.abs(want)), dt)[flagged]).all()      # one storage ulp
    variants = ["late", "bins", "wave"] + (["odd-tail"] if win % 2 else []) + (["no-bl-xh"] if regime == "lo-b" else [])
    for v in variants:
        S, lg = c.wrong(v)
        touched = S != c.S
        assert touched.any(), v
        assert (np.abs(lg - c.ref)[touched] > c.tol32()[touched]).all(), v
        with pytest.raises(AssertionError, match="outside the bound"):
            X.check_log_f32(lg, c, v)
    assert X.check_log_f32(c.ref.astype(np.float32), c) <= 0.5
    for dt in X.DT16:
        assert X.check_log_stored(store(c.ref, dt), c, dt) < 0.01
        with pytest.raises(AssertionError, match="differ"):
            X.check_log_stored(store(c.wrong("wave")[1], dt), c, dt)


def _chunked(a, b, order):
    """a @ b in fp32, the K axis summed one slice at a time in the given order."""
    k = a.shape[-1]
    acc = np.zeros(a.shape[:-1] + (b.shape[1],), np.float32)
    for i in range(k)[::order]:
        acc = acc + a[..., i:i + 1] * b[i][None, :]
    return acc


@pytest.mark.parametrize("case", [c for c in X.stft_cases() if c[-1] == "exact" and c[0] in (401, 37, 2)], ids=lambda v: str(v).replace(" ", ""))
def test_stft_fp32_in_two_orders_is_the_reference(case):
    """re, im, P and S + floor in fp32 with the sample axis and the bin axis summed forward and backward, and the f16 kernel's form
    (samples x 256, power x 2^-16): all equal to float64 bit for bit."""
    win, hop, T, n_mels, i16, regime = case
    c = X.StftCase(*case)
    fr = X.frames_of(c.raw, win, hop, T)
    for order in (1, -1):
        for scale in (1.0, 256.0):
            X32 = _chunked((fr * scale).astype(np.float32), c.basis.astype(np.float32), order)
            re, im = X32[..., :256], X32[..., 256:]
            P = ((re * re + im * im) * np.float32(1.0 / (scale * scale))).astype(np.float32)
            S = _chunked(P, c.melw.astype(np.float32), -order) + np.float32(c.floor)
            assert S.dtype == np.float32 and np.array_equal(S.astype(np.float64), c.S + c.floor)


def test_references_are_the_oracle():
    """The two float64 references of spectro_exact.py against the CPU oracle, which is written independently of them (numpy.fft; torch
    conv2d): logmel() with the shipped basis and mel matrix is logmel_features, conv2d_first is a SAME 3 x 3 cross-correlation."""
    from oracle import voicemap_oracle as O
    from voicemap_amd import spectro as S
    r = np.random.default_rng(3)
    raw = r.normal(0, 0.1, (2, 400 + 160 * 4 + 7))
    fr = X.frames_of(raw, 400, 160, 5)
    _, got = X.logmel(fr, S.dft_basis().astype(np.float64), S.mel_filterbank(64).astype(np.float64), 1e-6)
    assert np.abs(got - O.logmel_features(raw, n_mels=64)).max() < 1e-5          # (the shipped basis is fp32)
    c = X.conv2d_case((2, 3, 37, 32), "small", "f16")
    w = torch.tensor(c.w).permute(2, 1, 0)[:, None]                               # (C, 1, km, kt)
    ref = torch.nn.functional.conv2d(torch.tensor(c.x)[:, None], w, torch.tensor(c.b), padding=1)      # (n, C, M, L)
    assert np.array_equal(ref.permute(0, 2, 3, 1).numpy(), c.pre)
