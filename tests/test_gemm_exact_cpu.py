"""Host-side checks of tests/gemm_exact.py (the helper of tests/test_gpu_conv_exact.py): every generated case meets its precondition,
an fp32 evaluation in another summation order reproduces the float64 reference exactly, and the comparator catches the defects a
Frobenius ratio at the parity suite's tolerances lets through."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gemm_exact as G
from tests.gemm_exact import assert_exact

# every (shape, regime, operand class) any test of the device file constructs: its own tables
ALL_CONV = sorted({(reg, G.case_key(dt, reg)) + tuple(s) for dt, reg, *s in G.ALL_CONV_CASES})


def rel_err(a, b):      # tests/gpu_util.py's, which a host-only test cannot import (it loads the HIP library's binding)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("regime,dt,n,l,cin,cout", ALL_CONV)
def test_conv_cases_meet_their_preconditions(regime, dt, n, l, cin, cout):
    """Constructing a case asserts: sum |product| (+ |bias|) < 2^24 grid units for every forward, dgrad and wgrad output; operands exact
    in the storage type; `small` outputs unrounded in every type with exact statistics; `wide` outputs >= 0.5 % rounded, >= 100 ties."""
    c = G.ConvCase((n, l, cin, cout), regime, dt)
    assert max(c.head_fwd, c.head_dgrad, c.head_wgrad) < G.LIMIT
    for d in (("f32", "f32s", "bf16", "f16") if regime == "small" else (dt,)):
        z, ss, sq, ok_sq = c.forward(d)                    # asserts the precondition of the sum, and in `small` of the sum of squares
        assert regime != "small" or (ok_sq and np.array_equal(z, c.z))


def test_every_device_table_is_among_the_checked_cases():
    """Default dispatch, pinned fallbacks, wgrad variants, persistent loop, split plans, vm_conv_fwd_e / _pool and vm_conv_dgrad_bnred
    (small and wide, both 16-bit types) all draw from ALL_CONV; the tiny shapes keep their `wide` regime."""
    tables = (G.DEFAULT_CASES, G.FALLBACK_CASES, G.WGRAD_VARIANT_CASES, G.PERSISTENT_CASES, G.SPLIT_CASES, G.FWD_E_CASES, G.FWD_POOL_CASES,
              [c[:6] for c in G.BNRED_CASES])
    for table in tables:
        assert table and all((reg, G.case_key(dt, reg)) + tuple(s) in ALL_CONV for dt, reg, *s in table)
    for shape in G.FUSED_SHAPES + [s[:4] for s in G.BNRED_SHAPES] + [(2, 5, 24, 8), (1, 62, 64, 64)]:
        for k in ("bf16", "f16"):
            assert ("wide", k) + tuple(shape) in ALL_CONV


def test_reference_is_the_oracle_convolution():
    from oracle import voicemap_oracle as O
    c = G.conv_case((2, 300, 128, 256), "wide", "f16")
    T = lambda a: torch.tensor(a, dtype=torch.float64)
    assert np.array_equal(O.conv1d_same_relu(T(c.x), T(c.w), T(c.b)).numpy(), c.z)


def test_persistent_shapes_pass_the_grid_cap():
    """More (window, 128-position tile) groups than launch_nt's 512 workgroups; 520 % 8 == 0 (XCD order), 515 % 8 != 0 (sequential)."""
    groups = sorted({n * -(-l // 128) for n, l, _, _ in G.PERSISTENT_SHAPES})
    assert groups == [515, 520]


@pytest.mark.parametrize("shape", G.SPLIT_SHAPES)
def test_split_cases_meet_their_preconditions(shape):
    n, wpt, l, cin, cout = shape
    c = G.ConvCase((n, l, cin, cout), "small", "f32")
    f = G.FoldFactors(shape, c.x, c.du_w)           # asserts the precondition of the folded sum and of dsum
    assert set(np.abs(f.scale).ravel()) <= {0.5, 1.0, 2.0} and (f.scale < 0).any() and np.array_equal(f.shift, np.round(f.shift))
    # the definition: the layer's input is y = scale_t * x + shift_t inside the window, 0 in the padding
    y = (c.x.reshape(n // wpt, wpt, l, cin) * f.scale[:, None, None, :] + f.shift[:, None, None, :]).reshape(n, l, cin)
    assert np.array_equal(G.conv_wgrad(y, c.du_w), f.gw)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", G.FUSED_SHAPES)
def test_fold_cases_meet_their_preconditions(shape, dt):
    f = G.FoldCase(shape, dt)
    assert (f.gamma < 0).any() and (f.gamma == 0).any() and not np.array_equal(f.scale[0], f.scale[1])
    if dt == "f16":
        assert np.array_equal(f.ctr, np.round(f.ctr)) and (f.ctr > 0).any()


@pytest.mark.parametrize("dt,regime,n,l,cin,cout,padded_a", G.BNRED_CASES)
def test_bnred_sums_meet_their_precondition(dt, regime, n, l, cin, cout, padded_a):
    """Both sum rows of vm_conv_dgrad_bnred (red_a is an integer in 0 .. 3) in both regimes and types: the device test asserts them
    wherever this holds, which is everywhere."""
    dx = G.store(G.conv_case((n, l, cin, cout), regime, dt).dx, dt)
    assert G.sums_exact(np.abs(dx).sum(1) * 3, 1.0)


@pytest.mark.parametrize("regime,dt", [("small", "f32"), ("wide", "bf16"), ("wide", "f16"), ("lo-w", "f16"), ("lo-x", "f16")])
@pytest.mark.parametrize("shape", G.CONV1_SHAPES + [G.CONV1_WGRAD_SHAPE] + G.CONV1_FUSED_SHAPES)
def test_conv1_cases_meet_their_preconditions(shape, regime, dt):
    c = G.Conv1Case(shape, regime, dt)
    if regime in ("small", "wide"):
        ok = c.stats(G.store(c.z, dt) if regime == "wide" else c.z)       # asserts the sum's precondition; `small`: the squares' too
        assert ok[2] and (regime == "wide" or ok[3])
    if regime == "lo-x":
        assert (c.z_xhi != c.z).mean() > 0.2         # dropping x_lo * w_hi is visible
    if regime == "lo-w":
        assert (c.z_hi != c.z).mean() > 0.2          # dropping the lo product is visible


@pytest.mark.parametrize("regime,dt", [("small", "f32"), ("wide", "bf16"), ("wide", "f16"), ("lo-x", "f32s"), ("lo-w", "f32s")])
def test_fp32_evaluation_in_shuffled_order_equals_float64(regime, dt):
    """fp32 arithmetic throughout, taps and 32-channel chunks in a shuffled order, the bias added last: array_equal to the float64
    reference -- forward (3 x 512 terms), dgrad and wgrad."""
    shape = (3, 520, 512, 256)
    c = G.ConvCase(shape, regime, dt)
    n, l, cin, cout = shape
    r = np.random.default_rng(0)
    f = np.float32
    xp, dp, w = G.pad1(c.x).astype(f), G.pad1(c.du_d).astype(f), c.w.astype(f)
    acc = np.zeros((n * l, cout), f)
    for j in r.permutation(3 * cin // 32):
        k, ch = j % 3, slice(32 * (j // 3), 32 * (j // 3) + 32)
        acc = acc + xp[:, k:k + l, ch].reshape(n * l, 32) @ w[k, ch]
    z = np.maximum(acc + c.b.astype(f), f(0)).reshape(n, l, cout)
    assert z.dtype == f and np.array_equal(z.astype(np.float64), c.z)
    acc = np.zeros((n * l, cin), f)
    for j in r.permutation(3 * cout // 32):
        k, ch = j % 3, slice(32 * (j // 3), 32 * (j // 3) + 32)
        acc = acc + dp[:, 2 - k:2 - k + l, ch].reshape(n * l, 32) @ w[k][:, ch].T
    assert np.array_equal(acc.reshape(n, l, cin).astype(np.float64), c.dx)
    gw = np.zeros((3, cin, cout), f)
    du = c.du_w.astype(f)
    for j in r.permutation(n * 5):                            # split-K over shuffled ranges of positions
        i, t0 = j // 5, (j % 5) * 104
        for k in range(3):
            gw[k] += xp[i, t0 + k:t0 + k + 104].T @ du[i, t0:t0 + 104]
    assert np.array_equal(gw.astype(np.float64), c.gw)


def test_split_bf16_products_need_both_cross_terms():
    """VM_F32S on the lo regimes: hi * hi + hi * lo + lo * hi is the exact product (lo * lo is identically zero), and leaving out the
    cross term the regime is named after changes the result."""
    for regime in ("lo-x", "lo-w"):
        c = G.ConvCase((2, 260, 32, 64), regime, "f32s")
        (xh, xl), (wh, wl) = G.bf16_halves(c.x), G.bf16_halves(c.w)
        assert not (G.conv_same(np.abs(xl), np.abs(wl))).any()
        full = G.conv_same(xh, wh) + G.conv_same(xh, wl) + G.conv_same(xl, wh)
        assert np.array_equal(np.maximum(full + c.b, 0.0), c.z)
        assert not np.array_equal(np.maximum(G.conv_same(xh, wh) + c.b, 0.0), c.z)


# ---- the comparator against the Frobenius ratio: why the device file exists -----------------------------------------------------------------
BIG = (16, 1030, 256, 256)
TOL_BF16 = 1e-2                             # tests/test_gpu_kernels.py's tolerance for bf16 storage


@pytest.fixture(scope="module")
def big():
    return G.ConvCase(BIG, "small", "f32")


def _mutations(c):
    """The three defects of a tiling bug, applied to the correct forward output: one element zeroed, tap 0 dropped at one position of
    one window (a window-edge tap), one whole position row written from its neighbour."""
    z = c.z
    zero = z.copy()
    i = np.unravel_index(int(np.argmax(z)), z.shape)
    zero[i] = 0.0
    tap = z.copy()
    pos = 512                                           # first position of a 128-tile: tap 0 reads the previous tile's last row
    tap[7, pos] = np.maximum(G.conv_same(c.x[7:8], c.w)[0, pos] + c.b - c.x[7, pos - 1] @ c.w[0], 0.0)
    row = z.copy()
    row[3, 254] = z[3, 253]
    return {"element zeroed": zero, "tap 0 dropped at one position": tap, "position row from its neighbour": row}


@pytest.mark.parametrize("defect", ["element zeroed", "tap 0 dropped at one position", "position row from its neighbour"])
def test_comparator_catches_what_the_ratio_passes(big, defect):
    bad = _mutations(big)[defect]
    assert not np.array_equal(bad, big.z)
    for dt in ("bf16", "f16"):
        got = torch.as_tensor(bad).to(G.STORE[dt])
        if dt == "bf16":
            assert rel_err(got.to(torch.float64).numpy(), big.z) < TOL_BF16       # the parity suite's check passes the defect ...
        with pytest.raises(AssertionError, match="elements differ; first at \\(window"):
            assert_exact(got, G.store(big.z, dt), "nlc", neg_zero=True)           # ... the exact one names its coordinates
        assert_exact(torch.as_tensor(big.z).to(G.STORE[dt]), G.store(big.z, dt), "nlc", neg_zero=True)


def test_comparator_catches_two_products_missing_from_one_wgrad_element():
    """A split-K edge that skips two (position, tap) products of one grad_w element, here two products of one grid unit each among
    operands of the `wide` regime: wgrad's 2e-5 on the Frobenius ratio passes it, the exact comparison names the element."""
    c = G.conv_case(BIG, "wide", "f16")
    gw = c.gw.copy()
    k, ci, co = 2, 100, 37
    prod = c.x[:, 1:, ci] * c.du_w[:, :-1, co]              # tap 2 of position t reads x[t + 1]
    idx = np.argwhere(prod == 1.0)[:2]
    assert len(idx) == 2
    gw[k, ci, co] -= 2.0
    assert rel_err(gw, c.gw) < 2e-5
    with pytest.raises(AssertionError, match="1 of 196608 elements differ; first at \\(tap 2, c_in 100, c_out 37\\)"):
        assert_exact(torch.as_tensor(gw).to(torch.float32), c.gw, "kio")


def test_comparator_zero_signs_and_report():
    want = np.array([[[0.0, 1.0], [2.0, 3.0]]])
    got = torch.tensor([[[-0.0, 1.0], [2.0, 3.0]]], dtype=torch.float16)
    assert_exact(got, want, "nlc", neg_zero=True)
    with pytest.raises(AssertionError, match="1 of 4 elements differ"):
        assert_exact(got, want, "nlc")
    with pytest.raises(AssertionError, match="not exact"):
        assert_exact(got, want + 2.0 ** -12, "nlc")
    got = torch.zeros(2, 600, 8)
    want = np.zeros((2, 600, 8))
    want[1, 300, 5], want[1, 599, 2] = 1.0, 4.0
    with pytest.raises(AssertionError) as e:
        assert_exact(got, want, "nlc")
    msg = str(e.value)
    assert "2 of 9600" in msg and "first at (window 1, position 300, channel 5 [128-tile 2, 254-tile 1, 299 from the window edge]" in msg
    assert "worst at (window 1, position 599, channel 2 [128-tile 4, 254-tile 2, 0 from the window edge]" in msg
    with pytest.raises(AssertionError, match="1 of 3 elements differ"):
        assert_exact(torch.tensor([1.0, float("nan"), 3.0]), np.array([1.0, 2.0, 3.0]), "c")


# ---- the fused block-1 backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,l,f,wpt,regime,pool,drop", G.ALL_CONV1_BWD_CASES)
def test_conv1_bwd_cases_meet_their_preconditions(n, l, f, wpt, regime, pool, drop):
    """Constructing a case asserts: the folded constants and every intermediate of du are fp32 numbers; sum |bf16(x)| |du| and sum |du|
    < 2^24 grid units; the sign plan by (tower, 32-channel tile); `small`: du exact in bf16, >= 5 % of the pool windows tied for the
    extreme (>= 1 % with a positive extreme and a gradient on it), >= 5 % with no positive pre-activation, >= 6 x head-room; `rounded`:
    >= 5 % of the non-zero du changed by the bf16 rounding, >= 100 exact ties; lo-x / lo-w: leaving the lo product out of the recompute
    changes >= 1 % of gw, and (lo-x) the filter gradient of x differs from that of bf16(x)."""
    c = G.Conv1BwdCase((n, l, f), regime, pool, wpt, drop)
    kinds = set(c.paths.values())
    assert kinds == {"max", "min"} or (len(c.paths) == 1 and kinds == {"max" if drop else "min"})
    if f == 16:
        assert c.paths[(0, 0)] == "max" and c.paths[(1, 0)] == "min"         # one tile per tower: the two paths in different towers
    for u, kind in c.paths.items():                                          # the kernel's own rule, per wave
        t, j = u
        assert (kind == "max") == (not (c.scale[t, 32 * j:32 * j + 32] < 0).any())
    assert (c.drop is None) == (not drop) and (not drop or ({0.0, 2.0} == set(np.unique(c.drop))))
    assert c.du.shape == (n, l, f) and c.gw.shape == (32, 1, f) and c.gb.shape == (f,)
    assert np.array_equal(c.du, G.store(c.du_exact, "bf16")) and (regime != "rounded" or not G.exact_in(c.du_exact, "bf16"))
    rem = c.du[:, c.lq * pool:]
    assert l % pool == 0 or rem.any(), "the remainder rows carry no du: dropping them would go unseen"


def test_conv1_bwd_tables_reach_what_they_name():
    """Every regime, pool, drop form and sign path at every shape it can differ on, both storage types; the grid forms: `window` one
    workgroup per window wherever there is more than one chunk, `split` a short last split at three chunks and 3 + 3 at six."""
    cases = G.CONV1_BWD_CASES
    for shape, wpt in G.CONV1_BWD_SHAPES:
        mine = [c for c in cases if c[2:6] == shape + (wpt,)]
        regimes = {"small"} | ({"rounded"} if shape[1] >= 256 else set()) | ({"lo-x", "lo-w"} if (shape, wpt) in G.CONV1_BWD_LO_SHAPES else set())
        assert {c[1] for c in mine} == regimes
        for regime in regimes:
            sub = [c for c in mine if c[1] == regime]
            for dt in G.DT16:
                assert {(c[6], c[7]) for c in sub if c[0] == dt and c[8] == "default"} == {(2, False), (2, True), (4, False), (4, True)}
                forms = {c[8] for c in sub if c[0] == dt}
                assert forms == set(G.conv1_bwd_grids(shape[0], shape[1]))
                for form in forms - {"default"}:
                    assert {(c[6], c[7]) for c in sub if c[0] == dt and c[8] == form} == {(2, False), (4, True)}
    chunks = lambda l: -(-l // 256)
    assert [chunks(s[1]) for s, _ in G.CONV1_BWD_SHAPES] == [3, 3, 6, 6, 2, 2, 1]
    assert G.f1_grid(4, 701, "default") == (3, 1) and G.f1_grid(4, 701, "window") == (1, 3)
    assert G.f1_grid(4, 701, "split") == (2, 2) and G.f1_grid(2, 534, "split") == (2, 2)      # 2 + 1 chunks: the clamp of ch_hi
    assert G.f1_grid(3, 1283, "split") == (2, 3) and G.f1_grid(3, 1283, "window") == (1, 6)
    assert G.conv1_bwd_grids(1, 512) == ["default", "window"] and G.conv1_bwd_grids(1, 5) == ["default"]
    # the single-unit shapes take both sign paths across their (pool, drop) pairs
    for shape in ((1, 512, 32), (1, 5, 8)):
        for pool in (2, 4):
            assert {tuple(G.conv1_bwd_case(shape, "small", pool, 1, d).paths.values()) for d in (False, True)} == {("max",), ("min",)}
    assert all(c in G.ALL_CONV1_BWD_CASES for c in {k[1:4] + (k[4], k[0], k[5], k[6]) for k in G.CONV1_BWD_PRODUCT_CASES})


def test_conv1_bwd_du_is_the_autograd_gradient():
    """du_exact against an independent derivation: torch autograd in float64 through conv -> ReLU -> per-tower BatchNorm -> dropout ->
    max-pool, at the pre-activation.  The gradient formula holds for the TRUE batch statistics, so this sub-case takes mean / invstd
    from z and c1 / c2 from bn_exact.finalize (which casts them to fp32 once: the comparison is at that round-off, not equality)."""
    from tests import bn_exact as B
    shape, pool, wpt = (4, 701, 16), 2, 2
    n, l, f = shape
    c = G.Conv1BwdCase(shape, "small", pool, wpt, True)
    u = G.conv32(c.c.x, c.c.w) + c.c.b
    z = np.maximum(u, 0.0)
    assert np.array_equal(z, c.c.z)
    zt = z.reshape(n // wpt, wpt * l, f)
    mean, invstd = zt.mean(1), 1.0 / np.sqrt(zt.var(1) + 1e-3)
    gamma = c.scale                                                        # (towers, F): any per-tower factor of both signs, one 0
    scale = gamma * invstd
    dy, zhat, _, sdy, sdyz = B.backward(z, c.dp, scale, mean, invstd, c.drop, 0.0 * mean, 0.0 * mean, wpt, pool)
    c1, c2, _, _ = B.finalize(sdy, sdyz, wpt, float(wpt * l))
    du = B.backward(z, c.dp, scale, mean, invstd, c.drop, c1, c2, wpt, pool)[2]

    ut = torch.tensor(u, dtype=torch.float64, requires_grad=True)
    zz = torch.relu(ut).view(n // wpt, wpt * l, f)
    m, v = zz.mean(1, keepdim=True), zz.var(1, unbiased=False, keepdim=True)
    y = ((zz - m) / torch.sqrt(v + 1e-3) * torch.tensor(gamma)[:, None, :]).view(n, l, f) * torch.tensor(c.drop)[:, None, :]
    out = torch.nn.functional.max_pool1d(y.transpose(1, 2), pool).transpose(1, 2)
    (out * torch.tensor(c.dp)).sum().backward()
    want = ut.grad.numpy()
    # c1, c2 carry one fp32 rounding each (2^-24 relative); everything else is float64
    bound = 2.0 ** -23 * np.abs(B.per_window(scale, wpt)) * (np.abs(B.per_window(c1, wpt)) + np.abs(zhat * B.per_window(c2, wpt))) + 1e-12
    assert want.any() and (np.abs(du - want) <= bound).all(), float(np.abs(du - want).max())
    assert np.abs(du - want).max() < 1e-6 * np.abs(want).max()


# ---- the length-masked fused inference kernels ------------------------------------------------------------------------------------------
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voicemap_amd", "csrc")
POOL_CASES = [(s,) for s in G.POOL_VARLEN_SHAPES]
CONV1_CASES = [(s, reg, pool) for s in G.CONV1_VARLEN_SHAPES for reg in G.CONV1_VARLEN_REGIMES for pool in (2, 4)]


def _const(fname, name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, fname)).read())
    assert m, (fname, name)
    return int(m.group(1))


def test_varlen_constants_are_the_kernels():
    """The tile edges of the length tables are the kernels' own: a changed constant fails here and does not silently move them."""
    assert _const("conv_gemm.hip", "TROWS") == G.TROWS and _const("conv1_fused.hip", "F1_CHUNK") == G.F1_CHUNK
    src = open(os.path.join(CSRC, "conv1_fused.hip")).read()
    dead = re.search(r"if \(INFER && t0 \+ (\d+) \* rt >= Lv\)", src)
    fast = re.search(r"if \(cok && t0 \+ (\d+) \* rt \+ (\d+) <= Lv\)", src)
    assert dead and fast and {int(dead.group(1)), int(fast.group(1)), int(fast.group(2))} == {G.F1_TILE}
    assert G.F1_CHUNK % G.F1_TILE == 0 and G.TROWS % 2 == 0 and G.F1_TILE % 4 == 0      # no pool group straddles a tile


def test_pool_varlen_table_reaches_every_class():
    """Per shape: lens == L, L - 1 (odd), past L, 0 .. 3, and at every tile edge t0 > 0 the six (valid pooled rows - t0 / 2, parity of lens)
    classes of t0 - 2 .. t0 + 3; over the shapes: two full tiles and more, a ragged last tile, both tile-to-window mappings, c_in that
    conv_nt3_kernel serves and one it does not, two column tiles."""
    for n, l, cin, cout in G.POOL_VARLEN_SHAPES:
        lens = G.pool_varlen_case((n, l, cin, cout)).lens
        assert len(lens) == n and l % 2 == 0 and cout % 128 == 0
        have = set(int(v) for v in lens)
        assert {l, l - 1, l + G.OVER, 0, 1, 2, 3} <= have and (l - 1) % 2 == 1
        tiles = -(-l // G.TROWS)
        assert tiles >= 2
        for tl in range(1, tiles):
            t0 = tl * G.TROWS
            got = {((v >> 1) - (t0 >> 1), v & 1) for v in have if v <= l}
            assert {(d, par) for d in (-1, 0, 1) for par in (0, 1)} <= got, (l, tl)
            # ... which are: the tile before one row short and exactly full, this tile dead, and this tile with dq == 1
            cls = lambda v, q: G.pool_tile_class(l, v, q)
            assert cls(t0 - 2, t0 >> 1) == "dead" and cls(t0 - 2, (t0 >> 1) - 1) == "live-partial"      # (the class of the row's TILE)
            assert cls(t0, (t0 >> 1) - 1) == "live-full" and cls(t0, t0 >> 1) == "dead" and cls(t0 + 1, t0 >> 1) == "dead"
            assert cls(t0 + 2, t0 >> 1) == "live-partial" and cls(t0 + 3, (t0 >> 1) + 1) == "live-partial"
        assert all(G.pool_tile_class(l, v, q) == "dead" for v in (0, 1) for q in range(l // 2))
        assert G.pool_tile_class(l, l + G.OVER, l // 2 - 1) == "live-full" == G.pool_tile_class(l, l, l // 2 - 1)
    shapes = G.POOL_VARLEN_SHAPES
    assert any(l % G.TROWS and l > 2 * G.TROWS for _, l, _, _ in shapes) and any(l % G.TROWS == 0 for _, l, _, _ in shapes)
    groups = [n * -(-l // G.TROWS) for n, l, _, _ in shapes]
    assert any(g % 8 == 0 for g in groups) and any(g % 8 for g in groups)
    assert {128, 256} <= {s[2] for s in shapes} and any(s[2] in (32, 64) for s in shapes) and any(s[3] == 256 for s in shapes)


@pytest.mark.parametrize("pool", [2, 4])
def test_conv1_varlen_table_reaches_every_class(pool):
    """Per shape and pool: lens == L, past L, pool, below pool, every lens % pool, and for every kind of edge the shape has -- a tile edge
    inside a whole chunk, a chunk edge, a tile edge inside the ragged last chunk, the start of the ragged last tile -- Lv on it and one
    pool group either side; over the shapes every kind occurs."""
    kinds = set()
    for shape in G.CONV1_VARLEN_SHAPES:
        n, l, f = shape
        lens = [int(v) for v in G.conv1_varlen_case(shape, "small", pool).lens]
        assert len(lens) == n and {l, l + G.OVER, pool} <= set(lens) and min(lens) < pool
        assert {v % pool for v in lens} == set(range(pool))
        lv = {v // pool * pool for v in lens if v <= l}
        c0, s = (l - 1) // G.F1_CHUNK * G.F1_CHUNK, (l - 1) // G.F1_TILE * G.F1_TILE
        is_kind = {"tile": lambda e: e % G.F1_TILE == 0 and e % G.F1_CHUNK and 0 < e < c0,
                   "chunk": lambda e: e % G.F1_CHUNK == 0 and 0 < e < l,
                   "last-chunk": lambda e: l % G.F1_CHUNK and e % G.F1_TILE == 0 and c0 < e < l,
                   "last-tile": lambda e: l % G.F1_TILE and e == s}
        for kind, edges in G.conv1_edges(l, pool).items():
            assert all(is_kind[kind](e) for e in edges)
            if not edges:
                continue
            kinds.add(kind)
            hit = [e for e in edges if {e - pool, e, e + pool} <= lv]
            assert hit, (shape, kind)
            e = hit[0]
            cls = lambda v, t: G.conv1_tile_class(l, pool, v, t // pool)
            # Lv on the edge: fast next to dead, no boundary tile; one group either side: a boundary tile
            assert cls(e, e - 1) == "fast" and cls(e, e) == "dead" and cls(e + pool - 1, e) == "dead"
            assert cls(e - pool, e - pool - 1) == "boundary" and cls(e - pool, e - pool) == "boundary" and cls(e - pool, e) == "dead"
            assert cls(e + pool, e) == "boundary" and cls(e + pool, e + pool) == "boundary" and cls(e + pool, e - 1) == "fast"
        assert {"tile", "chunk", "last-tile"} <= {k for k, v in G.conv1_edges(l, pool).items() if v}, shape
        assert G.conv1_tile_class(l, pool, l + G.OVER, l // pool - 1) == G.conv1_tile_class(l, pool, l, l // pool - 1)
    assert kinds == {"tile", "chunk", "last-chunk", "last-tile"}
    assert [s for s in G.CONV1_VARLEN_SHAPES if s[1] + G.OVER >= -(-s[1] // G.F1_TILE) * G.F1_TILE], "no lens past the last tile's end"


def _cases(kernel):
    if kernel == "pool":
        return [(G.pool_varlen_case(s), s[1], 2, G.TROWS, False) for s in G.POOL_VARLEN_SHAPES]
    return [(G.conv1_varlen_case(*a), a[0][1], a[2], G.F1_TILE, True) for a in CONV1_CASES]


@pytest.mark.parametrize("kernel", ["pool", "conv1"])
def test_masked_reference_is_each_recording_alone(kernel):
    """The property embed_varlen promises, on the cases in use: window n truncated to lens[n] and run alone gives the valid rows of the
    bucket's reference; the rows behind them are +0; the sound host model of the tiles is the mask helper."""
    for c, l, pool, tile, fast in _cases(kernel):
        want = c.want("f32")
        for i, ln in enumerate(c.lens):
            rows = min(int(ln), l) // pool
            alone = c.alone(i)
            assert alone.shape[0] == rows and np.array_equal(alone, want[i, :rows]) and not want[i, rows:].any()
            assert not np.signbit(want[i, rows:]).any()
        assert np.array_equal(G.mask_model(c.full, c.lens, l, pool, tile, fast), want)
        assert (want != c.full).any() and (c.full[c.lens >= l] == want[c.lens >= l]).all()
        for dt in G.DT16:
            assert np.array_equal(c.want(dt), G.store(want, dt))         # masking and storage rounding commute


@pytest.mark.parametrize("defect", G.MASK_DEFECTS)
@pytest.mark.parametrize("kernel", ["pool", "conv1"])
def test_a_planted_mask_defect_changes_the_expected_output(kernel, defect):
    """Every defect of the host model moves the stored 16-bit expectation of at least one case of the tables -- in both storage types, so
    the device comparison fails on it.  (`fast-early` has no counterpart in the GEMM kernels: a full tile runs the same drain.)"""
    if kernel == "pool" and defect == "fast-early":
        assert all(not fast for _, _, _, _, fast in _cases(kernel))
        return
    for dt in G.DT16:
        moved = 0
        for c, l, pool, tile, fast in _cases(kernel):
            bad = G.store(G.mask_model(c.full, c.lens, l, pool, tile, fast, defect), dt)
            moved += int((bad != c.want(dt)).sum())
        assert moved > 0, (kernel, defect, dt)


@pytest.mark.parametrize("defect", G.MASK_NEUTRAL)
@pytest.mark.parametrize("kernel", ["pool", "conv1"])
def test_the_other_direction_of_a_branch_test_changes_no_bit(kernel, defect):
    """`>` for `>=` in the dead-tile test and `<` for `<=` in the fast-tile test send a tile to the slower branch, which masks per row:
    the same output, so no comparison of outputs can see it (it costs time, not bits)."""
    for c, l, pool, tile, fast in _cases(kernel):
        assert np.array_equal(G.mask_model(c.full, c.lens, l, pool, tile, fast, defect), c.want("f32"))


def test_varlen_note_names_lens_and_tile_class():
    c = G.pool_varlen_case(G.POOL_VARLEN_SHAPES[1])
    got = c.want("bf16").copy()
    i = int(np.argmax(c.lens == 256))
    q, ch = 127, int(np.argmax(got[i, 127] != 0))
    got[i, q, ch] = 0.0
    with pytest.raises(AssertionError, match=r"first at \(window %d, position 127, channel %d \[.*\] \{lens\[%d\] = 256, live-partial tile\}\)" % (i, ch, i)):
        assert_exact(torch.as_tensor(got).to(torch.bfloat16), c.want("bf16"), "nlc", note=c.note())


@pytest.mark.parametrize("dt", G.DT16)
@pytest.mark.parametrize("pool", [2, 4])
def test_chain_case_meets_its_preconditions(pool, dt):
    """Constructing the case asserts the exact-sum precondition of both layers (the second on the first's STORED outputs) and that both
    affines are exact fmas; here: each recording alone reproduces its rows of every tensor of the bucket, the lengths are mixed (odd
    ones, one pooled row at the end)."""
    c = G.chain_case(pool, dt)
    n, l, f, cout = G.CHAIN_SHAPE
    assert len(c.lens) == n and (c.lens % 2 == 1).any() and (c.lens == l).any() and (c.lens1 % 2 == 1).any()
    assert (l // pool) % 2 == 0
    for i in range(n):
        a1, a2, g, gi = c.alone(i)
        assert np.array_equal(a1, c.act1[i, :c.lens1[i]]) and not c.act1[i, c.lens1[i]:].any()
        assert np.array_equal(a2, c.act2[i, :c.lens2[i]]) and not c.act2[i, c.lens2[i]:].any()
        assert g.shape == (cout,) and (gi < c.lens2[i]).all()
    if pool == 2:
        t = G.TROWS
        assert {t - 1, t, t + 2} <= set(int(v) for v in c.lens1)        # the second layer's tile edge: full, dead behind, dq == 1
