"""Host-side checks of tests/gemm_exact.py (the helper of tests/test_gpu_conv_exact.py): every generated case meets its precondition,
an fp32 evaluation in another summation order reproduces the float64 reference exactly, and the comparator catches the defects a
Frobenius ratio at the parity suite's tolerances lets through."""
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
