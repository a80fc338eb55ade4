"""-m gpu: the conv GEMM kernels on exactly representable inputs (tests/gemm_exact.py), every assertion at tolerance zero.  The operands
sit on a power-of-two grid and are small enough that every product and partial sum is an fp32 number, so summation order, tile shape,
split-K plan, MFMA shape and the hi / lo split of VM_F32S cannot change a result: fp32 outputs equal the float64 reference bit for
bit, 16-bit outputs its round-to-nearest-even, and a mismatch is reported with its window, position, channel and tile indices.

Which test reaches which kernel form (vm_set_tuning's GEMM keys; conv_gemm.hip / conv_wgrad.hip dispatch):

  kernel form                                        reached by
  -------------------------------------------------  ------------------------------------------------------------------------------
  conv_nt2r_kernel fwd / dgrad (nt_n2 bits 0, 1)     test_default_dispatch[bf16 / f16] on the 128-multiple channel shapes
  conv_nt_kernel (register-staged 128 x 128)         test_default_dispatch[f32] K tails (c_in 8, 24); test_pinned_fallbacks[register-
                                                     staged-128]; test_persistent_loop on (.., 8, 16)
  conv_nt_kernel SPLIT (VM_F32S)                     test_default_dispatch[f32s small / lo-x / lo-w]; test_persistent_loop[f32s]
  conv_nt_glds_kernel<128>, <64> (nt_glds 1)         test_default_dispatch[f32]; test_pinned_fallbacks[lds-dma-128+tn256];
                                                     test_persistent_loop on (.., 64, 256) with nt_n2 = 0
  persistent loop, second trip                       test_persistent_loop: n_windows * ceil(L / 128) = 520 (XCD order, 520 % 8 == 0) and
                                                     515 (sequential order) > 512 workgroups
  conv_nt3_kernel, K loops of 4 / 8 / 12 / 16        test_fwd_fold / test_fwd_pool (c_in 128 / 256 / 384 / 512) and test_dgrad_bnred (c_out
  chunks, lean prologue (nt3_lean 3) and first (0)   128 / 256 / 384 / 512), each at nt3_lean 3 and 0; c_in 64 / 192: the packed pointer
                                                     falls back to conv_nt2r_kernel
  conv_tn9_kernel (tn_x 1, tn9 1), stage splits      test_default_dispatch[bf16 / f16] wgrad; test_wgrad_split_plans[stage-splits]
  conv_tn9_kernel, window splits (tn9_stages 0)      test_wgrad_variants[window-splits]; test_wgrad_split_plans[window-splits]
  conv_tn9_kernel with producer waves (tn9 2)        test_wgrad_variants[tn9-producer-waves]; test_wgrad_split_plans[stage-splits+producer-waves]
  conv_tn8x_kernel (tn9 0)                           test_wgrad_variants[tn8x-slots]
  conv_tn256_kernel (tn_x 0, tn_tile 256)            test_default_dispatch[f32 / f32s] wide layers; test_pinned_fallbacks[lds-dma-128+tn256]
  conv_tn_kernel (tn_tile 128 or narrow layers)      test_default_dispatch[f32 / f32s] narrow layers; test_pinned_fallbacks[register-staged-128]
  slab_fold_kernel via vm_conv_wgrad_fold and        test_wgrad_split_plans (real per-tower factors, dsum from vm_du_tower_sums; one-call
  vm_conv_wgrad_fold_finish                          and two-call forms bit-identical)
  block 1: conv1 fwd / wgrad, fused fwd modes 0-2    test_conv1_fwd_wgrad, test_conv1_fused_fwd, test_conv1_fused_fwd_products (f1_products
                                                     1 / 2 / 3)
  block 1: conv1_fused_bwd_kernel (all_max and       test_conv1_fused_bwd (three grid forms of f1_blocks), test_conv1_fused_bwd_products
  use_min fast tiles, the ragged slow tile, slabs)   (f1_products 1 / 2 / 3), test_conv1_fused_bwd_refuses

The length-masked inference forms (vm_conv_fwd_pool_varlen, vm_conv1_fused_fwd_varlen; tables and tile classes in gemm_exact.py):

  conv_nt2r_kernel EPI_FWD_POOL + valid_len:         test_fwd_pool_varlen, staged weights (every shape; c_in 64 also with the packed
  dead tile (n2_pool_dead_tile), live-partial        pointer): lens 0 / 1 all dead; t - 2 .. t + 3 at every 254-edge t: the tile before
  (dq < vq) and live-full (dq == vq) drains, the     one row short and full, the tile behind dead and with dq == 1; L, L - 1, L + 5;
  8-group swizzle and the plain tile-to-window map   72 tile groups (swizzle) and 26 / 57 (plain); test_masked_chain_.. (layer 2)
  conv_nt3_kernel, the same three tile classes,      test_fwd_pool_varlen with packed weights on c_in 128 (72 groups, two column tiles)
  lean prologue and first                            and c_in 256 (26 groups), nt3_lean 3 and 0
  conv1_fused_fwd_kernel + valid_len: dead, fast     test_conv1_fused_fwd_varlen: Lv on a 32-edge (fast | dead), one pool group either
  and boundary tiles; per-chunk workgroups and the   side (boundary), at a tile edge, a 256-chunk edge, inside the ragged last chunk and
  double-buffered chunk loop (f1_fwd_blocks = n)     at the ragged last tile; every lens % pool; lens pool, < pool, L, L + 5 (clamped)
  rows past the valid length never matter            test_varlen_ignores_what_no_valid_row_reads (NaN behind the last tap)
  the three masked launches in a row                 test_masked_chain_equals_each_recording_alone
"""
import numpy as np
import pytest
import torch

from tests import gemm_exact as G
from tests import test_gpu_kernels as K
from tests.gemm_exact import assert_exact
from tests.gpu_util import DTYPES, L, dev, p, padded, stream
from tests.test_gpu_kernels import gemm_kernels  # noqa: F401  (the fixture that pins a kernel selection and restores the defaults)

pytestmark = pytest.mark.gpu

DT16 = G.DT16


def _nan(*shape, dtype=torch.float32):
    """An output buffer no element of which is a valid result: one the kernel leaves out is a mismatch."""
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _f64(t):
    return t.to(torch.float64)


def _prep(w, cin, cout, vm, tdt):
    wf = torch.empty(cout * 3 * cin, dtype=tdt, device="cuda")
    wd = torch.empty(cin * 3 * cout, dtype=tdt, device="cuda")
    L().call("vm_prep_conv_weights", p(dev(w)), cin, cout, vm, p(wf), p(wd), stream())
    return wf, wd


def _stat_rows(n, rows, c):
    """NaN-filled partial rows: the kernel owes every one of them, a row whose true sum is zero included."""
    return _nan(n * rows, c), _nan(n * rows, c)


def _check_stats(ss, sq, n, c, ss_ref, sq_ref, ok_sq, what):
    """The sum of the stored values in every regime; the sum of squares where its precondition holds (gemm_exact asserts that it does
    in the `small` regime of every case; in `wide` the squares of a window pass 2^24 grid units almost everywhere)."""
    assert_exact(_rows_sum(ss, n, c), ss_ref, "nc", what=what + " stat_sum")
    if ok_sq:
        assert_exact(_rows_sum(sq, n, c), sq_ref, "nc", what=what + " stat_sq")


def _rows_sum(t, n, c):
    """(n * rows, c) fp32 partial rows -> (n, c) in float64 (exact: every row is an integer multiple of the grid below 2^24 units)."""
    return _f64(t).view(n, -1, c).sum(1)


def test_shape_tables_are_the_parity_tests_lists():
    params = lambda f, i=0: [tuple(a) for a in [m for m in f.pytestmark if m.name == "parametrize" and "n," in m.args[0]][i].args[1]]
    assert G.GEMM_SHAPES == K.GEMM_SHAPES
    assert G.RESIDENT_SHAPES == params(K.test_conv_input_resident_kernel_shapes)
    assert G.FALLBACK_SHAPES == params(K.test_conv_fwd_dgrad_wgrad_fallback_kernels)
    assert G.WGRAD_VARIANT_SHAPES == params(K.test_conv_wgrad_kernel_variants)
    assert G.SPLIT_SHAPES == params(K.test_conv_wgrad_split_granularity)


# ---- forward + statistics + inference launch, dgrad, wgrad --------------------------------------------------------------------------------
def _fwd_dgrad_wgrad(dt, regime, shape, ops=("fwd", "dgrad", "wgrad")):
    vm, tdt = DTYPES[dt]
    n, l, cin, cout = shape
    c = G.conv_case(shape, regime, dt)
    wf, wd = _prep(c.w, cin, cout, vm, tdt)
    xp = padded(c.x, tdt)
    tag = "%s %s %s" % (dt, regime, shape)
    if "fwd" in ops:
        z_ref, ss_ref, sq_ref, ok_sq = c.forward(dt)
        z = _nan(n, l, cout, dtype=tdt)
        ss, sq = _stat_rows(n, L().query("vm_conv_stat_rows", l), cout)
        L().call("vm_conv_fwd", p(xp), p(wf), p(dev(c.b)), n, l, cin, cout, vm, p(z), p(ss), p(sq), stream())
        assert_exact(z, z_ref, "nlc", neg_zero=True, what="vm_conv_fwd z " + tag)       # (a ReLU output: the sign of a zero is free)
        _check_stats(ss, sq, n, cout, ss_ref, sq_ref, ok_sq, "vm_conv_fwd " + tag)
        z2 = _nan(n, l, cout, dtype=tdt)
        L().call("vm_conv_fwd", p(xp), p(wf), p(dev(c.b)), n, l, cin, cout, vm, p(z2), None, None, stream())
        assert_exact(z2, z_ref, "nlc", neg_zero=True, what="vm_conv_fwd inference z " + tag)
    if "dgrad" in ops:
        dx = _nan(n, l, cin, dtype=tdt)
        L().call("vm_conv_dgrad", p(padded(c.du_d, tdt)), p(wd), n, l, cin, cout, vm, p(dx), stream())
        assert_exact(dx, G.store(c.dx, dt), "nlc", what="vm_conv_dgrad dx " + tag)
    if "wgrad" in ops:
        ws = torch.empty(L().query("vm_conv_wgrad_workspace_bytes", n, l, cin, cout) // 4 + 16, device="cuda")
        gw = _nan(3, cin, cout)
        L().call("vm_conv_wgrad", p(xp), p(padded(c.du_w, tdt)), n, l, cin, cout, vm, p(ws), p(gw), stream())
        assert_exact(gw, c.gw, "kio", what="vm_conv_wgrad " + tag)


@pytest.mark.parametrize("dt,regime,n,l,cin,cout", G.DEFAULT_CASES)
def test_default_dispatch(dt, regime, n, l, cin, cout):
    """The default dispatch of vm_conv_fwd / vm_conv_dgrad / vm_conv_wgrad on GEMM_SHAPES and the input-resident kernels' list, every
    storage type in every regime it has (f32: small, wide; f32s: small, lo-x, lo-w; bf16 / f16: small, wide)."""
    _fwd_dgrad_wgrad(dt, regime, (n, l, cin, cout))


@pytest.mark.parametrize("gemm_kernels", [{"nt_n2": 0, "tn_x": 0}, {"nt_n2": 0, "nt_glds": 0, "tn_x": 0, "tn_tile": 128}],
                         indirect=True, ids=["lds-dma-128+tn256", "register-staged-128"])
@pytest.mark.parametrize("dt,regime,n,l,cin,cout", G.FALLBACK_CASES)
def test_pinned_fallbacks(dt, regime, n, l, cin, cout, gemm_kernels):
    """The 128 x 128 forward / dgrad kernels and the register-transposing wgrad kernels where the default dispatch would take the
    input-resident ones (bf16 included: its MFMA and its 8-bit rounding are not f16's)."""
    _fwd_dgrad_wgrad(dt, regime, (n, l, cin, cout))


@pytest.mark.parametrize("gemm_kernels", [{"tn9": 0}, {"tn9": 2}, {"tn9_stages": 0}], indirect=True,
                         ids=["tn8x-slots", "tn9-producer-waves", "window-splits"])
@pytest.mark.parametrize("dt,regime,n,l,cin,cout", G.WGRAD_VARIANT_CASES)
def test_wgrad_variants(dt, regime, n, l, cin, cout, gemm_kernels):
    """conv_tn8x_kernel, conv_tn9_kernel with producer waves and conv_tn9_kernel split by whole windows."""
    _fwd_dgrad_wgrad(dt, regime, (n, l, cin, cout), ops=("wgrad",))


@pytest.mark.parametrize("gemm_kernels", [{}, {"nt_n2": 0}], indirect=True, ids=["default", "nt_n2-off"])
@pytest.mark.parametrize("dt,regime,n,l,cin,cout", G.PERSISTENT_CASES)
def test_persistent_loop(dt, regime, n, l, cin, cout, gemm_kernels):
    """More (window, 128-position tile) groups than launch_nt's 512 workgroups: the second trip of conv_nt_kernel's `group +=
    gridDim.x` and conv_nt_glds_kernel's `it * gridDim.x`, in the XCD tile order (520 groups) and the sequential one (515).  c_in = 8:
    K * sizeof(T) is no multiple of 64 in 16-bit storage -> the register-staged kernel; c_in = 64, c_out = 256 with nt_n2 = 0: the
    LDS-DMA kernel with two N tiles (100-position windows are too short for conv_nt2r_kernel, so the default dispatch lands there too)."""
    _fwd_dgrad_wgrad(dt, regime, (n, l, cin, cout), ops=("fwd", "dgrad"))


# ---- wgrad split plans, the folded weight gradient and its two-call form ------------------------------------------------------------------
@pytest.mark.parametrize("gemm_kernels", [{"tn9_stages": 1}, {"tn9_stages": 0}, {"tn9": 2, "tn9_stages": 1}], indirect=True,
                         ids=["stage-splits", "window-splits", "stage-splits+producer-waves"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("n,wpt,l,cin,cout", G.SPLIT_SHAPES)
def test_wgrad_split_plans(dt, n, wpt, l, cin, cout, gemm_kernels):
    """conv_tn9_kernel's split-K ranges (stages of a tower's window stream against whole windows): vm_conv_wgrad, and vm_conv_wgrad_fold
    with real per-tower factors -- scale in +-{0.5, 1, 2}, integer shift, dsum from vm_du_tower_sums on the same du -- in its one-call
    form and as vm_conv_wgrad_fold(dsum = NULL) + vm_conv_wgrad_fold_finish: equal to each other and to the float64 definition."""
    vm, tdt = DTYPES[dt]
    c = G.conv_case((n, l, cin, cout), "small", dt)
    f = G.FoldFactors((n, wpt, l, cin, cout), c.x, c.du_w)
    xp, dup = padded(c.x, tdt), padded(c.du_w, tdt)
    tag = "%s %s" % (dt, (n, wpt, l, cin, cout))
    ws = torch.empty(L().query("vm_conv_wgrad_workspace_bytes", n, l, cin, cout) // 4 + 16, device="cuda")
    gw = _nan(3, cin, cout)
    L().call("vm_conv_wgrad", p(xp), p(dup), n, l, cin, cout, vm, p(ws), p(gw), stream())
    assert_exact(gw, c.gw, "kio", what="vm_conv_wgrad " + tag)
    towers = n // wpt
    prow = L().query("vm_bn_part_rows")
    pdu = np.zeros((n, prow, cout), np.float32)
    pdu[:, 0] = c.du_w.sum(1)                           # the apply pass's partial column sums of du: one live row per window
    gb, ds = _nan(cout), _nan(towers, 3, cout)
    cws = torch.empty(L().query("vm_colreduce_workspace_bytes", towers, cout) // 8, dtype=torch.float64, device="cuda")
    L().call("vm_du_tower_sums", p(dev(pdu.reshape(n * prow, cout))), p(dup), n, wpt, l, cout, vm, p(gb), p(ds), p(cws), stream())
    assert_exact(ds, f.dsum, "tkc", what="vm_du_tower_sums dsum " + tag)
    assert_exact(gb, c.du_w.sum((0, 1)), "c", what="vm_du_tower_sums grad_b " + tag)
    nws = L().query("vm_conv_wgrad_fold_workspace_bytes", n, wpt, l, cin, cout) // 4 + 16
    sc, sh = dev(f.scale), dev(f.shift)
    ws1, g1 = torch.empty(nws, device="cuda"), _nan(3, cin, cout)
    L().call("vm_conv_wgrad_fold", p(xp), p(dup), n, wpt, l, cin, cout, vm, p(sc), p(sh), p(ds), p(ws1), p(g1), stream())
    assert_exact(g1, f.gw, "kio", what="vm_conv_wgrad_fold " + tag)
    ws2, g2 = torch.empty(nws, device="cuda"), _nan(3, cin, cout)
    L().call("vm_conv_wgrad_fold", p(xp), p(dup), n, wpt, l, cin, cout, vm, None, None, None, p(ws2), None, stream())
    L().call("vm_conv_wgrad_fold_finish", p(ws2), n, wpt, l, cin, cout, p(sc), p(sh), p(ds), p(g2), stream())
    assert_exact(g2, f.gw, "kio", what="vm_conv_wgrad_fold_finish " + tag)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))


# ---- fused forwards ---------------------------------------------------------------------------------------------------------------------
def _served(query, shape, dt, *extra):
    return bool(L().query(query, *shape, DTYPES[dt][0], *extra))


def test_fused_lists_have_served_shapes():
    """The skips below follow the *_supported queries at default tuning; every entry point must still be reached in every type it has."""
    for dt in DT16:
        assert sum(_served("vm_conv_fwd_e_supported", s, dt) for s in G.FUSED_SHAPES) >= 4, dt
        assert sum(_served("vm_conv_fwd_fold_supported", s, dt, 1) for s in G.FUSED_SHAPES) >= 4, dt
        assert sum(_served("vm_conv_dgrad_bnred_supported", s[:4], dt) for s in G.BNRED_SHAPES) >= 4, dt
        assert sum(_served("vm_conv_fwd_pool_supported", s, dt) for s in G.FUSED_SHAPES) >= 4, dt


def _packed_runs(rows, ac, vm):
    """[(weights packed?, nt3_lean)]: staged weights, then vm_pack_nt_weights' copy with the lean prologue and with the first one."""
    return [(False, 3)] + ([(True, 3), (True, 0)] if L().query("vm_pack_nt_weights_supported", rows, ac, vm) else [])


@pytest.fixture
def nt3_lean():
    yield lambda v: L().call("vm_set_tuning", b"nt3_lean", v)
    L().call("vm_set_tuning", b"nt3_lean", K.GEMM_DEFAULTS["nt3_lean"])


@pytest.mark.parametrize("dt,regime,n,l,cin,cout", G.FWD_E_CASES)
def test_fwd_e(dt, regime, n, l, cin, cout):
    """vm_conv_fwd_e: z, the statistics and the pair extreme of the STORED z by sign(gamma), negative and zero gammas included."""
    vm, tdt = DTYPES[dt]
    if not L().query("vm_conv_fwd_e_supported", n, l, cin, cout, vm):
        pytest.skip("shape not served by the input-resident kernel")
    c = G.conv_case((n, l, cin, cout), regime, dt)
    z_ref, ss_ref, sq_ref, ok_sq = c.forward(dt)
    gamma = G.signs(cout, seed=l + cin)
    wf, _ = _prep(c.w, cin, cout, vm, tdt)
    z, e = _nan(n, l, cout, dtype=tdt), _nan(n, l // 2, cout, dtype=tdt)
    ss, sq = _stat_rows(n, L().query("vm_conv_stat_rows", l), cout)
    L().call("vm_conv_fwd_e", p(padded(c.x, tdt)), p(wf), p(dev(c.b)), p(dev(gamma)), n, l, cin, cout, vm, p(z), p(ss), p(sq), p(e), stream())
    tag = "%s %s %s" % (dt, regime, (n, l, cin, cout))
    assert_exact(z, z_ref, "nlc", neg_zero=True, what="vm_conv_fwd_e z " + tag)
    assert_exact(e, G.pair_extreme(z_ref, gamma)[0], "nlc", neg_zero=True, what="vm_conv_fwd_e e " + tag)
    _check_stats(ss, sq, n, cout, ss_ref, sq_ref, ok_sq, "vm_conv_fwd_e " + tag)


@pytest.mark.parametrize("dt,regime,n,l,cin,cout", G.FWD_POOL_CASES)
def test_fwd_pool(dt, regime, n, l, cin, cout, nt3_lean):
    """vm_conv_fwd_pool: store(max over the pair of scale * z + shift), scale +-2^k (outputs past 256: the second rounding happens),
    integer shift; halo rows are the caller's; staged and packed weights, both conv_nt3_kernel prologues."""
    vm, tdt = DTYPES[dt]
    if not L().query("vm_conv_fwd_pool_supported", n, l, cin, cout, vm):
        pytest.skip("shape / storage type not served")
    c = G.conv_case((n, l, cin, cout), regime, dt)
    r = np.random.default_rng(l + cout)
    scale = r.choice([0.5, 1.0, 2.0, 4.0], cout) * r.choice([-1.0, 1.0], cout)
    shift = r.integers(-3, 4, cout).astype(np.float64)
    y = c.forward(dt)[0] * scale + shift                # exact: |y| < 2^10 on a grid of 1/2
    want = G.store(np.maximum(y[:, 0::2], y[:, 1::2]), dt)
    wf, _ = _prep(c.w, cin, cout, vm, tdt)
    wfp = torch.empty_like(wf)
    for packed, lean in _packed_runs(cout, cin, vm):
        nt3_lean(lean)
        if packed:
            L().call("vm_pack_nt_weights", p(wf), 1, cout, cin, vm, p(wfp), stream())
        act = torch.full((n, l // 2 + 2, cout), 7.0, dtype=tdt, device="cuda")
        L().call("vm_conv_fwd_pool", p(padded(c.x, tdt)), p(wf), p(dev(c.b)), p(dev(scale)), p(dev(shift)), n, l, cin, cout, vm, p(act),
                 p(wfp) if packed else None, stream())
        assert_exact(act[:, 1:-1], want, "nlc", what="vm_conv_fwd_pool %s %s packed %d lean %d" % (dt, (n, l, cin, cout), packed, lean))
        assert (act[:, 0] == 7.0).all() and (act[:, -1] == 7.0).all()


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("n,l,cin,cout", G.FUSED_SHAPES)
def test_fwd_fold(dt, n, l, cin, cout, nt3_lean):
    """vm_conv_fwd_fold on weights folded by vm_fold_bn_weights (scales +-{1, 2}, integer shifts, two towers with different
    affines): the z form with the extreme, the (e, o) pair form, and for f16 the centred pair form (integer ctr) with the statistics of
    the centred values; staged and packed weights, both conv_nt3_kernel prologues.  e's halo rows are the caller's."""
    vm, tdt = DTYPES[dt]
    if not L().query("vm_conv_fwd_fold_supported", n, l, cin, cout, vm, 1):
        pytest.skip("shape not served by conv_nt2r_kernel")
    f = G.fold_case((n, l, cin, cout), dt)
    towers, wpt = 2, n // 2
    rows = L().query("vm_conv_stat_rows", l)
    wt = np.ascontiguousarray(f.w.transpose(2, 0, 1).reshape(cout, 3 * cin))
    ep = padded(f.e, tdt)
    tag = "%s %s" % (dt, (n, l, cin, cout))
    for centred in ((False, True) if dt == "f16" else (False,)):
        wf = torch.empty(towers, cout, 3 * cin, dtype=tdt, device="cuda")
        hb = _nan(towers, 4, cout)
        ctr = _nan(towers, cout) if centred else None
        L().call("vm_fold_bn_weights", p(dev(wt)), p(dev(f.scale)), p(dev(f.shift)), p(dev(f.b)), towers, cin, cout, vm, p(wf), None, p(hb),
                 p(ctr), stream())
        assert_exact(wf.view(towers, cout, 3, cin), f.wf, "tokc", neg_zero=True, what="vm_fold_bn_weights wf " + tag)   # (0 * a negative scale)
        assert_exact(hb[:, :3], f.hb, "tkc", what="vm_fold_bn_weights hb " + tag)
        if centred:
            assert_exact(ctr, f.ctr, "tc", what="vm_fold_bn_weights ctr " + tag)
        z_ref = f.z_st - (np.repeat(f.ctr, wpt, axis=0)[:, None, :] if centred else 0.0)      # the stored tile (centred: t = relu(z) - ctr)
        ext, oth, second = G.pair_extreme(f.z_st, f.gamma)
        e_ref = ext - (np.repeat(f.ctr, wpt, axis=0)[:, None, :] if centred else 0.0)
        ss_ref, sq_ref = z_ref.sum(1), (z_ref * z_ref).sum(1)
        wfp = torch.empty_like(wf)
        for packed, lean in _packed_runs(cout, cin, vm):
            nt3_lean(lean)
            if packed:
                L().call("vm_pack_nt_weights", p(wf), towers, cout, cin, vm, p(wfp), stream())
            run = "%s centred %d packed %d lean %d" % (tag, centred, packed, lean)
            forms = ("pairs",) if centred else ("z", "pairs")
            for form in forms:
                z = _nan(n, l, cout, dtype=tdt) if form == "z" else None
                e = torch.full((n, l // 2 + 2, cout), 7.0, dtype=tdt, device="cuda")
                o = _nan(n, l // 2, cout, dtype=tdt) if form == "pairs" else None
                ss, sq = _nan(n * rows, cout), _nan(n * rows, cout)
                L().call("vm_conv_fwd_fold", p(ep), p(wf), p(dev(f.b)), p(hb), p(dev(f.gamma)), n, wpt, l, cin, cout, vm, p(z), p(ss), p(sq),
                         p(e), p(o), p(wfp) if packed else None, p(ctr), stream())
                if form == "z":
                    assert_exact(z, z_ref, "nlc", neg_zero=True, what="vm_conv_fwd_fold z " + run)
                else:
                    ob = o.view(torch.int16).cpu().numpy().view(np.uint16)
                    flag = (ob >> 15).astype(bool)
                    mag = torch.from_numpy((ob & 0x7fff).view(np.int16)).view(tdt)
                    assert_exact(mag, oth, "nlc", what="vm_conv_fwd_fold o " + run)            # (sign bit = the position flag: masked off)
                    assert np.array_equal(flag, second), "vm_conv_fwd_fold o flags " + run
                assert_exact(e[:, 1:-1], e_ref, "nlc", neg_zero=True, what="vm_conv_fwd_fold e " + run)
                assert (e[:, 0] == 7.0).all() and (e[:, -1] == 7.0).all(), "vm_conv_fwd_fold wrote e's halo rows " + run
                assert_exact(_rows_sum(ss, n, cout), ss_ref, "nc", what="vm_conv_fwd_fold stat_sum " + run)
                assert_exact(_rows_sum(sq, n, cout), sq_ref, "nc", what="vm_conv_fwd_fold stat_sq " + run)


@pytest.mark.parametrize("dt,regime,n,l,cin,cout,padded_a", G.BNRED_CASES)
def test_dgrad_bnred(dt, regime, n, l, cin, cout, padded_a, nt3_lean):
    """vm_conv_dgrad_bnred: dx and both sum rows (of the stored dx, and of dx * red_a with an integer red_a in either layout, its halo
    rows holding a large value that must not be read); staged and packed weights, both conv_nt3_kernel prologues."""
    vm, tdt = DTYPES[dt]
    if not L().query("vm_conv_dgrad_bnred_supported", n, l, cin, cout, vm):
        pytest.skip("shape not served by the input-resident kernel")
    c = G.conv_case((n, l, cin, cout), regime, dt)
    dx_ref = G.store(c.dx, dt)
    a = np.random.default_rng(l + cin).integers(0, 4, (n, l, cin)).astype(np.float64)
    s0_ref, s1_ref = dx_ref.sum(1), (dx_ref * a).sum(1)
    ok0, ok1 = G.sums_exact(np.abs(dx_ref).sum(1), 1.0), G.sums_exact((np.abs(dx_ref) * a).sum(1), 1.0)
    assert regime != "small" or (ok0 and ok1)
    if padded_a:
        ap = torch.full((n, l + 2, cin), 6e4, dtype=tdt, device="cuda")
        ap[:, 1:l + 1] = torch.as_tensor(a).to("cuda", tdt)
    else:
        ap = dev(a, tdt)
    _, wd = _prep(c.w, cin, cout, vm, tdt)
    wdp = torch.empty_like(wd)
    rows = L().query("vm_conv_dgrad_bnred_rows", l)
    for packed, lean in _packed_runs(cin, cout, vm):
        nt3_lean(lean)
        if packed:
            L().call("vm_pack_nt_weights", p(wd), 1, cin, cout, vm, p(wdp), stream())
        dx, s0, s1 = _nan(n, l, cin, dtype=tdt), _nan(n * rows, cin), _nan(n * rows, cin)
        L().call("vm_conv_dgrad_bnred", p(padded(c.du_d, tdt)), p(wd), n, l, cin, cout, vm, p(dx), p(ap), int(padded_a), p(s0), p(s1),
                 p(wdp) if packed else None, stream())
        run = "%s %s %s packed %d lean %d" % (dt, regime, (n, l, cin, cout), packed, lean)
        assert_exact(dx, dx_ref, "nlc", what="vm_conv_dgrad_bnred dx " + run)
        if ok0:
            assert_exact(_rows_sum(s0, n, cin), s0_ref, "nc", what="vm_conv_dgrad_bnred red_s0 " + run)
        if ok1:
            assert_exact(_rows_sum(s1, n, cin), s1_ref, "nc", what="vm_conv_dgrad_bnred red_s1 " + run)


# ---- block 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["small", "wide"])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n,l,f", G.CONV1_SHAPES + [G.CONV1_WGRAD_SHAPE])
def test_conv1_fwd_wgrad(dt, regime, n, l, f):
    """vm_conv1_fwd (z as stored, the statistics of the stored values) and vm_conv1_wgrad."""
    vm, tdt = DTYPES[dt]
    c = G.conv1_case((n, l, f), regime, dt)
    tag = "%s %s %s" % (dt, regime, (n, l, f))
    xd = dev(G.pad_wave(c.x))
    z = _nan(n, l, f, dtype=tdt)
    ss, sq = _stat_rows(n, L().query("vm_conv1_stat_rows", l), f)
    L().call("vm_conv1_fwd", p(xd), p(dev(c.w)), p(dev(c.b)), n, l, f, vm, p(z), p(ss), p(sq), stream())
    z_ref = G.store(c.z, dt)
    ss_ref, sq_ref, ok_sum, ok_sq = c.stats(z_ref)
    assert_exact(z, z_ref, "nlc", neg_zero=True, what="vm_conv1_fwd z " + tag)
    assert ok_sum                                            # (Conv1Case.stats: always outside the lo regimes)
    _check_stats(ss, sq, n, f, ss_ref, sq_ref, ok_sq, "vm_conv1_fwd " + tag)
    ws = torch.empty(L().query("vm_conv1_wgrad_workspace_bytes", n, f) // 4 + 16, device="cuda")
    gw = _nan(32, 1, f)
    L().call("vm_conv1_wgrad", p(xd), p(padded(c.du, tdt)), n, l, f, vm, p(ws), p(gw), stream())
    assert_exact(gw, c.gw, "k1f", what="vm_conv1_wgrad " + tag)


@pytest.fixture
def f1_tuning():
    """vm_set_tuning for the fused block-1 kernels, restored to the defaults (f1_products 2, 1024 target workgroups)."""
    yield lambda k, v: L().call("vm_set_tuning", k, v)
    for k, v in ((b"f1_products", 2), (b"f1_fwd_blocks", 1024), (b"f1_blocks", 1024)):
        L().call("vm_set_tuning", k, v)


def _conv1_fused_modes(dt, c, z, shape, pool, tag):
    """The three modes of vm_conv1_fused_fwd against z = the fp32 accumulator's exact value (never stored: the statistics are its own)."""
    vm, tdt = DTYPES[dt]
    n, l, f = shape
    lq = l // pool
    xd, wd_, bd = dev(G.pad_wave(c.x)), dev(c.w), dev(c.b)
    rows = L().query("vm_conv1_stat_rows", l)
    gamma = G.signs(f, seed=l + f)
    ext = G.pool_extreme(z, gamma, pool)
    ss_ref, sq_ref, ok_sum, ok_sq = c.stats(z)
    for mode in (0, 1, 2):
        if mode == 1:
            r = np.random.default_rng(l + f + pool)
            scale = r.choice([0.5, 1.0, 2.0, 4.0], f) * r.choice([-1.0, 1.0], f)
            shift = r.integers(-3, 4, f).astype(np.float64)
            out = torch.full((n, lq + 2, f), 7.0, dtype=tdt, device="cuda")
            L().call("vm_conv1_fused_fwd", p(xd), p(wd_), p(bd), p(dev(scale)), p(dev(shift)), n, l, f, pool, 1, vm, p(out), None, None, stream())
            want = G.store(G.pool_extreme(z, scale, pool) * scale + shift, dt)       # one rounding: fma(extreme, scale, shift)
            assert_exact(out[:, 1:-1], want, "nlc", what="vm_conv1_fused_fwd mode 1 " + tag)
            assert (out[:, 0] == 7.0).all() and (out[:, -1] == 7.0).all(), "mode 1 wrote the halo rows " + tag
            continue
        ss, sq = _stat_rows(n, rows, f)
        if mode == 0:
            out = _nan(n, lq, f, dtype=tdt)
            want = G.store(ext, dt)
        else:
            out = torch.full((n, lq + 2, f), 7.0, dtype=tdt, device="cuda")
            want = G.store(ext - np.maximum(c.b, 0.0), dt)                               # stored centred: e - max(bias, 0)
        L().call("vm_conv1_fused_fwd", p(xd), p(wd_), p(bd), p(dev(gamma)), None, n, l, f, pool, mode, vm, p(out), p(ss), p(sq), stream())
        if mode == 2:
            assert (out[:, 0] == 7.0).all() and (out[:, -1] == 7.0).all(), "mode 2 wrote the halo rows " + tag
            out = out[:, 1:-1]
        assert_exact(out, want, "nlc", neg_zero=True, what="vm_conv1_fused_fwd mode %d e %s" % (mode, tag))
        if ok_sum:      # (asserted by Conv1Case.stats in `small` and `wide`; a lo regime's 2^-9 / 2^-12 grid can miss it at L >= 1200)
            _check_stats(ss, sq, n, f, ss_ref, sq_ref, ok_sq, "vm_conv1_fused_fwd mode %d %s" % (mode, tag))


@pytest.mark.parametrize("per_window", [0, 1], ids=["default-grid", "one-workgroup-per-window"])
@pytest.mark.parametrize("pool", [2, 4])
@pytest.mark.parametrize("regime", ["small", "wide", "lo-x", "lo-w"])
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("n,l,f", G.CONV1_FUSED_SHAPES)
def test_conv1_fused_fwd(dt, regime, n, l, f, pool, per_window, f1_tuning):
    """vm_conv1_fused_fwd in modes 0 (extreme), 1 (inference: fma(extreme, scale, shift), scale +-2^k, integer shift) and 2 (padded,
    centred extreme); one workgroup per window walks the double-buffered multi-chunk loop that small batches otherwise never run.
    lo-x / lo-w: a waveform / filters with a non-zero lo half -- bf16 storage forms x_hi * w_hi + x_lo * w_hi + x_hi * w_lo, so each
    cross product is needed for an exact result; f16 storage (default f1_products = 2) holds the lo-x waveform in a half and splits
    the lo-w filters into two."""
    if per_window:
        f1_tuning(b"f1_fwd_blocks", n)
    c = G.conv1_case((n, l, f), regime, dt)
    _conv1_fused_modes(dt, c, c.z, (n, l, f), pool, "%s %s %s pool %d" % (dt, regime, (n, l, f), pool))


@pytest.mark.parametrize("products", [1, 2, 3])
@pytest.mark.parametrize("pool", [2, 4])
@pytest.mark.parametrize("n,l,f", [(2, 1200, 128), (2, 532, 40)])
def test_conv1_fused_fwd_products(n, l, f, pool, products, f1_tuning):
    """f1_products 1 / 2 / 3 (VM_F16), modes 0, 1 and 2, pool 2 and 4.  Filters on an 8-bit grid (small): the same exact result under
    all three.  Filters a + b * 2^-12 (lo-w), exact only as hi + lo halves: exact under 2 and 3, and under 1 equal to the reference
    with the filters rounded to half -- so the lo product is really issued where it is asked for.  A waveform a + b * 2^-9 (lo-x): a
    half holds it (1, 2), and under 3 its bf16 lo half makes x_lo * w_hi necessary."""
    f1_tuning(b"f1_products", products)
    for regime in ("small", "lo-w", "lo-x"):
        c = G.conv1_case((n, l, f), regime, "f16")
        z = c.z_hi if (regime == "lo-w" and products == 1) else c.z
        _conv1_fused_modes("f16", c, z, (n, l, f), pool, "f16 %s %s pool %d f1_products %d" % (regime, (n, l, f), pool, products))


# ---- block 1, the fused backward -----------------------------------------------------------------------------------------------------------
GUARD = 64                  # fp32 words behind the queried workspace size
GUARD_WORD = -12345.0


def _conv1_fused_bwd(dt, c, n, l, f, wpt, pool, want_gw, want_gb, tag):
    """One call of vm_conv1_fused_bwd on the operands of a Conv1BwdCase: grad_w and grad_b (NaN before the call: it overwrites them)
    bit for bit, the words behind the queried workspace size and every input untouched.  The workspace size is queried here, after
    the caller has set its tuning."""
    vm, tdt = DTYPES[dt]
    words = L().query("vm_conv1_fused_bwd_workspace_bytes", n, l, f) // 4
    ws = torch.full((words + GUARD,), GUARD_WORD, dtype=torch.float32, device="cuda")
    ins = [dev(G.pad_wave(c.c.x)), dev(c.c.w), dev(c.c.b), dev(c.dp, tdt), dev(c.scale), dev(c.mean), dev(c.invstd),
           None if c.drop is None else dev(c.drop), dev(c.c1), dev(c.c2)]
    before = [None if t is None else t.clone() for t in ins]
    gw, gb = _nan(32, 1, f), _nan(f)
    L().call("vm_conv1_fused_bwd", *[p(t) for t in ins], n, wpt, l, f, pool, vm, p(ws), p(gw), p(gb), stream())
    assert_exact(gw, want_gw, "k1f", what="vm_conv1_fused_bwd grad_w " + tag)
    assert_exact(gb, want_gb, "c", what="vm_conv1_fused_bwd grad_b " + tag)
    assert (ws[words:] == GUARD_WORD).all(), "vm_conv1_fused_bwd wrote behind its workspace " + tag
    for name, t, t0 in zip(("x", "w", "bias", "dp", "scale", "mean", "invstd", "drop", "c1", "c2"), ins, before):
        assert t is None or torch.equal(t.view(G.INT_VIEW[t.dtype]), t0.view(G.INT_VIEW[t.dtype])), "vm_conv1_fused_bwd changed %s %s" % (name, tag)


@pytest.mark.parametrize("dt,regime,n,l,f,wpt,pool,drop,form", G.CONV1_BWD_CASES)
def test_conv1_fused_bwd(dt, regime, n, l, f, wpt, pool, drop, form, f1_tuning):
    """vm_conv1_fused_bwd against gemm_exact.Conv1BwdCase: grad_w = sum bf16(x)[t + k] * bf16(du)[t] and grad_b = sum bf16(du) with du
    from bn_exact.backward on the unrounded z -- the first maximum of a pool window, the first minimum where scale < 0, remainder rows
    in the sums with no pooled gradient.  Grid forms (f1_blocks): the default (one workgroup per chunk), `window` (n: one workgroup
    walks a window's chunks through the double-buffered loop), `split` (2 n: two workgroups per window, 2 + 1 chunks at three chunks).
    The default f1_products = 2 under f16."""
    if form != "default":
        f1_tuning(b"f1_blocks", n if form == "window" else 2 * n)
    c = G.conv1_bwd_case((n, l, f), regime, pool, wpt, drop)
    tag = "%s %s %s wpt %d pool %d drop %d grid %s" % (dt, regime, (n, l, f), wpt, pool, drop, form)
    _conv1_fused_bwd(dt, c, n, l, f, wpt, pool, c.gw, c.gb, tag)


@pytest.mark.parametrize("products", [1, 2, 3])
@pytest.mark.parametrize("regime,n,l,f,wpt,pool,drop", G.CONV1_BWD_PRODUCT_CASES)
def test_conv1_fused_bwd_products(regime, n, l, f, wpt, pool, drop, products, f1_tuning):
    """f1_products 1 / 2 / 3 (VM_F16): the same exact gradients under all three on filters of 8 bits (small) and a waveform a half
    holds (lo-x: under 3 its bf16 lo half makes x_lo * w_hi necessary); lo-w filters, exact only as hi + lo, under 2 and 3 -- and
    under 1 the gradients of z = relu(x * half(w) + b), which the host file has shown to differ: mask and routing follow the
    recomputed z, and the lo product is issued exactly where it is asked for."""
    f1_tuning(b"f1_products", products)
    c = G.conv1_bwd_case((n, l, f), regime, pool, wpt, drop)
    gw, gb = (c.gw_hi, c.gb_hi) if (regime == "lo-w" and products == 1) else (c.gw, c.gb)
    _conv1_fused_bwd("f16", c, n, l, f, wpt, pool, gw, gb, "f16 %s %s pool %d f1_products %d" % (regime, (n, l, f), pool, products))


@pytest.mark.parametrize("what,l,f,pool,dt", [("L < pool", 3, 8, 4, "bf16"), ("pool = 3", 64, 8, 3, "bf16"), ("VM_F32", 64, 8, 2, "f32"),
                                              ("F % 8 != 0", 64, 12, 2, "f16")],
                         ids=["short-window", "pool-3", "fp32-storage", "filters-not-by-8"])
def test_conv1_fused_bwd_refuses(what, l, f, pool, dt):
    """Bad arguments return non-zero before anything is launched: grad_w stays as it was."""
    vm, tdt = DTYPES[dt]
    n, lq = 2, max(l // pool, 1)
    z = lambda *s: torch.zeros(*s, device="cuda")
    gw, gb = _nan(32, 1, f), _nan(f)
    ws = torch.zeros(L().query("vm_conv1_fused_bwd_workspace_bytes", n, 64, 16) // 4, device="cuda")
    dp = torch.zeros(n, lq, f, dtype=tdt, device="cuda")
    rc = L().query("vm_conv1_fused_bwd", p(z(n, l + 31)), p(z(32, 1, f)), p(z(f)), p(dp), p(z(n, f)), p(z(n, f)), p(z(n, f)), None,
                   p(z(n, f)), p(z(n, f)), n, 1, l, f, pool, vm, p(ws), p(gw), p(gb), stream())
    torch.cuda.synchronize()
    assert rc != 0, what
    assert torch.isnan(gw).all() and torch.isnan(gb).all(), what + ": the gradients were written"


# ---- the length-masked inference forms ---------------------------------------------------------------------------------------------------
SENTINEL = 7.0


def _bits(t):
    return t.contiguous().view(G.INT_VIEW[t.dtype])


def _sentinel(n, rows, c, tdt):
    """A padded activation buffer (n, rows + 2, c) no row of which is a result: a row the kernel leaves out keeps the sentinel."""
    return torch.full((n, rows + 2, c), SENTINEL, dtype=tdt, device="cuda")


def _check_masked(act, want, lens, pool, what, note):
    """The masked expectation bit for bit (so the rows at or past lens // pool are +0 in bits: asserted on its own as well) and the
    halo rows untouched."""
    assert_exact(act[:, 1:-1], want, "nlc", what=what, note=note)
    q = torch.arange(want.shape[1], device="cuda")[None, :] >= torch.as_tensor(np.asarray(lens) // pool, device="cuda")[:, None]
    assert not _bits(act[:, 1:-1])[q].any(), what + ": a masked row is not +0"
    assert (act[:, 0] == SENTINEL).all() and (act[:, -1] == SENTINEL).all(), what + ": wrote the halo rows"


def test_varlen_lists_have_served_shapes():
    """Nothing below is skipped: every shape of the masked tables is served in both 16-bit types, packed weights exist where
    conv_nt3_kernel is to be reached, and the hand-off's second layer is served behind either pool."""
    n, l, f, cout = G.CHAIN_SHAPE
    for dt in DT16:
        vm = DTYPES[dt][0]
        for s in G.POOL_VARLEN_SHAPES:
            assert _served("vm_conv_fwd_pool_supported", s, dt), (s, dt)
            assert s[2] not in (128, 256) or L().query("vm_pack_nt_weights_supported", s[3], s[2], vm), (s, dt)
        for pool in (2, 4):
            assert l % pool == 0 and _served("vm_conv_fwd_pool_supported", (n, l // pool, f, cout), dt), (pool, dt)


def _pool_varlen_call(c, x, lens, dt, wf, wfp, varlen=True):
    vm, tdt = DTYPES[dt]
    n, l, cin, cout = c.shape
    act = _sentinel(n, l // 2, cout, tdt)
    args = [p(x), p(wf), p(dev(c.b)), p(dev(c.scale)), p(dev(c.shift))] + ([p(dev(lens, torch.int32))] if varlen else [])
    L().call("vm_conv_fwd_pool_varlen" if varlen else "vm_conv_fwd_pool", *args, n, l, cin, cout, vm, p(act), p(wfp), stream())
    return act


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("n,l,cin,cout", G.POOL_VARLEN_SHAPES)
def test_fwd_pool_varlen(dt, n, l, cin, cout, nt3_lean):
    """vm_conv_fwd_pool_varlen on test_fwd_pool's scale / shift grid, the lengths of gemm_exact.pool_varlen_lens mixed in one launch;
    staged and packed weights, both conv_nt3_kernel prologues.  The masked expectation bit for bit with +0 behind the valid rows, the
    halo rows untouched, and with every lens[n] == L the bytes of vm_conv_fwd_pool on the same input."""
    vm, tdt = DTYPES[dt]
    c = G.pool_varlen_case((n, l, cin, cout))
    want = c.want(dt)
    wf, _ = _prep(c.w, cin, cout, vm, tdt)
    wfp = torch.empty_like(wf)
    xp = padded(c.x, tdt)
    for packed, lean in _packed_runs(cout, cin, vm):
        nt3_lean(lean)
        if packed:
            L().call("vm_pack_nt_weights", p(wf), 1, cout, cin, vm, p(wfp), stream())
        run = "vm_conv_fwd_pool_varlen %s %s packed %d lean %d" % (dt, (n, l, cin, cout), packed, lean)
        act = _pool_varlen_call(c, xp, c.lens, dt, wf, wfp if packed else None)
        _check_masked(act, want, c.lens, 2, run, c.note())
        full = _pool_varlen_call(c, xp, np.full(n, l), dt, wf, wfp if packed else None)
        plain = _pool_varlen_call(c, xp, None, dt, wf, wfp if packed else None, varlen=False)
        assert torch.equal(_bits(full), _bits(plain)), run + ": lens == L differs from vm_conv_fwd_pool"
        assert_exact(plain[:, 1:-1], G.store(c.full, dt), "nlc", what=run + " (vm_conv_fwd_pool on the zero-tailed input)")


def _conv1_varlen_call(c, x, lens, dt, varlen=True):
    vm, tdt = DTYPES[dt]
    n, l, f = c.shape
    out = _sentinel(n, l // c.pool, f, tdt)
    head = [p(x), p(dev(c.w)), p(dev(c.b)), p(dev(c.scale)), p(dev(c.shift))]
    if varlen:
        L().call("vm_conv1_fused_fwd_varlen", *head, p(dev(lens, torch.int32)), n, l, f, c.pool, vm, p(out), stream())
    else:
        L().call("vm_conv1_fused_fwd", *head, n, l, f, c.pool, 1, vm, p(out), None, None, stream())
    return out


@pytest.mark.parametrize("per_window", [0, 1], ids=["default-grid", "one-workgroup-per-window"])
@pytest.mark.parametrize("pool", [2, 4])
@pytest.mark.parametrize("regime", G.CONV1_VARLEN_REGIMES)
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("n,l,f", G.CONV1_VARLEN_SHAPES)
def test_conv1_fused_fwd_varlen(dt, regime, n, l, f, pool, per_window, f1_tuning):
    """vm_conv1_fused_fwd_varlen on test_conv1_fused_fwd's mode-1 grid, the lengths of gemm_exact.conv1_varlen_lens mixed in one launch,
    on the default grid (a workgroup per chunk) and with one workgroup per window (the double-buffered multi-chunk loop).  The same
    assertions as test_fwd_pool_varlen; lens == L against mode 1 of vm_conv1_fused_fwd."""
    if per_window:
        f1_tuning(b"f1_fwd_blocks", n)
    c = G.conv1_varlen_case((n, l, f), regime, pool)
    run = "vm_conv1_fused_fwd_varlen %s %s %s pool %d per-window %d" % (dt, regime, (n, l, f), pool, per_window)
    xd = dev(G.pad_wave(c.x))
    out = _conv1_varlen_call(c, xd, c.lens, dt)
    _check_masked(out, c.want(dt), c.lens, pool, run, c.note())
    full = _conv1_varlen_call(c, xd, np.full(n, l), dt)
    plain = _conv1_varlen_call(c, xd, None, dt, varlen=False)
    assert torch.equal(_bits(full), _bits(plain)), run + ": lens == L differs from mode 1 of vm_conv1_fused_fwd"
    assert_exact(plain[:, 1:-1], G.store(c.full, dt), "nlc", what=run + " (mode 1 on the zero-tailed input)")


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("kernel", ["pool", "conv1"])
def test_varlen_ignores_what_no_valid_row_reads(kernel, dt):
    """Pooled rows at or past lens[n] / pool are zero unconditionally: with NaN at every input position no valid output's taps reach
    (gemm_exact.unreached_from: the reference's own tap range) the whole output, halo rows included, is bit-identical to the clean run."""
    vm, tdt = DTYPES[dt]
    if kernel == "pool":
        c = G.pool_varlen_case(G.POOL_VARLEN_SHAPES[0])
        n, l, cin, cout = c.shape
        x = c.x.copy()
        for i, ln in enumerate(c.lens):
            x[i, G.unreached_from(int(ln), l, "pool"):] = np.nan
        assert np.isnan(x).any() and np.array_equal(np.nan_to_num(x), c.x)
        wf, _ = _prep(c.w, cin, cout, vm, tdt)
        wfp = torch.empty_like(wf)
        L().call("vm_pack_nt_weights", p(wf), 1, cout, cin, vm, p(wfp), stream())
        for packed in (None, wfp):
            clean = _pool_varlen_call(c, padded(c.x, tdt), c.lens, dt, wf, packed)
            dirty = _pool_varlen_call(c, padded(x, tdt), c.lens, dt, wf, packed)
            assert not torch.isnan(clean).any() and torch.equal(_bits(clean), _bits(dirty)), (dt, packed is not None)
    else:
        for pool in (2, 4):
            c = G.conv1_varlen_case(G.CONV1_VARLEN_SHAPES[0], "small", pool)
            n, l, f = c.shape
            x = c.x.copy()
            for i, ln in enumerate(c.lens):
                x[i, G.unreached_from(int(ln), l, "conv1", pool):] = np.nan
            assert np.isnan(x).any() and np.array_equal(np.nan_to_num(x), c.x)
            clean = _conv1_varlen_call(c, dev(G.pad_wave(c.x)), c.lens, dt)
            dirty = _conv1_varlen_call(c, dev(G.pad_wave(x)), c.lens, dt)
            assert not torch.isnan(clean).any() and torch.equal(_bits(clean), _bits(dirty)), (dt, pool)


@pytest.mark.parametrize("pool", [2, 4])
@pytest.mark.parametrize("dt", DT16)
def test_masked_chain_equals_each_recording_alone(dt, pool):
    """vm_conv1_fused_fwd_varlen -> vm_conv_fwd_pool_varlen (lens // pool) -> vm_global_maxpool_fwd_varlen (lens // pool // 2) on one
    bucket of mixed lengths against each recording alone in float64 (gemm_exact.ChainCase.alone): the zeros one launch writes are
    exactly the SAME padding the next one needs.  The buffers between the launches are sentinel-filled except for their halo rows."""
    vm, tdt = DTYPES[dt]
    c = G.chain_case(pool, dt)
    n, l, f, cout = G.CHAIN_SHAPE
    l1, l2 = l // pool, l // pool // 2
    tag = "chain %s pool %d" % (dt, pool)
    act1, act2 = _sentinel(n, l1, f, tdt), _sentinel(n, l2, cout, tdt)
    act1[:, 0], act1[:, -1] = 0, 0                      # the caller's halo rows: the second layer reads them
    L().call("vm_conv1_fused_fwd_varlen", p(dev(G.pad_wave(c.x))), p(dev(c.w1)), p(dev(c.b1)), p(dev(c.s1)), p(dev(c.h1)),
             p(dev(c.lens, torch.int32)), n, l, f, pool, vm, p(act1), stream())
    wf, _ = _prep(c.w2, f, cout, vm, tdt)
    L().call("vm_conv_fwd_pool_varlen", p(act1), p(wf), p(dev(c.b2)), p(dev(c.s2)), p(dev(c.h2)), p(dev(c.lens1, torch.int32)), n, l1, f,
             cout, vm, p(act2), None, stream())
    ws = torch.empty(L().query("vm_bn_drop_pool_gmax_workspace_bytes", n, cout) // 4, device="cuda")
    gmax, gidx = _nan(n, cout), torch.full((n, cout), -7, dtype=torch.int32, device="cuda")
    act2[:, 0], act2[:, -1] = 0, 0
    L().call("vm_global_maxpool_fwd_varlen", p(act2), p(dev(c.lens2, torch.int32)), n, l2, cout, vm, p(gmax), p(gidx), p(ws), stream())
    alone = [c.alone(i) for i in range(n)]
    want1, want2 = np.zeros((n, l1, f)), np.zeros((n, l2, cout))
    for i, (a1, a2, _, _) in enumerate(alone):
        want1[i, :len(a1)], want2[i, :len(a2)] = a1, a2
    assert_exact(act1[:, 1:-1], want1, "nlc", what=tag + " layer 1", note=G.varlen_note(c.lens, lambda ln, q: G.conv1_tile_class(l, pool, ln, q)))
    assert_exact(act2[:, 1:-1], want2, "nlc", what=tag + " layer 2", note=G.varlen_note(c.lens1, lambda ln, q: G.pool_tile_class(l1, ln, q)))
    assert_exact(gmax, np.stack([a[2] for a in alone]), "nc", what=tag + " gmax")
    gi, want_i = gidx.cpu().numpy(), np.stack([a[3] for a in alone])
    assert np.array_equal(gi, want_i), "%s gidx: first at %s" % (tag, np.argwhere(gi != want_i)[:1])
