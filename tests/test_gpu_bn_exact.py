"""-m gpu: the BatchNorm / dropout / max-pool passes of csrc/bnpool.hip on exactly representable inputs (tests/bn_exact.py), every
assertion at tolerance zero -- the one exception, vm_bn_finalize's moving variance, is marked where it is made.  z holds small integers
and every per-channel constant of a call sits on a power-of-two grid, so every product and partial sum is an fp32 number: segment count,
pool groups in flight, reduction order and FMA contraction cannot change a result.  fp32 outputs equal the float64 reference bit for
bit, 16-bit outputs its round-to-nearest-even, and a mismatch is named by window, position and channel.  Outputs start as NaN (halo rows
the caller owns as zero): an element no workgroup wrote is a mismatch.  Partial-row tensors are compared per window after their
vm_bn_part_rows() rows are added in float64; where vm_bn_part_rows_used() is 1, rows 1..7 must be +0.

Which test reaches which path (bn_exact.BN_SHAPES derives each from bn_segs / lanes_for):

  path                                                  reached by
  ----------------------------------------------------  ---------------------------------------------------------------------------
  8 segments per window, two pool groups in flight      every test on (4, 2, 601, 64, 2) in all types, on (3, 3, 1026, 64, 4) (16-bit: exactly
  and the loop's tail                                   the 2048 threshold) and on (2, 2, 64, 512, 1); pairs on (4, 2, 600, 64), (2, 1, 1200, 128)
  1 segment in 16-bit, 8 in fp32                        (3, 3, 1022, 64, 4)
  remainder rows of a floor pool, L % pool 1 / 2 / 3    test_apply on (.., 601, .., 2) / (.., 1026 | 1022 | 10, .., 4) / (.., 67, .., 4)
  idle channel lanes (C / vec no power of two)          (2, 1, 67, 136, 4), (2, 2, 9, 24, 4)
  second trip of the cvb channel loop (C / vec > 256)   f32 on (2, 2, 10, 1032, 4); 16-bit there: P = 256, one row lane
  three towers                                          (6, 2, 50, 16, 2); test_sparse on (390, 130, ..); test_bn_finalize with 3 towers
  first extreme of tied positive values, strict >,      every case (bn_exact asserts >= 1 % of the groups tied with dp != 0), negative
  sgn of negative scale * drop, sign-bit flag           scale * drop and dropped channels in every case; pairs: test_pairs
  bn_bwd_gmax_finalize_kernel: odd tower count,         test_sparse on (1, 1, ..) and (390, 130, ..) / on (258, 129, ..) and (390, 130, ..)
  second trip of w0 += 32 * U
  scale == 0 vector of the pooled / from-sums forms     channel 5 of every case in test_reduce
  colreduce stage 1 + finalize, fused and two-launch    test_reduce, test_bn_finalize, test_bn_bwd_finalize under fuse_finalize 0 / 17 / 31 / 15
  apply_order 0 / 1 / 2                                 test_apply, test_pairs
"""
import numpy as np
import pytest
import torch

from tests import bn_exact as B
from tests.gemm_exact import assert_exact, store
from tests.gpu_util import DTYPES, L, dev, p, padded, stream

pytestmark = pytest.mark.gpu

ROWS = B.PART_ROWS
APPLY_ORDERS, APPLY_ORDER_DEFAULT = (0, 1, 2), 2      # tests/test_abi.py pins the defaults
FUSE_MASKS, FUSE_DEFAULT = (0, 17, 31, 15), 17        # 15: every reduction finishes in its stage-1 launch, wide layers included


def _nan(*shape, dtype=torch.float32, halo=False):
    """An output buffer no element of which is a valid result; halo: rows 0 and -1 are the caller's zeros."""
    t = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
    if halo:
        t[:, 0] = 0
        t[:, -1] = 0
    return t


def _ints(*shape):
    return torch.full(shape, -7, dtype=torch.int32, device="cuda")


def _f64(t):
    return t.detach().cpu().to(torch.float64)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def assert_int_exact(got, want, what):
    g, w = got.cpu().numpy(), np.asarray(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = g != w
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d positions differ; first at (window %d, channel %d): got %d, want %d" % (
            what, bad.sum(), bad.size, i[0], i[-1], g[i], w[i]))


def _check_halo(t, what):
    assert_exact(t[:, [0, -1]], np.zeros((t.shape[0], 2, t.shape[2])), "nlc", what=what + " halo rows")


def _check_rows(part, n, c, want, used, what):
    """fp32 partial rows (n * ROWS, c) against the per-window reference (n, c)."""
    assert_exact(_f64(part).view(n, ROWS, c).sum(1), want, "nc", neg_zero=True, what=what)     # (a factor may be exactly 0: drop)
    if used == 1:
        assert_exact(part.view(n, ROWS, c)[:, 1:], np.zeros((n, ROWS - 1, c)), "nrc", what=what + " rows 1..%d" % (ROWS - 1))


class Dev:
    """Device copies of a BnCase in one storage type."""

    def __init__(self, c, dt):
        self.vm, self.tdt = DTYPES[dt]
        n, wpt, l, ch, pool, _ = c.shape
        self.z, self.dp = dev(c.z, self.tdt), dev(c.dp, self.tdt)
        self.scale, self.shift, self.mean, self.invstd = dev(c.scale), dev(c.shift), dev(c.mean), dev(c.invstd)
        self.c1, self.c2, self.dg = dev(c.c1), dev(c.c2), dev(c.dg)
        self.drop = None if c.drop is None else dev(c.drop)
        self.bn = (p(self.scale), p(self.shift), p(self.mean), p(self.invstd), p(self.drop))
        self.fwd = (p(self.scale), p(self.shift), p(self.drop))
        self.dims = (n, wpt, l, ch)
        self.used = L().query("vm_bn_part_rows_used", l, ch, pool, self.vm)
        assert self.used == B.bn_segs(l // pool, ch, dt)
        self.crws = torch.empty(L().query("vm_colreduce_workspace_bytes", n // wpt, ch) // 8, dtype=torch.float64, device="cuda")
        self.gws = torch.empty(L().query("vm_bn_drop_pool_gmax_workspace_bytes", max(n, 4), ch) // 4, device="cuda")


def _at_each(key, values, default, launch):
    """launch() under every value of the tuning key; the default is restored whatever happens."""
    outs = []
    try:
        for v in values:
            L().call("vm_set_tuning", key, v)
            outs.append(launch())
            torch.cuda.synchronize()
    finally:
        L().call("vm_set_tuning", key, default)
    return outs


def _same_bits(outs, what):
    for v, o in enumerate(outs[1:], 1):
        for a, b in zip(outs[0], o):
            assert torch.equal(_bits(a), _bits(b)), "%s: variant %d differs from variant 0" % (what, v)


def test_part_rows():
    assert L().query("vm_bn_part_rows") == ROWS


# ---- forward: BN apply + dropout + max-pool, the global-max forms ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", B.DTS)
@pytest.mark.parametrize("shape", B.BN_SHAPES, ids=str)
def test_forward(shape, dt):
    c = B.bn_case(shape)
    d = Dev(c, dt)
    n, wpt, l, ch, pool, _ = shape
    lq, tag = c.lq, "%s %s" % (dt, shape)
    out = _nan(n, lq + 2, ch, dtype=d.tdt, halo=True)
    L().call("vm_bn_drop_pool_fwd", p(d.z), *d.fwd, n, wpt, l, ch, pool, d.vm, p(out), stream())
    assert_exact(out[:, 1:-1], c.out, "nqc", neg_zero=True, what="vm_bn_drop_pool_fwd " + tag)      # ((..) * drop with drop == 0)
    _check_halo(out, "vm_bn_drop_pool_fwd " + tag)
    gmax_ref, gidx_ref = B.global_max(c.out, dt)
    assert np.array_equal(gidx_ref, c.gidx)

    g, gi = _nan(n, ch), _ints(n, ch)
    L().call("vm_bn_drop_pool_gmax_fwd", p(d.z), *d.fwd, n, wpt, l, ch, pool, d.vm, p(g), p(gi), p(d.gws), stream())
    assert_exact(g, gmax_ref, "nc", neg_zero=True, what="vm_bn_drop_pool_gmax_fwd gmax " + tag)
    assert_int_exact(gi, gidx_ref, "vm_bn_drop_pool_gmax_fwd gidx " + tag)

    pv, pi = _nan(n * ROWS, ch), _ints(n * ROWS, ch)
    L().call("vm_bn_drop_pool_gmax_partials", p(d.z), *d.fwd, n, wpt, l, ch, pool, d.vm, p(pv), p(pi), stream())
    pvn, pin = pv.cpu().numpy().reshape(n, ROWS, ch), pi.cpu().numpy().reshape(n, ROWS, ch)
    bv, bi = B.reduce_partials(pvn, pin)
    assert_exact(torch.tensor(bv), gmax_ref, "nc", neg_zero=True, what="vm_bn_drop_pool_gmax_partials, reduced: gmax " + tag)
    assert_int_exact(torch.tensor(bi), gidx_ref, "vm_bn_drop_pool_gmax_partials, reduced: gidx " + tag)
    assert np.array_equal(bv, g.cpu().numpy().astype(np.float64)) and np.array_equal(bi, gi.cpu().numpy())
    if d.used == 1:                       # one workgroup per window: the other rows are "empty"
        assert (pin[:, 1:] == B.EMPTY).all() and (pvn[:, 1:] == -np.inf).all()
    else:                                 # every segment holds a row of its own: its position is one of its rows
        seg = np.arange(ROWS)[None, :, None]
        assert ((pin == B.EMPTY) | (pin % ROWS == seg)).all() and ((pin != B.EMPTY) | (lq <= seg)).all()

    # GlobalMaxPool1D on the pooled tensor, and its backward
    act = padded(c.out, d.tdt)
    g2, gi2 = _nan(n, ch), _ints(n, ch)
    L().call("vm_global_maxpool_fwd", p(act), n, lq, ch, d.vm, p(g2), p(gi2), stream())
    assert_exact(g2, gmax_ref, "nc", neg_zero=True, what="vm_global_maxpool_fwd gmax " + tag)
    assert_int_exact(gi2, gidx_ref, "vm_global_maxpool_fwd gidx " + tag)
    for which, gix in (("fwd", c.gidx), ("rand", c.gidx_r)):
        dpd = _nan(n, lq, ch, dtype=d.tdt)
        L().call("vm_global_maxpool_bwd", p(d.dg), p(dev(gix, torch.int32)), n, lq, ch, d.vm, p(dpd), stream())
        assert_exact(dpd, B.dense_dp(c.dg, gix, lq, dt), "nqc", what="vm_global_maxpool_bwd (%s) %s" % (which, tag))


@pytest.mark.parametrize("dt", B.DTS)
@pytest.mark.parametrize("shape", [s for s in B.BN_SHAPES if s[2] > s[4] + 1], ids=str)
def test_forward_varlen(shape, dt):
    """The three length-masked forwards, lens in {pool, pool + 1, L - 1, L} mixed in one call (one tower, no dropout)."""
    c = B.bn_case(shape)
    vm, tdt = DTYPES[dt]
    _, _, l, ch, pool, _ = shape
    n, lq, tag = 4, c.lq, "%s %s" % (dt, shape)
    z = c.z[np.arange(n) % shape[0]]
    lens = np.array([pool, pool + 1, l - 1, l], dtype=np.int32)
    scale, shift = c.scale[:1], c.shift[:1]
    full = B.forward(z, scale, shift, None, n, pool)
    valid = np.arange(lq)[None, :, None] < (lens // pool)[:, None, None]
    zd, sc, sh, ld = dev(z, tdt), dev(scale), dev(shift), dev(lens, torch.int32)
    out = _nan(n, lq + 2, ch, dtype=tdt, halo=True)
    L().call("vm_bn_drop_pool_fwd_varlen", p(zd), p(sc), p(sh), p(ld), n, l, ch, pool, vm, p(out), stream())
    assert_exact(out[:, 1:-1], np.where(valid, full, 0.0), "nqc", neg_zero=True, what="vm_bn_drop_pool_fwd_varlen " + tag)
    _check_halo(out, "vm_bn_drop_pool_fwd_varlen " + tag)
    gmax_ref, gidx_ref = B.global_max(full, dt, lens // pool)
    ws = torch.empty(L().query("vm_bn_drop_pool_gmax_workspace_bytes", n, ch) // 4, device="cuda")
    g, gi = _nan(n, ch), _ints(n, ch)
    L().call("vm_bn_drop_pool_gmax_fwd_varlen", p(zd), p(sc), p(sh), p(ld), n, l, ch, pool, vm, p(g), p(gi), p(ws), stream())
    assert_exact(g, gmax_ref, "nc", neg_zero=True, what="vm_bn_drop_pool_gmax_fwd_varlen gmax " + tag)
    assert_int_exact(gi, gidx_ref, "vm_bn_drop_pool_gmax_fwd_varlen gidx " + tag)
    # GlobalMaxPool1D over the first rows of the (unmasked) pooled tensor: 1, 2, Lq - 1, Lq of them
    rows = np.array([1, min(2, lq), max(lq - 1, 1), lq], dtype=np.int32)
    gmax_ref, gidx_ref = B.global_max(full, dt, rows)
    g, gi = _nan(n, ch), _ints(n, ch)
    L().call("vm_global_maxpool_fwd_varlen", p(padded(full, tdt)), p(dev(rows, torch.int32)), n, lq, ch, vm, p(g), p(gi), p(ws), stream())
    assert_exact(g, gmax_ref, "nc", what="vm_global_maxpool_fwd_varlen gmax " + tag)
    assert_int_exact(gi, gidx_ref, "vm_global_maxpool_fwd_varlen gidx " + tag)


# ---- backward, pass 1: the two sums and their finalize ---------------------------------------------------------------------------------------
def _finalize_outputs(towers, ch):
    return _nan(towers, ch), _nan(towers, ch), _nan(ch), _nan(ch)


def _check_finalize(outs, ref, what):
    for got, want, name, lay in zip(outs, ref, ("c1", "c2", "grad_gamma", "grad_beta"), ("tc", "tc", "c", "c")):
        assert_exact(got, want, lay, neg_zero=True, what="%s %s" % (what, name))


@pytest.mark.parametrize("dt", B.DTS)
@pytest.mark.parametrize("shape", B.BN_SHAPES, ids=str)
def test_reduce(shape, dt):
    c = B.bn_case(shape)
    d = Dev(c, dt)
    n, wpt, l, ch, pool, _ = shape
    towers, tag = c.towers, "%s %s" % (dt, shape)
    tail = (n, wpt, l, ch, pool, d.vm)
    pa, pb = _nan(n * ROWS, ch), _nan(n * ROWS, ch)
    L().call("vm_bn_pool_bwd_reduce", p(d.z), p(d.dp), *d.bn, *tail, p(pa), p(pb), stream())
    _check_rows(pa, n, ch, c.sdy, d.used, "vm_bn_pool_bwd_reduce part_dy " + tag)
    _check_rows(pb, n, ch, c.sdyz, d.used, "vm_bn_pool_bwd_reduce part_dyz " + tag)
    # the pooled form: on the grid act is exact, so the recovered extreme is the extreme (the scale == 0 vector comes from z)
    qa, qb = _nan(n * ROWS, ch), _nan(n * ROWS, ch)
    L().call("vm_bn_pool_bwd_reduce_pooled", p(d.z), p(padded(c.out, d.tdt)), p(d.dp), *d.bn, *tail, p(qa), p(qb), stream())
    _check_rows(qa, n, ch, c.sdy, d.used, "vm_bn_pool_bwd_reduce_pooled part_dy " + tag)
    _check_rows(qb, n, ch, c.sdyz, d.used, "vm_bn_pool_bwd_reduce_pooled part_dyz " + tag)
    assert_exact(qa, _f64(pa), "nc", neg_zero=True, what="pooled form == z form, part_dy " + tag)
    assert_exact(qb, _f64(pb), "nc", neg_zero=True, what="pooled form == z form, part_dyz " + tag)

    ref = B.finalize(c.sdy, c.sdyz, wpt, c.count)

    def fin():
        o = _finalize_outputs(towers, ch)
        L().call("vm_bn_bwd_finalize", p(pa), p(pb), n, wpt, ch, c.count, *map(p, o), p(d.crws), stream())
        return o
    outs = _at_each(b"fuse_finalize", FUSE_MASKS, FUSE_DEFAULT, fin)
    _check_finalize(outs[0], ref, "vm_bn_bwd_finalize " + tag)
    _same_bits(outs, "vm_bn_bwd_finalize under fuse_finalize " + tag)

    # the same sums from S0 = sum dp and SA = sum dp * A left behind by the dgrad epilogue, A the pooled output or the extreme
    r = np.random.default_rng(n + l)
    for a_is_act, sa in ((1, c.sa_act), (0, c.sa_ext)):
        for rows in (1, 3):
            s0d, sad = dev(B.split_rows(r, c.s0, rows)), dev(B.split_rows(r, sa, rows))
            head = (p(s0d), p(sad), rows, p(d.z), p(d.dp), *d.bn, n, wpt, l, ch, pool, d.vm, a_is_act)
            what = "(a_is_act %d, %d rows) %s" % (a_is_act, rows, tag)
            fa, fb = _nan(n * ROWS, ch), _nan(n * ROWS, ch)
            L().call("vm_bn_bwd_from_sums", *head, p(fa), p(fb), stream())
            _check_rows(fa, n, ch, c.sdy, 1, "vm_bn_bwd_from_sums part_dy " + what)
            _check_rows(fb, n, ch, c.sdyz, 1, "vm_bn_bwd_from_sums part_dyz " + what)

            def fin2():
                o = _finalize_outputs(towers, ch)
                L().call("vm_bn_bwd_from_sums_finalize", *head, c.count, *map(p, o), p(d.crws), stream())
                return o
            outs = _at_each(b"fuse_finalize", FUSE_MASKS[:3], FUSE_DEFAULT, fin2)
            _check_finalize(outs[0], ref, "vm_bn_bwd_from_sums_finalize " + what)
            _same_bits(outs, "vm_bn_bwd_from_sums_finalize under fuse_finalize " + what)


# ---- backward, pass 2: du and its column sums ---------------------------------------------------------------------------------------------------
def _apply_each_order(launch, n, l, ch, tdt):
    def run():
        du, pdu = _nan(n, l + 2, ch, dtype=tdt, halo=True), _nan(n * ROWS, ch)
        launch(du, pdu)
        return du, pdu
    return _at_each(b"apply_order", APPLY_ORDERS, APPLY_ORDER_DEFAULT, run)


def _check_apply(outs, du_ref, dt, n, ch, used, what):
    du, pdu = outs[0]
    want = store(du_ref, dt)
    assert_exact(du[:, 1:-1], want, "nlc", neg_zero=True, what=what + " du")         # ([z > 0] * (..): the sign of a zero is free)
    _check_halo(du, what + " du")
    _check_rows(pdu, n, ch, want.sum(1), used, what + " part_du")
    _same_bits(outs, what + " under apply_order")


@pytest.mark.parametrize("dt", B.DTS)
@pytest.mark.parametrize("shape", B.BN_SHAPES, ids=str)
def test_apply(shape, dt):
    c = B.bn_case(shape)
    d = Dev(c, dt)
    n, wpt, l, ch, pool, _ = shape
    tag = "%s %s" % (dt, shape)
    tail = (p(d.c1), p(d.c2), n, wpt, l, ch, pool, d.vm)
    outs = _apply_each_order(lambda du, pdu: L().call("vm_bn_pool_bwd_apply", p(d.z), p(d.dp), *d.bn, *tail, p(du), p(pdu), stream()),
                             n, l, ch, d.tdt)
    _check_apply(outs, c.du, dt, n, ch, d.used, "vm_bn_pool_bwd_apply " + tag)
    for which in ("fwd", "rand"):
        gix, _, ref = c.sparse(which, dt)
        gd = dev(gix, torch.int32)
        outs = _apply_each_order(lambda du, pdu: L().call("vm_bn_pool_bwd_apply_gmax", p(d.z), p(d.dg), p(gd), *d.bn, *tail, p(du), p(pdu),
                                                          stream()), n, l, ch, d.tdt)
        _check_apply(outs, ref[2], dt, n, ch, d.used, "vm_bn_pool_bwd_apply_gmax (%s) %s" % (which, tag))


# ---- the sparse (GlobalMaxPool1D-backward) sums ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", B.DTS)
@pytest.mark.parametrize("shape", B.SPARSE_SHAPES, ids=str)
def test_sparse(shape, dt):
    c = B.bn_case(shape)
    d = Dev(c, dt)
    n, wpt, l, ch, pool, _ = shape
    for which in ("fwd", "rand"):
        gix, _, (_, _, _, sdy, sdyz) = c.sparse(which, dt)
        gd = dev(gix, torch.int32)
        what = "(%s) %s %s" % (which, dt, shape)
        pa, pb = _nan(n * ROWS, ch), _nan(n * ROWS, ch)
        L().call("vm_bn_pool_bwd_reduce_gmax", p(d.z), p(d.dg), p(gd), *d.bn, n, wpt, l, ch, pool, d.vm, p(pa), p(pb), stream())
        _check_rows(pa, n, ch, sdy, 1, "vm_bn_pool_bwd_reduce_gmax part_dy " + what)
        _check_rows(pb, n, ch, sdyz, 1, "vm_bn_pool_bwd_reduce_gmax part_dyz " + what)
        o = _finalize_outputs(c.towers, ch)
        L().call("vm_bn_bwd_gmax_finalize", p(d.z), p(d.dg), p(gd), *d.bn, n, wpt, l, ch, pool, d.vm, c.count, *map(p, o), stream())
        _check_finalize(o, B.finalize(sdy, sdyz, wpt, c.count), "vm_bn_bwd_gmax_finalize " + what)


# ---- the pair forms (e, o) of vm_conv_fwd_fold ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", B.DT16)
@pytest.mark.parametrize("shape", B.PAIR_SHAPES, ids=str)
def test_pairs(shape, dt):
    c = B.bn_case(shape)
    d = Dev(c, dt)
    n, wpt, l, ch, pool, _ = shape
    lq, tag = c.lq, "%s %s" % (dt, shape)
    tail = (p(d.c1), p(d.c2), n, wpt, l, ch)
    on_z = _apply_each_order(lambda du, pdu: L().call("vm_bn_pool_bwd_apply", p(d.z), p(d.dp), *d.bn, *tail, 2, d.vm, p(du), p(pdu), stream()),
                             n, l, ch, d.tdt)
    for centred in (False, True):
        ctr = c.e_center if centred else None
        e, o = (t.cuda() for t in B.pair_encode(c.z, c.gamma, dt, ctr, wpt))
        ctrd = dev(ctr) if centred else None
        outs = _apply_each_order(lambda du, pdu: L().call("vm_bn_pool_bwd_apply_pairs", p(e), p(o), p(d.dp), *d.bn, *tail, d.vm, p(du), p(pdu),
                                                          p(ctrd), stream()), n, l, ch, d.tdt)
        what = "vm_bn_pool_bwd_apply_pairs (e_center %s) %s" % (centred, tag)
        _check_apply(outs, c.du, dt, n, ch, d.used, what)
        _same_bits([on_z[0], outs[0]], what + " == vm_bn_pool_bwd_apply on z")
        torch.cuda.synchronize()
    e, o = (t.cuda() for t in B.pair_encode(c.z, c.gamma, dt))
    gmax_ref, gidx_ref = B.global_max(c.out, dt)
    parts = []
    for name, args in (("vm_bn_drop_pool_gmax_partials_e", (p(e), *d.fwd, n, wpt, lq, ch, d.vm)),
                       ("vm_bn_drop_pool_gmax_partials", (p(d.z), *d.fwd, n, wpt, l, ch, 2, d.vm))):
        pv, pi = _nan(n * ROWS, ch), _ints(n * ROWS, ch)
        L().call(name, *args, p(pv), p(pi), stream())
        bv, bi = B.reduce_partials(pv.cpu().numpy().reshape(n, ROWS, ch), pi.cpu().numpy().reshape(n, ROWS, ch))
        assert_exact(torch.tensor(bv), gmax_ref, "nc", neg_zero=True, what="%s, reduced: gmax %s" % (name, tag))
        assert_int_exact(torch.tensor(bi), gidx_ref, "%s, reduced: gidx %s" % (name, tag))
        parts.append((pv, pi))
    # the two forms row by row (a dropped channel's zeros may differ in sign: the z form keeps the first element's, e holds the extreme)
    assert_exact(parts[0][0], _f64(parts[1][0]), "nc", neg_zero=True, what="vm_bn_drop_pool_gmax_partials_e == _partials on z, part_v " + tag)
    assert torch.equal(parts[0][1], parts[1][1]), "vm_bn_drop_pool_gmax_partials_e == _partials on z, part_i " + tag
    for which in ("fwd", "rand"):
        gix, _, (_, _, du_ref, sdy, sdyz) = c.sparse(which, dt)
        gd = dev(gix, torch.int32)
        what = "(%s) %s" % (which, tag)
        fins = []
        for name, args in (("vm_bn_bwd_gmax_finalize_e", (p(e), p(d.dg), p(gd), *d.bn, n, wpt, lq, ch, d.vm)),
                           ("vm_bn_bwd_gmax_finalize", (p(d.z), p(d.dg), p(gd), *d.bn, n, wpt, l, ch, 2, d.vm))):
            f = _finalize_outputs(c.towers, ch)
            L().call(name, *args, c.count, *map(p, f), stream())
            _check_finalize(f, B.finalize(sdy, sdyz, wpt, c.count), "%s %s" % (name, what))
            fins.append(f)
        _same_bits(fins, "vm_bn_bwd_gmax_finalize_e == _finalize on z " + what)
        outs = _apply_each_order(lambda du, pdu: L().call("vm_bn_pool_bwd_apply_pairs_gmax", p(e), p(o), p(d.dg), p(gd), *d.bn, *tail, d.vm,
                                                          p(du), p(pdu), stream()), n, l, ch, d.tdt)
        _check_apply(outs, du_ref, dt, n, ch, d.used, "vm_bn_pool_bwd_apply_pairs_gmax " + what)
        torch.cuda.synchronize()


# ---- the statistics ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("center", [None, "bias", "tile"])
@pytest.mark.parametrize("shape", B.FINALIZE_SHAPES, ids=str)
def test_bn_finalize(shape, center):
    """vm_bn_finalize on sums chosen so that every output is an fp32 number (bn_exact.FinalizeCase): mean, invstd, scale, shift, shift_adj,
    mean_adj, the moving mean and the zero-debias mean accumulators bit for bit, in the zero-debias and the plain form, under every
    fuse_finalize mask.  THE ONE TOLERANCE of this file: the moving variance carries count / (count - (1 + eps)), which is not dyadic; it
    is held to 1 fp32 ulp of the float64 value in the zero-debias form and to bn_exact.PLAIN_MV_ULPS ulp per tower in the plain form, whose
    towers chain their roundings (the bound is derived there)."""
    f = B.FinalizeCase(shape, center)
    rows, towers, c = shape
    ssum, ssq, gamma, beta = dev(f.stat_sum), dev(f.stat_sq), dev(f.gamma), dev(f.beta)
    cb = None if f.center_bias is None else dev(f.center_bias)
    tc = None if f.tile_center is None else dev(f.tile_center)
    ws = torch.empty(L().query("vm_colreduce_workspace_bytes", towers, c) // 8, dtype=torch.float64, device="cuda")
    for zero_debias in (True, False):
        def run():
            o = dict(mm=dev(f.mm0).clone(), mv=dev(f.mv0).clone(), zd=dev(f.zd0).clone() if zero_debias else None)
            for k in ("mean", "invstd", "scale", "shift", "shift_adj", "mean_adj"):
                o[k] = _nan(towers, c)
            adj = (p(o["shift_adj"]), p(o["mean_adj"])) if center else (None, None)
            L().call("vm_bn_finalize", p(ssum), p(ssq), rows, towers, c, f.COUNT, p(gamma), p(beta), f.EPS, f.MOMENTUM, 1, p(o["mm"]),
                     p(o["mv"]), p(o["mean"]), p(o["invstd"]), p(o["scale"]), p(o["shift"]), p(ws), p(o["zd"]),
                     f.ZD_CORRECTION if zero_debias else 0.0, p(cb), adj[0], adj[1], p(tc), stream())
            return o
        outs = _at_each(b"fuse_finalize", FUSE_MASKS, FUSE_DEFAULT, run)
        what = "vm_bn_finalize (%s, center %s) %s" % ("zero-debias" if zero_debias else "plain", center, shape)
        o = outs[0]
        for k, want in (("mean", f.m), ("invstd", f.istd), ("scale", f.scale), ("shift", f.shift)):
            assert_exact(o[k], want, "tc", neg_zero=True, what="%s %s" % (what, k))            # (gamma == 0: scale, mean * scale)
        if center:
            assert_exact(o["shift_adj"], f.shift_adj, "tc", neg_zero=True, what=what + " shift_adj")
            assert_exact(o["mean_adj"], f.mean_adj, "tc", what=what + " mean_adj")
        assert_exact(o["mm"], f.mm_zd if zero_debias else f.mm_plain, "c", what=what + " moving_mean")
        mv_ref = f.mv_zd if zero_debias else f.mv_plain
        ulps = 1.0 if zero_debias else B.PLAIN_MV_ULPS * towers
        err = np.abs(_f64(o["mv"]).cpu().numpy() - mv_ref) / B.ulp32(mv_ref)
        assert err.max() <= ulps, "%s moving_var: %.2f ulp at channel %d (allowed: %.1f)" % (what, err.max(), int(err.argmax()), ulps)
        if zero_debias:
            assert_exact(o["zd"][:, 0], f.zd[:, 0], "tc", what=what + " zero-debias mean accumulators")
            err = np.abs(_f64(o["zd"][:, 1]).cpu().numpy() - f.zd[:, 1]) / B.ulp32(f.zd[:, 1])
            assert err.max() <= 1.0, "%s zero-debias variance accumulators: %.2f ulp" % (what, err.max())
        keys = [k for k in o if o[k] is not None and (center or k not in ("shift_adj", "mean_adj"))]
        _same_bits([[v[k] for k in keys] for v in outs], what + " under fuse_finalize")


@pytest.mark.parametrize("shape", B.FINALIZE_SHAPES, ids=str)
def test_bn_bwd_finalize(shape):
    """vm_bn_bwd_finalize on partial rows that are inputs: `shape[0]` windows per tower, 8 rows each, multiples of 1/8."""
    wpt, towers, c = shape
    n, count = wpt * towers, 3000.0
    r = np.random.default_rng([wpt, towers, c, 5])
    pa, pb = (r.integers(-64, 65, (n * ROWS, c)).astype(np.float64) / 8 for _ in range(2))
    ref = B.finalize(pa.reshape(n, ROWS, c).sum(1), pb.reshape(n, ROWS, c).sum(1), wpt, count)
    pad, pbd = dev(pa), dev(pb)
    ws = torch.empty(L().query("vm_colreduce_workspace_bytes", towers, c) // 8, dtype=torch.float64, device="cuda")

    def fin():
        o = _finalize_outputs(towers, c)
        L().call("vm_bn_bwd_finalize", p(pad), p(pbd), n, wpt, c, count, *map(p, o), p(ws), stream())
        return o
    outs = _at_each(b"fuse_finalize", FUSE_MASKS, FUSE_DEFAULT, fin)
    _check_finalize(outs[0], ref, "vm_bn_bwd_finalize %s" % (shape,))
    _same_bits(outs, "vm_bn_bwd_finalize under fuse_finalize %s" % (shape,))


@pytest.mark.parametrize("c", [8, 40, 264])
def test_bn_infer_affine(c):
    """moving_var + eps = 4^k exactly (eps = 2^-10): scale = gamma / sqrt(..) and shift = beta - moving_mean * scale are fp32 numbers."""
    r = np.random.default_rng(c)
    eps = 2.0 ** -10
    istd = r.choice([0.5, 1.0, 2.0], c)
    mv = 1.0 / istd ** 2 - eps
    gamma = r.choice([0.5, 1.0, 2.0], c) * r.choice([-1.0, 1.0], c)
    gamma[5] = 0.0
    beta, mm = r.integers(-8, 9, c) / 4, r.integers(-8, 9, c) / 4
    sc, sh = _nan(c), _nan(c)
    L().call("vm_bn_infer_affine", p(dev(gamma)), p(dev(beta)), p(dev(mm)), p(dev(mv)), eps, c, p(sc), p(sh), stream())
    assert_exact(sc, gamma * istd, "c", neg_zero=True, what="vm_bn_infer_affine scale")
    assert_exact(sh, beta - mm * gamma * istd, "c", neg_zero=True, what="vm_bn_infer_affine shift")
