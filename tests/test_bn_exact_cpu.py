"""Host checks of tests/bn_exact.py: every case tests/test_gpu_bn_exact.py runs is constructed here (its preconditions and census
conditions are assertions of the constructors), the float64 references are checked against autograd, the pair encoder against its
decoder, and the comparator against three planted errors of the kind a ratio of norms passes."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_exact as B
from tests.gemm_exact import assert_exact, exact_in, store
from tests.gpu_util import rel_err
from tests.test_gpu_kernels import _bn_block_oracle

ALL_SHAPES = list(dict.fromkeys(B.BN_SHAPES + B.PAIR_SHAPES + B.SPARSE_SHAPES))


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_cases_meet_their_preconditions(shape):
    c = B.bn_case(shape)          # asserts exact_in, require_exact_sums and the census conditions
    n, wpt, l, ch, pool, use_drop = shape
    print("%s: positive-tie share %.3f, bf16 du rounded %.3f with %d ties, largest sum %.3g grid units" % (
        shape, c.tie_share, c.bf16_rounded, c.bf16_ties, max(c.head.values())))
    assert max(c.head.values()) < 2.0 ** 24
    for dt in B.DTS:
        for which in ("fwd", "rand"):           # the sparse form: one routed value per (window, channel)
            gi, dp, (dy, zhat, du, sdy, sdyz) = c.sparse(which, dt)
            assert exact_in(dp, dt) and exact_in(du, "f32") and (dp != 0).sum(1).max() <= 1
            assert gi.min() >= 0 and gi.max() < c.lq


def test_shape_tables_reach_the_edges_their_comments_claim():
    """From the launch arithmetic alone (bn_segs, lanes_for): what each entry of the tables is there for."""
    L = {s[:5]: {dt: B.launch(s[2], s[3], s[4], dt) for dt in B.DTS} for s in B.BN_SHAPES + B.PAIR_SHAPES}
    seg = lambda s, dt: L[s][dt][3]
    assert all(seg((4, 2, 601, 64, 2), dt) == 8 for dt in B.DTS) and L[(4, 2, 601, 64, 2)]["f32"][5] == 1
    for dt in B.DTS:                            # the two-in-flight loop runs and leaves a tail
        stride, lq = L[(4, 2, 601, 64, 2)][dt][4], 300
        assert stride < lq and lq % (2 * stride) != 0
    assert 256 * (64 // 8) == 2048 and seg((3, 3, 1026, 64, 4), "bf16") == 8 and L[(3, 3, 1026, 64, 4)]["f32"][5] == 2
    assert [seg((3, 3, 1022, 64, 4), dt) for dt in B.DTS] == [8, 1, 1]
    assert L[(2, 1, 67, 136, 4)]["f32"][:2] == (34, 64) and L[(2, 1, 67, 136, 4)]["f16"][:2] == (17, 32) and L[(2, 1, 67, 136, 4)]["f32"][5] == 3
    assert L[(2, 2, 10, 1032, 4)]["f32"][:2] == (258, 256) and L[(2, 2, 10, 1032, 4)]["bf16"][:3] == (129, 256, 1)
    assert {s[2] % s[4] for s in B.BN_SHAPES} == {0, 1, 2, 3}
    assert any(s[0] // s[1] == 3 for s in B.BN_SHAPES) and any(s[2] == s[4] for s in B.BN_SHAPES) and any(s[4] == 1 for s in B.BN_SHAPES)
    assert all(s[4] == 2 and s[2] % 2 == 0 for s in B.PAIR_SHAPES)
    assert [seg(s[:5], "f16") for s in B.PAIR_SHAPES] == [8, 8, 1, 1]
    wpts = [s[1] for s in B.SPARSE_SHAPES]
    assert any(w > 128 for w in wpts) and any((s[0] // s[1]) % 2 == 1 for s in B.SPARSE_SHAPES) and any(32 < w < 128 for w in wpts)
    assert B.SPARSE_SHAPES[-1] == B.BN_SHAPES[0]


@pytest.mark.parametrize("pool,l", [(2, 23), (4, 23), (1, 7)])
def test_references_equal_autograd_on_true_batch_statistics(pool, l):
    """Non-dyadic inputs, the statistics of the batch itself: the pooled output, du, dgamma and dbeta of bn_exact's references equal
    those of _bn_block_oracle (O.batchnorm_train -> dropout -> O.maxpool1d under autograd) to 1e-12.  The gamma == 0 channel is left
    out of dgamma: there y is constant, autograd routes dp to the group's first element and the library to its largest z (the
    documented rule); that channel is checked against the rule written out."""
    n, wpt, c, eps = 4, 2, 16, 1e-3
    r = np.random.default_rng(pool)
    z = np.maximum(r.normal(0.2, 1.0, (n, l, c)), 0.0)
    gamma = r.normal(1.0, 0.3, c) * np.where(r.random(c) < 0.3, -1, 1)
    gamma[5] = 0.0
    beta = r.normal(0, 0.3, c)
    drop = (r.random((n, c)) > 0.3) / 0.7
    drop[:, 5] = 1 / 0.7
    dp = r.normal(0, 1, (n, l // pool, c))
    zt = z.reshape(n // wpt, wpt * l, c)
    mean, var = zt.mean(1), zt.var(1)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma[None, :] * invstd
    shift = beta[None, :] - mean * scale
    out = B.forward(z, scale, shift, drop, wpt, pool)
    zero = np.zeros_like(scale)
    _, _, _, sdy, sdyz = B.backward(z, dp, scale, mean, invstd, drop, zero, zero, wpt, pool)
    cnt = float(wpt * l)
    c1, c2 = sdy.reshape(n // wpt, wpt, c).sum(1) / cnt, sdyz.reshape(n // wpt, wpt, c).sum(1) / cnt
    du = B.backward(z, dp, scale, mean, invstd, drop, c1, c2, wpt, pool)[2]

    zr, gr, br = (torch.tensor(v, requires_grad=True) for v in (z, gamma, beta))
    out_ref, _ = _bn_block_oracle(zr, gr, br, torch.tensor(drop), pool, wpt, eps)
    gz, gg, gb = torch.autograd.grad((out_ref * torch.tensor(dp)).sum(), [zr, gr, br])
    assert np.abs(out - out_ref.detach().numpy()).max() < 1e-12
    assert np.abs(du - (gz.numpy() * (z > 0))).max() < 1e-12
    assert np.abs(sdy.sum(0) - gb.numpy()).max() < 1e-12
    live = np.arange(c) != 5
    assert np.abs(sdyz.sum(0) - gg.numpy())[live].max() < 1e-12
    # the documented rule at gamma == 0 (scale * drop == 0 -> the maximum of z), written out
    zmax = B.groups(z, pool)[..., 5].max(2)
    want = (drop[:, None, 5] * dp[..., 5] * (zmax - np.repeat(mean[:, 5], wpt)[:, None]) * np.repeat(invstd[:, 5], wpt)[:, None]).sum()
    assert abs(sdyz.sum(0)[5] - want) < 1e-12
    if pool > 1:
        assert abs(sdyz.sum(0)[5] - gg.numpy()[5]) > 1e-6        # and it IS a deviation from the oracle there


@pytest.mark.parametrize("shape", [B.BN_SHAPES[0], B.BN_SHAPES[3], B.BN_SHAPES[5], B.BN_SHAPES[9], B.BN_SHAPES[10]], ids=str)
def test_dy_equals_autograd_of_max_pool1d(shape):
    """On the grid cases (ties everywhere): dy of the reference == torch.autograd through F.max_pool1d, on every channel but gamma == 0."""
    c = B.bn_case(shape)
    n, wpt, l, ch, pool, _ = shape
    yb = torch.tensor(c.z * B.per_window(c.scale, wpt) + B.per_window(c.shift, wpt), requires_grad=True)
    y = yb if c.drop is None else yb * torch.tensor(c.drop)[:, None, :]
    out = F.max_pool1d(y.transpose(1, 2), pool, pool).transpose(1, 2)
    assert np.array_equal(out.detach().numpy(), c.out)
    g = torch.autograd.grad((out * torch.tensor(c.dp)).sum(), [yb])[0].numpy()
    live = c.gamma != 0
    assert np.array_equal(g[:, :, live], c.dy[:, :, live])
    assert not np.array_equal(g[:, :, ~live], c.dy[:, :, ~live]) or pool == 1


@pytest.mark.parametrize("dt", B.DT16)
@pytest.mark.parametrize("shape", B.PAIR_SHAPES, ids=str)
def test_pair_encoder_round_trips(shape, dt):
    c = B.bn_case(shape)
    wpt = shape[1]
    for ctr in (None, c.e_center):
        e, o = B.pair_encode(c.z, c.gamma, dt, ctr, wpt)
        assert np.array_equal(B.pair_decode(e, o, ctr, wpt), c.z)
        assert not e[:, 0].any() and not e[:, -1].any()
    e, o = B.pair_encode(c.z, c.gamma, dt)
    second = (o.view(torch.int16) < 0).numpy()
    assert 0.05 < second.mean() < 0.6                            # both flag values occur
    # e is what the global-max pass may read instead of z: the affine of the extreme is the maximum of the affine
    y = (e[:, 1:-1].double().numpy() * B.per_window(c.scale, wpt) + B.per_window(c.shift, wpt)) * (1.0 if c.drop is None else c.drop[:, None, :])
    assert np.array_equal(y + 0.0, c.out)


def _message(got, want, layout="nlc"):
    with pytest.raises(AssertionError) as ei:
        assert_exact(got, want, layout)
    m = re.search(r"(\d+) of \d+ elements differ; first at \(window (\d+), position (\d+), channel (\d+)", str(ei.value))
    return int(m.group(1)), (int(m.group(2)), int(m.group(3)), int(m.group(4)))


def test_comparator_catches_three_planted_errors_at_their_index():
    """One gradient moved to the other element of a tied pool group, one remainder row zeroed, one channel vector that took the other
    tower's scale: each is named by (window, position, channel); the ratio of norms at the limit the 16-bit parity
    tests give du (test_bn_drop_pool_fwd_bwd: 1e-2) passes the first two (the third is one vector of 8 in 4 windows here: it shows in a
    ratio at this size, and less with every window a batch adds)."""
    shape = B.BN_SHAPES[0]
    n, wpt, l, ch, pool, _ = shape
    c = B.bn_case(shape)
    want = c.du_stored("f32")
    assert_exact(torch.tensor(want, dtype=torch.float32), want, "nlc")

    # 1. the first extreme of a tied group -> the second
    g = B.groups(c.z, pool)
    tied = (g[:, :, 0] == g[:, :, 1]) & (g[:, :, 0] > 0) & (c.dp != 0) & np.broadcast_to(c.ka != 0, c.dp.shape)
    w, q, k = (int(v) for v in np.argwhere(tied)[len(np.argwhere(tied)) // 2])
    assert c.arg[w, q, k] == 0
    got = want.copy()
    ady = c.ka[w, 0, k] * c.dp[w, q, k]
    got[w, 2 * q, k] -= ady
    got[w, 2 * q + 1, k] += ady
    assert exact_in(got, "f32")
    count, first = _message(torch.tensor(got, dtype=torch.float32), want)
    assert count == 2 and first == (w, 2 * q, k)
    assert rel_err(got, want) < 1e-2

    # 2. a remainder row (t >= (L // pool) * pool) zeroed
    got = want.copy()
    got[3, l - 1] = 0.0
    k0 = int(np.argwhere(want[3, l - 1] != 0)[0][0])
    count, first = _message(torch.tensor(got, dtype=torch.float32), want)
    assert count == int((want[3, l - 1] != 0).sum()) and first == (3, l - 1, k0)
    assert rel_err(got, want) < 1e-2

    # 3. channels 8..15 of window 2 (tower 1) computed with tower 0's scale
    other = B.backward(c.z, c.dp, c.scale[::-1], c.mean, c.invstd, c.drop, c.c1, c.c2, wpt, pool)[2]
    got = want.copy()
    got[2, :, 8:16] = other[2, :, 8:16]
    diff = np.argwhere(got != want)
    assert len(diff) > 0 and set(diff[:, 0]) == {2} and set(diff[:, 2]) <= set(range(8, 16))
    count, first = _message(torch.tensor(got, dtype=torch.float32), want)
    assert count == len(diff) and first == tuple(int(v) for v in diff[0])


@pytest.mark.parametrize("center", [None, "bias", "tile"])
@pytest.mark.parametrize("shape", B.FINALIZE_SHAPES, ids=str)
def test_finalize_cases_are_dyadic(shape, center):
    """The chosen sums give back the chosen statistics in float64 arithmetic as the header states it, every output but the moving
    variance is an fp32 number, and an fp32 evaluation of the moving-variance update stays within what the device test allows: 1 ulp in
    the zero-debias form (every tower its own accumulator), bn_exact.PLAIN_MV_ULPS per tower in the chained plain form."""
    f = B.FinalizeCase(shape, center)
    rows, towers, c = shape
    ss = f.stat_sum.reshape(towers, rows, c).sum(1)
    sq = f.stat_sq.reshape(towers, rows, c).sum(1)
    if center == "tile":
        sq = sq + 2.0 * f.tile_center * ss + f.COUNT * f.tile_center ** 2
        ss = ss + f.COUNT * f.tile_center
    m = ss / f.COUNT
    var = sq / f.COUNT - m * m
    assert np.array_equal(m, f.m) and np.array_equal(1.0 / np.sqrt(var + f.EPS), f.istd)
    if center is not None:
        assert exact_in(f.shift_adj, "f32") and exact_in(f.mean_adj, "f32")
    # fp32 evaluation of  mv -= (mv - (float)vv) * (1 - momentum), tower by tower
    vv = (var * (f.COUNT / (f.COUNT - (1.0 + f.EPS)))).astype(np.float32)
    mv = f.mv0.astype(np.float32)
    for t in range(towers):
        mv = mv - (mv - vv[t]) * np.float32(0.5)
    assert (np.abs(mv.astype(np.float64) - f.mv_plain) <= B.PLAIN_MV_ULPS * towers * B.ulp32(f.mv_plain)).all()
    bv = f.zd0[:, 1].astype(np.float32)
    nbv = bv - (bv - vv) * np.float32(0.5)
    assert (np.abs((nbv[-1] * np.float32(2.0)).astype(np.float64) - f.mv_zd) <= B.ulp32(f.mv_zd)).all()
