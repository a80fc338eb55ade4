"""-m gpu: the accumulator map of the 256 x 128 conv GEMM kernels (conv_nt3_kernel, conv_nt2r_kernel) on v_mfma_f32_16x16x32: a wave's
128 x 64 tile is 8 position blocks of 16 rows x 4 channel blocks of 16, lane l holds row l & 15 and channels 4 (l >> 4) .. + 3 of a
block, a K tile (32 channels of one tap) is one instruction deep with k slot 8 (l >> 4) + e = channel 8 (l >> 4) + e of the chunk.
Inputs are on the integer grid of tests/gemm_exact.py, every assertion is at tolerance zero against the float64 definition; the
packed-against-staged comparison on random data is bit for bit.

Lengths.  The entry points refuse windows that conv_nt2r_kernel's shape rule does not take (conv_gemm.hip n2r_shape): a window must
fill its 256-row tiles to within 0.10 of what 128-row tiles would reach, and a forward with statistics needs 2 * ceil(L / 254) ==
ceil(L / 128).  The second condition puts the last position of a window at tile row 2 k + 126 or later of the last of its k tiles --
never in the first wave row -- so of the lengths 256, 270, 272, 382, 384, 508 (last row at tile rows 1, 15, 17, 127, 129, 253) only 508
is served by vm_conv_fwd_fold, and L = 300 by none of vm_conv_fwd_fold / vm_conv_fwd_pool / vm_conv_dgrad_bnred (59 % of two 256-row
tiles against 78 % of three 128-row ones).  test_fold_edge keeps the six lengths -- those the entry point refuses must be refused, no
kernel may run on them -- and adds 386, 398, 399, 400, 507: the last row at tile rows 131, 143, 144, 145, 252, i.e. either side of a
16-row block boundary inside the second wave row (odd lengths take the z output without the pair extreme, which needs an even L).  The
one-hot and the packed-against-staged tests run at L = 400, the shortest round length all three entry points serve, with the hot
positions 0, 15, 16, 253, 254 and L - 1 unchanged."""
import numpy as np
import pytest
import torch

from tests import gemm_exact as G
from tests import test_gpu_kernels as K
from tests.gemm_exact import assert_exact
from tests.gpu_util import DTYPES, L, dev, p, padded, stream
from voicemap_amd._lib import VoicemapHipError

pytestmark = pytest.mark.gpu

DT16 = G.DT16
ISSUE_LENGTHS = (256, 270, 272, 382, 384, 508)
SERVED_LENGTHS = (386, 398, 399, 400, 507)
L_HOT = 400


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


@pytest.fixture
def nt3_lean():
    yield lambda v: L().call("vm_set_tuning", b"nt3_lean", v)
    L().call("vm_set_tuning", b"nt3_lean", K.GEMM_DEFAULTS["nt3_lean"])


def _fold(w_oki, scale, shift, bias, towers, cin, cout, dt):
    """vm_fold_bn_weights -> (wf_folded, hb, packed copy)."""
    vm, tdt = DTYPES[dt]
    wf = torch.empty(towers, cout, 3 * cin, dtype=tdt, device="cuda")
    hb = _nan(towers, 4, cout)
    L().call("vm_fold_bn_weights", p(dev(w_oki)), p(dev(scale)), p(dev(shift)), p(dev(bias)), towers, cin, cout, vm, p(wf), None, p(hb), None,
             stream())
    wfp = torch.empty_like(wf)
    L().call("vm_pack_nt_weights", p(wf), towers, cout, cin, vm, p(wfp), stream())
    return wf, hb, wfp


# ---- 1. the fold edge at 16-row granularity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cout", [128, 256])
@pytest.mark.parametrize("l", ISSUE_LENGTHS + SERVED_LENGTHS)
def test_fold_edge(dt, l, cout, nt3_lean):
    """vm_conv_fwd_fold with packed weights, both prologues, two towers of one window: z, the pair extreme (even L) and both statistics
    rows.  The constants of the taps that fall into the SAME padding come off the accumulators of ONE lane group (row l & 15 of one
    16-row block of one wave row): a wrong block, row or channel quarter moves whole rows of z by the integer shift terms."""
    vm, tdt = DTYPES[dt]
    n, cin, towers, wpt = 2, 128, 2, 1
    assert L().query("vm_pack_nt_weights_supported", cout, cin, vm) == 1
    with_e = l % 2 == 0
    if not L().query("vm_conv_fwd_fold_supported", n, l, cin, cout, vm, int(with_e)):
        # 2 * ceil(L / 254) != ceil(L / 128): the statistics rows of a 254-position tile would not be those of vm_conv_stat_rows
        assert l in ISSUE_LENGTHS and 2 * -(-l // 254) != -(-l // 128)
        junk = torch.zeros(n * (l + 2) * max(cin, cout), dtype=tdt, device="cuda")
        with pytest.raises(VoicemapHipError, match="not served"):
            L().call("vm_conv_fwd_fold", p(junk), p(junk), p(junk.float()), p(junk.float()), None, n, wpt, l, cin, cout, vm, p(junk),
                     p(junk.float()), p(junk.float()), None, None, None, None, stream())
        return
    f = G.fold_case((n, l, cin, cout), dt)
    wt = np.ascontiguousarray(f.w.transpose(2, 0, 1).reshape(cout, 3 * cin))
    wf, hb, wfp = _fold(wt, f.scale, f.shift, f.b, towers, cin, cout, dt)
    rows = L().query("vm_conv_stat_rows", l)
    ep = padded(f.e, tdt)
    ext = G.pair_extreme(f.z_st, f.gamma)[0]
    ss_ref, sq_ref = f.z_st.sum(1), (f.z_st * f.z_st).sum(1)
    last = (l - 1) % 254
    for lean in (3, 0):
        nt3_lean(lean)
        run = "%s L %d (last row: tile row %d) c_out %d lean %d" % (dt, l, last, cout, lean)
        z = _nan(n, l, cout, dtype=tdt)
        e = torch.full((n, l // 2 + 2, cout), 7.0, dtype=tdt, device="cuda") if with_e else None
        ss, sq = _nan(n * rows, cout), _nan(n * rows, cout)
        L().call("vm_conv_fwd_fold", p(ep), p(wf), p(dev(f.b)), p(hb), p(dev(f.gamma)) if with_e else None, n, wpt, l, cin, cout, vm, p(z),
                 p(ss), p(sq), p(e), None, p(wfp), None, stream())
        assert_exact(z, f.z_st, "nlc", neg_zero=True, what="z " + run)
        if with_e:
            assert_exact(e[:, 1:-1], ext, "nlc", neg_zero=True, what="e " + run)
            assert (e[:, 0] == 7.0).all() and (e[:, -1] == 7.0).all(), "e's halo rows " + run
        assert_exact(ss.to(torch.float64).view(n, -1, cout).sum(1), ss_ref, "nc", what="stat_sum " + run)
        assert_exact(sq.to(torch.float64).view(n, -1, cout).sum(1), sq_ref, "nc", what="stat_sq " + run)


# ---- 2. one-hot localisation -------------------------------------------------------------------------------------------------------------
def _code_weights(ck, cn):
    """(3, ck, cn) positive integers <= 251 (exact in bf16) that change with the tap (by 37), the K-side channel (5) and the N-side
    channel (3): a product taken from a neighbouring tap, k slot or output channel is a different number."""
    k, i, o = np.meshgrid(np.arange(3), np.arange(ck), np.arange(cn), indexing="ij")
    return (1 + (k * 37 + i * 5 + o * 3) % 251).astype(np.float64)


def _hot(ck, channel):
    """(6, L_HOT, ck): window i is 1 at (its hot position, channel), 0 elsewhere."""
    pos = (0, 15, 16, 253, 254, L_HOT - 1)
    x = np.zeros((len(pos), L_HOT, ck))
    for i, t in enumerate(pos):
        x[i, t, channel] = 1.0
    return x


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("ck", [128, 512])
def test_one_hot(dt, ck, nt3_lean):
    """An input that is 1 at a single (position, K-side channel): the output is the three weight rows at the three neighbouring positions
    and zero elsewhere -- which input row, which 16-byte chunk and which k slot of the chunk an MFMA lane reads, and where its four
    output channels go.  Hot channels 0, 7, 8, 31, 32, ck - 1 (k slots either side of a lane quarter, of a K tile, and the last chunk),
    six windows with the hot positions 0, 15, 16, 253, 254, L - 1 (16-row block and tile boundaries).  Forward: vm_conv_fwd_fold under
    the identity fold (scale 1, shift 0, bias 0; the weights are positive, so the ReLU changes nothing); backward: vm_conv_dgrad_bnred
    with the channel count on ITS K side, c_out.  Staged and packed weights, both prologues."""
    vm, tdt = DTYPES[dt]
    n, cn, towers = 6, 128, 2
    assert L().query("vm_conv_fwd_fold_supported", n, L_HOT, ck, cn, vm, 0) and L().query("vm_conv_dgrad_bnred_supported", n, L_HOT, cn, ck, vm)
    # forward: c_in = ck
    w = _code_weights(ck, cn)                                               # (3, c_in, c_out)
    wt = np.ascontiguousarray(w.transpose(2, 0, 1).reshape(cn, 3 * ck))
    wf, hb, wfp = _fold(wt, np.ones((towers, ck)), np.zeros((towers, ck)), np.zeros(cn), towers, ck, cn, dt)
    assert not hb.any()
    # backward: c_out = ck is summed over, c_in = cn comes out; W (3, c_in, c_out)
    wb = _code_weights(ck, cn).transpose(0, 2, 1).copy()
    wd = torch.empty(cn * 3 * ck, dtype=tdt, device="cuda")
    L().call("vm_prep_conv_weights", p(dev(wb)), cn, ck, vm, p(torch.empty(ck * 3 * cn, dtype=tdt, device="cuda")), p(wd), stream())
    wdp = torch.empty_like(wd)
    L().call("vm_pack_nt_weights", p(wd), 1, cn, ck, vm, p(wdp), stream())
    rows_f, rows_b = L().query("vm_conv_stat_rows", L_HOT), L().query("vm_conv_dgrad_bnred_rows", L_HOT)
    zero_bias, ones_a = dev(np.zeros(cn)), dev(np.ones((n, L_HOT, cn)), tdt)
    for channel in (0, 7, 8, 31, 32, ck - 1):
        x = _hot(ck, channel)
        z_ref, dx_ref = G.conv_same(x, w), G.conv_dgrad(x, wb)
        assert (z_ref != 0).sum() == (3 * n - 2) * cn and (dx_ref != 0).sum() == (3 * n - 2) * cn       # three rows, two at the window ends
        xp = padded(x, tdt)
        for packed, lean in ((False, 3), (True, 3), (True, 0)):
            nt3_lean(lean)
            run = "%s K-side %d hot channel %d packed %d lean %d" % (dt, ck, channel, packed, lean)
            z, ss, sq = _nan(n, L_HOT, cn, dtype=tdt), _nan(n * rows_f, cn), _nan(n * rows_f, cn)
            L().call("vm_conv_fwd_fold", p(xp), p(wf), p(zero_bias), p(hb), None, n, n // towers, L_HOT, ck, cn, vm, p(z), p(ss), p(sq), None,
                     None, p(wfp) if packed else None, None, stream())
            assert_exact(z, z_ref, "nlc", neg_zero=True, what="vm_conv_fwd_fold z " + run)
            dx, s0, s1 = _nan(n, L_HOT, cn, dtype=tdt), _nan(n * rows_b, cn), _nan(n * rows_b, cn)
            L().call("vm_conv_dgrad_bnred", p(xp), p(wd), n, L_HOT, cn, ck, vm, p(dx), p(ones_a), 0, p(s0), p(s1), p(wdp) if packed else None,
                     stream())
            assert_exact(dx, dx_ref, "nlc", what="vm_conv_dgrad_bnred dx " + run)
            assert_exact(s0.to(torch.float64).view(n, -1, cn).sum(1), dx_ref.sum(1), "nc", what="vm_conv_dgrad_bnred red_s0 " + run)


# ---- 3. packed against staged on random data ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cin", [128, 512])
def test_pool_packed_equals_staged_on_random_data(dt, cin, nt3_lean):
    """vm_conv_fwd_pool and vm_conv_fwd_pool_varlen: conv_nt3_kernel (packed weights, both prologues) against conv_nt2r_kernel (staged)
    on random data, bit for bit -- the two read their weight fragments from different places (L2 in fragment order, the LDS stage) and
    must multiply the same products in the same k slots in the same order.  Varlen: a full window and one that ends inside the first
    tile, so its second tile is dead."""
    vm, tdt = DTYPES[dt]
    n, l, cout = 2, L_HOT, 128
    assert L().query("vm_conv_fwd_pool_supported", n, l, cin, cout, vm)
    g = torch.Generator(device="cuda").manual_seed(cin + len(dt))
    x = torch.zeros(n, l + 2, cin, dtype=tdt, device="cuda")
    x[:, 1:l + 1] = torch.randn(n, l, cin, device="cuda", generator=g).to(tdt)
    w = torch.randn(3, cin, cout, device="cuda", generator=g) * (0.6 / np.sqrt(3 * cin))
    wf, wd = torch.empty(cout * 3 * cin, dtype=tdt, device="cuda"), torch.empty(cin * 3 * cout, dtype=tdt, device="cuda")
    L().call("vm_prep_conv_weights", p(w.contiguous()), cin, cout, vm, p(wf), p(wd), stream())
    wfp = torch.empty_like(wf)
    L().call("vm_pack_nt_weights", p(wf), 1, cout, cin, vm, p(wfp), stream())
    bias = torch.randn(cout, device="cuda", generator=g) * 0.1
    scale = torch.randn(cout, device="cuda", generator=g)
    shift = torch.randn(cout, device="cuda", generator=g)
    lens = torch.tensor([l, 130], dtype=torch.int32, device="cuda")

    def run(packed, varlen):
        act = torch.full((n, l // 2 + 2, cout), 7.0, dtype=tdt, device="cuda")
        if varlen:
            L().call("vm_conv_fwd_pool_varlen", p(x), p(wf), p(bias), p(scale), p(shift), p(lens), n, l, cin, cout, vm, p(act),
                     p(wfp) if packed else None, stream())
        else:
            L().call("vm_conv_fwd_pool", p(x), p(wf), p(bias), p(scale), p(shift), n, l, cin, cout, vm, p(act), p(wfp) if packed else None,
                     stream())
        torch.cuda.synchronize()
        return act

    for varlen in (False, True):
        staged = run(False, varlen)
        assert torch.isfinite(staged.float()).all() and staged[:, 1:-1].float().abs().max() > 0.1      # a real result, not a constant
        if varlen:
            assert (staged[1, 1 + 65:-1] == 0).all() and (staged[1, 1:1 + 65] != 0).any()
        for lean in (3, 0):
            nt3_lean(lean)
            got = run(True, varlen)
            assert torch.equal(got.view(torch.int16), staged.view(torch.int16)), "%s c_in %d varlen %d lean %d" % (dt, cin, varlen, lean)
