"""-m gpu: the kernels of csrc/spectro.hip on exactly representable inputs (tests/spectro_exact.py).  Part A -- the first Conv2D, its
weight gradient, the fused block-1 boundary and vm_fold_pool_windows_bwd -- at tolerance zero: fp32 outputs equal the float64
reference bit for bit, 16-bit outputs its round-to-nearest-even, a mismatch is named by clip, band, position and channel.  Part B --
STFT, power, mel, log: everything in front of logf is exact, so an fp32 output lies within K_LOG = 3 fp32 ulps of float64 log (the
OpenCL bound for log: no document under the ROCm tree states one for device logf; the library is built without fast-math), and a
16-bit output equals store(reference) except at the elements the reference alone flags as within that bound of a rounding boundary
(under 1 % of any case; one storage ulp allowed there).  No blanket share of mismatches anywhere.
Worst logf error observed on an MI355X over every case below: see test_stft_logmel's docstring.

Which test reaches which kernel form:

  kernel form                                          reached by
  ---------------------------------------------------  ----------------------------------------------------------------------------
  conv2d_first_fwd_mfma_kernel<.., CB, SPLIT = false>  test_first_conv_mfma: CB = 1 (2, 3, 37, 32) and (3, 1, 5, 32); CB = 2 (1, 2, 129, 64);
                                                       CB = 3 (2, 5, 298, 96); CB = 4 (1, 2, 256, 128); bf16 and f16, four regimes each
  conv2d_first_fwd_mfma_kernel<.., CB, SPLIT = true>   test_first_conv_mfma, the same shapes: vm_conv2d_first_fwd_split with and without z_lo
  conv2d_first_bn_pool_stack_kernel<.., CB>            test_fused_boundary: CB = 1 .. 4 on the first four shapes (M = 1 has no pair), one and
                                                       two towers
  conv2d_first_wgrad_mfma_kernel<.., CB16 = 2 .. 8>    test_first_conv_wgrad on the same shapes; wpb = 2: (1025, 2, 3, 32) and (683, 3, 3, 32);
                                                       the guarded gather and du past L: (2, 3, 33, 32), (1, 2, 70, 64)
  conv2d_first_fwd_kernel, shuffle reduction           test_first_conv_valu (1, 3, 5, 8) f32
  conv2d_first_fwd_kernel, LDS reduction (64 % CV)     test_first_conv_valu (2, 3, 37, 24), (2, 2, 140, 40) f32 / bf16 / f16; (1, 2, 130, 120) f32
  conv2d_first_wgrad_kernel, both reductions           test_first_conv_wgrad on the four shapes above; wpb = 2: (683, 3, 3, 24) LDS,
                                                       (1025, 2, 3, 8) shuffle; every fp32 case of the matrix-pipe shapes (shuffle)
  fold_pool_windows_bwd_kernel<T, 4 / 8 / 1>           test_fold_pool_windows_bwd
  stft_logmel_kernel<TOUT, NMB = 1 .. 4>               test_stft_logmel: n_mels cycles 32 / 64 / 96 / 128 over the geometries, each with int16
  stft_logmel_f16s_kernel<TOUT, NMB = 1 .. 4>          and fp32 samples; TOUT = f32, bf16, f16 in every case; out_lo: vm_stft_logmel_f16s_split
  stft_split_basis_kernel                              every test_stft_logmel case (the whole buffer, K padding rows included)
  win_length = 512 (more than 64 KiB of LDS)           test_stft_window_512_against_the_lds_limit
"""
import numpy as np
import pytest
import torch

from tests import spectro_exact as X
from tests.gemm_exact import assert_exact
from tests.gpu_util import DTYPES, L, dev, p, report, stream

pytestmark = pytest.mark.gpu

DT16 = X.DT16
ALL = ("small", "wide", "lo-x", "lo-w")


def _nan(*shape, dtype=torch.float32):
    """An output buffer no element of which is a valid result: one the kernel leaves out is a mismatch."""
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _sentinel(*shape, dtype=torch.float32):
    return torch.full(shape, X.SENTINEL, dtype=dtype, device="cuda")


def _image(plane, tdt):
    """(n, M, L) -> the block input (n * M, L + 2, 1) with zero halo rows."""
    n, M, Lw = plane.shape
    return dev(X.padded_rows(plane.reshape(n * M, Lw, 1)), tdt)


def _check_rows(ss, sq, ss_ref, sq_ref, ok_sq, what):
    """Every statistics row by itself (a row whose sum is zero is still owed: the buffers were NaN-filled); the squares where their
    precondition holds (always in `small`)."""
    assert_exact(ss, ss_ref, "rowc", what=what + " stat_sum")
    if ok_sq:
        assert_exact(sq, sq_ref, "rowc", what=what + " stat_sq")


def _forward(c, dt, split, with_lo=True):
    vm, tdt = DTYPES[dt]
    n, M, Lw, C = c.shape
    Cs = 8
    hi, lo = c.planes(dt)
    zs, zl, ss_ref, sq_ref, ok_sq = c.forward(dt, split)
    rows = L().query("vm_conv_stat_rows", Lw)
    assert rows == -(-Lw // 128)
    w, b = dev(c.weights(Cs)), dev(c.b)
    tag = "%s %s %s %s" % ("split" if split else "one-plane", dt, c.regime, c.shape)
    out = []
    for stats in (True, False):
        z, z_lo = _nan(n * M, Lw, C, dtype=tdt), (_nan(n * M, Lw, C, dtype=tdt) if split and with_lo else None)
        ss, sq = (_nan(n * M * rows, C), _nan(n * M * rows, C)) if stats else (None, None)
        if split:
            L().call("vm_conv2d_first_fwd_split", p(_image(hi, tdt)), p(_image(lo, tdt)), p(w), p(b), n, M, Lw, Cs, C, vm, p(z), p(z_lo), p(ss), p(sq),
                     stream())
        else:
            L().call("vm_conv2d_first_fwd", p(_image(hi, tdt)), p(w), p(b), n, M, Lw, Cs, C, vm, p(z), p(ss), p(sq), stream())
        torch.cuda.synchronize()
        assert_exact(z.view(n, M, Lw, C), zs, "bmtc", neg_zero=True, what="z " + tag)          # (a ReLU output: the sign of a zero is free)
        if z_lo is not None:
            assert_exact(z_lo.view(n, M, Lw, C), zl, "bmtc", neg_zero=True, what="z_lo " + tag)
        if stats:
            _check_rows(ss, sq, ss_ref, sq_ref, ok_sq, tag)
        out.append(z)
    assert torch.equal(out[0], out[1])
    return out[0]


@pytest.mark.parametrize("regime", ALL)
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("shape", X.MFMA_SHAPES, ids=str)
def test_first_conv_mfma(shape, dt, regime):
    """vm_conv2d_first_fwd (the high plane times the filters rounded to the storage type) and vm_conv2d_first_fwd_split (27 products)
    on the matrix pipe: z with and without statistics pointers, z_lo, every statistics row (split: of z + z_lo; stored or not), and
    where in_lo == 0 and w_lo == 0 the split call's z is the one-plane call's."""
    c = X.conv2d_case(shape, regime, dt)
    z1 = _forward(c, dt, split=False)
    z2 = _forward(c, dt, split=True)
    z3 = _forward(c, dt, split=True, with_lo=False)
    assert torch.equal(z2, z3)
    if regime in ("small", "wide"):
        assert torch.equal(z1, z2)


@pytest.mark.parametrize("shape,dt,regime", [(s, dt, reg) for s in X.VALU_SHAPES for dt in ("f32",) + DT16 for reg in (ALL if dt != "f32" else ALL[:2])] +
                         [(s, "f32", reg) for s in X.VALU_F32_SHAPES for reg in ALL[:2]], ids=str)
def test_first_conv_valu(shape, dt, regime):
    """The vector-ALU forward: C = 24 / 40 / 120 take the LDS reduction (idle threads included), C = 8 the shuffles."""
    assert L().query("vm_conv2d_first_supported", shape[3], DTYPES[dt][0]) == 1
    _forward(X.conv2d_case(shape, regime, dt), dt, split=False)


WGRAD = ([(s, dt) for s in X.MFMA_SHAPES + X.WPB_MFMA_SHAPES + X.WGRAD_TAIL_SHAPES for dt in DT16] +
         [(s, dt) for s in X.VALU_SHAPES for dt in ("f32",) + DT16] + [(s, "f32") for s in X.VALU_F32_SHAPES + X.WPB_VALU_SHAPES + X.MFMA_SHAPES[:2]])


@pytest.mark.parametrize("shape,dt", WGRAD, ids=str)
def test_first_conv_wgrad(shape, dt):
    """(3, Cs, C) exact with the padding entries km >= 3 exactly zero, Cs = 8 and 3, `small` and `wide` operands.  du's halo rows hold
    3.0 and the image is dense: a position past L that is not read as zero, or a sample of the next band taken for this one, shows."""
    vm, tdt = DTYPES[dt]
    n, M, Lw, C = shape
    for regime in ("small", "wide"):
        c = X.conv2d_case(shape, regime, dt)
        xin = _image(c.planes(dt)[0], tdt)
        du = dev(X.padded_rows(c.du.reshape(n * M, Lw, C), halo=3.0), tdt)
        ws = torch.empty(L().query("vm_conv2d_first_wgrad_workspace_bytes", n, M, C) // 4 + 16, dtype=torch.float32, device="cuda")
        for Cs in (8, 3):
            gw = _nan(3, Cs, C)
            L().call("vm_conv2d_first_wgrad", p(xin), p(du), n, M, Lw, Cs, C, vm, p(ws), p(gw), stream())
            torch.cuda.synchronize()
            assert_exact(gw, c.gw(Cs, dt), "ksc", what="vm_conv2d_first_wgrad %s %s %s Cs %d" % (dt, regime, shape, Cs))


@pytest.mark.parametrize("regime", ("small", "lo-x", "lo-w"))
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("shape,cpt", [(s, 1) for s in X.MFMA_SHAPES[:4]] + [((2, 5, 298, 96), 2)], ids=str)
def test_fused_boundary(shape, cpt, dt, regime):
    """vm_conv2d_first_bn_pool_stack: q and xs bit for bit against the header's formula on the two-plane image, xs from the STORED q,
    every never-written entry (halo rows, out-of-clip band slots, channels [3 C, Cs2)) still the sentinel and every owed one written;
    clips_per_tower = 1 with two clips: each tower's clips under their own constants."""
    vm, tdt = DTYPES[dt]
    n, M, Lw, C = shape
    c = X.conv2d_case(shape, regime, dt)
    Cs, Cs2 = 8, 3 * C + 8
    b = X.Boundary(c, dt, cpt, Cs2)
    hi, lo = c.planes(dt)
    Lq, Mo = Lw // 2, M // 2
    q, xs = _sentinel(n * M, Lq + 2, C, dtype=tdt), _sentinel(n * Mo, Lq + 2, Cs2, dtype=tdt)
    L().call("vm_conv2d_first_bn_pool_stack", p(_image(hi, tdt)), p(_image(lo, tdt)), p(dev(c.weights(Cs))), p(dev(c.b)), p(dev(b.scale)),
             p(dev(b.shift)), p(dev(b.drop)), n, M, cpt, Lw, Cs, C, Cs2, vm, p(q), p(xs), stream())
    torch.cuda.synchronize()
    tag = "%s %s %s cpt %d" % (dt, regime, shape, cpt)
    assert_exact(q.view(n, M, Lq + 2, C), b.q.reshape(n, M, Lq + 2, C), "bmrc", neg_zero=True, what="q " + tag)     # (0 * a negative affine)
    assert_exact(xs.view(n, Mo, Lq + 2, Cs2), b.xs.reshape(n, Mo, Lq + 2, Cs2), "bprs", neg_zero=True, what="xs " + tag)


@pytest.mark.parametrize("dt", ("f32",) + DT16)
@pytest.mark.parametrize("shape", X.FOLD_SHAPES, ids=str)
def test_fold_pool_windows_bwd(shape, dt):
    """dq, s0 and sa exact on integer dxs and q, both source layouts (the padded one with 5.0 in its halo rows), every row owed."""
    vm, tdt = DTYPES[dt]
    n, M, Lw, C, Cs = shape
    c = X.FoldPoolCase(shape)
    Mo = M // 2
    q = dev(X.padded_rows(c.q.reshape(n * M, Lw, C)), tdt)
    assert L().query("vm_fold_pool_windows_rows", Lw, C, Cs, vm) == 1
    for src_padded in (0, 1):
        g = c.dxs.reshape(n * Mo, Lw, Cs)
        g = dev(X.padded_rows(g, halo=5.0) if src_padded else g, tdt)
        dq, s0, sa = _nan(n * M, Lw, C, dtype=tdt), _nan(n * M, C), _nan(n * M, C)
        L().call("vm_fold_pool_windows_bwd", p(g), p(q), n, M, Lw, C, Cs, src_padded, vm, p(dq), p(s0), p(sa), stream())
        torch.cuda.synchronize()
        tag = "vm_fold_pool_windows_bwd %s %s padded %d" % (dt, shape, src_padded)
        assert_exact(dq.view(n, M, Lw, C), c.dq, "bmtc", neg_zero=True, what=tag + " dq")
        assert_exact(s0, c.s0, "wc", neg_zero=True, what=tag + " s0")
        assert_exact(sa, c.sa, "wc", neg_zero=True, what=tag + " sa")


# ---- the front end ---------------------------------------------------------------------------------------------------------------------
def _basis16_reference(c, win):
    """[hi | lo][Kp / 16 steps][16 row blocks][64 lanes][8] (csrc/spectro.hip: the A operand in register order), zero for k >= win."""
    Kp = -(-win // 16) * 16
    i = np.arange(512 * Kp)
    e, lane, rb, step = i & 7, (i >> 3) & 63, (i >> 9) & 15, i >> 13
    row, k = 32 * rb + (lane & 31), 16 * step + 8 * (lane >> 5) + e
    bh, bl = X.f16_halves(c.basis)
    pad = lambda a: np.concatenate([a, np.zeros((Kp - win, 512))])[k, row]
    return np.concatenate([pad(bh), pad(bl)]), k >= win


def _stft(c, dtypes=("f32", "bf16", "f16")):
    """Every entry point on one case.  Returns the worst fp32 error in ulps of the reference (fp32 kernel, f16 kernel)."""
    win, hop, T = c.geom
    n, n_mels = c.n, c.n_mels
    raw = dev(c.samples_i16, torch.int16) if c.i16 else dev(c.raw)
    basis, melw = dev(c.basis), dev(c.melw)
    assert L().query("vm_stft_frames", c.raw_len, win, hop) == T
    nb = L().query("vm_stft_split_basis_bytes", win)
    b16 = _nan(nb // 2, dtype=torch.float16)
    L().call("vm_stft_split_basis", p(basis), win, p(b16), stream())
    torch.cuda.synchronize()
    want16, padding = _basis16_reference(c, win)
    assert want16.size == nb // 2
    got16 = b16.double().cpu().numpy()
    assert np.array_equal(got16, want16) and not got16[np.concatenate([padding, padding])].any()      # the K padding rows are zero
    tag = "win %d hop %d T %d n_mels %d i16 %d %s" % (c.geom + (n_mels, int(c.i16), c.regime))
    worst = [0.0, 0.0]
    for which, fn, bas in ((0, "vm_stft_logmel", basis), (1, "vm_stft_logmel_f16s", b16)):
        for dt in dtypes:
            vm, tdt = DTYPES[dt]
            out = _sentinel(n * n_mels, T + 2, 1, dtype=tdt)
            L().call(fn, p(raw), int(c.i16), n, c.raw_len, win, hop, p(bas), p(melw), n_mels, c.floor, vm, p(out), stream())
            torch.cuda.synchronize()
            o = out.double().cpu().numpy().reshape(n, n_mels, T + 2)
            assert (o[:, :, 0] == X.SENTINEL).all() and (o[:, :, -1] == X.SENTINEL).all(), "halo rows written: " + fn + " " + tag
            got = o[:, :, 1:-1].transpose(0, 2, 1)
            if dt == "f32":
                worst[which] = X.check_log_f32(got, c, "%s f32 %s" % (fn, tag))
                report("stft_exact", "%s worst_ulp[%s]" % (fn, tag), worst[which])
            else:
                X.check_log_stored(got, c, dt, "%s %s %s" % (fn, dt, tag))
            if which == 1 and dt != "f32":
                hi, lo = _sentinel(n * n_mels, T + 2, 1, dtype=tdt), _sentinel(n * n_mels, T + 2, 1, dtype=tdt)
                L().call("vm_stft_logmel_f16s_split", p(raw), int(c.i16), n, c.raw_len, win, hop, p(bas), p(melw), n_mels, c.floor, vm, p(hi), p(lo),
                         stream())
                torch.cuda.synchronize()
                assert torch.equal(hi, out)
                l = lo.double().cpu().numpy().reshape(n, n_mels, T + 2)
                assert (l[:, :, 0] == X.SENTINEL).all() and (l[:, :, -1] == X.SENTINEL).all()
                two = got + l[:, :, 1:-1].transpose(0, 2, 1)
                # out + out_lo: the fp32 bound plus half an ulp of the low plane, whose value is at most |ref - out| + the bound
                # (an f16 low plane under 2^-14 is subnormal: spacing 2^-24)
                bound = c.tol32() + 0.5 * np.maximum(X.ulp_of(np.abs(c.ref - got) + c.tol32(), dt), 2.0 ** -24 if dt == "f16" else 0.0)
                assert (np.abs(two - c.ref) <= bound).all(), "out + out_lo %s %s" % (dt, tag)
    return worst


@pytest.mark.parametrize("case", X.stft_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_stft_logmel(case):
    """vm_stft_logmel, vm_stft_logmel_f16s, vm_stft_logmel_f16s_split and vm_stft_split_basis on every geometry, sample type and regime.
    Chosen K_LOG = 3 ulps.  Worst error observed on an MI355X: 2.10 fp32 ulps of the reference in the exact regime, where logf is the only
    inexact step (both kernels, win 401 / hop 1, 96 mels; the results lie in 8 .. 16 and a base-2 logarithm good to one ulp of ITS result,
    which lies in 16 .. 32, already carries 1.4 of them), and 2.76 ulps of a bound of 3 + 2.3 in the lo regimes (lo-x, win 401, 64 mels)."""
    _stft(X.stft_case(*case))


def test_stft_window_512_against_the_lds_limit():
    """win_length = 512 needs 65 664 bytes (fp32 kernel) / 66 560 bytes (f16 kernels) of dynamic LDS.  What must happen follows from the
    device's per-block limit, read from its properties: below the need every entry point refuses before launching and `out` keeps its
    sentinel; otherwise the row is as exact as every other."""
    limit = torch.cuda.get_device_properties(0).shared_memory_per_block
    win, hop, T = X.STFT_LDS_GEOMETRY
    report("stft_exact", "shared_memory_per_block", float(limit))
    for n_mels, i16 in ((128, False), (64, True)):
        c = X.stft_case(win, hop, T, n_mels, i16, "exact")
        need32, need16 = X.lds_bytes(win, n_mels)
        if limit >= need16:
            _stft(c)
            continue
        assert limit < need32                 # (a limit between the two needs would split the entry points: no such device)
        raw = dev(c.samples_i16, torch.int16) if i16 else dev(c.raw)
        basis, melw = dev(c.basis), dev(c.melw)
        b16 = _nan(L().query("vm_stft_split_basis_bytes", win) // 2, dtype=torch.float16)
        L().call("vm_stft_split_basis", p(basis), win, p(b16), stream())
        for fn, bas, extra in (("vm_stft_logmel", basis, 0), ("vm_stft_logmel_f16s", b16, 0), ("vm_stft_logmel_f16s_split", b16, 1)):
            vm, tdt = DTYPES["f16"]
            out, lo = _sentinel(2 * n_mels, T + 2, 1, dtype=tdt), _sentinel(2 * n_mels, T + 2, 1, dtype=tdt)
            with pytest.raises(Exception, match="LDS"):
                L().call(fn, p(raw), int(i16), 2, c.raw_len, win, hop, p(bas), p(melw), n_mels, c.floor, vm, p(out), *((p(lo),) if extra else ()),
                         stream())
            torch.cuda.synchronize()
            assert (out == X.SENTINEL).all() and (lo == X.SENTINEL).all()
