"""-m gpu: the waveform front end (csrc/preproc.hip, csrc/augment.hip) against tests/wave_exact.py through the C ABI.

The FIR alone (whitening = 0, K = 0, gain in 1, 0.5, 2: out[:, 15 : 15 + L0] is gain * a exactly) at bit equality with the int64
convolution, over ds in 1, 2, 3, 4, 7 x the tap counts at which a phase, an 8-tap block, the 256-tap chunk or the limit is crossed x
the lengths around the 8 outputs of a thread and the 2048 of a tile, both ends of raw_len, int16 and fp32 sources, windows with and
without an RIR in one launch, offsets 0 and total - raw_len -- a mismatch reported by window, output, tile and slot in grid units.
Then the sums, g, the gain and the whitening (exact plants at bit equality, general cases under the counted-roundings rule of
wave_exact.accept), and the three plain entries on the same grid, the varlen form with large values everywhere it must not read.
Every output and the exactly-sized workspace lie between guard words."""
import numpy as np
import pytest
import torch

from tests import wave_exact as W
from tests.gpu_util import L, dev, p, stream

pytestmark = pytest.mark.gpu
PATTERN = 0x7FC5A5A5      # the guard word (as fp32: a NaN with a payload no kernel produces)
GUARD = 64                # words on either side: the inner buffer stays 256-byte aligned


class Guarded:
    """n 4-byte words between two runs of guard words; the inner words start as the pattern too, so an entry the kernel never wrote
    shows (as a NaN).  ``fetch`` copies everything back, asserts the guards and returns the inner words."""

    def __init__(self, n):
        self.n = int(n)
        self.raw = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.int32, device="cuda")

    def ptr(self):
        return self.raw.data_ptr() + 4 * GUARD

    def fetch(self, what):
        h = self.raw.cpu().numpy()
        assert (h[:GUARD] == PATTERN).all(), "%s: written in front of the buffer" % what
        assert (h[GUARD + self.n:] == PATTERN).all(), "%s: written behind the buffer" % what
        return h[GUARD:GUARD + self.n].view(np.float32)


def _src(buf):
    buf = np.ascontiguousarray(buf)
    return dev(buf, torch.int16 if buf.dtype == np.int16 else torch.float32), int(buf.dtype == np.int16)


def launch_aug(audio, offsets, raw_len, ds, whitening, wpt, gain, noise=None, noff=None, snr=None, rirs=None, rir_id=None):
    """One guarded vm_crop_augment_decimate_whiten launch on host arrays -> (n, L0 + 31) fp32 on the host."""
    n, L0 = len(offsets), W.n_out(raw_len, ds)
    K = 0 if noff is None else int(np.asarray(noff).reshape(n, -1).shape[1])
    a_t, a16 = _src(audio)
    n_t, n16 = _src(noise) if K else (None, 0)
    o_t = dev(offsets, torch.int64)
    no_t = dev(noff, torch.int64) if K else None
    s_t = dev(np.zeros(n) if snr is None else snr)
    g_t = dev(gain)
    r_t = None if rirs is None else dev(rirs)
    id_t = None if rirs is None else dev(rir_id, torch.int32)
    nbytes = L().query("vm_crop_augment_workspace_bytes", n, L0)
    assert nbytes % 4 == 0
    out, ws = Guarded(n * (L0 + W.HALO)), Guarded(nbytes // 4)          # the workspace: exactly the size the library asks for
    L().call("vm_crop_augment_decimate_whiten", p(a_t), a16, p(o_t), n, raw_len, ds, int(whitening), W.RMS, wpt, p(n_t), n16, p(no_t), K,
             p(s_t), p(g_t), p(r_t), 0 if rirs is None else int(rirs.shape[0]), 0 if rirs is None else int(rirs.shape[1]), p(id_t),
             out.ptr(), ws.ptr(), stream())
    torch.cuda.synchronize()
    ws.fetch("workspace")
    return out.fetch("out").reshape(n, L0 + W.HALO)


def launch_plain(entry, audio, offsets, raw_len, ds, whitening, wpt, raw_lens=None, L0=None):
    """vm_decimate_whiten ("rows"), vm_crop_decimate_whiten ("crop") or vm_crop_decimate_whiten_varlen ("varlen"), guarded."""
    n = len(offsets)
    L0 = W.n_out(raw_len, ds) if L0 is None else L0
    a_t, a16 = _src(audio)
    o_t = dev(offsets, torch.int64)
    nbytes = L().query("vm_decimate_whiten_workspace_bytes", n)
    out, ws = Guarded(n * (L0 + W.HALO)), Guarded(nbytes // 4)
    if entry == "rows":
        L().call("vm_decimate_whiten", p(a_t), a16, n, raw_len, ds, int(whitening), W.RMS, wpt, out.ptr(), ws.ptr(), stream())
    elif entry == "crop":
        L().call("vm_crop_decimate_whiten", p(a_t), a16, p(o_t), n, raw_len, ds, int(whitening), W.RMS, wpt, out.ptr(), ws.ptr(), stream())
    else:
        L().call("vm_crop_decimate_whiten_varlen", p(a_t), a16, p(o_t), p(dev(raw_lens, torch.int64)), n, L0, ds, int(whitening), W.RMS,
                 out.ptr(), ws.ptr(), stream())
    torch.cuda.synchronize()
    ws.fetch("workspace")
    return out.fetch("out").reshape(n, L0 + W.HALO)


# ---- the FIR alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.FIR_CASES, ids=W.fir_id)
def test_fir_equals_the_integer_convolution_bit_for_bit(c):
    fc = W.fir_case(c)
    got = launch_aug(W.as_source(fc.k, fc.src), fc.offsets, fc.raw_len, fc.ds, 0, 1, fc.gain, rirs=W.as_rirs(fc.t), rir_id=fc.rir_id)
    msg = W.fir_report(got, fc.expected(), fc.g, W.fir_id(c))
    assert msg is None, msg


# ---- sums, g, gain, whitening ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,wh", [(c, wh) for c in W.MIX_CASES for wh in W.whitenings(c[2])], ids=lambda v: W.mix_id(v) if isinstance(v, tuple) else "wh%d" % v)
def test_mixture_and_whitening_follow_the_rule(c, wh):
    """Exact plants (K = 1, noise = 2^j speech, snr = 4^m, gain 2^e: g = 2^-(j + m) exactly) with whitening off are fp32 numbers: no
    sample is ambiguous and the rule is bit equality; everything else is held to fp32(x) outside the ambiguous samples."""
    mc = W.mix_case(c)
    ref = mc.reference(wh)
    got = launch_aug(W.as_source(mc.k, mc.src), mc.offsets, mc.raw_len, mc.ds, wh, mc.wpt, mc.gain, noise=W.as_source(mc.nk, mc.nsrc),
                     noff=mc.noff, snr=mc.snr, rirs=None if mc.t is None else W.as_rirs(mc.t), rir_id=mc.rir_id)
    if mc.kind == "plant" and not wh:
        assert not ref["amb"].any()
    msg = W.rule_report(got, ref, "%s whitening %d" % (W.mix_id(c), wh))
    assert msg is None, msg


# ---- the plain entries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.PLAIN_CASES, ids=W.plain_id)
def test_plain_entries_follow_the_rule(c):
    pc = W.plain_case(c)
    for wh in W.whitenings(pc.L0):
        got = launch_plain(pc.entry, W.as_source(pc.k, pc.src), pc.offsets, pc.raw_len, pc.ds, wh, pc.wpt)
        msg = W.rule_report(got, pc.reference(wh), "%s whitening %d" % (W.plain_id(c), wh))
        assert msg is None, msg


@pytest.mark.parametrize("c", W.VARLEN_CASES, ids=W.varlen_id)
def test_varlen_reads_nothing_past_a_row_s_length_or_off_the_grid(c):
    vc = W.varlen_case(c)
    for wh in (0, 1):
        ref = vc.reference(wh)
        clean = launch_plain("varlen", vc.source(False), vc.offsets, 0, vc.ds, wh, 1, vc.raw_lens, vc.L0)
        msg = W.rule_report(clean, ref, "%s whitening %d" % (W.varlen_id(c), wh))
        assert msg is None, msg
        for w in range(vc.n):                                    # the tail of every row: exact zeros (the rule already says so)
            assert not clean[w, 15 + vc.Ln[w]:].any() and not clean[w, :15].any()
        poisoned = launch_plain("varlen", vc.source(True), vc.offsets, 0, vc.ds, wh, 1, vc.raw_lens, vc.L0)
        assert np.array_equal(clean.view(np.uint32), poisoned.view(np.uint32)), "%s: a sample off the grid or at / past raw_lens was read" % W.varlen_id(c)


@pytest.mark.parametrize("c", W.VARLEN_CASES, ids=W.varlen_id)
def test_varlen_with_equal_lengths_is_the_crop_with_one_window_per_tower(c):
    vc = W.varlen_case(c)
    buf = vc.source(False)
    for raw_len in (W.raw_len_of(vc.L0, vc.ds, "lo"), W.raw_len_of(vc.L0, vc.ds, "hi")):
        for wh in (0, 1):
            a = launch_plain("varlen", buf, vc.offsets, 0, vc.ds, wh, 1, np.full(vc.n, raw_len, dtype=np.int64), vc.L0)
            b = launch_plain("crop", buf, vc.offsets, raw_len, vc.ds, wh, 1)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
