"""Host checks of tests/wave_exact.py, the exact references of the waveform front end (tests/test_gpu_wave_exact.py runs them against
the kernels): the exactness preconditions hold for every input of the device file, the fp32 FIR in two summation orders equals the
integer reference, the ambiguity cap holds from the reference alone, every planted defect of the host models fails the comparison the
device file makes, and the FIR defects at real tap counts stay under the bound tests/test_gpu_augment.py holds the kernel to."""
import numpy as np
import pytest

from tests import wave_exact as W
from voicemap_amd import augment as A


# ---- coverage of the tables -----------------------------------------------------------------------------------------------------------
def test_the_tables_hold_every_edge_value():
    ids = [W.fir_id(c) for c in W.FIR_CASES]
    assert len(set(ids)) == len(ids)
    for ds in W.DS_VALUES:
        got = {c[1] for c in W.FIR_CASES if c[0] == ds}
        want = {1, 2, ds, ds + 1, 8 * ds - 1, 8 * ds + 1, 255 * ds, 256 * ds, 256 * ds + 1, 257 * ds, 512 * ds + ds - 1, 8192} | ({ds - 1} - {0})
        assert got == want, (ds, sorted(want - got))
    for L0 in W.L0_SMALL + W.L0_LARGE:
        assert {(c[3], c[4]) for c in W.FIR_CASES if c[2] == L0} == {("lo", "i16"), ("lo", "f32"), ("hi", "i16"), ("hi", "f32")}, L0
        for end in ("lo", "hi"):
            T = W.raw_len_of(L0, 4, end)
            assert W.n_out(T, 4) == L0 and W.n_out(T - (end == "lo"), 4) == L0 - (end == "lo") and W.n_out(T + (end == "hi"), 4) == L0 + (end == "hi")
    assert {c[5] for c in W.FIR_CASES} == set(W.FIR_GAINS)
    assert (1, 8192, 2049) in {c[:3] for c in W.FIR_CASES}          # the clipped-causal case
    assert {c[5] for c in W.MIX_CASES} >= set(W.WPT_VALUES) and {c[5] for c in W.PLAIN_CASES} >= set(W.WPT_VALUES)
    assert {c[2] for c in W.MIX_CASES} >= set(W.L0_SMALL) and {c[6] for c in W.MIX_CASES if c[0] == "general"} == {1, 3}
    assert any((c[2] + W.HALO) % W.N_SPLIT for c in W.MIX_CASES)
    for ds, L0, _ in W.VARLEN_CASES:
        lens, Ln = W.varlen_lens(ds, L0)
        assert set(Ln) == {1, L0 - 1, L0} and len(lens) >= 8
        for want in (L0 - 1, L0):
            assert {int(v) % ds for v, l in zip(lens, Ln) if l == want} == set(range(ds))


# ---- the FIR: preconditions, two fp32 orders, the model ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.FIR_CASES, ids=W.fir_id)
def test_fir_inputs_are_on_the_grid_and_inside_the_fp32_limit(c):
    fc = W.fir_case(c)
    assert np.all(fc.k % 2 != 0) and np.abs(fc.k).max() <= 255 and np.all(np.abs(fc.t) >= 1) and np.abs(fc.t).max() <= 4
    a, peak = fc.a_units()                                  # fir_exact asserts peak < 2^24 per window
    assert peak <= 255 * 4 * fc.R < W.LIMIT
    for src in ("i16", "f32"):
        assert np.array_equal(A._as_float64(W.as_source(fc.k, src)), fc.k * W.S_UNIT)
    assert np.array_equal(W.as_rirs(fc.t).astype(np.float64), fc.t * W.T_UNIT)
    x = fc.expected()
    assert x.shape == (3, fc.L0 + 31) and np.all(x[:, :15] == 0) and np.all(x[:, 15 + fc.L0:] == 0)
    # the same numbers through the float64 statement of the semantics
    ref = A.augment_reference(W.as_source(fc.k, fc.src), fc.offsets, fc.raw_len, fc.ds, gain=fc.gain, rirs=W.as_rirs(fc.t),
                              rir_id=fc.rir_id, whitening=False)
    assert np.array_equal(ref, x.astype(np.float64))


def test_the_largest_sum_of_the_table_is_far_below_the_fp32_limit():
    peak = max(W.fir_case(c).a_units()[1] for c in W.FIR_CASES if c[1] == W.MAX_R and c[2] == 2049)
    print("R = 8192: the largest sum |t| |k| of the table is 2^%.2f grid units" % np.log2(peak))
    assert 2 ** 19 < peak < 2 ** 23


_MODEL_CASES = [c for c in W.FIR_CASES if c[2] in (9, 2049) and c[1] in (c[0] + 1, 8 * c[0] + 1, 256 * c[0] + 1, 512 * c[0] + c[0] - 1, 8192)
                and (c[1] < 8192 or c[0] in (1, 4))]


@pytest.mark.parametrize("c", _MODEL_CASES, ids=W.fir_id)
def test_fp32_fir_in_two_summation_orders_equals_the_integer_reference(c):
    """The kernel's order (phase, chunk, 8-tap block) and the ascending-tap order, product and sum each rounded to fp32: both are the
    int64 convolution bit for bit -- on this grid the FIR rounds nothing."""
    fc = W.fir_case(c)
    a, _ = fc.a_units()
    s32, r32 = W.as_source(fc.k, "f32"), W.as_rirs(fc.t)
    for w in (0, 2):
        want = (a[w] * W.A_UNIT).astype(np.float32)
        got = W.model_fir(s32, int(fc.offsets[w]), fc.raw_len, fc.ds, r32[fc.rir_id[w]], dtype=np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert np.array_equal(W.model_fir(fc.k, int(fc.offsets[w]), fc.raw_len, fc.ds, fc.t[fc.rir_id[w]]), a[w])
        if fc.R <= 2100:
            assert np.array_equal(W.fir_f32_ascending(s32[fc.offsets[w]:fc.offsets[w] + fc.raw_len], r32[fc.rir_id[w]], fc.ds), want)


# (defect, (ds, R, L0) that shows it): values of the device file's table
_FIR_DEFECT_CASES = (
    ("drop_last_tap", (4, 1028, 2049)), ("drop_last_tap", (7, 8192, 2049)), ("drop_last_tap", (7, 8, 9)),
    ("drop_chunk_edge_block", (4, 1028, 2049)), ("drop_chunk_edge_block", (1, 257, 2049)), ("drop_chunk_edge_block", (7, 3590, 2049)),
    ("causal_strict", (1, 8192, 2049)), ("causal_strict", (3, 25, 9)), ("causal_strict", (4, 33, 9)),
    ("history", (4, 1028, 2049)), ("history", (2, 2, 9)),
    ("phase_sign", (4, 1028, 2049)), ("phase_sign", (2, 2, 9)), ("phase_sign", (7, 8, 9)),
)


def _find(ds, R, L0):
    """The table's case of that (ds, R, L0), or -- the table pairs every (ds, R) with two of the lengths -- one built like it."""
    got = [c for c in W.FIR_CASES if c[:3] == (ds, R, L0)]
    assert R in W.r_values(ds) and L0 in W.L0_SMALL + W.L0_LARGE
    return got[0] if got else (ds, R, L0, "hi", "i16", 1.0)


@pytest.mark.parametrize("defect,key", _FIR_DEFECT_CASES, ids=lambda v: v if isinstance(v, str) else "ds%d-R%d-L%d" % v)
def test_a_defective_fir_fails_the_exact_comparison(defect, key):
    fc = W.fir_case(_find(*key))
    want = fc.expected()
    got = np.zeros_like(want)
    a, _ = fc.a_units()
    for w in range(3):
        aw = a[w] if fc.rir_id[w] < 0 else W.model_fir(fc.k, int(fc.offsets[w]), fc.raw_len, fc.ds, fc.t[fc.rir_id[w]], defect=defect)
        got[w, 15:15 + fc.L0] = aw * W.A_UNIT * fc.g
    msg = W.fir_report(got, want, fc.g, defect)
    assert msg is not None and "grid units" in msg and "tile" in msg and "slot" in msg
    print(msg)
    bad = got != want
    assert not bad[1].any()                                      # the window without an RIR runs no FIR
    assert np.abs((got - want)[bad]).min() >= W.A_UNIT * fc.g   # a missing or misplaced product is at least one grid unit


def test_the_sound_model_passes_and_the_reporter_is_silent():
    fc = W.fir_case(_find(4, 1028, 2049))
    want = fc.expected()
    assert W.fir_report(want.copy(), want, fc.g, "sound") is None
    nan = want.copy()
    nan[2, 15 + 2048] = np.nan                                   # an output never written
    assert "window 2, output 2048 (tile 1, thread 0, slot 0)" in W.fir_report(nan, want, fc.g, "unwritten")


# ---- the gap: the same defects under today's bound ---------------------------------------------------------------------------------
def _zeroed(rirs, which, ds):
    r = rirs.copy()
    R = r.shape[1]
    if which == "last tap":
        r[:, R - 1] = 0
    elif which == "last 8 taps":
        r[:, R - 8:] = 0
    else:                                # taps m = 248..255 of phase 1, the 8-tap block at the chunk edge (those the phase has)
        r[:, [1 + m * ds for m in range(248, 256) if 1 + m * ds < R]] = 0
    return r


@pytest.mark.parametrize("R,rt60,which", [(1000, (0.01, 0.05), "last tap"), (1000, (0.01, 0.05), "chunk-edge block"),
                                          (4096, (0.2, 0.4), "last 8 taps"), (4096, (0.2, 0.4), "last tap")],
                         ids=lambda v: str(v).replace(" ", "_") if not isinstance(v, tuple) else "rt60")
def test_fir_defects_at_real_tap_counts_pass_the_fp32_bound(R, rt60, which):
    """What tests/test_gpu_augment.py would see of a kernel that drops taps at a loop edge, on its own kind of inputs (int16 noise,
    synth_rir_bank responses with decaying tails, ds = 4): the defective output is the reference's with those taps zeroed; its
    distance from the true reference stays UNDER that file's ``_bound``, so its assertion passes."""
    from tests.test_gpu_augment import _bound, _buffers
    n, wpt, raw_len, ds, total = 6, 3, 12000, 4, 40000
    audio, _ = _buffers(total, True, seed=5)
    rirs = A.synth_rir_bank(3, rt60=rt60, max_taps=R, seed=R)
    rir_id = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    offsets = np.array([0, total - raw_len, 5000, 17001, 123, 9000], dtype=np.int64)
    kw = dict(rir_id=rir_id, windows_per_tower=wpt, details=True)
    d = A.augment_reference(audio, offsets, raw_len, ds, rirs=rirs, **kw)
    bad = A.augment_reference(audio, offsets, raw_len, ds, rirs=_zeroed(rirs, which, ds), **kw)
    L0 = d["a"].shape[1]
    err = np.abs(bad["x"] - d["x"])[:, 15:15 + L0]
    ratio = float(np.max(err / _bound(d, R, rir_id, wpt)))
    print("R = %d, %s dropped: worst |defective - reference| / bound = %.4f" % (R, which, ratio))
    assert err.max() > 0 and ratio < 1.0


# ---- the mixture: exact sums, exact plants, the cap ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.MIX_CASES, ids=W.mix_id)
def test_mixture_sums_are_exact_and_the_reference_stays_under_the_ambiguity_cap(c):
    mc = W.mix_case(c)
    assert np.all(mc.nk % 2 != 0 if mc.kind == "general" else mc.nk != 0) and np.abs(mc.nk).max() <= 255 * 8
    a, v, sums, room = mc.sums()                              # window_sums asserts the exactness with Python integers
    assert room < 1 << 53
    q_tower = max(sum(int(e) ** 2 for w in range(t0, t0 + mc.wpt) for e in a[w]) for t0 in range(0, mc.n, mc.wpt))
    assert q_tower < 1 << 53
    for wh in W.whitenings(mc.L0):
        ref = mc.reference(wh)
        share = W.ambiguous_share(ref)
        print("%s whitening %d: %d of %d samples ambiguous" % (W.mix_id(c), wh, int(ref["amb"].sum()), ref["samples"]))
        assert share <= W.AMBIGUOUS_CAP
        assert not ref["amb"][:, :15].any() and not ref["amb"][:, 15 + mc.L0:].any()
        assert np.isfinite(ref["x"]).all() and np.all(ref["d"] >= 0)
    if mc.kind == "plant":
        ref = mc.reference(0)
        assert np.array_equal(ref["g"], 2.0 ** -(mc.j + mc.m).astype(np.float64))
        y = mc.gain.astype(np.float64)[:, None] * (a * W.A_UNIT) * (1.0 + 2.0 ** -mc.m.astype(np.float64))[:, None]
        assert np.array_equal(ref["x"][:, 15:15 + mc.L0], y) and np.array_equal(y.astype(np.float32).astype(np.float64), y)
        assert not ref["amb"].any()                              # whitening off: the plant is an fp32 number, nothing to round
    else:
        assert (mc.rir_id >= 0).any() and (mc.rir_id < 0).any() and np.all((mc.snr > 0) | (np.log2(mc.gain) % 1 == 0))


@pytest.mark.parametrize("c", [c for c in W.MIX_CASES if c[0] == "general" and c[2] * c[4] <= 600], ids=W.mix_id)
def test_the_rule_covers_the_device_s_contractions(c):
    """The reference with y = G fma(g, v, a) and S = G fma(g, Sv, Sa) -- what the compiler may make of aug_apply_kernel's y + g b and
    aug_finalize_kernel's pa + g pv -- against the plain one: inside the rule, sample by sample."""
    mc = W.mix_case(c)
    assert W.fma(0.1, 10.0, -1.0) == 2.0 ** -54 * 1.0 and 0.1 * 10.0 - 1.0 == 0.0        # one rounding, not two
    for wh in W.whitenings(mc.L0):
        plain, fused = mc.reference(wh), mc.reference(wh, True)
        ratio = np.abs(fused["x"] - plain["x"]) / np.maximum(plain["d"], 1e-300)
        print("%s whitening %d: worst |contracted - plain| / d = %.3f" % (W.mix_id(c), wh, ratio.max()))
        assert not W.violations(fused["x"].astype(np.float32), plain).any()
        far = np.abs(plain["y"]) >= 1e-4          # no cancellation of a against g v (module docstring): there d bounds the difference
        assert np.all(ratio[:, 15:15 + mc.L0][far] <= 1.0)


# ---- the plain entries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.PLAIN_CASES, ids=W.plain_id)
def test_plain_references_stay_under_the_cap_and_the_model_passes(c):
    pc = W.plain_case(c)
    for wh in W.whitenings(pc.L0):
        ref = pc.reference(wh)
        print("%s whitening %d: %d of %d samples ambiguous" % (W.plain_id(c), wh, int(ref["amb"].sum()), ref["samples"]))
        assert W.ambiguous_share(ref) <= W.AMBIGUOUS_CAP
        if not wh:
            assert not ref["amb"].any() and np.array_equal(ref["x"].astype(np.float32).astype(np.float64), ref["x"])
        if pc.n * pc.L0 <= 1000:
            got = W.model_plain(pc.k, pc.offsets, np.full(pc.n, pc.raw_len), pc.ds, pc.L0, pc.wpt, wh)
            assert W.rule_report(got, ref, W.plain_id(c)) is None
        # the float64 statement of the semantics agrees (|x| < 1; its sums are taken in another order)
        full = A.augment_reference(W.as_source(pc.k, pc.src), pc.offsets, pc.raw_len, pc.ds, whitening=bool(wh), rms=W.RMS,
                                   windows_per_tower=pc.wpt)
        assert np.abs(full - ref["x"]).max() <= 1e-12


@pytest.mark.parametrize("c", W.VARLEN_CASES, ids=W.varlen_id)
def test_varlen_references_stay_under_the_cap(c):
    vc = W.varlen_case(c)
    assert vc.unread.sum() > vc.n * 16 and not vc.unread[vc.offsets].any()
    for wh in (0, 1):
        ref = vc.reference(wh)
        print("%s whitening %d: %d of %d samples ambiguous" % (W.varlen_id(c), wh, int(ref["amb"].sum()), ref["samples"]))
        assert W.ambiguous_share(ref) <= W.AMBIGUOUS_CAP
        for w in range(vc.n):
            assert np.all(ref["x"][w, 15 + vc.Ln[w]:] == 0) and np.all(ref["lo"][w, 15 + vc.Ln[w]:] == 0) and np.all(ref["hi"][w, 15 + vc.Ln[w]:] == 0)
    # the poisoned buffer differs from the clean one exactly where nothing may be read
    clean, poisoned = vc.source(False), vc.source(True)
    assert np.array_equal(clean != poisoned, vc.unread)


def _small_varlen(ds, L0, seed):
    rng = np.random.default_rng(seed)
    lens, _ = W.varlen_lens(ds, L0)
    stride = L0 * ds + 16
    return W.grid_samples(rng, len(lens) * stride), np.arange(len(lens), dtype=np.int64) * stride, lens


@pytest.mark.parametrize("defect", W.DEFECTS_PLAIN)
def test_a_defective_whitening_fails_the_rule(defect):
    """The varlen form at ds = 4, L0 = 21 (Ln in 1, 20, 21, every raw_lens % 4): the sound model passes, the defective one does not."""
    ds, L0 = 4, 21
    k, offsets, lens = _small_varlen(ds, L0, 77)
    ref = W.plain_reference(k, offsets, lens, ds, L0, 1, 1)
    assert W.rule_report(W.model_plain(k, offsets, lens, ds, L0, 1, 1), ref, "sound") is None
    msg = W.rule_report(W.model_plain(k, offsets, lens, ds, L0, 1, 1, defect=defect), ref, defect)
    assert msg is not None
    print(msg)
    if defect == "scale_L0":      # ... and with equal lengths (Ln = L0 everywhere) that defect is invisible: the varlen rows are what shows it
        full = np.full(len(lens), L0 * ds)
        assert W.rule_report(W.model_plain(k, offsets, full, ds, L0, 1, 1, defect=defect), W.plain_reference(k, offsets, full, ds, L0, 1, 1), defect) is None
