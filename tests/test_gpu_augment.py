"""-m gpu tests of vm_crop_augment_decimate_whiten (voicemap_amd/csrc/augment.hip) against augment_reference (float64), and of the
augmented training step through the public surface."""
import numpy as np
import pytest
import torch

from voicemap_amd import augment as A

pytestmark = pytest.mark.gpu

RMS = 0.038021
U = 2.0 ** -24


def _launch(audio, offsets, raw_len, ds, wpt, noise=None, noff=None, snr=None, gain=None, rirs=None, rir_id=None, whitening=True):
    """One vm_crop_augment_decimate_whiten launch on host arrays -> (n, L0 + 31) float32 on the host."""
    from voicemap_amd import _lib
    lib = _lib.lib()
    dev = "cuda"
    n = len(offsets)
    L0 = (raw_len + ds - 1) // ds
    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev, dt).contiguous()  # noqa: E731
    a_d = torch.as_tensor(audio).to(dev)
    n_d = None if noise is None else torch.as_tensor(noise).to(dev)
    K = 0 if noff is None else int(np.asarray(noff).reshape(n, -1).shape[1])
    o_d, no_d = t(offsets, torch.int64), t(noff, torch.int64)
    s_d = t(np.zeros(n) if snr is None else snr, torch.float32)
    g_d = t(np.ones(n) if gain is None else gain, torch.float32)
    r_d, id_d = t(rirs, torch.float32), t(rir_id, torch.int32)
    out = torch.full((n, L0 + 31), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty(lib.query("vm_crop_augment_workspace_bytes", n, L0) // 8 + 1, dtype=torch.float64, device=dev)
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    lib.call("vm_crop_augment_decimate_whiten", p(a_d), int(a_d.dtype == torch.int16), p(o_d), n, raw_len, ds, int(whitening), RMS, wpt,
             p(n_d) if K else None, int(K > 0 and n_d.dtype == torch.int16), p(no_d) if K else None, K, p(s_d), p(g_d),
             p(r_d), 0 if rirs is None else int(np.asarray(rirs).shape[0]), 0 if rirs is None else int(np.asarray(rirs).shape[1]), p(id_d),
             p(out), p(ws), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _plain(audio, offsets, raw_len, ds, wpt, whitening=True):
    from voicemap_amd import _lib
    lib = _lib.lib()
    n = len(offsets)
    L0 = (raw_len + ds - 1) // ds
    a_d = torch.as_tensor(audio).cuda()
    o_d = torch.as_tensor(np.asarray(offsets, dtype=np.int64)).cuda()
    out = torch.full((n, L0 + 31), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.query("vm_decimate_whiten_workspace_bytes", n) // 8, dtype=torch.float64, device="cuda")
    lib.call("vm_crop_decimate_whiten", a_d.data_ptr(), int(a_d.dtype == torch.int16), o_d.data_ptr(), n, raw_len, ds, int(whitening), RMS,
             wpt, out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _buffers(total, i16, seed):
    r = np.random.RandomState(seed)
    x = r.normal(0, 0.1, total) * (0.5 + 0.5 * np.sin(np.arange(total) / 700.0) ** 2)
    v = r.normal(0, 0.2, total)
    if i16:
        return (np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16), np.clip(np.round(v * 32768), -32768, 32767).astype(np.int16))
    return x.astype(np.float32), v.astype(np.float32)


def _bound(d, R, rir_id, wpt):
    """Per-sample bound of |device - reference| (module docstring of the test below)."""
    n, L0 = d["a"].shape
    gam = R * U / (1 - R * U)
    has = (np.asarray(rir_id) >= 0)[:, None]
    ea = np.where(has, gam * d["fir_abs"], 0.0)                                  # |a^ - a|
    rel_g = np.sum(ea * np.abs(d["a"]), axis=1) / np.maximum(np.sum(d["a"] ** 2, axis=1), 1e-300)   # |dg / g| <= |dPa| / (2 Pa), first order
    ey = d["gain"][:, None] * (ea + (d["g"] * rel_g)[:, None] * np.abs(d["v"]))   # |y^ - y|
    out = np.zeros((n, L0))
    for t0 in range(0, n, wpt):
        sl = slice(t0, t0 + wpt)
        y, e = d["y"][sl], ey[sl]
        rel_s = np.sum(e * np.abs(y)) / np.sum(y ** 2)                            # |dscale / scale|, first order
        xc = d["x"][sl, 15:15 + L0]
        out[sl] = d["scale"][sl, None] * (e + e.mean(axis=1, keepdims=True)) + np.abs(xc) * rel_s
    out *= 1.01                                                                    # the second-order terms
    return out + U * (np.abs(d["x"][:, 15:15 + L0]) + out) * 1.0000001            # + one fp32 rounding of the output


@pytest.mark.parametrize("raw_len", [2003, 4801])
@pytest.mark.parametrize("ds", [1, 3, 4])
def test_kernel_vs_reference_at_the_loop_edges(raw_len, ds):
    """n = 6, wpt = 3, int16 and fp32 audio, K in {0, 1, 3}, R in {1, 7, 64, 257, 1000}, RIR and no-RIR windows in one launch, offsets
    including 0 and total - raw_len.

    Windows with an RIR: the FIR accumulates in fp32, so for any summation order |a^_i - a_i| <= gamma_R sum_j |r_j| |s_{i ds - j}|,
    gamma_R = R 2^-24 / (1 - R 2^-24) (computed per sample in float64 = ``fir_abs``).  Everything after it is float64, so the error is
    propagated to first order (+ 1 % for the higher orders): through g (which depends on Pa), the gain, the mean that the whitening
    subtracts (the mean of the per-sample errors) and the tower's scale (its relative change times |x_i|), plus one fp32 rounding of
    the output.  Windows without an RIR: float64 until the final cast -- the plain kernel's own bound, 1e-7 absolute at rms 0.038021."""
    n, wpt, total = 6, 3, 30011
    rir_id = np.array([-1, 0, 1, -1, 2, 0], dtype=np.int32)
    snr = np.array([4.0, 0.5, 0.0, 10.0, 1.0, 2.0], dtype=np.float32)
    gain = np.array([1.0, 0.5, 2.0, 1.5, 1.0, 0.7], dtype=np.float32)
    offsets = np.array([0, total - raw_len, 1234, 7, 9001, total - raw_len - 1], dtype=np.int64)
    worst = 0.0
    for i16 in (True, False):
        audio, noise = _buffers(total, i16, seed=raw_len + ds)
        for K in (0, 1, 3):
            noff = None if K == 0 else np.array([[0, total - raw_len, 555][:K], [17, 4000, 0][:K], [1, 2, 3][:K], [total - raw_len, 0, 9][:K],
                                                 [8000, 8001, 12000][:K], [333, 21000, 15000][:K]], dtype=np.int64)
            for R in (1, 7, 64, 257, 1000):
                rirs = A.synth_rir_bank(3, rt60=(0.01, 0.05), max_taps=R, seed=R)
                kw = dict(noise=noise if K else None, snr_lin=snr, gain=gain, rirs=rirs, rir_id=rir_id)
                d = A.augment_reference(audio, offsets, raw_len, ds, noise_offsets=noff, windows_per_tower=wpt, details=True, **kw)
                got = _launch(audio, offsets, raw_len, ds, wpt, noise=kw["noise"], noff=noff, snr=snr, gain=gain, rirs=rirs, rir_id=rir_id)
                L0 = d["a"].shape[1]
                assert got.shape == (n, L0 + 31) and np.isfinite(got).all()
                assert np.all(got[:, :15] == 0) and np.all(got[:, 15 + L0:] == 0), "halo"
                err = np.abs(got[:, 15:15 + L0].astype(np.float64) - d["x"][:, 15:15 + L0])
                bound = _bound(d, R, rir_id, wpt)
                has = rir_id >= 0
                ratio = float(np.max(err[has] / bound[has]))
                worst = max(worst, ratio)
                assert np.all(err[has] <= bound[has]), (i16, K, R, ratio)
                assert err[~has].max() <= 1e-7, (i16, K, R, err[~has].max())
    print("raw_len %d ds %d: worst error / bound over the RIR windows %.3f" % (raw_len, ds, worst))


def test_kernel_vs_reference_at_a_real_tap_count():
    """n = 4, raw_len = 12000, R = 4096: the tap loop over four 256-tap chunks in each of the four phases, two output tiles per window."""
    n, wpt, raw_len, ds, R, total = 4, 2, 12000, 4, 4096, 40000
    audio, noise = _buffers(total, True, seed=5)
    rirs = A.synth_rir_bank(2, rt60=(0.2, 0.4), max_taps=R, seed=3)
    rir_id = np.array([0, -1, 1, 1], dtype=np.int32)
    offsets = np.array([0, total - raw_len, 5000, 17001], dtype=np.int64)
    noff = np.array([[100, 20000], [0, 1], [total - raw_len, 300], [9000, 9001]], dtype=np.int64)
    snr = np.array([3.0, 1.0, 0.0, 8.0], dtype=np.float32)
    gain = np.array([1.0, 2.0, 0.5, 1.0], dtype=np.float32)
    d = A.augment_reference(audio, offsets, raw_len, ds, noise=noise, noise_offsets=noff, snr_lin=snr, gain=gain, rirs=rirs, rir_id=rir_id,
                            windows_per_tower=wpt, details=True)
    got = _launch(audio, offsets, raw_len, ds, wpt, noise=noise, noff=noff, snr=snr, gain=gain, rirs=rirs, rir_id=rir_id)
    L0 = 3000
    err = np.abs(got[:, 15:15 + L0].astype(np.float64) - d["x"][:, 15:15 + L0])
    bound = _bound(d, R, rir_id, wpt)
    has = rir_id >= 0
    print("R = 4096: worst error / bound %.3f, no-RIR max abs err %.2e" % (np.max(err[has] / bound[has]), err[~has].max()))
    assert np.all(got[:, :15] == 0) and np.all(got[:, 15 + L0:] == 0)
    assert np.all(err[has] <= bound[has])
    assert err[~has].max() <= 1e-7
    # the SNR realised on the device is the request: y recovered from the whitened output of the noisy window 3 against the reference's
    # (x = (y - mean) scale is affine in y: compare the noise part's energy through the reference's own scale)
    w = 3
    y_dev = got[w, 15:15 + L0].astype(np.float64) / d["scale"][w] + d["y"][w].mean()
    nz = y_dev / d["gain"][w] - d["a"][w]                       # g v as the device realised it (+ the FIR's fp32 error)
    realised = 10 * np.log10(np.mean(d["a"][w] ** 2) / np.mean(nz ** 2))
    assert abs(realised - 10 * np.log10(float(snr[w]))) < 1e-3, realised


@pytest.mark.parametrize("i16", [True, False])
def test_identity_is_the_plain_kernel_bit_for_bit_and_launches_repeat(i16):
    total = 30011
    audio, noise = _buffers(total, i16, seed=1)
    if not i16:
        audio[100:110] = -0.0    # signed zeros survive too
    for raw_len, ds, n, wpt in ((4801, 4, 6, 3), (2003, 3, 6, 6), (2003, 1, 4, 1)):
        offsets = np.array([0, total - raw_len, 1234, 7, 9001, 100][:n], dtype=np.int64)
        for wh in (True, False):
            plain = _plain(audio, offsets, raw_len, ds, wpt, whitening=wh)
            ident = _launch(audio, offsets, raw_len, ds, wpt, whitening=wh)
            assert np.array_equal(plain.view(np.uint32), ident.view(np.uint32))
            # ... also with a bank present but nobody using it
            ident2 = _launch(audio, offsets, raw_len, ds, wpt, whitening=wh, rirs=A.synth_rir_bank(2, max_taps=33), rir_id=np.full(n, -1))
            assert np.array_equal(plain.view(np.uint32), ident2.view(np.uint32))
    raw_len, ds, n, wpt = 4801, 4, 6, 3
    offsets = np.array([0, total - raw_len, 1234, 7, 9001, 100], dtype=np.int64)
    kw = dict(noise=noise, noff=np.arange(12).reshape(6, 2) * 1000, snr=np.array([1, 2, 3, 0, 5, 6.0]), gain=np.linspace(0.5, 2, 6),
              rirs=A.synth_rir_bank(2, rt60=(0.01, 0.03), max_taps=700, seed=2), rir_id=np.array([0, 1, -1, 0, -1, 1]))
    r1 = _launch(audio, offsets, raw_len, ds, wpt, **kw)
    r2 = _launch(audio, offsets, raw_len, ds, wpt, **kw)
    assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32))
    assert not np.array_equal(r1, _plain(audio, offsets, raw_len, ds, wpt))


def test_nothing_outside_the_crop_is_read():
    """Poison values (1e30; no out-of-bounds access anywhere): fp32 audio with 1e30 right before every crop start and at every crop end
    -- and, for the windows WITHOUT an RIR, in the ds - 1 skipped positions too (this design reads them only for the FIR, which needs
    them).  The noise crops get the same treatment in a buffer of their own.  The output is the clean buffers' output bit for bit."""
    raw_len, ds, n, wpt, total = 2003, 4, 4, 2, 12000
    audio, noise = _buffers(total, False, seed=8)
    offsets = np.array([1, 2500, 5200, total - raw_len - 1], dtype=np.int64)
    noff = np.array([[1], [3000], [6000], [total - raw_len - 1]], dtype=np.int64)
    snr, gain = np.array([2.0, 1.0, 4.0, 0.5]), np.array([1.0, 2.0, 0.5, 1.5])
    rirs = A.synth_rir_bank(2, rt60=(0.01, 0.03), max_taps=300, seed=4)
    skip = np.ones(raw_len, bool)
    skip[::ds] = False
    for rir_id in (np.array([-1, -1, -1, -1]), np.array([0, 1, 0, 1])):
        pa, pn = audio.copy(), noise.copy()
        for o in offsets:
            pa[o - 1] = pa[o + raw_len] = 1e30
            if rir_id[0] < 0:
                pa[o:o + raw_len][skip] = 1e30
        for o in noff[:, 0]:
            pn[o - 1] = pn[o + raw_len] = 1e30
            pn[o:o + raw_len][skip] = 1e30       # the noise is only ever read on the decimated grid
        kw = dict(noff=noff, snr=snr, gain=gain, rirs=rirs, rir_id=rir_id)
        clean = _launch(audio, offsets, raw_len, ds, wpt, noise=noise, **kw)
        poisoned = _launch(pa, offsets, raw_len, ds, wpt, noise=pn, **kw)
        assert np.isfinite(poisoned).all()
        assert np.array_equal(clean.view(np.uint32), poisoned.view(np.uint32))


def test_zero_noise_windows_have_no_noise_and_finite_output():
    raw_len, ds, n, wpt, total = 2003, 3, 4, 2, 12000
    audio, noise = _buffers(total, True, seed=9)
    noise[4000:4000 + raw_len] = 0                     # window 1's only noise crop is silent: Pv = 0
    offsets = np.array([0, 2500, 5200, 9000], dtype=np.int64)
    noff = np.array([[100], [4000], [7000], [9000]], dtype=np.int64)
    snr = np.array([2.0, 2.0, 0.0, -3.0])              # window 2: snr_lin = 0, window 3: negative
    got = _launch(audio, offsets, raw_len, ds, wpt, noise=noise, noff=noff, snr=snr)
    ref = A.augment_reference(audio, offsets, raw_len, ds, noise=noise, noise_offsets=noff, snr_lin=snr, windows_per_tower=wpt, details=True)
    assert np.isfinite(got).all()
    assert ref["g"][0] > 0 and np.all(ref["g"][1:] == 0)
    assert np.abs(got - ref["x"]).max() <= 1e-7
    # tower 1 (windows 2, 3) has no noise at all: it is the plain kernel's output
    plain = _plain(audio, offsets, raw_len, ds, wpt)
    assert np.array_equal(got[2:].view(np.uint32), plain[2:].view(np.uint32))
    assert not np.array_equal(got[0], plain[0])


# ---- through the public surface --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resident(tmp_path_factory):
    from voicemap_amd import shards
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    d = str(tmp_path_factory.mktemp("aug_shards"))
    src = SyntheticSpeechDataset(num_speakers=10, files_per_speaker=3, seconds=0.6, min_file_seconds=0.7, max_file_seconds=1.2, seed=9)
    shards.write_shards(src, d, shard_samples=500000)
    sd = shards.ShardedSpeechDataset(d, 0.6, stochastic=True)
    sd.to_device("cuda")
    return sd


def _net():
    from voicemap_amd import keras_like as K
    from voicemap_amd import models
    enc = models.get_baseline_convolutional_encoder(16, 24, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (2400, 1), distance_metric="uniform_euclidean")
    net.compile(loss="binary_crossentropy", optimizer=K.Adam(clipnorm=1.), metrics=["accuracy"])
    return net


def _calls(eng):
    calls = []
    orig = eng._call
    eng._call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    return calls


def _policy():
    return A.AugmentPolicy(p_noise=1.0, snr_db=(5.0, 15.0), babble=(2, 2), p_reverb=0.5, gain_db=(-3.0, 3.0), seed=3,
                           rirs=A.synth_rir_bank(4, rt60=(0.02, 0.05), max_taps=512, seed=1), downsampling=4)


def test_augmented_batch_trains_on_another_input_than_the_clean_batch(resident):
    """The test that fails without the feature: one training step from augmented DeviceWindows issues the augmenting launch, and its
    network input differs from the clean batch's (same pairs, same crops) and is the reference's (augment_reference through
    np.asarray(DeviceWindows), then the host preprocessing) to 1e-6 -- the kernel tests above hold the real bound; here |x| < 1 and the
    fp32 FIR's error at R = 512 is a few 1e-7 of it."""
    from voicemap_amd import utils
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    np.random.seed(4)
    (w1, w2), y = resident.build_verification_batch_device(8, _policy())
    np.random.seed(4)
    (c1, c2), _ = resident.build_verification_batch_device(8)
    assert w1.aug is not None and np.array_equal(w1.offsets_host, c1.offsets_host)
    net, clean_net = _net(), _net()
    calls = _calls(net._ensure_engine())
    ([x1, x2], yy) = bp(([w1, w2], y))
    pl = net._train_step([x1, x2], yy)
    torch.cuda.synchronize()
    assert calls.count("vm_crop_augment_decimate_whiten") == 1 and "vm_crop_decimate_whiten" not in calls
    assert np.isfinite(pl["loss_acc"].cpu().numpy()).all()
    ([k1, k2], _) = bp(([c1, c2], y))
    x0_clean = clean_net._train_step([k1, k2], yy)["x0"]
    assert pl["x0"].shape == x0_clean.shape and not torch.equal(pl["x0"], x0_clean)
    ref = np.concatenate([np.asarray(x1), np.asarray(x2)])[:, :, 0]
    got = pl["x0"].cpu().numpy().astype(np.float64)
    assert np.all(got[:, :15] == 0) and np.all(got[:, 15 + ref.shape[1]:] == 0)
    assert np.abs(got[:, 15:15 + ref.shape[1]] - ref).max() < 1e-6


def _exact_policy():
    """Noise, gain and reverb on every window, with RIRs whose fp32 FIR is EXACT on int16 speech: a unit direct tap and seven taps on
    the 1/16 grid, |tap| <= 1/4.  A product tap x sample is a multiple of 2^-19 below 1 in size and so is every partial sum, below
    sum |tap| <= 2.75: 22 significand bits at the most, so fp32 (24) rounds nothing in any order and a is the float64 reference's."""
    r = np.random.RandomState(6)
    rirs = np.concatenate([np.ones((4, 1)), r.randint(-4, 5, (4, 7)) / 16.0], axis=1).astype(np.float32)
    return A.AugmentPolicy(p_noise=1.0, snr_db=(5.0, 15.0), babble=(2, 2), p_reverb=1.0, gain_db=(-3.0, 3.0), seed=3, rirs=rirs,
                           downsampling=4)


def test_augmented_train_on_batch_equals_the_step_on_the_reference_windows(resident):
    """One train_on_batch from augmented DeviceWindows against the same step from host windows materialised by the reference path
    (augment_reference through np.asarray(DeviceWindows), then the host preprocessing: decimate, utils.whiten per tower), f32 storage,
    compared on the loss and the updated weights at the tolerance tests/test_gpu_api.py::test_device_side_crop_equals_host_crop uses
    for device crop against host crop: equality.

    Equality of two routes needs the same numbers to go in, so the case is one where they can be the same.  (1) The RIRs are
    ``_exact_policy``'s: the fp32 FIR rounds nothing, so the only fp32 operation left on the device is the final cast, as on the host
    route.  (2) The host whitening gets the target rms the device gets: the C ABI takes ``rms`` as fp32, i.e. float32(0.038021), where
    utils.whiten's default is the double 0.038021 -- a relative 1e-8 that moves fp32 roundings of the network input (with the double,
    and with synth_rir_bank's RIRs, this comparison measured: loss equal, network input within 1.7e-7, updated weights differing by up
    to 1.8e-6).  What remains are float64 sums taken in another order: a relative 1e-16 before a cast to 24 bits.  RIRs with fp32
    rounding are held to their bound by the kernel tests above and by test_augmented_batch_trains_on_another_input_than_the_clean_batch."""
    from voicemap_amd import utils
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    np.random.seed(4)
    (w1, w2), y = resident.build_verification_batch_device(8, _exact_policy())
    assert np.all(w1.aug.rir_id >= 0) and np.all(w1.aug.snr_lin > 0) and w1.aug.K == 2 and not np.all(w1.aug.gain == 1)
    dev_net, host_net = _net(), _net()
    host_net.set_weights(dev_net.get_weights())
    ([x1, x2], yy) = bp(([w1, w2], y))
    pl = dev_net._train_step([x1, x2], yy)
    torch.cuda.synchronize()
    x0_dev = pl["x0"].cpu().numpy()
    loss_dev = pl["loss_acc"].cpu().numpy().copy()
    rms32 = float(np.float32(RMS))
    h1, h2 = (utils.whiten(np.asarray(w)[:, ::4, :], rms=rms32) for w in (w1, w2))   # augment_reference -> decimate -> whiten, float64
    ref = np.concatenate([h1, h2])[:, :, 0].astype(np.float32)
    got = x0_dev[:, 15:15 + ref.shape[1]]
    print("augmented x0: %d of %d samples differ from the reference's, max |difference| %.3e"
          % (int((got != ref).sum()), ref.size, np.abs(got.astype(np.float64) - ref).max()))
    loss_host = np.array(host_net.train_on_batch([h1, h2], yy))
    wd, wh = dev_net.get_weights(), host_net.get_weights()
    wdiff = max(float(np.abs(a - b).max()) for a, b in zip(wd, wh))
    print("loss device %.9g host %.9g; max |weight difference| %.3e" % (loss_dev[0], loss_host[0], wdiff))
    assert float(loss_dev[0]) == float(loss_host[0])
    for a, b in zip(wd, wh):
        assert np.array_equal(a, b)


def test_evaluation_paths_and_clean_training_never_augment(resident):
    from voicemap_amd import retrieval, utils
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    net = _net()
    calls = _calls(net._ensure_engine())
    np.random.seed(3)
    utils.n_shot_task_evaluation(net, resident, bp, 4, 1, 5, network_type="siamese")
    retrieval.embed_corpus(net, resident, bp, network_type="siamese", batch=16)
    (c1, c2), y = resident.build_verification_batch_device(8)          # augmentation off: the plain launch
    net.train_on_batch(*bp(([c1, c2], y)))
    assert "vm_crop_decimate_whiten" in calls
    assert "vm_crop_augment_decimate_whiten" not in calls
    # and three augmented steps in a row (eager, recorded, replayed from the native program) stay finite and keep augmenting
    pol = _policy()
    eng = net._ensure_engine()
    for step in range(4):
        (w1, w2), y = resident.build_verification_batch_device(8, pol)
        loss, _ = net.train_on_batch(*bp(([w1, w2], y)))
        assert np.isfinite(loss)
    ref_in = np.concatenate([np.asarray(x) for x in bp(([w1, w2], y))[0]])[:, :, 0]
    got = eng.plan(16, 2400, True)["x0"][:, 15:15 + 2400].cpu().numpy()
    assert np.abs(got - ref_in).max() < 1e-5      # the replayed step preprocessed THIS batch's parameters
