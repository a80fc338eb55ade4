"""Waveform augmentation for device-resident siamese training: additive babble at a drawn SNR, reverberation, level perturbation.

With ``ShardedSpeechDataset.to_device()`` a batch is nothing but start offsets into a buffer that lives in HBM and the crop happens
inside the preprocessing launch; augmenting on the host would bring the waveforms back over the bus.  Here the host only draws a few
more numbers per window (``AugmentPolicy``) and ``vm_crop_augment_decimate_whiten`` applies them inside that launch.  Nothing is
downloaded: the noise is babble cut from the resident corpus itself (or from a second resident buffer, ``NoiseBank``), the room impulse
responses are synthesised from a seed (``synth_rir_bank``) or given as an array.

Semantics -- ``augment_reference`` below is their float64 statement, and what every test compares against.  Window n of a batch with
raw length T, decimation ds and L0 = ceil(T / ds):  s[t] = audio[off[n] + t], 0 <= t < T (int16 read as v / 32768).  The reference
decimates with ``x[::ds]`` and no anti-alias filter, so the network only ever sees the positions t = i ds, i = 0..L0-1, and everything
is defined THERE:

1. reverb   a_i = sum_{j=0}^{min(i ds, R-1)} r[j] s[i ds - j]  with r = rirs[rir_id[n]] (R taps, causal, direct path at tap 0); the
            history before the crop start is zero; rir_id[n] < 0: a_i = s[i ds].  (A decimating FIR: L0 R multiply-adds per window.)
2. noise    v_i = sum_{k<K} noise[noff[n, k] + i ds]  (K launch-wide);  Pa = mean_i a_i^2, Pv = mean_i v_i^2;
            g = sqrt(Pa / (Pv snr_lin[n])), snr_lin = 10^(snr_dB / 10);  g = 0 if K == 0, Pa == 0, Pv == 0 or snr_lin[n] <= 0
            (a non-positive snr_lin means "no noise for this window").
3. gain     y_i = gain[n] (a_i + g v_i)
4. the whitening of the plain path on y: per-window mean, one scale per tower of ``windows_per_tower`` windows, conv 1's 15 / 16
            zero halo.

Augmentation is for training batches only: n-shot tasks, ``embed_corpus``, ``embed_varlen`` and every evaluation path never augment.
Whether it improves EER on real data has not been measured here.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

INT16_SCALE = 32768.0
MAX_RIR_TAPS = 8192   # vm_crop_augment_decimate_whiten's limit
HALO_L, HALO_R = 15, 16


def _as_float64(buf) -> np.ndarray:
    buf = np.asarray(buf)
    return buf.astype(np.float64) / INT16_SCALE if buf.dtype == np.int16 else buf.astype(np.float32).astype(np.float64)


def augment_reference(audio, offsets, raw_len: int, downsampling: int, noise=None, noise_offsets=None, snr_lin=None, gain=None,
                      rirs=None, rir_id=None, whitening: bool = True, rms: float = 0.038021,
                      windows_per_tower: Optional[int] = None, details: bool = False):
    """The semantics in the module docstring, numpy float64.  ``audio`` / ``noise``: 1-D int16 or float buffers; ``offsets`` (n,),
    ``noise_offsets`` (n, K) or None (K = 0), ``snr_lin`` / ``gain`` (n,) or None (no noise / unit gain), ``rirs`` (n_rirs, R) with
    ``rir_id`` (n,) or None.  Returns the network input (n, L0 + 31) with the halo; ``details=True`` returns a dict with it (``x``) and
    ``a``, ``v``, ``g``, ``y`` (the mixture before whitening, (n, L0)), ``scale`` (per window: its tower's) and ``fir_abs`` =
    sum_j |r_j| |s_{i ds - j}| (what an fp32 FIR's rounding error is bounded against; |s_{i ds}| where there is no RIR)."""
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    n, T, ds = offsets.size, int(raw_len), int(downsampling)
    L0 = (T + ds - 1) // ds
    K = 0 if noise_offsets is None else int(np.asarray(noise_offsets).reshape(n, -1).shape[1])
    snr = np.zeros(n) if snr_lin is None else np.asarray(snr_lin, dtype=np.float32).astype(np.float64).reshape(n)
    G = np.ones(n) if gain is None else np.asarray(gain, dtype=np.float32).astype(np.float64).reshape(n)
    rid = np.full(n, -1, dtype=np.int64) if rir_id is None or rirs is None else np.asarray(rir_id, dtype=np.int64).reshape(n)
    a, v, g, fir_abs = np.zeros((n, L0)), np.zeros((n, L0)), np.zeros(n), np.zeros((n, L0))
    for w in range(n):
        s = _as_float64(np.asarray(audio)[offsets[w]:offsets[w] + T])
        if rid[w] >= 0:
            r = np.asarray(rirs, dtype=np.float32).astype(np.float64)[rid[w]]
            a[w] = np.convolve(s, r)[:T][::ds]            # zero history: the full convolution's first T samples
            fir_abs[w] = np.convolve(np.abs(s), np.abs(r))[:T][::ds]
        else:
            a[w] = s[::ds]
            fir_abs[w] = np.abs(a[w])
        if K:
            no = np.asarray(noise_offsets, dtype=np.int64).reshape(n, K)[w]
            for k in range(K):
                v[w] += _as_float64(np.asarray(noise)[no[k]:no[k] + T:ds])
        Pa, Pv = np.mean(a[w] ** 2), np.mean(v[w] ** 2)
        if K and Pa > 0 and Pv > 0 and snr[w] > 0:
            g[w] = np.sqrt(Pa / (Pv * snr[w]))
    y = G[:, None] * (a + g[:, None] * v)
    wpt = n if windows_per_tower is None else int(windows_per_tower)
    assert n % wpt == 0
    scale = np.ones(n)
    x = y
    if whitening:
        x = y - y.mean(axis=1, keepdims=True)
        for t0 in range(0, n, wpt):
            scale[t0:t0 + wpt] = rms / np.sqrt(np.mean(y[t0:t0 + wpt] ** 2))
        x = x * scale[:, None]
    x = np.pad(x, ((0, 0), (HALO_L, HALO_R)))
    if details:
        return {"x": x, "a": a, "v": v, "g": g, "y": y, "scale": scale, "fir_abs": fir_abs, "gain": G}
    return x


def synth_rir_bank(n: int, rt60: Tuple[float, float] = (0.2, 0.8), sr: int = 16000, max_taps: int = 4096, seed: int = 0) -> np.ndarray:
    """(n, R) float32 synthetic room impulse responses, R = ``max_taps``: a unit direct tap at index 0, then Gaussian noise under an
    exponential envelope that falls by 60 dB in the row's RT60 (drawn uniformly from ``rt60`` seconds), the row normalised to unit
    energy.  The same arguments give the same bank."""
    if not 1 <= max_taps <= MAX_RIR_TAPS:
        raise ValueError("max_taps must be in [1, %d]" % MAX_RIR_TAPS)
    rng = np.random.RandomState(seed)
    t = np.arange(max_taps) / float(sr)
    bank = np.zeros((n, max_taps), dtype=np.float64)
    for i in range(n):
        t60 = rng.uniform(rt60[0], rt60[1])
        tail = rng.standard_normal(max_taps) * np.exp(-3.0 * np.log(10.0) * t / t60)   # amplitude 10^(-3 t / RT60): -60 dB at RT60
        tail[0] = 0.0
        # direct-to-reverberant ratio 0 dB before the normalisation: a tail of unit energy under a unit direct tap
        e = np.sum(tail ** 2)
        bank[i] = tail / np.sqrt(e) if e > 0 else tail
        bank[i, 0] = 1.0
        bank[i] /= np.sqrt(np.sum(bank[i] ** 2))
    bank = bank.astype(np.float32)
    # unit energy in the stored precision too (one more normalisation in float32 terms; the direct tap stays the row's first)
    bank /= np.sqrt(np.sum(bank.astype(np.float64) ** 2, axis=1, keepdims=True)).astype(np.float32)
    return bank


class NoiseBank:
    """A second resident buffer to cut the noise from: ``audio`` a 1-D int16 / fp32 device tensor (or host array, for host tests) of
    recordings back to back, ``starts`` / ``lengths`` the position of every recording in it.  Crops never straddle recordings."""

    def __init__(self, audio, starts, lengths):
        self.audio = audio
        self.starts = np.asarray(starts, dtype=np.int64).reshape(-1)
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        assert self.starts.size == self.lengths.size > 0


class AugmentRecord:
    """The per-window parameters of one augmented batch (host arrays) + the buffers they refer to.  ``noise_offsets`` (n, K) int64,
    ``snr_lin`` / ``gain`` (n,) float32, ``rir_id`` (n,) int32; ``noise`` the buffer the noise offsets index (a device tensor in
    training), ``rirs`` the device RIR bank or None, ``rirs_host`` its host copy (the reference path), ``downsampling`` the decimation
    the mixture is defined for."""

    def __init__(self, noise_offsets, snr_lin, gain, rir_id, noise, rirs, rirs_host, downsampling: int):
        n = np.asarray(snr_lin).size
        self.noise_offsets = np.ascontiguousarray(np.asarray(noise_offsets, dtype=np.int64).reshape(n, -1))
        self.snr_lin = np.ascontiguousarray(snr_lin, dtype=np.float32).reshape(n)
        self.gain = np.ascontiguousarray(gain, dtype=np.float32).reshape(n)
        self.rir_id = np.ascontiguousarray(rir_id, dtype=np.int32).reshape(n)
        self.noise, self.rirs, self.rirs_host, self.downsampling = noise, rirs, rirs_host, int(downsampling)

    @property
    def K(self) -> int:
        return int(self.noise_offsets.shape[1])

    def __len__(self):
        return int(self.snr_lin.size)

    def rows(self, lo: int, hi: int) -> "AugmentRecord":
        return AugmentRecord(self.noise_offsets[lo:hi], self.snr_lin[lo:hi], self.gain[lo:hi], self.rir_id[lo:hi], self.noise,
                             self.rirs, self.rirs_host, self.downsampling)


class AugmentPolicy:
    """Draws the per-window augmentation parameters of training batches.

    ``p_noise``: probability that a window gets noise, at an SNR drawn uniformly from ``snr_db`` (dB); the noise is the sum of K
    babble voices, K drawn uniformly from ``babble = (kmin, kmax)`` ONCE PER BATCH (the launch has one K).  ``p_reverb``: probability
    that a window is convolved with a row of ``rirs`` ((n_rirs, R) float32: ``synth_rir_bank`` or the user's own; None: no reverb).
    ``gain_db``: level perturbation, uniform in dB.  ``downsampling``: the decimation of the training preprocessor (the mixture is
    defined at the decimated positions).  ``noise``: None -- babble from the dataset's own resident corpus, from files of speakers
    other than the window's -- or a ``NoiseBank``.

    All draws come from the policy's OWN ``np.random.RandomState(seed)``, never from the global ``np.random`` stream the dataset's pair
    and offset draws consume: switching augmentation on leaves which pairs and crops are drawn unchanged."""

    def __init__(self, p_noise: float = 0.5, snr_db: Tuple[float, float] = (5.0, 20.0), babble: Tuple[int, int] = (1, 3),
                 p_reverb: float = 0.0, gain_db: Tuple[float, float] = (0.0, 0.0), seed: int = 0, rirs=None, downsampling: int = 4,
                 noise: Optional[NoiseBank] = None):
        if not (0.0 <= p_noise <= 1.0 and 0.0 <= p_reverb <= 1.0):
            raise ValueError("p_noise and p_reverb are probabilities")
        if not (0 <= int(babble[0]) <= int(babble[1])):
            raise ValueError("babble = (kmin, kmax) with 0 <= kmin <= kmax")
        if snr_db[0] > snr_db[1] or gain_db[0] > gain_db[1]:
            raise ValueError("ranges are (lo, hi) with lo <= hi")
        if p_reverb > 0 and rirs is None:
            raise ValueError("p_reverb > 0 needs an RIR bank (synth_rir_bank)")
        self.p_noise, self.snr_db, self.babble = float(p_noise), (float(snr_db[0]), float(snr_db[1])), (int(babble[0]), int(babble[1]))
        self.p_reverb, self.gain_db, self.seed = float(p_reverb), (float(gain_db[0]), float(gain_db[1])), int(seed)
        self.downsampling, self.noise = int(downsampling), noise
        self.rirs_host = None
        if rirs is not None:
            self.rirs_host = np.ascontiguousarray(rirs, dtype=np.float32)
            if self.rirs_host.ndim != 2 or not 1 <= self.rirs_host.shape[1] <= MAX_RIR_TAPS:
                raise ValueError("rirs must be (n_rirs, R) with 1 <= R <= %d" % MAX_RIR_TAPS)
        self._rirs_dev = None
        self.rng = np.random.RandomState(self.seed)

    def rirs_on(self, device):
        """The RIR bank as a device tensor (uploaded once)."""
        if self.rirs_host is None:
            return None
        if self._rirs_dev is None or self._rirs_dev.device != device:
            import torch
            self._rirs_dev = torch.from_numpy(self.rirs_host).to(device).contiguous()
        return self._rirs_dev

    def draw_params(self, n: int):
        """(K, snr_lin (n,) float32 with 0 = no noise, gain (n,) float32, rir_id (n,) int32 with -1 = no reverb) for one batch of n
        windows.  A fixed number of draws per batch, whatever they come out as: the stream position depends on n alone."""
        rng = self.rng
        K = int(rng.randint(self.babble[0], self.babble[1] + 1))
        noisy = rng.random_sample(n) < self.p_noise
        snr_db = rng.uniform(self.snr_db[0], self.snr_db[1], size=n)
        snr_lin = np.where(noisy & (K > 0), 10.0 ** (snr_db / 10.0), 0.0).astype(np.float32)
        gain = (10.0 ** (rng.uniform(self.gain_db[0], self.gain_db[1], size=n) / 20.0)).astype(np.float32)
        reverb = rng.random_sample(n) < self.p_reverb
        n_rirs = 0 if self.rirs_host is None else self.rirs_host.shape[0]
        pick = rng.randint(0, max(n_rirs, 1), size=n)
        rir_id = np.where(reverb & (n_rirs > 0), pick, -1).astype(np.int32)
        return K, snr_lin, gain, rir_id

    def draw_noise_offsets(self, n: int, K: int, raw_len: int, starts, lengths, speakers=None, own_speaker=None):
        """(n, K) start offsets of noise crops of ``raw_len`` samples, each inside ONE recording (``starts`` / ``lengths`` of the
        recordings in the noise buffer); with ``speakers`` (per recording) and ``own_speaker`` (per window) never from a recording of
        the window's own speaker."""
        starts, lengths = np.asarray(starts, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
        ok = np.flatnonzero(lengths >= raw_len)
        if K and not ok.size:
            raise ValueError("no recording is long enough for a noise crop of %d samples" % raw_len)
        out = np.zeros((n, K), dtype=np.int64)
        if not K:
            return out
        u_file, u_start = self.rng.random_sample((n, K)), self.rng.random_sample((n, K))
        for w in range(n):
            cand = ok
            if speakers is not None and own_speaker is not None:
                cand = ok[np.asarray(speakers)[ok] != own_speaker[w]]
                if not cand.size:
                    raise ValueError("babble needs recordings of at least two speakers")
            f = cand[np.minimum((u_file[w] * cand.size).astype(np.int64), cand.size - 1)]
            span = lengths[f] - raw_len + 1
            out[w] = starts[f] + np.minimum((u_start[w] * span).astype(np.int64), span - 1)
        return out

    def draw(self, dataset, file_ids, raw_len: int, device_audio=None) -> AugmentRecord:
        """The record of one batch: ``file_ids`` (n,) the dataset file every window was cut from (its speaker is excluded from that
        window's babble).  ``dataset``: a ``ShardedSpeechDataset`` (its ``global_offset`` / ``file_length`` table)."""
        file_ids = np.asarray(file_ids, dtype=np.int64).reshape(-1)
        n = file_ids.size
        K, snr_lin, gain, rir_id = self.draw_params(n)
        audio = dataset.device_audio if device_audio is None else device_audio
        if self.noise is not None:
            noff = self.draw_noise_offsets(n, K, raw_len, self.noise.starts, self.noise.lengths)
            noise = self.noise.audio
        else:
            spk = dataset.df['speaker_id'].values
            noff = self.draw_noise_offsets(n, K, raw_len, dataset.global_offset, dataset.file_length, spk, spk[file_ids])
            noise = audio
        rirs = self.rirs_on(audio.device) if (audio is not None and hasattr(audio, "device") and self.rirs_host is not None) else None
        return AugmentRecord(noff, snr_lin, gain, rir_id, noise, rirs, self.rirs_host, self.downsampling)


def policy_from_args(args, downsampling: int) -> Optional[AugmentPolicy]:
    """The policy the experiment scripts' ``--augment`` flags ask for (None without ``--augment``); ``add_augment_args`` declares them."""
    if not getattr(args, "augment", False):
        for name in ("aug_snr", "aug_babble", "aug_reverb", "aug_rt60", "aug_gain_db", "aug_seed"):
            if getattr(args, name, None) is not None:
                raise SystemExit("--%s needs --augment" % name.replace("_", "-"))
        return None
    if not getattr(args, "device_data", False):
        raise SystemExit("--augment needs --device-data: the augmentation runs inside the device-side crop of a resident corpus")
    p_reverb = 0.0 if args.aug_reverb is None else float(args.aug_reverb)
    seed = 0 if args.aug_seed is None else int(args.aug_seed)
    rirs = None
    if p_reverb > 0:
        rirs = synth_rir_bank(64, rt60=tuple(args.aug_rt60 or (0.2, 0.8)), seed=seed)
    return AugmentPolicy(p_noise=0.5, snr_db=tuple(args.aug_snr or (5.0, 20.0)), babble=tuple(int(k) for k in (args.aug_babble or (1, 3))),
                         p_reverb=p_reverb, gain_db=tuple(args.aug_gain_db or (0.0, 0.0)), seed=seed, rirs=rirs,
                         downsampling=downsampling)


def add_augment_args(parser):
    """``--augment`` and its parameters, all off by default; valid only with ``--device-data`` (``policy_from_args`` checks)."""
    parser.add_argument('--augment', action='store_true',
                        help='augment the training batches on the chip: babble noise cut from the resident corpus at a drawn SNR, '
                             'optional synthetic reverberation and level perturbation (needs --device-data; validation and '
                             'evaluation stay clean)')
    parser.add_argument('--aug-snr', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='SNR range in dB (default 5 20)')
    parser.add_argument('--aug-babble', type=int, nargs=2, metavar=('KMIN', 'KMAX'), default=None,
                        help='babble voices per batch, drawn uniformly (default 1 3)')
    parser.add_argument('--aug-reverb', type=float, metavar='P', default=None,
                        help='probability that a window is reverberated with a synthetic RIR (default 0)')
    parser.add_argument('--aug-rt60', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='RT60 range in seconds (default 0.2 0.8)')
    parser.add_argument('--aug-gain-db', type=float, nargs=2, metavar=('LO', 'HI'), default=None, help='level perturbation range in dB (default 0 0)')
    parser.add_argument('--aug-seed', type=int, default=None, help='seed of the augmentation draws and the RIR bank (default 0)')
    return parser
