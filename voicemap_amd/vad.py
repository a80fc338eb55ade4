"""Voice activity detection on the device-resident int16 corpus, and silence-trimmed corpora.

``whiten`` scales every window, and every whole utterance, by rms / sqrt(mean(x^2)): the more of a recording is pause, the louder its
speech enters the network.  This module marks the frames of every utterance that carry speech by an energy rule relative to the
utterance's own mean energy (``detect``: ``vm_vad_frames``, voicemap_amd/csrc/vad.hip) and copies the kept frames of all utterances
into a new buffer (``trim``: ``vm_vad_compact``).  The audio is int16 PCM (what ``ShardedSpeechDataset.to_device`` uploads), the energies
are integers and the rule compares products of doubles, so the kernels and ``vad_reference`` below -- the numpy statement every test
compares against -- agree bit for bit.

The rule, for one utterance of ``len`` samples s[0..len-1] and a frame of Fr samples:

  F = ceil(len / Fr) frames;  n_f = min(Fr, len - f Fr) (the last frame may be short);  E_f = sum of s_t^2 over frame f (int64);
  T = sum_f E_f (int64).  With D() the int64 -> double conversion and (x) ONE IEEE double multiply, frame f is ACTIVE when

      a_f = [E_f > 0]  and  [D(E_f) (x) D(len) >= rel (x) (D(T) (x) D(n_f))]  and  [D(E_f) >= floor (x) D(n_f)]

  i.e. its mean energy is at least ``rel`` = 10^(-threshold_db / 10) of the utterance's, and at least ``floor`` (int16^2 per sample).
  Only multiplies, no additions: nothing a fused multiply-add could contract.

  bursts   p_f = some run of ``min_run`` = m consecutive active frames a_g .. a_{g+m-1} inside [0, F) covers f
  hangover v_f = some p_g with |g - f| <= ``hang``, 0 <= g < F
  fallback V = sum_f v_f n_f;  V < ``min_keep``: the utterance is kept whole (every v_f = 1, V = len, fallback = 1)
  layout   dst_f = sum_{g<f} v_g n_g;  the trimmed utterance is the kept frames in order, out[dst_f + t] = s[f Fr + t]

Limits: 1 <= Fr <= 4096, 1 <= min_run <= 64, 0 <= hang <= 256, 1 <= len < 2^31 (so E_f <= 2^42 and T < 2^61).

Whether trimming improves EER on real data has not been measured here.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

MAX_FRAME, MAX_MIN_RUN, MAX_HANG, MAX_LEN = 4096, 64, 256, (1 << 31) - 1
DECIDE_CHUNK = 1024   # frames per chunk of the decide pass (VAD_CH of csrc/vad.hip): the tests place runs and hangovers on its edges


class VadPolicy:
    """The parameters of the rule in the module docstring.  ``frame`` = round(frame_ms * sampling_rate / 1000) samples;
    ``rel`` = 10^(-threshold_db / 10), or given directly (``VadPolicy(rel=0.25)``: an exactly representable ratio, for tests that plant
    ties); ``floor_energy`` in int16^2 per sample; ``min_keep`` in samples, None = the caller's default (a dataset's fragment length, the
    encoder's shortest input; 1 where there is none: an utterance never trims to nothing)."""

    def __init__(self, frame_ms: float = 10.0, threshold_db: float = 25.0, floor_energy: float = 0.0, min_run: int = 3, hang: int = 10,
                 min_keep: Optional[int] = None, sampling_rate: int = 16000, rel: Optional[float] = None):
        self.frame_ms, self.threshold_db, self.sampling_rate = float(frame_ms), float(threshold_db), int(sampling_rate)
        self.frame = int(round(self.frame_ms * self.sampling_rate / 1000.0))
        self.rel = float(10.0 ** (-self.threshold_db / 10.0)) if rel is None else float(rel)
        self.floor_energy, self.min_run, self.hang = float(floor_energy), int(min_run), int(hang)
        self.min_keep = None if min_keep is None else int(min_keep)
        if not 1 <= self.frame <= MAX_FRAME:
            raise ValueError("the frame must be 1..%d samples (frame_ms %g at %d Hz is %d)" % (MAX_FRAME, frame_ms, sampling_rate, self.frame))
        if not 1 <= self.min_run <= MAX_MIN_RUN:
            raise ValueError("min_run must be in [1, %d]" % MAX_MIN_RUN)
        if not 0 <= self.hang <= MAX_HANG:
            raise ValueError("hang must be in [0, %d]" % MAX_HANG)
        if not (np.isfinite(self.rel) and self.rel >= 0.0 and np.isfinite(self.floor_energy) and self.floor_energy >= 0.0):
            raise ValueError("rel (threshold_db) and floor_energy must be finite and non-negative")
        if self.min_keep is not None and self.min_keep < 1:
            raise ValueError("min_keep must be at least 1 sample")

    def keep(self, default: int = 1) -> int:
        """``min_keep``, or ``default`` where the policy leaves it open."""
        return int(default) if self.min_keep is None else self.min_keep

    def with_min_keep(self, default: int) -> "VadPolicy":
        """This policy with an open ``min_keep`` set to ``default`` (a policy that names one is returned as it is)."""
        if self.min_keep is not None:
            return self
        return VadPolicy(self.frame_ms, self.threshold_db, self.floor_energy, self.min_run, self.hang, int(default), self.sampling_rate,
                         rel=self.rel)


def _check_lens(lens: np.ndarray):
    if lens.size and (lens.min() < 1 or lens.max() > MAX_LEN):
        raise ValueError("every utterance must hold 1 <= len < 2^31 samples")


def _as_pcm(pcm) -> np.ndarray:
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16:
        raise TypeError("voice activity detection reads int16 PCM (shards.to_int16), not %s" % pcm.dtype)
    return pcm.reshape(-1)


def vad_reference(pcm, policy: VadPolicy) -> dict:
    """The rule of the module docstring for ONE utterance, numpy float64 / int64.  ``pcm``: 1-D int16.  Returns ``energy`` (F,) int64,
    ``active`` (a_f), ``mask`` (v_f after the fallback, uint8), ``dst`` (F,) int64, ``new_len``, ``fallback`` (0 / 1), ``info`` = (F,
    sum a, sum v, fallback) and ``pcm``: the trimmed utterance (int16)."""
    s = _as_pcm(pcm)
    n, Fr, m, h = int(s.size), policy.frame, policy.min_run, policy.hang
    _check_lens(np.array([n], dtype=np.int64))
    F = (n + Fr - 1) // Fr
    sq = np.zeros(F * Fr, dtype=np.int64)
    sq[:n] = s.astype(np.int64) ** 2
    E = sq.reshape(F, Fr).sum(axis=1)
    n_f = np.minimum(Fr, n - np.arange(F, dtype=np.int64) * Fr)
    T = int(E.sum())
    Ed, nd = E.astype(np.float64), n_f.astype(np.float64)
    a = (E > 0) & (Ed * np.float64(n) >= np.float64(policy.rel) * (np.float64(T) * nd)) & (Ed >= np.float64(policy.floor_energy) * nd)
    # bursts: the maximal runs of active frames that are at least m long
    edge = np.diff(np.concatenate([[0], a.astype(np.int8), [0]]))
    start, stop = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    p = np.zeros(F, dtype=bool)
    for b, e in zip(start, stop):
        if e - b >= m:
            p[b:e] = True
    # hangover: any p within h frames
    cs = np.concatenate([[0], np.cumsum(p)])
    f = np.arange(F)
    v = (cs[np.minimum(F, f + h + 1)] - cs[np.maximum(0, f - h)]) > 0
    V = int((v * n_f).sum())
    fallback = int(V < policy.keep())
    if fallback:
        v, V = np.ones(F, dtype=bool), n
    dst = np.concatenate([[0], np.cumsum(v * n_f)[:-1]]).astype(np.int64)
    out = s[np.repeat(v, Fr)[:n]]
    return {"energy": E, "active": a, "mask": v.astype(np.uint8), "dst": dst, "new_len": V, "fallback": fallback,
            "info": (F, int(a.sum()), int(v.sum()), fallback), "pcm": np.ascontiguousarray(out)}


class VadResult:
    """What ``detect`` leaves on the device: ``mask`` (one byte per frame), ``energy`` and ``dst`` (int64 per frame), flat over all
    frames with utterance u's at [frame_base[u], frame_base[u + 1]); ``new_lens`` (n,) int64; ``info`` (n, 4) int32 = (F, active frames,
    kept frames after the fallback, fallback); ``frame_base`` (n + 1,) int64.  ``lens`` / ``frame_base_host`` are the host's copies."""

    def __init__(self, policy, lens, frame_base_host, mask, energy, dst, new_lens, info, frame_base):
        self.policy, self.lens, self.frame_base_host = policy, lens, frame_base_host
        self.mask, self.energy, self.dst, self.new_lens, self.info, self.frame_base = mask, energy, dst, new_lens, info, frame_base
        self._host = None

    def _tables(self):
        if self._host is None:
            self._host = (self.info.cpu().numpy().astype(np.int64).reshape(-1, 4), self.new_lens.cpu().numpy().astype(np.int64))
        return self._host

    def counts(self) -> dict:
        """files, frames, active frames, samples, kept samples and files kept whole by the fallback, as integers (one read-back of the
        two per-utterance tables): what ``summarise`` adds up over several corpora."""
        info, new_lens = self._tables()
        return {"files": int(info.shape[0]), "frames": int(info[:, 0].sum()), "active": int(info[:, 1].sum()),
                "samples": int(np.asarray(self.lens).sum()), "kept": int(new_lens.sum()), "kept_whole": int(info[:, 3].sum())}

    def summary(self) -> dict:
        """files, frames, the share of frames the rule calls active, the share of samples kept, and the files the fallback kept whole."""
        return summarise([self.counts()])


def reference_counts(refs, lens) -> dict:
    """``VadResult.counts`` of a list of ``vad_reference`` results and the utterances' original lengths."""
    return {"files": len(refs), "frames": sum(r["info"][0] for r in refs), "active": sum(r["info"][1] for r in refs),
            "samples": int(np.sum(lens)) if len(refs) else 0, "kept": sum(r["new_len"] for r in refs),
            "kept_whole": sum(r["fallback"] for r in refs)}


def summarise(counts) -> dict:
    """One summary over the ``counts`` of several corpora."""
    tot = {k: sum(c[k] for c in counts) for k in ("files", "frames", "active", "samples", "kept", "kept_whole")}
    return {"files": tot["files"], "frames": tot["frames"], "active_share": tot["active"] / max(tot["frames"], 1),
            "kept_share": tot["kept"] / max(tot["samples"], 1), "kept_whole": tot["kept_whole"]}


def _tables(offsets, lens, policy):
    offsets = np.ascontiguousarray(np.asarray(offsets.cpu() if hasattr(offsets, "cpu") else offsets, dtype=np.int64).reshape(-1))
    lens = np.ascontiguousarray(np.asarray(lens.cpu() if hasattr(lens, "cpu") else lens, dtype=np.int64).reshape(-1))
    if offsets.size != lens.size:
        raise ValueError("offsets and lens differ in length")
    _check_lens(lens)
    F = (lens + policy.frame - 1) // policy.frame
    return offsets, lens, np.concatenate([[0], np.cumsum(F)]).astype(np.int64)


def _check_audio(audio, offsets, lens):
    import torch
    if not torch.is_tensor(audio) or audio.dtype != torch.int16:
        raise TypeError("voice activity detection reads the resident int16 PCM buffer (ShardedSpeechDataset.to_device), not %s"
                        % (audio.dtype if hasattr(audio, "dtype") else type(audio).__name__))
    if audio.dim() != 1 or not audio.is_cuda or not audio.is_contiguous():
        raise ValueError("audio must be a contiguous 1-D device tensor")
    if lens.size and (offsets.min() < 0 or int((offsets + lens).max()) > audio.numel()):
        raise ValueError("an utterance lies outside the audio buffer")


def detect(audio, offsets, lens, policy: VadPolicy) -> VadResult:
    """Mark the kept frames of every utterance ``audio[offsets[u] : offsets[u] + lens[u]]`` of a resident int16 buffer (two launches,
    no read-back).  ``offsets`` / ``lens``: (n,) int64, host arrays or tensors."""
    import torch
    from . import _lib
    offsets, lens, fb = _tables(offsets, lens, policy)
    _check_audio(audio, offsets, lens)
    n, total, dev = int(lens.size), int(fb[-1]), audio.device
    tab = torch.from_numpy(np.concatenate([offsets, lens, fb])).to(dev)   # one upload
    energy = torch.empty(total, dtype=torch.int64, device=dev)
    dst = torch.empty(total, dtype=torch.int64, device=dev)
    mask = torch.empty(total, dtype=torch.uint8, device=dev)
    new_lens = torch.empty(n, dtype=torch.int64, device=dev)
    info = torch.empty(n, 4, dtype=torch.int32, device=dev)
    res = VadResult(policy, lens, fb, mask, energy, dst, new_lens, info, tab[2 * n:])
    res._offsets_dev, res._lens_dev = tab[:n], tab[n:2 * n]
    if n:
        _lib.lib().call("vm_vad_frames", audio.data_ptr(), tab.data_ptr(), tab[n:].data_ptr(), tab[2 * n:].data_ptr(), n, policy.frame,
                        policy.rel, policy.floor_energy, policy.min_run, policy.hang, policy.keep(), energy.data_ptr(), mask.data_ptr(),
                        dst.data_ptr(), new_lens.data_ptr(), info.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return res


def trim(audio, offsets, lens, policy: VadPolicy):
    """(audio', offsets', lens', VadResult): the kept frames of every utterance back to back in a new device buffer of exactly their
    size; ``offsets'`` / ``lens'`` are host int64 arrays.  One synchronisation (the new lengths are read back to size the buffer):
    trimming is a per-corpus step."""
    import torch
    from . import _lib
    res = detect(audio, offsets, lens, policy)
    n = int(res.lens.size)
    new_lens = res._tables()[1]
    new_offsets = np.concatenate([[0], np.cumsum(new_lens)[:-1]]).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    out = torch.empty(int(new_lens.sum()), dtype=torch.int16, device=audio.device)
    if n and out.numel():
        no_dev = torch.from_numpy(new_offsets).to(audio.device)
        _lib.lib().call("vm_vad_compact", audio.data_ptr(), res._offsets_dev.data_ptr(), res._lens_dev.data_ptr(), res.frame_base.data_ptr(),
                        res.mask.data_ptr(), res.dst.data_ptr(), no_dev.data_ptr(), n, policy.frame, out.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
        res._new_offsets_dev = no_dev   # (kept until the launch has run)
    return out, new_offsets, new_lens, res


def add_vad_args(parser):
    """``--vad`` and its parameters, all off by default (``policy_from_args`` makes the policy)."""
    parser.add_argument('--vad', action='store_true',
                        help='trim the pauses out of every utterance first with the energy voice activity detector '
                             '(voicemap_amd/vad.py); off by default')
    parser.add_argument('--vad-threshold-db', type=float, default=None, help='a frame is speech within this many dB of the mean energy (default 25)')
    parser.add_argument('--vad-hang', type=int, default=None, help='frames kept on either side of speech (default 10)')
    parser.add_argument('--vad-min-run', type=int, default=None, help='shortest burst of active frames that counts as speech (default 3)')
    parser.add_argument('--vad-frame-ms', type=float, default=None, help='frame length in ms (default 10)')
    return parser


def policy_from_args(args, need_device_data: bool = False) -> Optional[VadPolicy]:
    """The policy the scripts' ``--vad`` flags ask for (None without ``--vad``).  ``need_device_data``: the training scripts, where the
    detector runs on the resident corpus of ``--device-data``."""
    names = ("vad_threshold_db", "vad_hang", "vad_min_run", "vad_frame_ms")
    if not getattr(args, "vad", False):
        for name in names:
            if getattr(args, name, None) is not None:
                raise SystemExit("--%s needs --vad" % name.replace("_", "-"))
        return None
    if need_device_data and not getattr(args, "device_data", False):
        raise SystemExit("--vad needs --device-data: the detector runs on the resident training corpus")
    kw = {}
    for name, key in zip(names, ("threshold_db", "hang", "min_run", "frame_ms")):
        if getattr(args, name, None) is not None:
            kw[key] = getattr(args, name)
    try:
        return VadPolicy(**kw)
    except ValueError as e:
        raise SystemExit("--vad: %s" % e)
