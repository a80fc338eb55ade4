"""Times the calibration pass of speaker-model trials (the CALIB mode of csrc/enrol_tile.hpp) at tools/enrol_time.py's shape
(train-clean-360: 104 014 rows, 921 speakers, 64 components): one vm_speaker_trial_calib_sums pass against one vm_speaker_trial_hist pass
over the same trials on the same card in the same run, and the same pair for multi-session PLDA at tools/plda_models_time.py's size
(D = 64, P = 68).

  python tools/model_calib_time.py [--rows 104014] [--speakers 921] [--dim 64] [--calls 20] [--warmup 5] [--hist-lib PATH]

Leave-one-out.  HIP events around `calls` calls after `warmup` warm-ups, one process; the two passes are timed in alternation (plain,
calib, calib, plain) and each pair is averaged, so that clock drift does not favour either.  --hist-lib: the histogram passes come from
another build of the library (the parent commit's, tools/build_base_variant.sh), loaded beside this one.  Prints one JSON line;
profiles/model_calib_time.txt keeps it."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from voicemap_amd import _lib  # noqa: E402
from voicemap_amd import enrolment as EN  # noqa: E402
from voicemap_amd import plda as PL  # noqa: E402
from voicemap_amd import verification as V  # noqa: E402
from voicemap_amd.retrieval import EmbeddingCache  # noqa: E402


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


class HistLib:
    """The two trial-histogram entry points of another build of the library, bound from this tree's header (they have not changed)."""

    def __init__(self, path):
        self.cdll = ctypes.CDLL(path)
        for name in ("vm_speaker_trial_hist", "vm_plda_speaker_trial_hist", "vm_speaker_trial_hist_workspace_bytes",
                     "vm_plda_speaker_trial_hist_workspace_bytes"):
            fn = getattr(self.cdll, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]

    def hist(self, q, q_label, models, windows, bins, out):
        """``enrolment._trial_hist`` (leave-one-out, no statistics) through this build; ``out`` is zeroed by the caller."""
        binding = EN._binding(q, *models.backend)
        prefix, model_args, dims = binding
        M = int(q.shape[0])
        ws = torch.empty(getattr(self.cdll, prefix + "trial_hist_workspace_bytes")(M, *dims) + 256, dtype=torch.uint8, device=q.device)
        win = np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1, 2))
        rc = getattr(self.cdll, prefix + "trial_hist")(q.data_ptr(), q_label.data_ptr(), M, *model_args, 1, win.ctypes.data, len(windows),
                                                       bins, out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=104014)
    p.add_argument("--speakers", type=int, default=921)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--hist-lib", default="", help="another build of the library for the histogram passes (default: this one)")
    a = p.parse_args()
    N, S, E = a.rows, a.speakers, a.dim
    r = np.random.default_rng(0)
    label = np.concatenate([np.arange(S), r.integers(0, S, N - S)]).astype(np.int32)
    r.shuffle(label)
    emb = torch.as_tensor((r.normal(0, 1, (S, E))[label] + r.normal(0, 1.0, (N, E))).astype(np.float32)).cuda()
    lab = torch.as_tensor(label).cuda()
    raw = EmbeddingCache(emb, label)
    geo = EN.enrol(raw, "euclidean")
    model = PL.fit_plda(raw)
    proj = model.project(raw)
    pld = EN.enrol(proj, plda=model)
    other = HistLib(a.hist_lib) if a.hist_lib else None
    out = {"card": torch.cuda.get_device_name(0), "rows": N, "speakers": S, "dim": E, "plda_dim": model.D, "plda_width": model.P,
           "calls": a.calls, "warmup": a.warmup, "hist_lib": os.path.basename(a.hist_lib) if a.hist_lib else "this build",
           "splits": int(_lib.lib().query("vm_speaker_trial_calib_sums_splits", N, S))}
    for name, models, q, win in (("euclidean", geo, emb, [V.pass1_window(0.0, 24.0)]), ("plda", pld, proj.emb, [EN._pass1(pld, proj.emb)])):
        keep = {}
        # a calibration that an evaluation would meet: the equal-variance start of the fit, from one pass at a = b = 0
        s0 = EN._trial_calib_sums(q, lab, *models.backend, True, 0.0, 0.0, 0.0).cpu().numpy()
        m0, m1 = s0[0, 6] / s0[0, 5], s0[1, 6] / s0[1, 5]
        v = 0.5 * ((s0[0, 7] / s0[0, 5] - m0 * m0) + (s0[1, 7] / s0[1, 5] - m1 * m1))
        ca, cb = float((m0 - m1) / v), float(-(m0 * m0 - m1 * m1) / (2 * v))

        def plain():
            if other is None:
                keep["h"] = EN._trial_hist(q, lab, *models.backend, True, win, 4096)
            else:
                keep["h"] = other.hist(q, lab, models, win, 4096, torch.zeros(1, 2, 4099, dtype=torch.int64, device=q.device))

        def calib():
            keep["c"] = EN._trial_calib_sums(q, lab, *models.backend, True, ca, cb, 0.0)

        t_p1, t_c1 = timed(plain, a.calls, a.warmup), timed(calib, a.calls, a.warmup)
        t_c2, t_p2 = timed(calib, a.calls, a.warmup), timed(plain, a.calls, a.warmup)
        t_p, t_c = 0.5 * (t_p1 + t_p2), 0.5 * (t_c1 + t_c2)
        c = keep["c"].cpu().numpy()
        out[name] = {"a": ca, "b": cb, "plain_hist_ms": t_p, "calib_ms": t_c, "calib_over_plain": t_c / t_p, "plain_hist_ms_runs": [t_p1, t_p2],
                     "calib_ms_runs": [t_c1, t_c2], "hist_total": int(keep["h"].sum().item()), "calib_trials": int(c[:, :2].sum()),
                     "calib_skipped": int(c[:, 1].sum()), "cllr": float((c[0, 2] / c[0, 0] + c[1, 2] / c[1, 0]) / (2 * np.log(2.0)))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
