"""Times multi-session PLDA speaker models (csrc/plda_enrol.hip) at train-clean-360's size, beside the euclidean speaker-model kernel
(csrc/enrol.hip) at the same shape in the same process.

  python tools/plda_models_time.py [--rows 104014] [--speakers 921] [--dim 64] [--lda-dim D] [--calls 10] [--warmup 2]

A PLDA back end is fitted on the generated rows (speaker centre + noise, as tools/enrol_time.py draws them), the rows are projected, and
vm_plda_speaker_identify (ranks, best, true scores; no score matrix) and vm_plda_speaker_trial_hist (one 4096-bin pass) run leave-one-out
over all rows against all models; then vm_speaker_identify / vm_speaker_trial_hist (euclidean) on the raw rows.  HIP events around
`calls` calls after `warmup` warm-ups.  The comparison point is the existing kernel, not a target: per (row, model, component) the PLDA
chain is a subtraction, a multiplication and an fma on three float64 operands where the euclidean one is a subtraction and an fma on two.
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=104014)
    p.add_argument("--speakers", type=int, default=921)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--lda-dim", type=int, default=None)
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    a = p.parse_args()
    N, S, E = a.rows, a.speakers, a.dim
    r = np.random.default_rng(0)
    label = np.concatenate([np.arange(S), r.integers(0, S, N - S)]).astype(np.int32)
    r.shuffle(label)
    emb = torch.as_tensor((r.normal(0, 1, (S, E))[label] + r.normal(0, 1.0, (N, E))).astype(np.float32)).cuda()
    lab = torch.as_tensor(label).cuda()
    raw = EmbeddingCache(emb, label)
    model = PL.fit_plda(raw, lda_dim=a.lda_dim)
    proj = model.project(raw)
    models = EN.enrol(proj, plda=model)
    rows = proj.emb
    keep = {}
    win_p = [EN._pass1(models, rows)]
    sums, msum, count = EN.speaker_sums(emb, lab, S, 0)
    win_e = [V.pass1_window(0.0, 24.0)]

    def plda_identify():
        keep["pid"] = EN.plda_speaker_identify(rows, lab, models.sums, models.count, models.tables, True)

    def plda_hist():
        keep["ph"] = EN.plda_speaker_trial_hist(rows, lab, models.sums, models.count, models.tables, True, win_p, 4096)

    def euc_identify():
        keep["eid"] = EN.speaker_identify(emb, lab, sums, msum, count, 0, True)

    def euc_hist():
        keep["eh"] = EN.speaker_trial_hist(emb, lab, sums, msum, count, 0, True, win_e, 4096)

    t_sums = timed(lambda: EN.speaker_sums(rows, lab, S, 0), 3, 1)
    t = {k: timed(f, a.calls, a.warmup) for k, f in (("plda_identify_ms", plda_identify), ("plda_trial_hist_ms", plda_hist),
                                                     ("euclidean_identify_ms", euc_identify), ("euclidean_trial_hist_ms", euc_hist))}
    D = model.D
    out = {"card": torch.cuda.get_device_name(0), "rows": N, "speakers": S, "dim": E, "plda_dim": D, "plda_width": model.P,
           "n_max": models.n_max, "calls": a.calls, "warmup": a.warmup, "speaker_sums_projected_ms": t_sums, **t,
           "identify_ratio": t["plda_identify_ms"] / t["euclidean_identify_ms"],
           "trial_hist_ratio": t["plda_trial_hist_ms"] / t["euclidean_trial_hist_ms"],
           "plda_f64_flops_per_s": 4.0 * N * S * D / (t["plda_identify_ms"] * 1e-3),
           "euclidean_f64_flops_per_s": 3.0 * N * S * E / (t["euclidean_identify_ms"] * 1e-3),
           "plda_rank1_accuracy": float((keep["pid"]["rank"] == 0).double().mean().item()),
           "euclidean_rank1_accuracy": float((keep["eid"]["rank"] == 0).double().mean().item()),
           "plda_hist_total": int(keep["ph"].sum().item()), "euclidean_hist_total": int(keep["eh"].sum().item())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
