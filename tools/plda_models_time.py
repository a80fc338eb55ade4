"""Times multi-session PLDA speaker models (csrc/plda_enrol.hip) at train-clean-360's size, beside the euclidean speaker-model kernel
(csrc/enrol.hip) at the same shape in the same process.

  python tools/plda_models_time.py [--rows 104014] [--speakers 921] [--dim 64] [--lda-dim D] [--calls 10] [--warmup 2]

A PLDA back end is fitted on the generated rows (speaker centre + noise, as tools/enrol_time.py draws them), the rows are projected, and
vm_plda_speaker_identify (ranks, best, true scores; no score matrix) and vm_plda_speaker_trial_hist (one 4096-bin pass) run leave-one-out
over all rows against all models; then vm_speaker_identify / vm_speaker_trial_hist (euclidean) on the raw rows.  HIP events around
`calls` calls after `warmup` warm-ups.  The comparison point is the existing kernel, not a target: per (row, model, component) the PLDA
chain is a subtraction, a multiplication and an fma on three float64 operands where the euclidean one is a subtraction and an fma on two.
Prints one JSON line.

  python tools/plda_models_time.py --other-lib PATH [--blocks 8] [--calls 10] [--out profiles/NAME.txt]

compares this build with another build of libvoicemap_hip.so (the parent commit's, tools/build_base_variant.sh) loaded beside it in the
same process, at the same shape: vm_speaker_identify and one 4096-bin vm_speaker_trial_hist pass for euclidean, cosine and dot_product,
vm_plda_speaker_identify / _trial_hist, and one _trial_hist_norm pass for euclidean and PLDA (constant finite statistics: only time and
equality are read).  Per entry point the builds are timed in alternating blocks of `calls` calls between device events -- other, this,
this, other, ... -- `blocks` blocks each; the outputs of the two builds (histograms; rank, true_score, best_val, best_idx) are
compared as bytes and must be equal.  Reports the median per build, the other build's own spread over its blocks (max - min) / median,
and whether this build's median stays within that spread of the other's.  Nothing here is a threshold for a test."""
import argparse
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


def same_bytes(x, y):
    if isinstance(x, dict):
        return all(same_bytes(x[k], y[k]) for k in ("rank", "true_score", "best_val", "best_idx"))
    return torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def compare_builds(a, raw, models, emb, rows, lab):
    builds = {"other": _lib.load(a.other_lib), "this": _lib.lib()}
    M, S = int(emb.shape[0]), models.S
    const = lambda n, v: torch.full((n,), v, dtype=torch.float32, device=emb.device)
    stats = (const(M, 1.0), const(M, 0.5), const(S, 2.0), const(S, 0.25), const(M, 1.5), const(M, 0.75))
    entries = []
    for name, m, q in [(d, EN.enrol(raw, distance=d), emb) for d in ("euclidean", "cosine", "dot_product")] + [("plda", models, rows)]:
        win = [EN._pass1(m, q)]
        entries.append((name + " identify", lambda m=m, q=q: EN._identify(q, lab, *m.backend, True)))
        entries.append((name + " trial_hist", lambda m=m, q=q, win=win: EN._trial_hist(q, lab, *m.backend, True, win, 4096)))
        if name in ("euclidean", "plda"):
            wn = [EN._pass1(m, q, stats=stats)]
            entries.append((name + " trial_hist_norm", lambda m=m, q=q, wn=wn: EN._trial_hist(q, lab, *m.backend, True, wn, 4096, stats)))
    lines = ["card: %s; %d rows x %d, %d speakers, leave-one-out; plda D = %d, P = %d; %d blocks of %d calls per build after %d warm-up calls"
             % (torch.cuda.get_device_name(0), M, int(emb.shape[1]), S, models.plda.D, models.plda.P, a.blocks, a.calls, a.warmup),
             "%-28s %12s %12s %9s %14s %9s  %s" % ("", "other med ms", "this med ms", "this/other", "other spread", "outputs", "verdict")]
    ok_all = True
    for name, fn in entries:
        ts, out = {"other": [], "this": []}, {}
        for b in range(a.blocks):
            for which in (("other", "this") if b % 2 == 0 else ("this", "other")):
                _lib.use(builds[which])
                if b == 0:
                    for _ in range(a.warmup):
                        fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.calls):
                    out[which] = fn()
                e1.record()
                torch.cuda.synchronize()
                ts[which].append(e0.elapsed_time(e1) / a.calls)
        _lib.use(builds["this"])
        mo, mt = float(np.median(ts["other"])), float(np.median(ts["this"]))
        spread = (max(ts["other"]) - min(ts["other"])) / mo
        same = same_bytes(out["other"], out["this"])
        within = mt <= mo * (1.0 + spread)
        ok_all = ok_all and same and within
        lines.append("%-28s %12.4f %12.4f %9.4f %13.2f%% %9s  %s" % (name, mo, mt, mt / mo, 100 * spread, "equal" if same else "DIFFER",
                                                                     "within" if within else "SLOWER"))
    lines.append("all outputs equal and every median within the other build's spread: %s" % ("yes" if ok_all else "NO"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok_all else 1


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=104014)
    p.add_argument("--speakers", type=int, default=921)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--lda-dim", type=int, default=None)
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--other-lib", default="")
    p.add_argument("--blocks", type=int, default=8)
    p.add_argument("--out", default="")
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

    if a.other_lib:
        return compare_builds(a, raw, models, emb, rows, lab)
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
    sys.exit(main())
