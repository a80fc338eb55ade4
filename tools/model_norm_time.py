"""Times model-trial score normalisation (csrc/enrol_norm.hip) at tools/enrol_time.py's shape (train-clean-360: 104 014 rows, 921
speakers, 64 components) with a 5 000-row cohort: one NORMALISED trial-histogram pass against the plain vm_speaker_trial_hist pass on
the same card in the same run, and the three statistics passes (query side, model side, own side) that come before it.

  python tools/model_norm_time.py [--rows 104014] [--speakers 921] [--dim 64] [--cohort 5000] [--cohort-speakers 250] [--top-k 300]
                                  [--calls 20] [--warmup 5]

Leave-one-out, euclidean.  HIP events around `calls` calls after `warmup` warm-ups, one process; the two histogram passes are timed in
alternation (plain, normalised, plain, normalised) and both orders' means are printed, so that clock drift does not favour either.
Prints one JSON line; profiles/model_norm_time.txt keeps it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from voicemap_amd import enrolment as EN  # noqa: E402
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
    p.add_argument("--cohort", type=int, default=5000)
    p.add_argument("--cohort-speakers", type=int, default=250)
    p.add_argument("--top-k", type=int, default=300)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    a = p.parse_args()
    N, S, E, C, Sc = a.rows, a.speakers, a.dim, a.cohort, a.cohort_speakers
    r = np.random.default_rng(0)
    label = np.concatenate([np.arange(S), r.integers(0, S, N - S)]).astype(np.int32)
    r.shuffle(label)
    emb = torch.as_tensor((r.normal(0, 1, (S, E))[label] + r.normal(0, 1.0, (N, E))).astype(np.float32)).cuda()
    cl = np.concatenate([np.arange(Sc), r.integers(0, Sc, C - Sc)]).astype(np.int32)
    coh = torch.as_tensor((r.normal(0, 1, (Sc, E))[cl] + r.normal(0, 1.0, (C, E))).astype(np.float32)).cuda()
    lab = torch.as_tensor(label).cuda()
    cache, cohort = EmbeddingCache(emb, label), EmbeddingCache(coh, cl)
    models, cm = EN.enrol(cache, "euclidean"), EN.enrol(cohort, "euclidean")
    sums, msum, count = models.sums, models.msum, models.count
    Kq, Ks = min(a.top_k, Sc), min(a.top_k, C)
    step = max(1, EN.LOO_CHUNK_BYTES // (8 * E))

    def own_side():
        for r0 in range(0, N, step):
            virt = EN.speaker_loo_sums(emb[r0:r0 + step], lab[r0:r0 + step], sums, msum, count, 0)
            EN.speaker_cohort_stats(coh, *virt, 0, 1, Ks)

    t_q = timed(lambda: EN.speaker_cohort_stats(emb, cm.sums, cm.msum, cm.count, 0, 0, Kq), 3, 1)
    t_s = timed(lambda: EN.speaker_cohort_stats(coh, sums, msum, count, 0, 1, Ks), 3, 1)
    t_o = timed(own_side, 2, 1)
    norm = EN.model_score_norm(models, cache, cohort, top_k=a.top_k)
    stats = norm.stats()
    win_raw, win_norm = [V.pass1_window(0.0, 24.0)], [V.pass1_window(-12.0, 12.0)]
    keep = {}

    def plain():
        keep["h"] = EN.speaker_trial_hist(emb, lab, sums, msum, count, 0, True, win_raw, 4096)

    def normed():
        keep["n"] = EN.speaker_trial_hist_norm(emb, lab, sums, msum, count, 0, True, win_norm, 4096, stats)

    t_p1, t_n1 = timed(plain, a.calls, a.warmup), timed(normed, a.calls, a.warmup)
    t_n2, t_p2 = timed(normed, a.calls, a.warmup), timed(plain, a.calls, a.warmup)
    t_p, t_n = 0.5 * (t_p1 + t_p2), 0.5 * (t_n1 + t_n2)
    out = {"card": torch.cuda.get_device_name(0), "rows": N, "speakers": S, "dim": E, "cohort_rows": C, "cohort_models": Sc,
           "top_k": a.top_k, "calls": a.calls, "warmup": a.warmup, "plain_hist_ms": t_p, "norm_hist_ms": t_n, "norm_over_plain": t_n / t_p,
           "plain_hist_ms_runs": [t_p1, t_p2], "norm_hist_ms_runs": [t_n1, t_n2], "stats_query_side_ms": t_q, "stats_model_side_ms": t_s,
           "stats_own_side_ms": t_o, "own_side_chunk_rows": step, "hist_total": int(keep["h"].sum().item()),
           "norm_hist_total": int(keep["n"].sum().item())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
