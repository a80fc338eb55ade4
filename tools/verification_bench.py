"""Timing of all-pairs verification (vm_pair_score_hist, voicemap_amd/verification.py) at train-clean-360's size: 104 014 x 64 seeded
rows (921 speakers: a speaker centroid plus per-file noise, so that the trials separate the way a trained encoder's do), 5.41e9 pairs.
Prints ONE JSON line:

* the pass-1 histogram over the whole triangle (one window, 4096 bins), each zoom pass of ``verification_metrics`` and the whole call;
* ``vm_pairdist_argmin`` in argmin-only mode over a 13 002-row shard in the same process (bench.py --full's config-5 comparison) and the
  per-pair rate ratio of the two;
* the fraction of the fp32 VALU issue bound, counted as bench.py counts it: 2 x pairs x E / 64 wave instructions against
  1024 SIMDs x 2.4 GHz / 2 clocks.

Timings are device events around back-to-back launches after a warm-up, in several blocks; the median and the spread of the blocks are
reported.  ``--rows N`` shrinks the matrix (a rehearsal)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def blocks(fn, reps, n_blocks, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return {"median_ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out)), "blocks": n_blocks, "reps": reps}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rows", type=int, default=104014)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--speakers", type=int, default=921)
    ap.add_argument("--shard-rows", type=int, default=13002)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("verification_bench needs a GPU")
    from voicemap_amd import _lib, verification as V
    from voicemap_amd.retrieval import EmbeddingCache
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, E = a.rows, a.dim
    g = torch.Generator(device=dev).manual_seed(0)
    spk = np.random.default_rng(0).integers(0, a.speakers, N)
    cent = torch.randn(a.speakers, E, device=dev, generator=g)
    emb = (cent[torch.as_tensor(spk, device=dev)] + 1.5 * torch.randn(N, E, device=dev, generator=g)).contiguous()
    cache = EmbeddingCache(emb, spk)
    pairs = N * (N - 1) // 2
    lib = _lib.lib()
    kind = V.SCORES["euclidean"]
    lo, hi = V.bounds(cache, kind)
    w1 = V.sampled_window(cache, kind, None, lo, hi)

    # the whole call, with its zoom passes recorded
    passes = []

    def hist_fn(wins, bins):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h = V.histogram(cache, kind, None, wins, bins)
        e1.record()
        e1.synchronize()
        passes.append({"windows": len(wins), "bins": bins, "ms": e0.elapsed_time(e1)})
        return h

    V.exact_sweep(hist_fn, w1)   # warm-up
    passes.clear()
    t0 = time.perf_counter()
    m = V.exact_sweep(hist_fn, w1)
    t_metrics = time.perf_counter() - t0
    whole = []
    for _ in range(a.blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        V.verification_metrics(cache, "euclidean")
        whole.append((time.perf_counter() - t0) * 1e3)

    # pass 1 alone, device-timed
    hist = torch.zeros(1, 2, V.PASS1_BINS + 3, dtype=torch.int64, device=dev)
    ws = lib.workspace("vm_pair_score_hist_workspace_bytes", N, E, device=dev)
    win = np.array([w1], dtype=np.int64)
    st = torch.cuda.current_stream(dev).cuda_stream
    p1 = blocks(lambda: lib.call("vm_pair_score_hist", emb.data_ptr(), cache.speaker_dev.data_ptr(), N, E, kind, None, 0, N, win.ctypes.data, 1,
                                 V.PASS1_BINS, hist.data_ptr(), ws.data_ptr(), st), a.reps, a.blocks)

    # vm_pairdist_argmin, argmin only, over one 1/8 row shard: bench.py --full's config-5 figure
    M = min(a.shard_rows, N)
    ws2 = lib.workspace("vm_pairdist_workspace_bytes", M, N, device=dev)
    bv, bi = torch.empty(M, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    pd = blocks(lambda: lib.call("vm_pairdist_argmin", emb.data_ptr(), emb.data_ptr(), M, N, E, 0, 0, None, bv.data_ptr(), bi.data_ptr(),
                                 ws2.data_ptr(), st), a.reps, a.blocks)
    rate_hist = pairs / (p1["median_ms"] * 1e-3)
    rate_pd = M * N / (pd["median_ms"] * 1e-3)
    peak = 1024 * 2.4 / 2.0   # G wave-instructions / s
    out = {
        "workload": "all-pairs verification, %d x %d fp32 rows, %d speakers, %d pairs, euclidean" % (N, E, a.speakers, pairs),
        "pass1_hist": p1,
        "zoom_passes_ms": [q["ms"] for q in passes[1:]],
        "zoom_passes": passes[1:],
        "verification_metrics_ms": {"median_ms": float(np.median(whole)), "min_ms": min(whole), "max_ms": max(whole), "blocks": a.blocks,
                                    "first_timed_ms": t_metrics * 1e3},
        "passes": m["passes"],
        "pairdist_argmin_shard": dict(pd, rows=M),
        "gpairs_per_s_hist": rate_hist / 1e9,
        "gpairs_per_s_pairdist": rate_pd / 1e9,
        "rate_ratio_hist_over_pairdist": rate_hist / rate_pd,
        "valu_bound_frac_pass1": (2.0 * pairs * E / 64 / (p1["median_ms"] * 1e-3) / 1e9) / peak,
        "valu_bound_ms_pass1": 2.0 * pairs * E / 64 / (peak * 1e9) * 1e3,
        "metrics": {k: m[k] for k in ("eer", "eer_threshold", "best_balanced_accuracy", "best_threshold", "auc", "auc_bound", "n_target",
                                      "n_nontarget", "n_nan")},
        "device": torch.cuda.get_device_name(dev),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
