"""Timing of cohort score normalisation (vm_cohort_topk_stats, vm_pair_score_hist_norm, verification_metrics(norm=)) at
train-clean-360's size: 104 014 x 64 seeded rows (921 speakers: a speaker centroid plus per-file noise), a cohort of 20 000 rows of the
same kind, AS-norm with K = 300.  Prints ONE JSON line:

* ``vm_cohort_topk_stats`` whole and on one score tile, and its per-pair rate against ``vm_pairdist_argmin``'s (argmin only, a
  13 002-row shard, the same process); the split between its scoring and selection kernels comes from a kernel trace of this tool;
* pass 1 of ``vm_pair_score_hist_norm`` against plain pass 1 of ``vm_pair_score_hist`` (one window, 4096 bins, whole triangle);
* the whole ``verification_metrics(..., norm=)`` call (host clock).

Device events around back-to-back launches after a warm-up, in several blocks: median and spread.  ``--rows N`` shrinks the set."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.verification_bench import blocks  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rows", type=int, default=104014)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--speakers", type=int, default=921)
    ap.add_argument("--cohort", type=int, default=20000)
    ap.add_argument("--top-k", type=int, default=300)
    ap.add_argument("--shard-rows", type=int, default=13002)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("score_norm_bench needs a GPU")
    from voicemap_amd import _lib, verification as V
    from voicemap_amd.retrieval import EmbeddingCache
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, E, C, K = a.rows, a.dim, a.cohort, a.top_k
    g = torch.Generator(device=dev).manual_seed(0)
    spk = np.random.default_rng(0).integers(0, a.speakers, N)
    cent = torch.randn(a.speakers, E, device=dev, generator=g)
    emb = (cent[torch.as_tensor(spk, device=dev)] + 1.5 * torch.randn(N, E, device=dev, generator=g)).contiguous()
    cspk = torch.randint(0, a.speakers, (C,), device=dev, generator=g)
    cohort = (cent[cspk] + 1.5 * torch.randn(C, E, device=dev, generator=g)).contiguous()
    cache = EmbeddingCache(emb, spk)
    lib = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    kind = V.SCORES["euclidean"]

    # cohort statistics, whole entry point
    mu, sig, rsig = (torch.empty(N, device=dev) for _ in range(3))
    cnt = torch.empty(N, dtype=torch.int32, device=dev)
    ws = lib.workspace("vm_cohort_stats_workspace_bytes", N, C, E, device=dev)
    stats = blocks(lambda: lib.call("vm_cohort_topk_stats", emb.data_ptr(), N, cohort.data_ptr(), C, E, kind, None, -1, K, mu.data_ptr(),
                                    sig.data_ptr(), rsig.data_ptr(), cnt.data_ptr(), None, ws.data_ptr(), st), a.reps, a.blocks)
    # one tile's rows (both kernels once): the split between scoring and selection comes from the kernel trace of this tool
    tile_rows = int(min(N, max(64, ((48 << 20) // C) // 64 * 64)))
    one_tile = blocks(lambda: lib.call("vm_cohort_topk_stats", emb.data_ptr(), tile_rows, cohort.data_ptr(), C, E, kind, None, -1, K,
                                       mu.data_ptr(), sig.data_ptr(), rsig.data_ptr(), cnt.data_ptr(), None, ws.data_ptr(), st),
                      a.reps, a.blocks)
    norm = V.score_norm(cache, cohort, "euclidean", top_k=K)

    # pass 1, plain and normalised
    lo, hi = V.bounds(cache, kind)
    w1 = V.sampled_window(cache, kind, None, lo, hi)
    nlo, nhi = V.norm_bounds(norm, lo, hi)
    w1n = V.sampled_window(cache, kind, None, nlo, nhi, norm=norm)
    hist = torch.zeros(1, 2, V.PASS1_BINS + 3, dtype=torch.int64, device=dev)
    wsh = lib.workspace("vm_pair_score_hist_workspace_bytes", N, E, device=dev)
    win, winn = np.array([w1], dtype=np.int64), np.array([w1n], dtype=np.int64)
    plain = blocks(lambda: lib.call("vm_pair_score_hist", emb.data_ptr(), cache.speaker_dev.data_ptr(), N, E, kind, None, 0, N, win.ctypes.data,
                                    1, V.PASS1_BINS, hist.data_ptr(), wsh.data_ptr(), st), a.reps, a.blocks)
    normed = blocks(lambda: lib.call("vm_pair_score_hist_norm", emb.data_ptr(), cache.speaker_dev.data_ptr(), N, E, kind, None, 0, N,
                                     winn.ctypes.data, 1, V.PASS1_BINS, norm.mu.data_ptr(), norm.rsig.data_ptr(), hist.data_ptr(),
                                     wsh.data_ptr(), st), a.reps, a.blocks)

    # vm_pairdist_argmin over one row shard: the per-pair yardstick
    M = min(a.shard_rows, N)
    ws2 = lib.workspace("vm_pairdist_workspace_bytes", M, N, device=dev)
    bv, bi = torch.empty(M, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    pd = blocks(lambda: lib.call("vm_pairdist_argmin", emb.data_ptr(), emb.data_ptr(), M, N, E, 0, 0, None, bv.data_ptr(), bi.data_ptr(),
                                 ws2.data_ptr(), st), a.reps, a.blocks)

    # the whole metrics call
    V.verification_metrics(cache, "euclidean", norm=norm)
    whole = []
    m = None
    for _ in range(a.blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = V.verification_metrics(cache, "euclidean", norm=norm)
        whole.append((time.perf_counter() - t0) * 1e3)
    raw = V.verification_metrics(cache, "euclidean")
    pairs = N * (N - 1) // 2
    rate_pd = M * N / (pd["median_ms"] * 1e-3)
    rate_stats = N * C / (stats["median_ms"] * 1e-3)
    out = {
        "workload": "cohort score normalisation, %d x %d fp32 rows, %d speakers, cohort %d, top_k %d, euclidean" % (N, E, a.speakers, C, K),
        "cohort_topk_stats": stats,
        "cohort_topk_stats_one_tile": dict(one_tile, rows=tile_rows),
        "gpairs_per_s_cohort_stats": rate_stats / 1e9,
        "pairdist_argmin_shard": dict(pd, rows=M),
        "gpairs_per_s_pairdist": rate_pd / 1e9,
        "rate_ratio_stats_over_pairdist": rate_stats / rate_pd,
        "pass1_plain": plain,
        "pass1_norm": normed,
        "rate_ratio_pass1_norm_over_plain": plain["median_ms"] / normed["median_ms"],
        "gpairs_per_s_pass1_norm": pairs / (normed["median_ms"] * 1e-3) / 1e9,
        "verification_metrics_norm_ms": {"median_ms": float(np.median(whole)), "min_ms": min(whole), "max_ms": max(whole),
                                         "blocks": a.blocks},
        "passes_norm": m["passes"],
        "eer_raw": raw["eer"], "eer_as_norm": m["eer"],
        "best_balanced_accuracy_raw": raw["best_balanced_accuracy"], "best_balanced_accuracy_as_norm": m["best_balanced_accuracy"],
        "device": torch.cuda.get_device_name(dev),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
