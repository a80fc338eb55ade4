"""Timing of score calibration (vm_pair_calib_sums, voicemap_amd/calibration.py) at train-clean-360's size: the 104 014 x 64 seeded rows
of tools/verification_bench.py (921 speakers, 5.41e9 pairs).  Prints ONE JSON line:

* one ``vm_pair_calib_sums`` pass over the first 13 002 rows' trials (the 13 002 x 104 014 x 64 shard of BASELINE.json config 5) and
  over the whole triangle, at a moderate (a, b, tau);
* ``vm_pair_score_hist`` pass 1 (one window, 4096 bins) over the same rows, as tools/verification_bench.py runs it, and the ratio;
* a whole ``fit_calibration`` on the whole triangle: wall time, Newton iterations and passes, the result.

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

from tools.verification_bench import blocks  # noqa: E402


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
        raise SystemExit("calibration_bench needs a GPU")
    from voicemap_amd import _lib, calibration as C, verification as V
    from voicemap_amd.retrieval import EmbeddingCache
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, E = a.rows, a.dim
    g = torch.Generator(device=dev).manual_seed(0)
    spk = np.random.default_rng(0).integers(0, a.speakers, N)
    cent = torch.randn(a.speakers, E, device=dev, generator=g)
    emb = (cent[torch.as_tensor(spk, device=dev)] + 1.5 * torch.randn(N, E, device=dev, generator=g)).contiguous()
    cache = EmbeddingCache(emb, spk)
    lib = _lib.lib()
    kind = V.SCORES["euclidean"]
    st = torch.cuda.current_stream(dev).cuda_stream
    M = min(a.shard_rows, N)
    pairs = lambda rows: V.pairs_before(rows, N)

    sums = torch.zeros(2, 8, dtype=torch.float64, device=dev)
    wsc = lib.workspace("vm_pair_calib_sums_workspace_bytes", N, E, device=dev)
    abt = (-0.5, 7.0, -2.0)   # z within a few units of 0 for these scores: no term is trivial
    calib = lambda hi: lib.call("vm_pair_calib_sums", emb.data_ptr(), cache.speaker_dev.data_ptr(), N, E, kind, None, 0, hi, None, None,
                                abt[0], abt[1], abt[2], sums.data_ptr(), wsc.data_ptr(), st)
    lo, hi = V.bounds(cache, kind)
    w1 = V.sampled_window(cache, kind, None, lo, hi)
    hist = torch.zeros(1, 2, V.PASS1_BINS + 3, dtype=torch.int64, device=dev)
    wsh = lib.workspace("vm_pair_score_hist_workspace_bytes", N, E, device=dev)
    win = np.array([w1], dtype=np.int64)
    hist1 = lambda hi: lib.call("vm_pair_score_hist", emb.data_ptr(), cache.speaker_dev.data_ptr(), N, E, kind, None, 0, hi, win.ctypes.data,
                                1, V.PASS1_BINS, hist.data_ptr(), wsh.data_ptr(), st)
    t = {"calib_shard": blocks(lambda: calib(M), a.reps, a.blocks), "hist_shard": blocks(lambda: hist1(M), a.reps, a.blocks),
         "calib_triangle": blocks(lambda: calib(N), a.reps, a.blocks), "hist_triangle": blocks(lambda: hist1(N), a.reps, a.blocks)}

    C.fit_calibration(cache, prior=0.01)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cal = C.fit_calibration(cache, prior=0.01)
    fit_ms = (time.perf_counter() - t0) * 1e3
    out = {
        "workload": "calibration sums, %d x %d fp32 rows, %d speakers, euclidean; shard = rows [0, %d): %d pairs; triangle: %d pairs"
                    % (N, E, a.speakers, M, pairs(M), pairs(N)),
        **t,
        "ratio_calib_over_hist_shard": t["calib_shard"]["median_ms"] / t["hist_shard"]["median_ms"],
        "ratio_calib_over_hist_triangle": t["calib_triangle"]["median_ms"] / t["hist_triangle"]["median_ms"],
        "gpairs_per_s_calib_shard": pairs(M) / (t["calib_shard"]["median_ms"] * 1e-3) / 1e9,
        "fit": {"wall_ms": fit_ms, "prior": 0.01, "iterations": cal.iterations, "passes": cal.passes, "converged": cal.converged, "a": cal.a,
                "b": cal.b, "objective": cal.objective, "cllr_train": cal.cllr_train},
        "device": torch.cuda.get_device_name(dev),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
