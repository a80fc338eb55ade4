"""Timing of hard-pair mining (vm_mine_pairs, voicemap_amd/mining.py) on one rank's share of train-clean-360 as BASELINE.json config 5
uses it: 13 002 anchor rows x 104 014 candidate rows x 64 components (921 speakers: a centroid plus per-file noise), k_neg = 8,
k_pos = 4, euclidean.  In the same process ``vm_pairdist_argmin`` in argmin-only mode (dist = NULL) on the same shape: the existing
kernel doing the same M x N x E score work while keeping ONE winner per row.  Prints ONE JSON line with both times and their ratio.

Timings are device events around back-to-back launches after a warm-up, in several blocks, the two kernels INTERLEAVED block by block;
the median and the spread of the blocks are reported.  ``--rows N --shard-rows M`` shrink the matrix (a rehearsal)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def block(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(ms, reps):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "blocks": len(ms), "reps": reps}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rows", type=int, default=104014)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--speakers", type=int, default=921)
    ap.add_argument("--shard-rows", type=int, default=13002)
    ap.add_argument("--k-neg", type=int, default=8)
    ap.add_argument("--k-pos", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mining_bench needs a GPU")
    from voicemap_amd import _lib
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, E, M = a.rows, a.dim, min(a.shard_rows, a.rows)
    g = torch.Generator(device=dev).manual_seed(0)
    spk = np.random.default_rng(0).integers(0, a.speakers, N)
    cent = torch.randn(a.speakers, E, device=dev, generator=g)
    emb = (cent[torch.as_tensor(spk, device=dev)] + 1.5 * torch.randn(N, E, device=dev, generator=g)).contiguous()
    label = torch.as_tensor(spk.astype(np.int32)).to(dev)
    lib = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    lo, hi = 0, M
    ws = lib.workspace("vm_mine_pairs_workspace_bytes", N, E, lo, hi, a.k_neg, a.k_pos, device=dev)
    ni, pi = (torch.empty(M, k, dtype=torch.int32, device=dev) for k in (a.k_neg, a.k_pos))
    nv, pv = (torch.empty(M, k, device=dev) for k in (a.k_neg, a.k_pos))
    ptr = lambda t, k: t.data_ptr() if k else None
    mine = lambda: lib.call("vm_mine_pairs", emb.data_ptr(), label.data_ptr(), N, E, 0, lo, hi, a.k_neg, a.k_pos, None, ptr(ni, a.k_neg),
                            ptr(nv, a.k_neg), ptr(pi, a.k_pos), ptr(pv, a.k_pos), ws.data_ptr(), st)
    ws2 = lib.workspace("vm_pairdist_workspace_bytes", M, N, device=dev)
    bv, bi = torch.empty(M, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    argmin = lambda: lib.call("vm_pairdist_argmin", emb.data_ptr(), emb.data_ptr(), M, N, E, 0, 0, None, bv.data_ptr(), bi.data_ptr(),
                              ws2.data_ptr(), st)
    for _ in range(a.warmup):
        mine()
        argmin()
    torch.cuda.synchronize()
    t_mine, t_arg = [], []
    for _ in range(a.blocks):   # interleaved: both kernels see the same state of a shared machine
        t_arg.append(block(argmin, a.reps))
        t_mine.append(block(mine, a.reps))
    # the two must agree where they answer the same question: the nearest other-speaker row is never nearer than the nearest row
    mine()
    argmin()
    torch.cuda.synchronize()
    peak = 1024 * 2.4 / 2.0   # G wave-instructions / s (fp32 VALU issue, as tools/verification_bench.py counts it)
    sm, sa = summary(t_mine, a.reps), summary(t_arg, a.reps)
    out = {
        "workload": "hard-pair mining, %d anchors x %d rows x %d, %d speakers, k_neg %d, k_pos %d, euclidean" % (M, N, E, a.speakers, a.k_neg,
                                                                                                        a.k_pos),
        "mine_pairs": sm,
        "pairdist_argmin": sa,
        "ratio_mine_over_argmin": sm["median_ms"] / sa["median_ms"],
        "gpairs_per_s_mine": M * N / (sm["median_ms"] * 1e-3) / 1e9,
        "valu_bound_ms": 2.0 * M * N * E / 64 / (peak * 1e9) * 1e3,
        "workspace_mb": ws.numel() / 2 ** 20,
        "nearest_negative_not_nearer_than_nearest_row": bool((nv[:, 0] >= bv).all().item()) if a.k_neg else None,
        "anchors_with_a_positive": float((pi[:, 0] >= 0).float().mean().item()) if a.k_pos else None,
        "device": torch.cuda.get_device_name(dev),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
