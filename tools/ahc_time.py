"""Times vm_ahc (csrc/cluster.hip) on a batch of recordings beside the host's hierarchical clustering of the same distance matrices.

  python tools/ahc_time.py [--recordings 256] [--windows 800] [--dim 64] [--repeats 10] [--warmup 2] [--out profiles/ahc_time.txt]

The batch: `recordings` recordings of `windows` windows each, embeddings of width `dim` drawn around 2 to 4 seeded centres per recording
(speaker-like blobs with noise of the centres' own scale, so merges happen at every level).  Cosine distance, average linkage, no
threshold and no target: the full dendrogram of every recording.  Rows:
  vm_ahc                 whole calls (the preparation launches, the distance launch, the merge launch) between HIP events, one call per
                         timing, after warm-ups: median and spread
  vm_ahc, nothing merges the same call with target = n_r for every recording: the preparation and distance launches, and a merge launch
                         whose workgroups find c <= T at once, never read their matrix and only write the fills and labels -- the
                         distance launch alone, to within that launch's few microseconds
  host                   scipy.cluster.hierarchy.linkage(method="average") on the condensed form of each of the same matrices (read back
                         from the workspace of the second call), one thread, wall clock around the linkage calls alone; without scipy,
                         the fast numpy form of tests/ahc_cases.py on the first 16 matrices.  The file names which one ran.
Nothing here is a threshold: the file records what was seen."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from voicemap_amd import _lib  # noqa: E402


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def batch(R, n, E, seed=0):
    r = np.random.RandomState(seed)
    out = np.empty((R, n, E), np.float32)
    for k in range(R):
        centres = r.randn(int(r.randint(2, 5)), E)
        out[k] = centres[r.randint(0, len(centres), n)] + r.randn(n, E)
    return out.reshape(R * n, E)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--recordings", type=int, default=256)
    p.add_argument("--windows", type=int, default=800)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert torch.cuda.is_available(), "ahc_time.py measures on the GPU"
    lib = _lib.lib()
    R, n, E = a.recordings, a.windows, a.dim
    N, sq = R * n, R * n * n
    emb = torch.from_numpy(batch(R, n, E)).cuda()
    tab = torch.from_numpy(np.concatenate([np.arange(R + 1) * n, np.arange(R + 1) * n * n]).astype(np.int64)).cuda()
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device="cuda")
    ma, mb, ms, lab, nc = i32(N), i32(N), i32(N), i32(N), i32(R)
    mh = torch.empty(N, dtype=torch.float32, device="cuda")
    keep = torch.full((R,), n, dtype=torch.int32, device="cuda")
    ws = lib.workspace("vm_ahc_workspace_bytes", N, E, R, sq, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(target):
        lib.call("vm_ahc", emb.data_ptr(), N, E, tab.data_ptr(), tab[R + 1:].data_ptr(), R, sq, _lib.DIST["cosine"],
                 _lib._ENUMS["VM_LINK_AVERAGE"], float("nan"), target, ma.data_ptr(), mb.data_ptr(), mh.data_ptr(), ms.data_ptr(),
                 lab.data_ptr(), nc.data_ptr(), ws.data_ptr(), st)

    full = timed(lambda: call(None), a.repeats, a.warmup)
    assert int(nc.min().item()) == int(nc.max().item()) == 1
    heights = mh.view(R, n)[:, :n - 1].double()
    dist = timed(lambda: call(keep.data_ptr()), a.repeats, a.warmup)
    assert int(nc.min().item()) == n
    torch.cuda.synchronize()
    D = ws[:sq * 4].view(torch.float32).view(R, n, n).cpu().numpy()
    try:
        from scipy.cluster.hierarchy import linkage
        from scipy.spatial.distance import squareform
        cond = [squareform(np.where(np.eye(n, dtype=bool), 0.0, d).astype(np.float64), checks=False) for d in D]
        t0 = time.perf_counter()
        Z = [linkage(c, method="average") for c in cond]
        host_s, host_n, host_name = time.perf_counter() - t0, R, "scipy.cluster.hierarchy.linkage(method='average'), one thread"
        # the two dendrograms agree where fp32 and fp64 can: the top heights of the first recording
        top = (float(heights[0].max().item()), float(Z[0][-1, 2]))
    except ImportError:
        from tests.ahc_cases import ahc_fast
        host_n = min(R, 16)
        t0 = time.perf_counter()
        Z = [ahc_fast(d, "average") for d in D[:host_n]]
        host_s, host_name = time.perf_counter() - t0, "the fast numpy form of tests/ahc_cases.py (scipy is not installed), first %d matrices" % host_n
        top = (float(heights[0].max().item()), float(np.nanmax(Z[0].merge_h)))
    lines = ["card: %s; %d recordings x %d windows x E = %d (%d rows, %.0f MB of matrices), cosine, average linkage, full dendrogram; "
             "%d repeats after %d warm-ups" % (torch.cuda.get_device_name(0), R, n, E, N, sq * 4 / 1e6, a.repeats, a.warmup),
             "%-40s %12s %12s %12s %16s" % ("", "median ms", "min ms", "max ms", "us / recording"),
             "%-40s %12.3f %12.3f %12.3f %16.1f" % (("vm_ahc",) + full + (full[0] * 1e3 / R,)),
             "%-40s %12.3f %12.3f %12.3f %16.1f" % (("vm_ahc, nothing merges (distances)",) + dist + (dist[0] * 1e3 / R,)),
             "host: %s: %.3f s for %d matrices, %.2f ms / recording" % (host_name, host_s, host_n, host_s * 1e3 / host_n),
             "last merge height of recording 0: device %.6f, host %.6f" % top]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
