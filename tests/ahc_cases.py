"""Cases of the agglomerative-clustering tests (tests/test_ahc_cpu.py, tests/test_gpu_ahc.py) and a FAST form of the statement
``voicemap_amd.diarization.ahc_reference`` for larger n: cached row minima and vectorised numpy, the same float32 operations in the
same order -- so it agrees with the statement bit for bit (checked on the CPU) and serves where the statement's full search per step
would take too long."""
import numpy as np

from voicemap_amd.diarization import Ahc, _keys, _thr, labels_of

KINDS = ("euclidean", "cosine", "dot_product")
LINKAGES = ("single", "complete", "average")
BIG = np.int64(1) << 40   # above every key: no partner


# ---- the fast form -------------------------------------------------------------------------------------------------------------------
def ahc_fast(D, linkage, threshold=None, target=1):
    """``ahc_reference(D, linkage, threshold, target, np.float32)`` with every row's nearest partner (the smallest (key, j) over the
    active j > k) cached, as the kernel keeps it."""
    f32 = np.float32
    D = np.array(D, dtype=f32)
    n = D.shape[0]
    iu = np.triu_indices(n, 1)
    D[iu[1], iu[0]] = D[iu]
    K = np.full((n, n), BIG, np.int64)     # keys of the upper triangle; BIG below it and in retired rows / columns
    K[iu] = _keys(D[iu], f32)
    nn_key = K.min(axis=1) if n else np.zeros(0, np.int64)
    nn_idx = K.argmin(axis=1) if n else np.zeros(0, np.int64)
    merge_a, merge_b = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    merge_h, merge_size = np.full(n, np.nan, f32), np.full(n, -1, np.int32)
    active, size, rep = np.ones(n, bool), np.ones(n, np.int64), np.arange(n)
    thr = _thr(threshold, f32)
    c, T, t = n, max(1, int(target)), 0
    with np.errstate(all="ignore"):
        while c > T:
            a = int(np.argmin(nn_key))     # the first minimum: the lowest row
            b = int(nn_idx[a])
            h = D[a, b]
            if thr is not None and not (h <= thr):
                break
            merge_a[t], merge_b[t], merge_h[t], merge_size[t] = a, b, h, size[a] + size[b]
            ks = np.flatnonzero(active)
            ks = ks[(ks != a) & (ks != b)]
            da, db = D[ks, a], D[ks, b]
            if linkage == "single":
                new = np.where(_keys(db, f32) < _keys(da, f32), db, da)
            elif linkage == "complete":
                new = np.where(_keys(db, f32) > _keys(da, f32), db, da)
            else:
                x = f32(size[a]) * da
                y = f32(size[b]) * db
                new = (x + y) / f32(size[a] + size[b])
                new[np.isnan(new)] = f32(np.nan)
            D[ks, a] = D[a, ks] = new
            kn = _keys(new, f32)
            lo, hi = ks < a, ks > a
            K[ks[lo], a] = kn[lo]
            K[a, ks[hi]] = kn[hi]
            K[b, :] = BIG
            K[:, b] = BIG
            active[b], rep[b] = False, a
            size[a] += size[b]
            # the cached minima: scan again where the partner was a or b, compare elsewhere
            hit = active & ((nn_idx == a) | (nn_idx == b)) & (np.arange(n) < b)
            hit[a] = True
            rows = np.flatnonzero(hit)
            nn_key[rows], nn_idx[rows] = K[rows].min(axis=1), K[rows].argmin(axis=1)
            sel = lo & ~hit[ks]
            rest, kr = ks[sel], kn[sel]
            better = (kr < nn_key[rest]) | ((kr == nn_key[rest]) & (a < nn_idx[rest]))
            nn_key[rest[better]], nn_idx[rest[better]] = kr[better], a
            nn_key[b] = BIG
            c, t = c - 1, t + 1
    return Ahc(merge_a, merge_b, merge_h, merge_size, labels_of(rep), c)


# ---- embeddings ------------------------------------------------------------------------------------------------------------------------
def random_points(n, E, seed):
    return np.random.RandomState(seed).randn(n, E).astype(np.float32)


def grid_points(n, E, seed, levels=3, duplicates=0.25):
    """Integer coordinates in [0, levels): many equal distances; the last ``duplicates`` share of the rows repeat earlier rows
    (distance 0) -- every decision is then made by (a, b)."""
    rng = np.random.RandomState(seed)
    x = rng.randint(0, levels, size=(n, E)).astype(np.float32)
    x[x.sum(axis=1) == 0, 0] = 1.0   # no zero row: the cosine distance of one is NaN, which is the NaN case's business
    k = int(n * duplicates)
    if k:
        x[n - k:] = x[rng.randint(0, n - k, size=k)]
    return x


def nan_points(n, E, seed, row=None):
    x = random_points(n, E, seed)
    x[n // 3 if row is None else row] = np.nan
    return x


def host_distances(x, kind):
    """A symmetric float32 distance matrix of the rows of x for the CPU tests (NOT the kernel's bits: those come from the device)."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        if kind == "euclidean":
            d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2, dtype=np.float32))
        else:
            g = (x[:, None, :] * x[None, :, :]).sum(axis=2, dtype=np.float32)
            if kind == "cosine":
                nrm = np.sqrt(np.diagonal(g)).astype(np.float32)
                d = np.float32(1.0) - g / (nrm[:, None] * nrm[None, :])
            else:
                d = -g
    d = np.triu(d, 1) + np.triu(d, 1).T
    np.fill_diagonal(d, np.nan)
    return d.astype(np.float32)


# ---- the capacity case -----------------------------------------------------------------------------------------------------------------
def gap_line(n, seed=0):
    """n points on a line (E = 1) at the cumulative sums of a permutation of the gaps 1 .. n - 1: every position (< 2^24) and every
    adjacent distance is exact in fp32 and all gaps differ, so single linkage under the euclidean distance must close the gaps in
    order of their size.  Returns (emb (n, 1) fp32, the expected merge_a, merge_b, merge_h, merge_size from a union-find)."""
    gaps = np.random.RandomState(seed).permutation(np.arange(1, n, dtype=np.int64))
    pos = np.concatenate([[0], np.cumsum(gaps)])
    assert pos[-1] < (1 << 24)
    last = np.arange(n)                        # per cluster slot (= its first point): its last point
    start_of = np.arange(n)                    # for a point that ends a cluster: that cluster's first point
    ma, mb = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    mh, ms = np.full(n, np.nan, np.float32), np.full(n, -1, np.int32)
    where = np.empty(n, np.int64)              # gap g lies between points where[g] and where[g] + 1
    where[gaps] = np.arange(n - 1)
    for t in range(n - 1):
        i = int(where[t + 1])
        a, b = int(start_of[i]), i + 1         # left cluster [a .. i], right cluster [i + 1 .. last[i + 1]]
        e = int(last[b])
        ma[t], mb[t], mh[t], ms[t] = a, b, t + 1, e - a + 1
        last[a] = e
        start_of[e] = a
    return pos.astype(np.float32).reshape(n, 1), ma, mb, mh, ms


# ---- the kernel's own distances (GPU tests) --------------------------------------------------------------------------------------------
def pairdist(rows_t, kind):
    """dist (n, n) of vm_pairdist_argmin of a block of device rows against itself, on the host."""
    import torch
    from voicemap_amd import _lib
    lib = _lib.lib()
    n, E = rows_t.shape
    dist = torch.empty(n, n, dtype=torch.float32, device=rows_t.device)
    bv, bi = torch.empty(n, dtype=torch.float32, device=rows_t.device), torch.empty(n, dtype=torch.int32, device=rows_t.device)
    ws = lib.workspace("vm_pairdist_workspace_bytes", n, n, device=rows_t.device)
    lib.call("vm_pairdist_argmin", rows_t.data_ptr(), rows_t.data_ptr(), n, n, E, _lib.DIST[kind], -1, dist.data_ptr(), bv.data_ptr(),
             bi.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dist.cpu().numpy()
