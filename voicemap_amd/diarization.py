"""Speaker diarization: who spoke when in a recording nobody has labelled (new; the reference has nothing like it).

A recording is cut into sliding windows (``sliding_windows``), every window is embedded alone (``embed_from_offsets``: windows are
offsets into the resident int16 buffer), the windows of each recording are clustered agglomeratively on the chip (``cluster``:
``vm_ahc``, voicemap_amd/csrc/cluster.hip -- one launch, one workgroup per recording, only merge lists and labels leave the chip)
and the window labels become segments (``window_segments``).  ``der`` scores a hypothesis against reference segments;
``make_conversations`` builds synthetic conversations from single-speaker files (with pauses, if asked); ``diarize`` is the whole path.
Two optional stages around the clustering: speech gating in front (``vad``: windows that are mostly pause are neither embedded nor
clustered, and no unvoiced frame carries a speaker) and Viterbi resegmentation behind (``resegment``: ``vm_reseg``,
voicemap_amd/csrc/reseg.hip -- one model per cluster, every window scored against every model, the label sequence decoded by a sticky
HMM, a few times over; ``reseg_reference`` is its numpy statement, the contract itself is in include/voicemap_hip.h).

The contract of the clustering, for ONE recording of n windows ("slots" 0 .. n - 1) and a symmetric distance matrix D (lower = more
alike), is ``ahc_reference`` -- the numpy statement every device test compares against, bit for bit:

  every slot starts as an active cluster of size 1; c = active clusters, T = max(1, target).  While c > T:
    among the active pairs a < b take the smallest by (key(D[a][b]), a, b); key = ``verification.score_keys`` with every NaN last;
    h = D[a][b]; if a threshold is given and not (h <= threshold): stop (a NaN h stops);
    record merge t = (a, b, h, size_a + size_b); for every other active k, D[k][a] = D[a][k] =
      single    the one of D[k][a], D[k][b] with the smaller key (equal keys keep D[k][a]);
      complete  the one with the larger key (equal keys keep D[k][a]);
      average   (size_a * D[k][a] + size_b * D[k][b]) / (size_a + size_b), every operation rounded on its own in the matrix's
                precision, a NaN result stored as the canonical quiet NaN;
    slot b is retired, size_a += size_b, c -= 1.
  merge lists have n entries, -1 / NaN where no merge is recorded (always the last); labels number the final clusters 0 .. c - 1 in
  ascending order of their slot (their lowest member).

What is checked: the kernel against this statement at equality, the statement against scipy's linkage in float64, ``der`` against
hand-computed cases.  NO claim about the DER of a trained model on real conversations: that has not been measured.
"""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional, Tuple

import numpy as np

MAX_N = 2048   # VM_AHC_MAX_N of include/voicemap_hip.h: a recording's matrix belongs to one workgroup
LINKAGES = ("single", "complete", "average")
SAMPLING_RATE = 16000

MAX_K = 64     # VM_RESEG_MAX_K: a decode step is one lane per model
MAX_ITERS = 16
Ahc = namedtuple("Ahc", "merge_a merge_b merge_h merge_size labels n_clusters")
Reseg = namedtuple("Reseg", "labels path_cost iters_run n_changed emis")
VBX_MAX_ITERS = 64
LOG_2PI = 1.8378770664093453   # the float64 next to log(2 pi): the constant of vm_vbx's G_t
Vbx = namedtuple("Vbx", "labels gamma pi elbo iters_run")


# ---- the contract --------------------------------------------------------------------------------------------------------------------
def _keys(x: np.ndarray, dtype) -> np.ndarray:
    """What the pair search and the single / complete updates compare: the uint32 score keys with every NaN last (float32), or the
    values themselves with a NaN taken as +inf (float64: the form that is compared with scipy)."""
    if dtype == np.float32:
        from .verification import score_keys
        return np.where(np.isnan(x), 0xFFFFFFFF, score_keys(x).astype(np.int64).reshape(x.shape))
    return np.where(np.isnan(x), np.inf, x) + 0.0


def _thr(threshold, dtype):
    return None if threshold is None or np.isnan(threshold) else dtype(threshold)


def labels_of(rep: np.ndarray) -> np.ndarray:
    """rep[k] = k for an active slot, else the (lower) slot it was merged into -> the final clusters numbered in ascending slot order."""
    n = len(rep)
    root = np.arange(n)
    for k in range(n):            # rep[k] < k for a retired slot: its root is already known
        root[k] = k if rep[k] == k else root[rep[k]]
    number = np.cumsum(rep == np.arange(n)) - 1
    return number[root].astype(np.int32)


def ahc_reference(D, linkage: str, threshold: Optional[float] = None, target: int = 1, dtype=np.float32) -> Ahc:
    """The statement of the module docstring on an (n, n) matrix, written for obviousness: a full masked search per step.  Only the
    upper triangle of ``D`` is read (the matrix is taken as symmetric).  Returns ``Ahc(merge_a, merge_b, merge_h, merge_size,
    labels, n_clusters)``."""
    if linkage not in LINKAGES:
        raise ValueError("linkage must be in %r" % (LINKAGES,))
    dtype = np.dtype(dtype).type
    D = np.array(D, dtype=dtype)
    n = D.shape[0]
    assert D.shape == (n, n)
    iu = np.triu_indices(n, 1)
    D[iu[1], iu[0]] = D[iu]
    merge_a, merge_b = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    merge_h, merge_size = np.full(n, np.nan, dtype), np.full(n, -1, np.int32)
    active, size, rep = np.ones(n, bool), np.ones(n, np.int64), np.arange(n)
    thr = _thr(threshold, dtype)
    upper = np.triu(np.ones((n, n), bool), 1)
    c, T, t = n, max(1, int(target)), 0
    with np.errstate(all="ignore"):
        while c > T:
            pairs = np.flatnonzero((upper & active[:, None] & active[None, :]).ravel())   # row-major: ascending (a, b)
            p = pairs[np.argmin(_keys(D.ravel()[pairs], dtype))]                          # the first minimum
            a, b = divmod(int(p), n)
            h = D[a, b]
            if thr is not None and not (h <= thr):
                break
            merge_a[t], merge_b[t], merge_h[t], merge_size[t] = a, b, h, size[a] + size[b]
            ks = np.flatnonzero(active)
            ks = ks[(ks != a) & (ks != b)]
            da, db = D[ks, a], D[ks, b]
            if linkage == "single":
                new = np.where(_keys(db, dtype) < _keys(da, dtype), db, da)
            elif linkage == "complete":
                new = np.where(_keys(db, dtype) > _keys(da, dtype), db, da)
            else:
                x = dtype(size[a]) * da
                y = dtype(size[b]) * db
                new = (x + y) / dtype(size[a] + size[b])
                new[np.isnan(new)] = dtype(np.nan)
            D[ks, a] = D[a, ks] = new
            active[b], rep[b] = False, a
            size[a] += size[b]
            c, t = c - 1, t + 1
    return Ahc(merge_a, merge_b, merge_h, merge_size, labels_of(rep), c)


def to_linkage(merge_a, merge_b, merge_h, merge_size, n: int) -> np.ndarray:
    """The recorded merges as scipy's ``Z`` matrix (one row per merge: the two cluster ids in ascending order, the height, the size);
    the cluster merge t creates is id n + t."""
    m = int((np.asarray(merge_a)[:n] >= 0).sum())
    ident = np.arange(n)
    Z = np.zeros((m, 4), np.float64)
    for t in range(m):
        a, b = int(merge_a[t]), int(merge_b[t])
        Z[t] = (min(ident[a], ident[b]), max(ident[a], ident[b]), merge_h[t], merge_size[t])
        ident[a] = n + t
    return Z


def cut(merge_a, merge_b, merge_h, n: int, threshold: Optional[float] = None, n_clusters: Optional[int] = None):
    """(labels, clusters) of a recorded dendrogram replayed under the stop rule of the statement: merges are taken in order while more
    than ``max(1, n_clusters)`` clusters remain and the height passes ``h <= threshold``.  On a FULL dendrogram (no threshold, target
    1) this is what a run with that threshold / target gives: the stop rule only ever cuts the merge list short."""
    merge_h = np.asarray(merge_h)
    thr = _thr(threshold, merge_h.dtype.type)
    rep = np.arange(n)
    c, T = n, max(1, int(n_clusters) if n_clusters is not None else 1)
    for t in range(n):
        if c <= T or merge_a[t] < 0 or (thr is not None and not (merge_h[t] <= thr)):
            break
        rep[merge_b[t]] = merge_a[t]
        c -= 1
    return labels_of(rep), c


# ---- the device call -------------------------------------------------------------------------------------------------------------------
class Clustering:
    """What ``cluster`` leaves on the device: ``merge_a`` / ``merge_b`` / ``merge_size`` (N,) int32 and ``merge_h`` (N,) fp32 with merge
    t of recording r at ``row0[r] + t`` (-1 / NaN where there is none), ``labels`` (N,) int32, ``n_clusters`` (R,) int32; ``row0`` is the
    host's (R + 1,) table.  ``recording(r)`` is recording r's part as numpy arrays (one read-back for all)."""

    def __init__(self, row0, merge_a, merge_b, merge_h, merge_size, labels, n_clusters, distance, linkage):
        self.row0, self.distance, self.linkage = row0, distance, linkage
        self.merge_a, self.merge_b, self.merge_h, self.merge_size = merge_a, merge_b, merge_h, merge_size
        self.labels, self.n_clusters = labels, n_clusters
        self._host = None

    def host(self) -> Ahc:
        if self._host is None:
            self._host = Ahc(*(t.cpu().numpy() for t in (self.merge_a, self.merge_b, self.merge_h, self.merge_size, self.labels,
                                                          self.n_clusters)))
        return self._host

    def recording(self, r: int) -> Ahc:
        h, lo, hi = self.host(), int(self.row0[r]), int(self.row0[r + 1])
        return Ahc(h.merge_a[lo:hi], h.merge_b[lo:hi], h.merge_h[lo:hi], h.merge_size[lo:hi], h.labels[lo:hi], int(h.n_clusters[r]))


def _row_table(row0, N: int, cap: Optional[int] = MAX_N) -> np.ndarray:
    row0 = np.ascontiguousarray(np.asarray(row0.cpu() if hasattr(row0, "cpu") else row0, dtype=np.int64).reshape(-1))
    if row0.size < 1 or row0[0] != 0 or row0[-1] != N:
        raise ValueError("row0 must run from 0 to the number of rows (%d)" % N)
    n_r = np.diff(row0)
    if n_r.size and n_r.min() < 0:
        raise ValueError("row0 must not decrease")
    if cap is not None and n_r.size and n_r.max() > cap:
        raise ValueError("recording %d holds %d windows: at most %d can be clustered" % (int(n_r.argmax()), int(n_r.max()), cap))
    return row0


def cluster(emb, row0, distance: str = "cosine", linkage: str = "average", threshold: Optional[float] = None,
            n_speakers=None) -> Clustering:
    """Cluster the windows of R recordings in one ``vm_ahc`` call.  ``emb``: (N, E) fp32 device tensor, recording r's windows at rows
    ``row0[r] .. row0[r + 1]`` (``row0``: R + 1 host values).  Merging stops at the first height that fails ``h <= threshold`` and
    when ``n_speakers`` clusters are left (an int, or one per recording); with neither, the full dendrogram is recorded (``cut``
    then gives any stop on the host).  distance="plda": the rows are PLDA-space rows (``plda.PldaModel.project``)."""
    import torch
    from . import _lib
    if distance not in _lib.PAIR_DIST:
        raise ValueError("Distance must be in (euclidean, cosine, dot_product, plda)")
    if linkage not in LINKAGES:
        raise ValueError("linkage must be in %r" % (LINKAGES,))
    if emb.dim() != 2 or emb.dtype != torch.float32:
        raise TypeError("emb must be an (N, E) fp32 tensor")
    emb = emb.contiguous()
    N, E = int(emb.shape[0]), int(emb.shape[1])
    row0 = _row_table(row0, N)
    R, dev = row0.size - 1, emb.device
    mat0 = np.concatenate([[0], np.cumsum(np.diff(row0) ** 2)]).astype(np.int64)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    res = Clustering(row0, i32(N), i32(N), torch.empty(N, dtype=torch.float32, device=dev), i32(N), i32(N),
                     torch.zeros(R, dtype=torch.int32, device=dev), distance, linkage)
    if R == 0 or N == 0:
        return res
    target = None
    if n_speakers is not None:
        t = np.broadcast_to(np.asarray(n_speakers, dtype=np.int64), (R,)) if np.ndim(n_speakers) == 0 else np.asarray(n_speakers, dtype=np.int64)
        if t.shape != (R,):
            raise ValueError("n_speakers must be one number or one per recording")
        target = torch.from_numpy(np.clip(t, 0, MAX_N).astype(np.int32)).to(dev)
    tab = torch.from_numpy(np.concatenate([row0, mat0])).to(dev)   # one upload
    lib = _lib.lib()
    ws = lib.workspace("vm_ahc_workspace_bytes", N, E, R, int(mat0[-1]), device=dev)
    lib.call("vm_ahc", emb.data_ptr(), N, E, tab.data_ptr(), tab[R + 1:].data_ptr(), R, int(mat0[-1]), _lib.PAIR_DIST[distance],
             _lib._ENUMS["VM_LINK_" + linkage.upper()], float("nan") if threshold is None else float(threshold),
             None if target is None else target.data_ptr(), res.merge_a.data_ptr(), res.merge_b.data_ptr(), res.merge_h.data_ptr(),
             res.merge_size.data_ptr(), res.labels.data_ptr(), res.n_clusters.data_ptr(), ws.data_ptr(),
             torch.cuda.current_stream(dev).cuda_stream)
    return res


# ---- resegmentation: the contract of vm_reseg and the device call ------------------------------------------------------------------
def _chain_table(chain_start, n: int) -> np.ndarray:
    start = np.zeros(n, dtype=bool)
    if chain_start is not None:
        start |= np.asarray(chain_start).reshape(-1) != 0
    if n:
        start[0] = True
    return start


def viterbi_reference(emis, chain_start, switch_cost: float) -> Tuple[np.ndarray, float]:
    """The decode of ``vm_reseg`` for ONE recording on its (n, K) fp32 emissions (lower = more alike): per chain, in float64,
    ``c[t0] = e[t0]``; then ``j* = `` the first minimum of ``c[t - 1]``, ``sw = c[t - 1][j*] + switch_cost``, ``c[t][k] = e[t][k] +
    (c[t - 1][k] if c[t - 1][k] <= sw else sw)`` (a tie stays); the chain ends in the first minimum of its last row and is traced back
    from there.  Returns (labels (n,) int32, the sum of the chains' final minima in chain order)."""
    e = np.asarray(emis, dtype=np.float32)
    n, K = e.shape
    start, sc = _chain_table(chain_start, n), np.float64(switch_cost)
    bounds = np.append(np.flatnonzero(start), n)
    labels, cost, ks = np.full(n, -1, np.int32), np.float64(0.0), np.arange(K)
    for t0, t1 in zip(bounds[:-1], bounds[1:]):
        c = e[t0].astype(np.float64)
        back = []
        for t in range(t0 + 1, t1):
            j = int(np.argmin(c))
            sw = c[j] + sc
            stay = c <= sw
            back.append(np.where(stay, ks, j))
            c = e[t].astype(np.float64) + np.where(stay, c, sw)
        k = int(np.argmin(c))
        cost = cost + c[k]
        for t in range(t1 - 1, t0 - 1, -1):
            labels[t] = k
            if t > t0:
                k = int(back[t - t0 - 1][k])
    return labels, float(cost)


def emissions_reference(emb, labels, K: int, kind) -> np.ndarray:
    """(n, K) fp32: every row of ONE recording against the models of its rows with ``labels == k`` -- the models and scores of
    ``enrolment.speaker_sums_numpy`` / ``trial_scores_numpy`` (no leave-one-out), rounded to fp32 once; +inf where the model has no row
    or the score is NaN."""
    from .enrolment import trial_scores_numpy
    emb = np.asarray(emb, dtype=np.float32)
    scores, trial = trial_scores_numpy(emb, labels, emb, np.full(len(emb), -1), kind, False, S=K)
    with np.errstate(over="ignore"):
        e = scores.astype(np.float32)
    e[~trial | np.isnan(e)] = np.inf
    return e


def reseg_reference(emb, row0, n_models, labels, chain_start, kind, switch_cost: float, iters: int) -> Reseg:
    """The numpy statement of ``vm_reseg`` (include/voicemap_hip.h).  ``emb`` (N, E), ``row0`` (R + 1,), ``n_models`` (R,), ``labels``
    (N,), ``chain_start`` (N,) or None.  Returns ``Reseg(labels (N,) int32, path_cost (R,) float64, iters_run (R,) int32, n_changed
    (R,) int32, emis (sum n_r K_r,) fp32)``; an empty recording has path_cost NaN and zeros (the device writes nothing for it but
    ``iters_run``)."""
    emb, row0 = np.asarray(emb, dtype=np.float32), np.asarray(row0, dtype=np.int64)
    labels_in, R = np.asarray(labels).astype(np.int32), len(row0) - 1
    n_models = np.broadcast_to(np.asarray(n_models, dtype=np.int64), (R,))
    if not (1 <= int(iters) <= MAX_ITERS and np.isfinite(switch_cost) and switch_cost >= 0):
        raise ValueError("iters in [1, %d], switch_cost finite and >= 0" % MAX_ITERS)
    out = np.full(len(emb), -1, np.int32)
    cost, run, chg, emis = np.full(R, np.nan), np.zeros(R, np.int32), np.zeros(R, np.int32), []
    for r in range(R):
        lo, hi, K = int(row0[r]), int(row0[r + 1]), int(n_models[r])
        if hi == lo:
            continue
        if not 1 <= K <= MAX_K:
            raise ValueError("recording %d has %d models: 1 .. %d can be decoded" % (r, K, MAX_K))
        x, lab = emb[lo:hi], labels_in[lo:hi]
        cs = None if chain_start is None else np.asarray(chain_start)[lo:hi]
        e = emissions_reference(x, lab, K, kind)
        if not ((lab >= 0) & (lab < K)).any():   # no model at all
            emis.append(e.ravel())
            continue
        for it in range(1, int(iters) + 1):
            if it > 1:
                e = emissions_reference(x, lab, K, kind)
            new, cost[r] = viterbi_reference(e, cs, switch_cost)
            run[r], chg[r] = it, int((new != lab).sum())
            lab = new
            if chg[r] == 0:
                break
        out[lo:hi] = lab
        emis.append(e.ravel())
    return Reseg(out, cost, run, chg, np.concatenate(emis).astype(np.float32) if emis else np.zeros(0, np.float32))


class Resegmentation:
    """What ``resegment`` leaves on the device: ``labels`` (N,) int32, ``path_cost`` (R,) float64, ``iters_run`` / ``n_changed`` (R,)
    int32, ``emis`` (sum n_r K_r,) fp32 with recording r's (n_r, K_r) matrix at ``em0[r]``; ``row0`` / ``em0`` / ``n_models`` are the
    host's tables.  ``host()`` is all of it as numpy arrays (one read-back), ``recording(r)`` recording r's part."""

    def __init__(self, row0, em0, n_models, labels, path_cost, iters_run, n_changed, emis, distance, switch_cost, iters):
        self.row0, self.em0, self.n_models = row0, em0, n_models
        self.labels, self.path_cost, self.iters_run, self.n_changed, self.emis = labels, path_cost, iters_run, n_changed, emis
        self.distance, self.switch_cost, self.iters = distance, switch_cost, iters
        self._host = None

    def host(self) -> Reseg:
        if self._host is None:
            self._host = Reseg(*(t.cpu().numpy() for t in (self.labels, self.path_cost, self.iters_run, self.n_changed, self.emis)))
        return self._host

    def recording(self, r: int) -> Reseg:
        h, lo, hi, K = self.host(), int(self.row0[r]), int(self.row0[r + 1]), int(self.n_models[r])
        return Reseg(h.labels[lo:hi], float(h.path_cost[r]), int(h.iters_run[r]), int(h.n_changed[r]),
                     h.emis[int(self.em0[r]):int(self.em0[r + 1])].reshape(hi - lo, K) if hi > lo else np.zeros((0, K), np.float32))


class ResegPolicy:
    """How ``diarize`` resegments: the cost of a speaker change (in units of the distance), the number of model / decode rounds, and
    -- optionally -- a finer hop at which the windows are cut, embedded and decoded while the clustering keeps the coarse one."""

    def __init__(self, switch_cost: float, iters: int = 3, hop_seconds: Optional[float] = None):
        self.switch_cost, self.iters, self.hop_seconds = float(switch_cost), int(iters), None if hop_seconds is None else float(hop_seconds)
        _check_decode(self.switch_cost, self.iters)
        if self.hop_seconds is not None and not self.hop_seconds > 0:
            raise ValueError("hop_seconds must be positive")


def _check_decode(switch_cost, iters):
    if not (np.isfinite(switch_cost) and switch_cost >= 0):
        raise ValueError("switch_cost must be finite and >= 0")
    if not 1 <= iters <= MAX_ITERS:
        raise ValueError("iters must be in [1, %d]" % MAX_ITERS)


def resegment(emb, row0, labels, n_models, chain_start=None, distance: str = "cosine", switch_cost: float = 0.5, iters: int = 3,
              return_emis: bool = True) -> Resegmentation:
    """Resegment the windows of R recordings in one ``vm_reseg`` call.  ``emb``: (N, E) fp32 device tensor, recording r's windows IN TIME
    ORDER at rows ``row0[r] .. row0[r + 1]``; ``labels`` (N,): the model (cluster) of every row within its recording, -1 for a row that
    belongs to none yet; ``n_models``: one count or one per recording, 1 .. 64 wherever the recording has rows; ``chain_start`` (N,),
    optional: non-zero where a row must not be tied to the row before it (a gap in time).  Any number of windows per recording.
    distance="plda" is refused: the models are means of rows, and the mean of PLDA-space rows is not a PLDA-space row."""
    import torch
    from . import _lib
    if distance == "plda":
        raise ValueError('resegment: distance="plda" is refused: a model is the mean of its rows, and the mean of PLDA-space rows is not '
                         "a PLDA-space row (their last column is quadratic in the row)")
    if distance not in _lib.DIST:
        raise ValueError("Distance must be in (euclidean, cosine, dot_product)")
    _check_decode(float(switch_cost), int(iters))
    if emb.dim() != 2 or emb.dtype != torch.float32:
        raise TypeError("emb must be an (N, E) fp32 tensor")
    emb = emb.contiguous()
    N, E, dev = int(emb.shape[0]), int(emb.shape[1]), emb.device
    row0 = _row_table(row0, N, cap=None)
    R, n_r = row0.size - 1, np.diff(row0)
    K = np.asarray(n_models.cpu() if hasattr(n_models, "cpu") else n_models, dtype=np.int64)
    K = np.broadcast_to(K, (R,)).copy() if K.ndim == 0 else K.reshape(-1)
    if K.shape != (R,):
        raise ValueError("n_models must be one number or one per recording")
    bad = np.flatnonzero((n_r > 0) & ((K < 1) | (K > MAX_K)))
    if bad.size:
        raise ValueError("recording %d has %d models: 1 .. %d can be decoded" % (int(bad[0]), int(K[bad[0]]), MAX_K))
    K = np.where(n_r > 0, K, 0)

    def rows(t, name):
        t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t).reshape(-1)))
        if t.numel() != N:
            raise ValueError("%s must hold one value per row of emb (%d), not %d" % (name, N, t.numel()))
        return t.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    lab = rows(labels, "labels")
    cs = None if chain_start is None else rows(chain_start, "chain_start")
    em0 = np.concatenate([[0], np.cumsum(n_r * K)]).astype(np.int64)
    total = int(em0[-1])
    res = Resegmentation(row0, em0, K, torch.full((N,), -1, dtype=torch.int32, device=dev),
                         torch.full((R,), float("nan"), dtype=torch.float64, device=dev), torch.zeros(R, dtype=torch.int32, device=dev),
                         torch.zeros(R, dtype=torch.int32, device=dev),
                         torch.empty(total if return_emis else 0, dtype=torch.float32, device=dev), distance, float(switch_cost), int(iters))
    if R == 0 or N == 0:
        return res
    tab = torch.from_numpy(np.concatenate([row0, em0])).to(dev)   # one upload
    km = torch.from_numpy(K.astype(np.int32)).to(dev)
    lib = _lib.lib()
    ws = lib.workspace("vm_reseg_workspace_bytes", N, E, R, total, device=dev)
    lib.call("vm_reseg", emb.data_ptr(), N, E, tab.data_ptr(), tab[R + 1:].data_ptr(), R, total, km.data_ptr(), lab.data_ptr(),
             None if cs is None else cs.data_ptr(), _lib.DIST[distance], float(switch_cost), int(iters), res.labels.data_ptr(),
             res.path_cost.data_ptr(), res.iters_run.data_ptr(), res.n_changed.data_ptr(), res.emis.data_ptr() if return_emis else None,
             ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return res


# ---- VBx: the contract of vm_vbx and the device call ---------------------------------------------------------------------------------
def vbx_tables(plda_model) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(psi, r, ib) of a fitted ``plda.PldaModel`` for ``vm_vbx``, on the columns w = sqrt(b) z, b = psi / (1 + 2 psi), of its PLDA-space
    rows: r = sqrt(psi / b) = sqrt(1 + 2 psi), so that rho = r w = sqrt(psi) z; ib = 1 / b, so that |z|^2 = sum ib w^2."""
    psi = np.ascontiguousarray(np.asarray(plda_model.psi, dtype=np.float64).reshape(-1))
    return psi, np.sqrt(1.0 + 2.0 * psi), (1.0 + 2.0 * psi) / psi


def _vbx_sum(v, stages):
    """SUM_k of vm_vbx: the butterfly over the next power of two, which is what one lane per speaker of a wave adds."""
    if len(stages) == 0:
        return v[0]
    x = np.zeros(len(stages[0]), v.dtype)
    x[:len(v)] = v
    for partner in stages:
        x = x + x[partner]
    return x[0]


def _check_vbx(loop_prob, fa, fb, init_smooth, iters, epsilon):
    if not 0.0 <= loop_prob < 1.0:
        raise ValueError("loop_prob must be in [0, 1)")
    if not (np.isfinite(fa) and fa > 0 and np.isfinite(fb) and fb > 0):
        raise ValueError("fa and fb must be finite and > 0")
    if not (np.isfinite(init_smooth) and init_smooth >= 0):
        raise ValueError("init_smooth must be finite and >= 0")
    if not 1 <= int(iters) <= VBX_MAX_ITERS:
        raise ValueError("iters must be in [1, %d]" % VBX_MAX_ITERS)
    if np.isnan(epsilon):
        raise ValueError("epsilon must not be NaN")


def vbx_reference(rows, row0, n_models, labels, chain_start, psi, loop_prob, fa, fb, init_smooth, iters, epsilon, gamma=None, pi=None,
                  dtype=np.float64) -> Vbx:
    """The numpy statement of ``vm_vbx`` (include/voicemap_hip.h), in the scaled form and with the sums in the order stated there; every
    operation is rounded on its own where the kernel has an fma.  ``rows`` (N, P) PLDA-space rows of which the columns 0 .. D - 1, D =
    len(psi), are read; ``psi`` alone, or the triple (psi, r, ib) when the tables are not ``vbx_tables``'.  ``gamma`` (sum n_r K_r,) /
    ``pi`` (R, 64): a warm start.  ``dtype=np.longdouble`` runs the same statement in extended precision (the inputs are the same
    float64 / fp32 numbers).  Returns ``Vbx(labels (N,) int32, gamma (sum n_r K_r,), pi (R, 64), elbo (R, iters), iters_run (R,)
    int32)``; an empty recording leaves zeros / NaN."""
    T = np.dtype(dtype).type
    if isinstance(psi, (tuple, list)):
        psi, rr, ib = (np.asarray(v, dtype=np.float64).reshape(-1) for v in psi)
    else:
        psi = np.asarray(psi, dtype=np.float64).reshape(-1)
        rr, ib = np.sqrt(1.0 + 2.0 * psi), (1.0 + 2.0 * psi) / psi
    D = len(psi)
    psi, rr, ib = psi.astype(T), rr.astype(T), ib.astype(T)
    rows, row0 = np.asarray(rows, dtype=np.float32), np.asarray(row0, dtype=np.int64)
    labels_in, R, iters = np.asarray(labels).astype(np.int32), len(row0) - 1, int(iters)
    n_models = np.broadcast_to(np.asarray(n_models, dtype=np.int64), (R,))
    _check_vbx(loop_prob, fa, fb, init_smooth, iters, epsilon)
    n_r = np.diff(row0)
    em0 = np.concatenate([[0], np.cumsum(n_r * np.where(n_r > 0, n_models, 0))]).astype(np.int64)
    out_lab, out_gamma = np.full(len(rows), -1, np.int32), np.zeros(int(em0[-1]), T)
    out_pi, out_elbo, run = np.zeros((R, MAX_K), T), np.full((R, iters), np.nan, T), np.zeros(R, np.int32)
    lam0, fa_, fb_, one, half_ = T(loop_prob), T(fa), T(fb), T(1.0), T(0.5)
    Fr, q0 = fa_ / fb_, T(np.exp(-np.float64(init_smooth)))
    for r in range(R):
        lo, hi, K = int(row0[r]), int(row0[r + 1]), int(n_models[r])
        n = hi - lo
        if n == 0:
            continue
        if not 1 <= K <= MAX_K:
            raise ValueError("recording %d has %d speakers: 1 .. %d can be modelled" % (r, K, MAX_K))
        w = rows[lo:hi, :D].astype(T)
        lab = labels_in[lo:hi]
        start = _chain_table(None if chain_start is None else np.asarray(chain_start)[lo:hi], n)
        lam = np.where(start, T(0.0), lam0).astype(T)
        Kp = 1
        while Kp < K:
            Kp *= 2
        stages, o = [], 1
        while o < Kp:
            stages.append(np.arange(Kp) ^ o)
            o *= 2
        if gamma is not None:
            g = np.asarray(gamma).reshape(-1)[int(em0[r]):int(em0[r + 1])].astype(T).reshape(n, K)
        else:
            den = one + T(K - 1) * q0
            g = np.where(lab[:, None] == np.arange(K)[None, :], one / den, q0 / den).astype(T)
            g[(lab < 0) | (lab >= K)] = one / T(K)
        pk = np.asarray(pi)[r, :K].astype(T) if pi is not None else np.full(K, one / T(K), T)
        rho = rr[None, :] * w
        acc = np.zeros(n, T)
        for d in range(D):
            acc = ib[d] * (w[:, d] * w[:, d]) + acc
        G = T(-0.5) * (acc + T(np.float64(D) * LOG_2PI))
        out_pi[r, :K] = pk
        labels_now, prev = None, T(0.0)
        for it in range(1, iters + 1):
            # speaker posteriors
            Nk, F = np.zeros(K, T), np.zeros((K, D), T)
            for t in range(n):
                Nk = Nk + g[t]
                F = g[t][:, None] * rho[t][None, :] + F
            invL = one / (one + (Fr * Nk)[:, None] * psi[None, :])
            alpha = (Fr * invL) * F
            q, ent = np.zeros(K, T), np.zeros(K, T)
            for d in range(D):
                a2 = alpha[:, d] * alpha[:, d]
                q = (invL[:, d] + a2) * psi[d] + q
                ent = ent + (((np.log(invL[:, d]) - invL[:, d]) - a2) + one)
            # emissions
            dot = np.zeros((n, K), T)
            for d in range(D):
                dot = rho[:, d][:, None] * alpha[:, d][None, :] + dot
            lp = fa_ * ((dot - half_ * q[None, :]) + G[:, None])
            m = lp.max(axis=1)
            p = np.exp(lp - m[:, None])
            # forward
            a, c, ap = np.zeros((n, K), T), np.zeros(n, T), np.zeros(K, T)
            ok = True
            for t in range(n):
                at = p[t] * (lam[t] * ap + (one - lam[t]) * pk)
                ct = _vbx_sum(at, stages)
                if not (ct > 0 and np.isfinite(ct)):
                    ok = False
                    break
                ap = at / ct
                a[t], c[t] = ap, ct
            if not ok:
                run[r], labels_now = -2, lab
                break
            # backward
            b = np.ones((n, K), T)
            for t in range(n - 2, -1, -1):
                pb = p[t + 1] * b[t + 1]
                s = _vbx_sum(pk * pb, stages)
                b[t] = (lam[t + 1] * pb + (one - lam[t + 1]) * s) / c[t + 1]
            g = a * b
            labels_now = g.argmax(axis=1).astype(np.int32)
            # priors, bound, stop
            pin, lpx = np.zeros(K, T), T(0.0)
            for t in range(n):
                pin = pin + ((((one - lam[t]) * pk) * p[t]) * b[t]) / c[t]
                lpx = lpx + (np.log(c[t]) + m[t])
            tot, es = T(0.0), T(0.0)
            for k in range(K):
                tot, es = tot + pin[k], es + ent[k]
            pk = pin / tot
            e = lpx + (fb_ * half_) * es
            out_elbo[r, it - 1], run[r] = e, it
            out_pi[r, :K] = pk
            if it > 1 and e - prev < epsilon:
                break
            prev = e
        out_lab[lo:hi] = labels_now
        out_gamma[int(em0[r]):int(em0[r + 1])] = g.ravel()
    return Vbx(out_lab, out_gamma, out_pi, out_elbo, run)


class VbxResult:
    """What ``vbx`` leaves on the device: ``labels`` (N,) int32, ``gamma`` (sum n_r K_r,) float64 with recording r's (n_r, K_r)
    posteriors at ``em0[r]``, ``pi`` (R, 64) float64, ``elbo`` (R, iters) float64 (NaN past ``iters_run``), ``iters_run`` (R,) int32;
    ``row0`` / ``em0`` / ``n_models`` are the host's tables.  ``host()`` is all of it as numpy arrays (one read-back), ``recording(r)``
    recording r's part."""

    def __init__(self, row0, em0, n_models, labels, gamma, pi, elbo, iters_run):
        self.row0, self.em0, self.n_models = row0, em0, n_models
        self.labels, self.gamma, self.pi, self.elbo, self.iters_run = labels, gamma, pi, elbo, iters_run
        self._host = None

    def host(self) -> Vbx:
        if self._host is None:
            self._host = Vbx(*(t.cpu().numpy() for t in (self.labels, self.gamma, self.pi, self.elbo, self.iters_run)))
        return self._host

    def recording(self, r: int) -> Vbx:
        h, lo, hi, K = self.host(), int(self.row0[r]), int(self.row0[r + 1]), int(self.n_models[r])
        return Vbx(h.labels[lo:hi], h.gamma[int(self.em0[r]):int(self.em0[r + 1])].reshape(hi - lo, K) if hi > lo
                   else np.zeros((0, K), np.float64), h.pi[r, :K], h.elbo[r], int(h.iters_run[r]))


class VbxPolicy:
    """How ``diarize`` runs VBx behind the clustering: the loop probability, the acoustic and speaker-regularisation factors fa / fb,
    the smoothing of the initial posteriors, the iteration cap and the ELBO gain below which a recording stops (the defaults are the
    VBx paper's), and -- optionally -- a finer hop at which the windows are cut, embedded and modelled while the clustering keeps the
    coarse one."""

    def __init__(self, loop_prob: float = 0.99, fa: float = 0.3, fb: float = 17.0, init_smooth: float = 5.0, iters: int = 20,
                 epsilon: float = 1e-4, hop_seconds: Optional[float] = None):
        self.loop_prob, self.fa, self.fb, self.init_smooth = float(loop_prob), float(fa), float(fb), float(init_smooth)
        self.iters, self.epsilon, self.hop_seconds = int(iters), float(epsilon), None if hop_seconds is None else float(hop_seconds)
        _check_vbx(self.loop_prob, self.fa, self.fb, self.init_smooth, self.iters, self.epsilon)
        if self.hop_seconds is not None and not self.hop_seconds > 0:
            raise ValueError("hop_seconds must be positive")


def vbx(rows, row0, labels, n_models, plda, chain_start=None, loop_prob: float = 0.99, fa: float = 0.3, fb: float = 17.0,
        init_smooth: float = 5.0, iters: int = 20, epsilon: float = 1e-4, gamma=None, pi=None) -> VbxResult:
    """VBx over the windows of R recordings in one ``vm_vbx`` call.  ``rows``: (N, P) fp32 device tensor of PLDA-space rows
    (``plda.project``), recording r's windows IN TIME ORDER at rows ``row0[r] .. row0[r + 1]``; ``labels`` (N,): the speaker (cluster)
    every row starts in, -1 for a row of none; ``n_models``: one count or one per recording, 1 .. 64 wherever the recording has rows;
    ``plda``: the fitted ``plda.PldaModel`` the rows were projected by (or the tables (psi, r, ib) themselves); ``chain_start`` (N,),
    optional: non-zero where a row must not be tied to the row before it.  ``gamma`` (sum n_r K_r,) / ``pi`` (R, 64) float64: a warm
    start in place of the labels / of uniform priors.  Any number of windows per recording."""
    import torch
    from . import _lib
    _check_vbx(float(loop_prob), float(fa), float(fb), float(init_smooth), int(iters), float(epsilon))
    if rows.dim() != 2 or rows.dtype != torch.float32:
        raise TypeError("rows must be an (N, P) fp32 tensor")
    rows = rows.contiguous()
    N, P, dev = int(rows.shape[0]), int(rows.shape[1]), rows.device
    tabs = vbx_tables(plda) if hasattr(plda, "psi") else tuple(np.asarray(v, dtype=np.float64).reshape(-1) for v in plda)
    D = len(tabs[0])
    if len(tabs) != 3 or any(len(v) != D for v in tabs) or not 1 <= D <= min(P, 255):
        raise ValueError("the tables psi, r, ib hold one value per column read: 1 .. min(P, 255) of them, not %d" % D)
    if not all(np.isfinite(v).all() for v in tabs):
        raise ValueError("the tables psi, r, ib must be finite")
    row0 = _row_table(row0, N, cap=None)
    R, n_r = row0.size - 1, np.diff(row0)
    K = np.asarray(n_models.cpu() if hasattr(n_models, "cpu") else n_models, dtype=np.int64)
    K = np.broadcast_to(K, (R,)).copy() if K.ndim == 0 else K.reshape(-1)
    if K.shape != (R,):
        raise ValueError("n_models must be one number or one per recording")
    bad = np.flatnonzero((n_r > 0) & ((K < 1) | (K > MAX_K)))
    if bad.size:
        raise ValueError("recording %d has %d speakers: 1 .. %d can be modelled" % (int(bad[0]), int(K[bad[0]]), MAX_K))
    K = np.where(n_r > 0, K, 0)

    def per_row(t, name):
        t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t).reshape(-1)))
        if t.numel() != N:
            raise ValueError("%s must hold one value per row (%d), not %d" % (name, N, t.numel()))
        return t.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()

    def f64(t, count, name):
        t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float64)))
        if t.numel() != count:
            raise ValueError("%s must hold %d values, not %d" % (name, count, t.numel()))
        return t.reshape(-1).to(device=dev, dtype=torch.float64).contiguous()
    lab = per_row(labels, "labels")
    cs = None if chain_start is None else per_row(chain_start, "chain_start")
    em0 = np.concatenate([[0], np.cumsum(n_r * K)]).astype(np.int64)
    total = int(em0[-1])
    g_in = None if gamma is None else f64(gamma, total, "gamma")
    pi_in = None if pi is None else f64(pi, R * MAX_K, "pi")
    res = VbxResult(row0, em0, K, torch.full((N,), -1, dtype=torch.int32, device=dev),
                    torch.zeros(total, dtype=torch.float64, device=dev), torch.zeros((R, MAX_K), dtype=torch.float64, device=dev),
                    torch.full((R, int(iters)), float("nan"), dtype=torch.float64, device=dev),
                    torch.zeros(R, dtype=torch.int32, device=dev))
    if R == 0 or N == 0:
        return res
    tab = torch.from_numpy(np.concatenate([row0, em0])).to(dev)   # one upload
    mod = torch.from_numpy(np.concatenate(tabs)).to(dev)
    km = torch.from_numpy(K.astype(np.int32)).to(dev)
    lib = _lib.lib()
    ws = lib.workspace("vm_vbx_workspace_bytes", N, D, R, total, device=dev)
    lib.call("vm_vbx", rows.data_ptr(), N, P, D, tab.data_ptr(), tab[R + 1:].data_ptr(), R, total, km.data_ptr(), lab.data_ptr(),
             None if cs is None else cs.data_ptr(), mod.data_ptr(), mod[D:].data_ptr(), mod[2 * D:].data_ptr(), float(loop_prob), float(fa),
             float(fb), float(init_smooth), float(epsilon), int(iters), None if g_in is None else g_in.data_ptr(),
             None if pi_in is None else pi_in.data_ptr(), res.labels.data_ptr(), res.gamma.data_ptr(), res.pi.data_ptr(),
             res.elbo.data_ptr(), res.iters_run.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return res


_run_vbx = vbx   # diarize's own argument is called vbx too


# ---- windows and segments ------------------------------------------------------------------------------------------------------------
def sliding_windows(lens, window: int, hop: int) -> List[np.ndarray]:
    """Per recording the start offsets 0, hop, 2 hop, ... of every window of ``window`` samples that fits, plus one last window flush
    with the end when those leave a tail uncovered.  A recording shorter than ``window`` raises ``ValueError`` naming it."""
    window, hop = int(window), int(hop)
    if window < 1 or hop < 1:
        raise ValueError("window and hop must be at least one sample")
    out = []
    for r, n in enumerate(np.asarray(lens, dtype=np.int64).reshape(-1)):
        n = int(n)
        if n < window:
            raise ValueError("recording %d holds %d samples: shorter than the window of %d" % (r, n, window))
        starts = np.arange(0, n - window + 1, hop, dtype=np.int64)
        if starts[-1] + window < n:
            starts = np.append(starts, n - window)
        out.append(starts)
    return out


def window_segments(starts, window: int, length: int, labels) -> np.ndarray:
    """Window labels -> hypothesis segments, (k, 3) int64 rows (start, end, label) that tile [0, length).  Sample s takes the label
    of the window whose centre ``start + window / 2`` is nearest, a tie going to the earlier window: the boundary between two
    consecutive windows is the midpoint of their centres, the sample ON it staying with the earlier one.  Neighbouring pieces with
    one label are joined.  ``starts`` ascending."""
    starts, labels = np.asarray(starts, dtype=np.int64).reshape(-1), np.asarray(labels).reshape(-1)
    if starts.size == 0 or starts.size != labels.size:
        raise ValueError("one label per window, at least one window")
    if np.any(np.diff(starts) <= 0):
        raise ValueError("starts must ascend")
    # s <= (c_i + c_j) / 2 with c = start + window / 2  <=>  s <= floor((start_i + start_j + window) / 2)
    first = np.clip((starts[:-1] + starts[1:] + int(window)) // 2 + 1, 0, int(length))
    edges = np.concatenate([[0], first, [int(length)]])
    segs = []
    for i, lab in enumerate(labels):
        b, e = int(edges[i]), int(edges[i + 1])
        if e <= b:
            continue
        if segs and segs[-1][2] == int(lab) and segs[-1][1] == b:
            segs[-1][1] = e
        else:
            segs.append([b, e, int(lab)])
    return np.array(segs, dtype=np.int64).reshape(-1, 3)


def lattice_windows(lens, window: int, hop: int, fine_hop: int) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """The windows of ``sliding_windows(lens, window, fine_hop)`` and, per recording, which of them ``sliding_windows(lens, window,
    hop)`` holds too: the ones on the coarse lattice plus the window flush with the end.  ``hop`` must be a multiple of ``fine_hop``
    (the coarse windows are then all among the fine ones)."""
    hop, fine_hop = int(hop), int(fine_hop)
    if fine_hop < 1 or hop % fine_hop:
        raise ValueError("the hop (%d samples) must be a multiple of the resegmentation hop (%d samples)" % (hop, fine_hop))
    fine, coarse = sliding_windows(lens, window, fine_hop), sliding_windows(lens, window, hop)
    return fine, [np.isin(f, c) for f, c in zip(fine, coarse)]


def voiced_share(mask, frame: int, starts, window: int) -> np.ndarray:
    """Per window [start, start + window) of ONE recording the share of its frames that ``mask`` (one value per frame of ``frame``
    samples, non-zero = voiced) keeps; a window's frames are those it overlaps, ``start // frame .. (start + window - 1) // frame``."""
    mask, starts = np.asarray(mask).reshape(-1) != 0, np.asarray(starts, dtype=np.int64).reshape(-1)
    cum = np.concatenate([[0], np.cumsum(mask)])
    first, last = starts // int(frame), np.minimum((starts + int(window) - 1) // int(frame), len(mask) - 1)
    return (cum[last + 1] - cum[first]) / np.maximum(last + 1 - first, 1)


def chain_starts(kept) -> np.ndarray:
    """For the kept windows of ONE recording (``kept``: one bool per window, in time order) 1 where a chain starts: at the first kept
    window and at every kept window with a dropped one between it and the kept window before."""
    idx = np.flatnonzero(np.asarray(kept, dtype=bool))
    return np.concatenate([[1], (np.diff(idx) > 1).astype(np.int32)]).astype(np.int32) if idx.size else np.zeros(0, np.int32)


def cut_to_voiced(segments, mask, frame: int, length: int) -> np.ndarray:
    """``segments`` ((k, 3) rows of start, end, label) cut to the voiced frames of ``mask``: every piece of a segment that lies in a run
    of voiced frames is kept, nothing else -- an unvoiced frame carries no speaker.  Frame f covers the samples ``f frame .. min((f +
    1) frame, length)``."""
    seg = np.asarray(segments, dtype=np.int64).reshape(-1, 3)
    edge = np.diff(np.concatenate([[0], (np.asarray(mask).reshape(-1) != 0).astype(np.int8), [0]]))
    lo = np.minimum(np.flatnonzero(edge == 1) * int(frame), int(length))
    hi = np.minimum(np.flatnonzero(edge == -1) * int(frame), int(length))
    out = [(max(b, a), min(e, z), lab) for b, e, lab in seg for a, z in zip(lo, hi) if max(b, a) < min(e, z)]
    return np.array(out, dtype=np.int64).reshape(-1, 3)


# ---- scoring ---------------------------------------------------------------------------------------------------------------------------
def assign_max(weights) -> np.ndarray:
    """The one-to-one mapping of rows to columns that maximises the mapped weight: ``col[i]`` for every row, -1 for a row left out
    (more rows than columns).  The O(n^3) shortest-augmenting-path form of the Hungarian method on ``max - weights``; integer weights
    are solved exactly."""
    W = np.asarray(weights)
    if W.ndim != 2:
        raise ValueError("a weight matrix")
    if W.shape[0] > W.shape[1]:   # rows <= columns below
        col_of = assign_max(W.T)
        out = np.full(W.shape[0], -1, np.int64)
        out[col_of[col_of >= 0]] = np.flatnonzero(col_of >= 0)
        return out
    n, m = W.shape
    if n == 0:
        return np.zeros(0, np.int64)
    C = (W.max() - W).astype(np.int64 if np.issubdtype(W.dtype, np.integer) else np.float64)
    inf = np.iinfo(np.int64).max // 4 if C.dtype == np.int64 else np.inf
    u, v = np.zeros(n + 1, C.dtype), np.zeros(m + 1, C.dtype)
    p, way = np.zeros(m + 1, np.int64), np.zeros(m + 1, np.int64)   # p[j]: the row (1-based) matched to column j
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = np.full(m + 1, inf, C.dtype), np.zeros(m + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used[1:]
            cur = C[i0 - 1] - u[i0] - v[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    out = np.full(n, -1, np.int64)
    for j in range(1, m + 1):
        if p[j]:
            out[p[j] - 1] = j - 1
    return out


def _seg_table(segments) -> np.ndarray:
    s = np.asarray(segments, dtype=np.int64).reshape(-1, 3)
    if np.any(s[:, 1] < s[:, 0]):
        raise ValueError("a segment ends before it starts")
    return s[s[:, 1] > s[:, 0]]


def der(reference_segments, hypothesis_segments) -> dict:
    """Diarization error between two segment tables ((k, 3) rows of start, end, label; samples, end exclusive), sample-exact, no
    collar.  Per sample with R reference speakers and H hypothesis clusters active: ``missed`` += max(0, R - H), ``false_alarm`` +=
    max(0, H - R), ``confusion`` += min(R, H) - (reference speakers whose mapped cluster is active), ``total`` += R.  The mapping is the
    one-to-one assignment of speakers to clusters with the largest mapped overlap (``assign_max`` on the overlap matrix in samples).
    ``der`` = (missed + false_alarm + confusion) / total (NaN when the reference is empty).  Segments of one table may overlap."""
    ref, hyp = _seg_table(reference_segments), _seg_table(hypothesis_segments)
    spk, ri = np.unique(ref[:, 2], return_inverse=True)
    clu, hi = np.unique(hyp[:, 2], return_inverse=True)
    cuts = np.unique(np.concatenate([ref[:, :2].ravel(), hyp[:, :2].ravel()]))
    dur = np.diff(cuts)
    K = len(dur)
    RA, HA = np.zeros((K, len(spk)), np.int64), np.zeros((K, len(clu)), np.int64)
    for tab, idx, act in ((ref, ri.reshape(-1), RA), (hyp, hi.reshape(-1), HA)):
        lo, hi_ = np.searchsorted(cuts, tab[:, 0]), np.searchsorted(cuts, tab[:, 1])
        for k in range(len(tab)):
            act[lo[k]:hi_[k], idx[k]] = 1
    overlap = (RA * dur[:, None]).T @ HA if K else np.zeros((len(spk), len(clu)), np.int64)
    mapping = assign_max(overlap) if overlap.size else np.full(len(spk), -1, np.int64)
    nr, nh = RA.sum(axis=1), HA.sum(axis=1)
    correct = np.zeros(K, np.int64)
    for i, j in enumerate(mapping):
        if j >= 0:
            correct += RA[:, i] * HA[:, j]
    missed = int((np.maximum(nr - nh, 0) * dur).sum())
    false_alarm = int((np.maximum(nh - nr, 0) * dur).sum())
    confusion = int(((np.minimum(nr, nh) - correct) * dur).sum())
    total = int((nr * dur).sum())
    return {"missed": missed, "false_alarm": false_alarm, "confusion": confusion, "total": total,
            "der": (missed + false_alarm + confusion) / total if total else float("nan"),
            "mapping": {int(spk[i]): int(clu[j]) for i, j in enumerate(mapping) if j >= 0}}


# ---- synthetic conversations -----------------------------------------------------------------------------------------------------------
class Conversations:
    """``audio``: the int16 buffer of all conversations back to back (a device tensor when the corpus is resident, else what
    ``to('cuda')`` uploads); ``offsets`` / ``lens`` (n,) int64; ``segments``: per conversation the reference table (turns, 3) of (start,
    end, speaker code), samples relative to the conversation; ``speakers``: per conversation the number of speakers present; ``turns``:
    per conversation the (file, start, length) of every turn; ``pauses``: per conversation the samples of silence in front of every turn."""

    def __init__(self, audio, offsets, lens, segments, turns, pauses=None):
        self.audio, self.offsets, self.lens, self.segments, self.turns = audio, offsets, lens, segments, turns
        self.pauses = pauses if pauses is not None else [[0] * len(t) for t in turns]
        self.speakers = np.array([len(np.unique(s[:, 2])) for s in segments], dtype=np.int64)

    def __len__(self):
        return len(self.lens)


def make_conversations(dataset, n: int, speakers: Tuple[int, int] = (2, 4), turns: Tuple[int, int] = (6, 12),
                       turn_seconds: Tuple[float, float] = (1.0, 6.0), seed: int = 0, pause_seconds: Tuple[float, float] = (0.0, 0.0),
                       pause_prob: float = 0.0) -> Conversations:
    """``n`` synthetic conversations from the single-speaker files of ``dataset``.  Per conversation: a speaker count in ``speakers`` and
    a turn count in ``turns`` (both inclusive) are drawn, that many distinct speakers, then per turn a speaker that is not the previous
    turn's, one of its files, a length in ``turn_seconds`` clamped to the file, and a crop position.  Turns follow each other without
    overlap; at the defaults also without pause, so the reference segments tile the conversation.  With ``pause_prob`` > 0 every turn
    but the first is, with that probability, preceded by digital silence (zeros) of a length drawn in ``pause_seconds``: the segments
    then leave gaps.  (At ``pause_prob`` = 0 no extra number is drawn: the conversations are the same as without the option.)  The
    draws come from this function's own
    ``numpy.random.Generator(seed)``: the dataset's stream (``np.random``) is not touched.  On a resident corpus
    (``dataset.device_audio``) the buffer is assembled on the device from slices; otherwise in numpy, and uploaded."""
    rng = np.random.default_rng(seed)
    code = np.asarray(dataset._code).astype(np.int64)
    length = np.asarray(getattr(dataset, "file_length", None) if getattr(dataset, "file_length", None) is not None
                        else dataset.df["length"].values, dtype=np.int64)
    files_of = [np.flatnonzero(code == s) for s in range(int(code.max()) + 1)]
    have = np.array([s for s, f in enumerate(files_of) if len(f)])
    if speakers[0] < 2 or speakers[1] < speakers[0] or speakers[1] > len(have):
        raise ValueError("speakers must be a range within 2 .. %d (the dataset's speakers)" % len(have))
    if turns[0] < 1 or turns[1] < turns[0] or not 0 < turn_seconds[0] <= turn_seconds[1]:
        raise ValueError("bad turn count or turn length range")
    if not (0.0 <= pause_prob <= 1.0 and 0.0 <= pause_seconds[0] <= pause_seconds[1]):
        raise ValueError("bad pause probability or pause length range")
    plan, segments, lens, pauses = [], [], [], []
    for _ in range(int(n)):
        cast = rng.choice(have, size=int(rng.integers(speakers[0], speakers[1] + 1)), replace=False)
        prev, pos, seg, turn, gaps = -1, 0, [], [], []
        for _ in range(int(rng.integers(turns[0], turns[1] + 1))):
            gap = 0
            if pause_prob > 0.0 and turn and rng.random() < pause_prob:
                gap = int(round(rng.uniform(pause_seconds[0], pause_seconds[1]) * SAMPLING_RATE))
            gaps.append(gap)
            pos += gap
            who = int(rng.choice(cast[cast != prev]))
            f = int(rng.choice(files_of[who]))
            want = int(round(rng.uniform(turn_seconds[0], turn_seconds[1]) * SAMPLING_RATE))
            take = max(1, min(want, int(length[f])))
            start = int(rng.integers(0, int(length[f]) - take + 1))
            turn.append((f, start, take))
            seg.append((pos, pos + take, who))
            pos, prev = pos + take, who
        plan.append(turn)
        pauses.append(gaps)
        segments.append(np.array(seg, dtype=np.int64))
        lens.append(pos)
    lens = np.array(lens, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
    import torch
    dev_audio = getattr(dataset, "device_audio", None)
    if dev_audio is not None:
        go = dataset.global_offset
        parts = [dev_audio[int(go[f]) + s:int(go[f]) + s + k] for turn in plan for f, s, k in turn]
        if pause_prob > 0.0:
            silence = torch.zeros(max([g for gaps in pauses for g in gaps] + [0]), dtype=torch.int16, device=dev_audio.device)
            parts = [x for gap, part in zip((g for gaps in pauses for g in gaps), parts) for x in (silence[:gap], part)]
        audio = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int16, device=dev_audio.device)
    else:
        from .shards import to_int16
        cache = {}

        def pcm(f):
            if f not in cache:
                cache[f] = np.asarray(dataset._pcm(f)) if hasattr(dataset, "_pcm") else to_int16(dataset._load(f))
            return cache[f]
        parts = [pcm(f)[s:s + k] for turn in plan for f, s, k in turn]
        if pause_prob > 0.0:
            parts = [x for gap, part in zip((g for gaps in pauses for g in gaps), parts) for x in (np.zeros(gap, np.int16), part)]
        host = np.concatenate(parts).astype(np.int16) if parts else np.zeros(0, np.int16)
        audio = torch.from_numpy(host)
        if torch.cuda.is_available():
            audio = audio.to("cuda")
    return Conversations(audio, offsets, lens, segments, plan, pauses)


# ---- the whole path --------------------------------------------------------------------------------------------------------------------
def diarize(model, audio, offsets, lens, preprocessor, window_seconds: float, hop_seconds: float, network_type: str = "siamese",
            distance: str = "cosine", linkage: str = "average", threshold: Optional[float] = None, n_speakers=None, batch: int = 256,
            plda=None, vad=None, min_voiced: float = 0.5, reseg: Optional[ResegPolicy] = None, vbx: Optional[VbxPolicy] = None):
    """Diarize the recordings ``audio[offsets[r] : offsets[r] + lens[r]]`` of a resident int16 buffer: sliding windows, every window
    embedded alone (``embed_from_offsets(..., windows_per_tower=1)``, ``batch`` windows per call), ``cluster``, ``window_segments``.
    Returns (segments per recording, the ``Clustering``); the clustering also carries ``emb`` (N, E), ``starts`` (per recording, relative
    to it) and ``window``.  An engine without resident input raises what ``require_resident_input`` raises.  distance="plda" needs
    ``plda``, a fitted ``plda.PldaModel``: the windows' embeddings are projected by it and clustered on minus the log-likelihood ratio;
    the clustering then also carries the projected rows as ``rows``.

    ``vad``: a ``vad.VadPolicy``.  One ``vad.detect`` call marks the frames of all recordings and the mask is read back once.  A window
    whose ``voiced_share`` is below ``min_voiced`` is neither embedded nor clustered; the hypothesis segments are cut to the voiced
    frames (``cut_to_voiced``); a recording left without a clustered window gets no segments.  (The detector keeps a recording it finds
    no speech in whole: that is its fallback, and the mask read back says so.)
    ``reseg``: a ``ResegPolicy``.  The cluster labels are resegmented (``resegment``, ``n_models`` = the clustering's ``n_clusters``, a
    chain break wherever gating dropped a window) and the segments are made from the decoded labels.  With ``reseg.hop_seconds`` = h
    (``hop_seconds`` a multiple of it) the windows are cut and embedded at hop h, the ones ``lattice_windows`` marks are clustered as
    without it, and every other row enters the decode with label -1.  distance="plda" is refused with ``reseg``.
    ``vbx``: a ``VbxPolicy``; needs distance="plda" and is refused together with ``reseg``.  The cluster labels start a VBx run on the
    projected rows (``vbx``: ``vm_vbx``, ``n_models`` = the clustering's ``n_clusters``, so the clustering should stop early: VBx drops
    speakers, it does not add any) over the same fine-hop lattice and chain breaks as ``reseg``, rows that were not clustered entering
    with label -1; the segments are made from its labels, and the clustering carries the ``VbxResult`` as ``vbx``.
    With either, the clustering also carries ``window_row0`` (the row table of ``emb``; ``row0`` is that of the clustered rows),
    ``kept`` (per recording, one bool per window of the lattice: embedded or not), ``clustered`` (per recording, one bool per embedded
    window), ``chain_start``, ``vad`` (the ``VadResult``), ``voiced`` (per recording, its frames' mask as read back) and ``reseg`` (the
    ``Resegmentation``); ``starts`` are the embedded windows'.
    With none of them, the calls and the results are what they were without the options."""
    import torch
    from .engine_core import require_resident_input
    from .retrieval import _encoder_engine
    if (distance == "plda") != (plda is not None):
        raise ValueError('distance="plda" and a fitted ``plda`` model come together')
    eng = _encoder_engine(model, network_type)
    require_resident_input(type(eng))
    inst = preprocessor.instance_preprocessor if hasattr(preprocessor, "instance_preprocessor") else preprocessor
    probe = inst(np.zeros((1, 8, 1)))
    if not hasattr(probe, "raw"):
        raise ValueError("diarize needs a preprocessor that decimates and whitens on the device (utils.preprocess_instances)")
    ds, wh = probe.downsampling, probe.whitening
    offsets = np.asarray(offsets.cpu() if hasattr(offsets, "cpu") else offsets, dtype=np.int64).reshape(-1)
    lens = np.asarray(lens.cpu() if hasattr(lens, "cpu") else lens, dtype=np.int64).reshape(-1)
    if offsets.size != lens.size:
        raise ValueError("offsets and lens differ in length")
    if lens.size and (offsets.min() < 0 or int((offsets + lens).max()) > audio.numel()):
        raise ValueError("a recording lies outside the audio buffer")
    window, hop = int(round(window_seconds * SAMPLING_RATE)), int(round(hop_seconds * SAMPLING_RATE))
    fine_hop = hop
    if reseg is not None:
        if distance == "plda":
            raise ValueError('diarize: reseg is refused with distance="plda": the mean of PLDA-space rows is not a PLDA-space row')
        if reseg.hop_seconds is not None:
            fine_hop = int(round(reseg.hop_seconds * SAMPLING_RATE))
    vbx_policy = vbx
    if vbx_policy is not None:
        if reseg is not None:
            raise ValueError("diarize: vbx and reseg are two resegmentations: one of them")
        if distance != "plda":
            raise ValueError('diarize: vbx needs distance="plda": its speaker models live in the PLDA space')
        if vbx_policy.hop_seconds is not None:
            fine_hop = int(round(vbx_policy.hop_seconds * SAMPLING_RATE))
    if not 0.0 <= min_voiced <= 1.0:
        raise ValueError("min_voiced is a share of a window's frames, in [0, 1]")
    R = len(lens)
    lattice, coarse = lattice_windows(lens, window, hop, fine_hop)
    kept, det, masks = [np.ones(len(s), dtype=bool) for s in lattice], None, None
    if vad is not None:
        from .vad import detect
        det = detect(audio, offsets, lens, vad)
        mask, fb = det.mask.cpu().numpy(), det.frame_base_host   # the one read-back
        masks = [mask[fb[r]:fb[r + 1]] for r in range(R)]
        for r in range(R):
            kept[r] = voiced_share(masks[r], vad.frame, lattice[r], window) >= min_voiced
            if not (kept[r] & coarse[r]).any():   # nothing to cluster: nothing to decode against either
                kept[r][:] = False
    starts, coarse = [s[k] for s, k in zip(lattice, kept)], [c[k] for c, k in zip(coarse, kept)]
    row0 = np.concatenate([[0], np.cumsum([len(s) for s in starts])]).astype(np.int64)
    crow0 = np.concatenate([[0], np.cumsum([int(c.sum()) for c in coarse])]).astype(np.int64)
    _row_table(crow0, int(crow0[-1]))   # a recording with too many windows fails before anything is embedded
    flat = np.concatenate([o + s for o, s in zip(offsets, starts)]) if len(starts) else np.zeros(0, np.int64)
    emb = torch.empty(len(flat), eng.E, dtype=torch.float32, device=eng.device)
    for b0 in range(0, len(flat), batch):
        offs = torch.as_tensor(flat[b0:b0 + batch])
        emb[b0:b0 + len(offs)].copy_(eng.embed_from_offsets(audio, offs, window, ds, wh, windows_per_tower=1))
    rows = plda.project(emb) if plda is not None else emb
    pick = None   # the clustered rows among the embedded ones, where they are not all of them
    if int(crow0[-1]) != len(flat):
        pick = torch.from_numpy(np.flatnonzero(np.concatenate(coarse))).to(emb.device)
    res = cluster(rows if pick is None else rows[pick], crow0, distance, linkage, threshold, n_speakers)
    res.emb, res.rows, res.starts, res.window = emb, rows, starts, window
    res.window_row0, res.kept, res.clustered, res.vad, res.voiced, res.reseg = row0, kept, coarse, det, masks, None
    res.vbx = None
    res.chain_start = np.concatenate([chain_starts(k) for k in kept]) if vad is not None and R else None
    if reseg is None and vbx_policy is None:
        labels = res.host().labels
    else:
        lab_in = res.labels
        if pick is not None:
            lab_in = torch.full((len(flat),), -1, dtype=torch.int32, device=emb.device)
            lab_in[pick] = res.labels
        if reseg is not None:
            res.reseg = resegment(emb, row0, lab_in, res.host().n_clusters, res.chain_start, distance, reseg.switch_cost, reseg.iters)
            labels = res.reseg.host().labels
        else:
            v = vbx_policy
            res.vbx = _run_vbx(rows, row0, lab_in, res.host().n_clusters, plda, res.chain_start, v.loop_prob, v.fa, v.fb,
                               v.init_smooth, v.iters, v.epsilon)
            labels = res.vbx.host().labels
    segments = []
    for r in range(R):
        seg = np.zeros((0, 3), np.int64)
        if row0[r + 1] > row0[r]:
            seg = window_segments(starts[r], window, int(lens[r]), labels[row0[r]:row0[r + 1]])
        segments.append(seg if masks is None else cut_to_voiced(seg, masks[r], vad.frame, int(lens[r])))
    return segments, res
