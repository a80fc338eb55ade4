"""All-pairs speaker verification over a cached embedding matrix: EER, ROC and a decision threshold.

The reference planned this (experiments/verification_accuracy.py: "determines the best verification distance threshold on the
validation set and then ... uses this to estimate the true verification accuracy on the test set") and never wrote it.  The trials are
all unordered pairs {i, j}, i < j, of the rows of a ``retrieval.EmbeddingCache``; a pair is a target if both rows have the same speaker.
A score is lower for more alike rows and a pair is accepted as "same" iff s < t:

* FRR(t) = #{targets, s >= t} / n_target, FAR(t) = #{non-targets, s < t} / n_nontarget; t runs over the distinct finite scores and
  +inf; NaN scores are counted apart and left out of both rates;
* EER = (FAR + FRR) / 2 at t* = argmin |FAR - FRR| (smallest t on ties); best balanced accuracy = max 1 - (FAR + FRR) / 2 (smallest t
  that reaches it) -- the expected accuracy on the reference's own 50 % same / 50 % different verification batches.

``vm_pair_score_hist`` scores every pair on the chip and bins it on the order-preserving uint32 key of the fp32 score, so the N x N
matrix never exists.  A histogram window gives the EXACT counts of scores below each of its bin edges, so the metrics are found like
this: pass 1 bins the bulk of the scores (a window placed by a sample of pairs, within cheap bounds; the under / over slots keep
the counts exact whatever falls outside); then every bin
that may hold t* or the best threshold is zoomed into (a window over the bin, log2(bins) bits finer) until those bins hold one key
value each.  EER, t*, the best balanced accuracy and its threshold then equal what a full sort of the fp32 scores gives.

Under torchrun every rank takes one ``triangle_shards`` range of rows and the int64 histograms are all-reduced, so every rank takes the
same zoom decisions.

Cohort score normalisation (``score_norm``, ``norm=``): S-norm and AS-norm.  ``vm_cohort_topk_stats`` gives every row i the mean mu_i
and the standard deviation sigma_i of its scores against the K cohort rows most like it (K = C: S-norm), and the pair {i, j} is scored
s' = 0.5 ((s - mu_i) / sigma_i + (s - mu_j) / sigma_j), in fp32 exactly as ``normalise_scores_numpy`` evaluates it
(``vm_pair_score_hist_norm``).  The exact metrics then work on s' unchanged.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, parallel
from ._lib import VM_SCORE_NEG_EUCLIDEAN, VM_SCORE_PLDA

SCORES = {**_lib.DIST, "weighted_l1": _lib.VM_SCORE_WEIGHTED_L1}
KEY_SPACE = 1 << 32
KEY_NEG_INF = 0x007FFFFF        # key(-inf)
KEY_FIN_LO = 0x00800000         # key(-FLT_MAX): the smallest finite key
KEY_POS_INF = 0xFF800000        # key(+inf); every finite key is below it
PASS1_BINS = 4096
MAX_WINDOWS = 4
LDS_WORDS = 2 * 4 * (1024 + 3)  # csrc/verif.hip VH_LDS_HIST_WORDS


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def score_keys(s) -> np.ndarray:
    """uint32 keys of fp32 scores: -0.0 -> +0.0, then bits | 2^31 (non-negative) or ~bits (negative).  NaN maps somewhere: mask it."""
    u = np.ascontiguousarray(np.asarray(s, dtype=np.float32)).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def key_of(t: float) -> int:
    return int(score_keys(np.array([t], np.float32))[0])


def key_value(k: int) -> float:
    """The fp32 value whose key is k (inverse of ``score_keys``)."""
    bits = (k & 0x7FFFFFFF) if k & 0x80000000 else (~k & 0xFFFFFFFF)
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def key_values(k: np.ndarray) -> np.ndarray:
    """``key_value`` of an array of keys, as float64."""
    k = np.asarray(k, dtype=np.int64)
    bits = np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k & 0xFFFFFFFF).astype(np.uint32)
    return bits.view(np.float32).astype(np.float64)


def bin_scores(scores, target, windows: Sequence[Tuple[int, int]], bins: int) -> np.ndarray:
    """numpy twin of ``vm_pair_score_hist``: (n_windows, 2, bins + 3) int64 counts of the scores (class 0 = target)."""
    s = np.asarray(scores, dtype=np.float32).ravel()
    cls = np.where(np.asarray(target, dtype=bool).ravel(), 0, 1)
    nan = np.isnan(s)
    k = score_keys(s).astype(np.int64)
    out = np.zeros((len(windows), 2, bins + 3), dtype=np.int64)
    for v, (lo, sh) in enumerate(windows):
        b = (k - lo) >> sh
        slot = np.where(k < lo, bins, np.where(b < bins, b, bins + 1))
        slot = np.where(nan, bins + 2, slot)
        out[v] = np.bincount(cls * (bins + 3) + slot, minlength=2 * (bins + 3)).reshape(2, bins + 3)
    return out


# ---- cohort score normalisation: the numpy twins -----------------------------------------------------------------------------------
def cohort_select_numpy(scores, top_k: int, self_row0: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """numpy twin of ``vm_cohort_topk_stats``'s selection on an (M, C) fp32 score matrix: (topk_idx (M, top_k) int32 in (key, index) order
    padded with -1, count (M) int32).  NaN scores and, with ``self_row0``, the pairs (m, self_row0 + m) are skipped."""
    s = np.asarray(scores, dtype=np.float32)
    M, C = s.shape
    idx = np.full((M, top_k), -1, dtype=np.int32)
    cnt = np.zeros(M, dtype=np.int32)
    cols = np.arange(C)
    for m in range(M):
        ok = ~np.isnan(s[m])
        if self_row0 is not None and self_row0 >= 0 and 0 <= self_row0 + m < C:
            ok[self_row0 + m] = False
        c = cols[ok]
        order = c[np.lexsort((c, score_keys(s[m, c])))][:top_k]
        idx[m, :len(order)] = order
        cnt[m] = len(order)
    return idx, cnt


def cohort_stats_numpy(scores, top_k: int, self_row0: Optional[int] = None) -> Dict[str, np.ndarray]:
    """numpy twin of ``vm_cohort_topk_stats``: ``mu``, ``sigma`` (float64 mean and population standard deviation of the selected scores,
    rounded to fp32 once), ``rsig`` = fp32(1 / float64(sigma)), ``count`` and ``topk_idx``."""
    s = np.asarray(scores, dtype=np.float32)
    idx, cnt = cohort_select_numpy(s, top_k, self_row0)
    M = s.shape[0]
    mu, sig = np.full(M, np.nan, np.float32), np.full(M, np.nan, np.float32)
    for m in range(M):
        if cnt[m]:
            v = s[m, idx[m, :cnt[m]]].astype(np.float64)
            mean = v.sum() / cnt[m]
            mu[m] = np.float32(mean)
            sig[m] = np.float32(np.sqrt(((v - mean) ** 2).sum() / cnt[m]))
    with np.errstate(divide="ignore", invalid="ignore"):
        rsig = (1.0 / sig.astype(np.float64)).astype(np.float32)
    return {"mu": mu, "sigma": sig, "rsig": rsig, "count": cnt, "topk_idx": idx}


def normalise_scores_numpy(s, i, j, mu, rsig) -> np.ndarray:
    """The normalised pair score of ``vm_pair_score_hist_norm`` in fp32: a = s - mu[i]; b = s - mu[j]; 0.5 (a rsig[i] + b rsig[j]), each
    operation rounded on its own."""
    s = np.asarray(s, dtype=np.float32)
    mu, rsig = np.asarray(mu, dtype=np.float32), np.asarray(rsig, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a = s - mu[i]
        b = s - mu[j]
        return np.float32(0.5) * (a * rsig[i] + b * rsig[j])


class ScoreNorm:
    """Per-row cohort statistics of an ``EmbeddingCache`` (``score_norm``): ``mu``, ``sigma``, ``rsig`` (fp32) and ``count`` (int32) on the
    device, with the ``score`` they were computed for, ``top_k`` (None: S-norm over the whole cohort) and ``cohort_size``."""

    def __init__(self, mu, sigma, rsig, count, score, top_k, cohort_size):
        self.mu, self.sigma, self.rsig, self.count = mu, sigma, rsig, count
        self.score, self.top_k, self.cohort_size = score, top_k, cohort_size

    @property
    def n(self) -> int:
        return int(self.mu.shape[0])


def cohort_topk_stats(q: torch.Tensor, cohort: torch.Tensor, kind: int, weights, top_k: int, self_row0: int = -1,
                      return_topk: bool = False):
    """``vm_cohort_topk_stats`` on device tensors: (mu, sigma, rsig, count[, topk_idx])."""
    lib = _lib.lib()
    dev = q.device
    M, E = q.shape
    C = cohort.shape[0]
    q, cohort = q.contiguous(), cohort.contiguous()
    mu, sig, rsig = (torch.empty(M, dtype=torch.float32, device=dev) for _ in range(3))
    cnt = torch.empty(M, dtype=torch.int32, device=dev)
    topk = torch.empty(M, top_k, dtype=torch.int32, device=dev) if return_topk else None
    if M > 0:
        ws = lib.workspace("vm_cohort_stats_workspace_bytes", M, C, E, device=dev)
        lib.call("vm_cohort_topk_stats", q.data_ptr(), M, cohort.data_ptr(), C, E, kind, None if weights is None else weights.data_ptr(),
                 self_row0, top_k, mu.data_ptr(), sig.data_ptr(), rsig.data_ptr(), cnt.data_ptr(),
                 None if topk is None else topk.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return (mu, sig, rsig, cnt, topk) if return_topk else (mu, sig, rsig, cnt)


def score_norm(cache, cohort, score: str = "euclidean", top_k: Optional[int] = 300, model=None) -> ScoreNorm:
    """Cohort statistics of every row of ``cache`` for S-norm (``top_k=None``: the whole cohort) or AS-norm (the ``top_k`` cohort rows most
    like the row).  ``cohort``: an ``EmbeddingCache`` or a (C, E) tensor; ``cohort is cache`` excludes each row from its own cohort.
    score="head" takes the siamese model's head score like ``verification_metrics``.  Under torchrun every rank computes its
    ``parallel.shard_range`` rows and the rows are all-gathered: every rank holds all N."""
    kind, weights, _ = score_kind(cache, score, model)
    self_ex = cohort is cache
    ce = cohort.emb if hasattr(cohort, "emb") else torch.as_tensor(cohort)
    ce = ce.to(device=cache.emb.device, dtype=torch.float32).contiguous()
    if ce.dim() != 2 or ce.shape[1] != cache.E or ce.shape[0] < 1:
        raise ValueError("the cohort must be a non-empty (C, %d) matrix" % cache.E)
    C = int(ce.shape[0])
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be >= 1 (or None for S-norm)")
    K = C if top_k is None else min(int(top_k), C)
    rank, world = parallel.rank_world()
    lo, hi = parallel.shard_range(cache.n, rank, world)
    mu, sig, rsig, cnt = cohort_topk_stats(cache.emb[lo:hi], ce, kind, weights, K, lo if self_ex else -1)
    if world > 1:
        loc = torch.stack([mu.double(), sig.double(), rsig.double(), cnt.double()], 1)
        allr = parallel.all_gather_rows(loc, cache.n)
        mu, sig, rsig = (allr[:, k].float().contiguous() for k in range(3))
        cnt = allr[:, 3].to(torch.int32).contiguous()
    return ScoreNorm(mu, sig, rsig, cnt, score, top_k, C)


def check_norm(cache, score, norm):
    if norm is None:
        return
    if norm.score != score:
        raise ValueError("the ScoreNorm was computed for score %r, not %r" % (norm.score, score))
    if norm.n != cache.n:
        raise ValueError("the ScoreNorm holds %d rows, the cache %d" % (norm.n, cache.n))


# ---- rows of the triangle --------------------------------------------------------------------------------------------------------
def pairs_before(i, N):
    """Pairs {i', j}, i' < i, j > i'."""
    return i * (N - 1) - i * (i - 1) // 2


def triangle_shards(N: int, world: int) -> List[Tuple[int, int]]:
    """Contiguous row ranges [lo, hi) of the triangle {i < j < N} with near-equal PAIR counts (the early rows hold the most pairs): each
    boundary is the row whose pair prefix is nearest to an even split of the pairs left to the remaining shards."""
    total = pairs_before(N, N)
    cuts = [0]
    for k in range(1, world):
        done = pairs_before(cuts[-1], N)
        goal = done + (total - done) / (world - k + 1)
        lo, hi = cuts[-1], N
        while lo < hi:   # first row i with prefix >= goal
            mid = (lo + hi) // 2
            if pairs_before(mid, N) >= goal:
                hi = mid
            else:
                lo = mid + 1
        if lo > cuts[-1] and goal - pairs_before(lo - 1, N) < pairs_before(lo, N) - goal:
            lo -= 1
        cuts.append(lo)
    cuts.append(N)
    return list(zip(cuts[:-1], cuts[1:]))


def triangle_sum(device_fn: Callable, n: int, rows: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """The pass of an all-pairs evaluator over the triangle of an n-row cache.  ``device_fn((lo, hi))`` returns a device tensor of
    integer counts or float64 sums over the pairs with i in [lo, hi).  ``rows`` given: that range alone, no communication.  Otherwise
    this rank's ``triangle_shards`` range, summed over the ranks (every rank then holds the same array)."""
    if rows is not None:
        return device_fn(rows).cpu().numpy()
    rank, world = parallel.rank_world()
    return parallel.sum_ranks(device_fn(triangle_shards(n, world)[rank])).cpu().numpy()


# ---- the device histogram --------------------------------------------------------------------------------------------------------
def score_kind(cache, score: str, model) -> Tuple[int, Optional[torch.Tensor], Optional[Tuple[float, float]]]:
    """(kernel score kind, weights, (w, b) of a uniform_euclidean head)."""
    if score in ("euclidean", "cosine", "dot_product"):
        return SCORES[score], None, None
    if score == "plda":   # the rows of ``cache`` are PLDA-space rows (plda.PldaModel.project): no weights, no head
        if cache.E < 4 or cache.E % 4:
            raise ValueError('score "plda" takes PLDA-space rows (plda.PldaModel.project): a width that is a multiple of 4, not %d' % cache.E)
        return VM_SCORE_PLDA, None, None
    if score == "weighted_l1":
        raise ValueError('score "weighted_l1" takes its weights from a model: use score="head" with a weighted_l1 siamese net')
    if score != "head":
        raise ValueError("score must be one of (euclidean, cosine, dot_product, head, plda)")
    from .retrieval import _siamese_head_engine
    eng = _siamese_head_engine(model) if model is not None else None
    if eng is None:
        raise ValueError('score="head" needs a siamese model with a uniform_euclidean or weighted_l1 head')
    kern = eng.view("head.kernel").reshape(-1).float()
    bias = float(eng.view("head.bias").reshape(-1)[0].item())
    if eng.head == "weighted_l1":
        return SCORES["weighted_l1"], kern.to(cache.emb.device).contiguous(), None
    w = float(kern[0].item())
    return (SCORES["euclidean"] if w >= 0 else VM_SCORE_NEG_EUCLIDEAN), None, (w, bias)


def _device_hist(cache, kind: int, weights, windows, bins: int, rows: Tuple[int, int], norm=None) -> np.ndarray:
    lib = _lib.lib()
    dev = cache.emb.device
    hist = torch.zeros(len(windows), 2, bins + 3, dtype=torch.int64, device=dev)
    lo, hi = rows
    if hi > lo:
        emb = cache.emb.contiguous()
        ws = lib.workspace("vm_pair_score_hist_workspace_bytes", cache.n, cache.E, device=dev)
        win = np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1, 2))
        if norm is None:
            lib.call("vm_pair_score_hist", emb.data_ptr(), cache.speaker_dev.data_ptr(), cache.n, cache.E, kind,
                     None if weights is None else weights.data_ptr(), lo, hi, win.ctypes.data, len(windows), bins, hist.data_ptr(), ws.data_ptr(),
                     torch.cuda.current_stream(dev).cuda_stream)
        else:
            lib.call("vm_pair_score_hist_norm", emb.data_ptr(), cache.speaker_dev.data_ptr(), cache.n, cache.E, kind,
                     None if weights is None else weights.data_ptr(), lo, hi, win.ctypes.data, len(windows), bins, norm.mu.data_ptr(),
                     norm.rsig.data_ptr(), hist.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return hist


def score_histogram(cache, score: str, windows: Sequence[Tuple[int, int]], bins: int, rows: Optional[Tuple[int, int]] = None,
                    model=None, norm: Optional[ScoreNorm] = None) -> np.ndarray:
    """(n_windows, 2, bins + 3) int64 counts of all pair scores of ``cache`` (class 0 = target) in windows (key_lo, shift).  ``rows``:
    only the pairs with i in [lo, hi); by default this rank's ``triangle_shards`` range, and under torchrun the histograms of all ranks
    are summed.  ``norm``: the counts of the normalised scores (``score_norm``)."""
    kind, weights, _ = score_kind(cache, score, model)
    check_norm(cache, score, norm)
    return histogram(cache, kind, weights, windows, bins, rows, norm)


def check_windows(windows, bins: int):
    """What one histogram launch can hold (csrc/verif.hip: the windows' counters live in LDS)."""
    if len(windows) > MAX_WINDOWS or len(windows) * 2 * (bins + 3) > LDS_WORDS:
        raise ValueError("at most %d windows and %d histogram words per launch" % (MAX_WINDOWS, LDS_WORDS))


def histogram(cache, kind, weights, windows, bins, rows=None, norm=None) -> np.ndarray:
    """``score_histogram`` for a kernel score kind and its weights (``score_kind``)."""
    check_windows(windows, bins)
    return triangle_sum(lambda r: _device_hist(cache, kind, weights, windows, bins, r, norm), cache.n, rows)


def counts_at_threshold(hist_fn: Callable, t: float) -> Dict:
    """Balanced accuracy, FAR, FRR and the trial counts at a fixed threshold t from any histogram source (``exact_sweep``): one
    1-bin window with key_lo = key(t), whose under slot is exactly {s < t}.  A NaN t takes the last key: every number is below it."""
    k = key_of(t) if not math.isnan(t) else KEY_SPACE - 1
    h = hist_fn([(k, 31)], 1)[0]
    nT, nN = int(h[0, :-1].sum()), int(h[1, :-1].sum())
    far = float(h[1, 1]) / nN if nN else float("nan")
    frr = float(nT - h[0, 1]) / nT if nT else float("nan")
    return {"balanced_accuracy": 1.0 - (far + frr) / 2, "far": far, "frr": frr, "n_target": nT, "n_nontarget": nN,
            "n_nan": int(h[0, -1] + h[1, -1])}


# ---- exact metrics from cumulative counts ----------------------------------------------------------------------------------------
def _ceil_log2(x: int) -> int:
    return max(0, (int(x) - 1).bit_length())


class _Cumulative:
    """Exact counts (targets, non-targets) of the scores whose key is below each known edge key; 0 and 2^32 are always known."""

    def __init__(self, total_t, total_n):
        self.c = {0: (0, 0), KEY_SPACE: (total_t, total_n)}

    def add_window(self, h, lo, sh, bins):
        """h: (2, bins + 3) counts of one window."""
        ct, cn = int(h[0, bins]), int(h[1, bins])
        for b in range(bins + 1):
            e = lo + (b << sh)
            if e > KEY_SPACE:
                break
            if e < KEY_SPACE:
                self.c[e] = (ct, cn)
            if b < bins:
                ct += int(h[0, b])
                cn += int(h[1, b])

    def segments(self):
        ks = sorted(self.c)
        return [(a, b, self.c[a], self.c[b]) for a, b in zip(ks[:-1], ks[1:])]


def _finite_part(lo, hi):
    return max(lo, KEY_FIN_LO) < min(hi, KEY_POS_INF)


def _dcf_weights(point) -> Tuple[int, int]:
    """Integers (wa, wb) in the exact ratio C_miss P : C_fa (1 - P) of a point (P, C_miss, C_fa) (the floats as the rationals they
    are): DCF(t) is then (wa FRR(t) + wb FAR(t)) / min(wa, wb), and every comparison of costs one of integers."""
    from fractions import Fraction
    pt, cm, cf = (Fraction(float(x)) for x in point)
    if not (0 < pt < 1 and cm > 0 and cf > 0):
        raise ValueError("a detection-cost point is (P_target in (0, 1), C_miss > 0, C_fa > 0), not %r" % (tuple(point),))
    A, B = cm * pt, cf * (1 - pt)
    den = A.denominator * B.denominator // math.gcd(A.denominator, B.denominator)
    return int(A * den), int(B * den)


def as_dcf_points(points) -> List[Tuple[float, float, float]]:
    """Detection-cost points as (P_target, C_miss, C_fa) triples: a bare P, or (P,), stands for (P, 1, 1)."""
    out = []
    for pt in points:
        pt = (pt,) if np.isscalar(pt) else tuple(pt)
        if len(pt) not in (1, 3):
            raise ValueError("a detection-cost point is P_target or (P_target, C_miss, C_fa)")
        pt = tuple(float(x) for x in (pt if len(pt) == 3 else (pt[0], 1.0, 1.0)))
        _dcf_weights(pt)
        out.append(pt)
    return out


def dcf_value(point, far: float, frr: float) -> float:
    """DCF = (C_miss P FRR + C_fa (1 - P) FAR) / min(C_miss P, C_fa (1 - P)) in float64, from the rates as floats."""
    pt, cm, cf = point
    return (cm * pt * frr + cf * (1.0 - pt) * far) / min(cm * pt, cf * (1.0 - pt))


def _plan(cum: _Cumulative, nT: int, nN: int, dcf_w: Sequence[Tuple[int, int]] = ()):
    """One step of the zoom: (result or None, segments [lo, hi) to refine).  Items in key order: known candidates (a single-key
    finite segment that holds scores, and +inf) and 'open' segments (several keys, holding scores, some of them finite).  ``dcf_w``:
    the integer weights of the detection-cost points, each treated as the balanced accuracy is."""
    items = []   # (kind, lo, hi, c_lo, c_hi): kind 'c' = candidate at key lo, 'o' = open segment
    pinf = None
    refine = []
    for lo, hi, c0, c1 in cum.segments():
        n = (c1[0] - c0[0]) + (c1[1] - c0[1])
        if lo <= KEY_POS_INF < hi or lo == KEY_POS_INF:
            if lo == KEY_POS_INF or n == 0:
                pinf = c0
            else:   # +inf's position is inside a segment holding scores: split it there
                refine.append((lo, hi))
        if n == 0 or not _finite_part(lo, hi):
            continue
        if hi - lo == 1:
            items.append(("c", lo, hi, c0, c1))
        else:
            items.append(("o", lo, hi, c0, c1))
    if refine:
        return None, refine
    items.append(("c", KEY_POS_INF, KEY_SPACE, pinf, pinf))
    g = lambda c: c[0] * nN - c[1] * nT                     # (1 - (FAR + FRR) / 2 - 1/2) x 2 nT nN: balanced accuracy
    d = lambda c: c[1] * nT + c[0] * nN - nT * nN          # (FAR - FRR) x nT nN: strictly increasing over the candidates
    # best balanced accuracy, and the minimum of each detection cost: maximise ga c_T nN - gb c_N nT over the candidates (ga = gb = 1:
    # balanced accuracy; a cost point: minus its cost x nT nN up to a constant), the smallest threshold on ties.
    # the best value known to be reached: at a candidate, or at the first score of an open segment (its lower edge) when that score
    # is finite -- the segment then holds that candidate, key unknown; best_at = the first item known to reach it
    def best_of(ga, gb):
        gv = lambda c: ga * c[0] * nN - gb * c[1] * nT
        best, best_at = None, None
        for it in items:
            if (it[0] == "c" or it[1] >= KEY_FIN_LO) and (best is None or gv(it[3]) > best):
                best, best_at = gv(it[3]), it
        for it in items:
            if it[0] == "o":
                ub = ga * it[4][0] * nN - gb * it[3][1] * nT           # every target of the segment below t, none of its non-targets
                if ub > best or (ub == best and it[1] <= best_at[1]):
                    refine.append((it[1], it[2]))
        return best_at
    best_at = best_of(1, 1)
    dcf_at = [best_of(wa, wb) for wa, wb in dcf_w]
    # EER: the first item that holds (or may hold) a candidate with d >= 0, and the item before it
    # (+inf's d is negative when +inf scores exist: then no candidate reaches d >= 0 and t* is the last one)
    first = next((i for i, it in enumerate(items) if (d(it[3]) >= 0 if it[0] == "c" else d(it[4]) >= 0)), len(items))
    for it in items[max(0, first - 1):first + 1]:
        if it[0] == "o":
            refine.append((it[1], it[2]))
    if refine:
        # the open neighbours of every segment to refine go into the same pass: once a zoom has split a segment, the candidate next
        # to the one found is often in the segment beside it, and a pass costs a full sweep of the triangle while a window costs little
        need = set(refine)
        opens = [it for it in items if it[0] == "o"]
        for k, it in enumerate(opens):
            if (it[1], it[2]) in need:
                for nb in opens[max(0, k - 1):k + 2]:
                    refine.append((nb[1], nb[2]))
        return None, sorted(set(refine))
    tb = items[first] if first < len(items) else None
    ta = items[first - 1] if first > 0 else None
    eer_it = ta if ta is not None and (tb is None or -d(ta[3]) <= d(tb[3])) else tb
    return (eer_it, best_at, dcf_at), []


def _windows_for(refine, bins=1024, gain=16):
    """Key ranges [lo, hi) of the windows that refine the segments: neighbouring segments share a window while its bins stay at least
    ``gain`` times narrower than the widest of them; a segment that holds +inf's key starts its window there (it is split at +inf)."""
    out = []
    for lo, hi in sorted(refine):
        if lo < KEY_POS_INF < hi:
            lo = KEY_POS_INF
        if out and hi - out[-1][0] <= (bins // gain) * max(out[-1][2], hi - lo):
            out[-1] = (out[-1][0], hi, max(out[-1][2], hi - lo))
        else:
            out.append((lo, hi, hi - lo))
    return [(lo, hi) for lo, hi, _ in out]


def exact_sweep(hist_fn: Callable, pass1: Tuple[int, int], max_passes: int = 10000, dcf_points: Sequence = ()) -> Dict:
    """The zoom loop on any histogram source ``hist_fn(windows, bins) -> (n_windows, 2, bins + 3) int64`` (the device histogram, or
    ``bin_scores`` on a score array in the CPU tests).  Returns the metrics dict of ``verification_metrics`` (without the model part).
    ``dcf_points``: detection-cost points (P_target, C_miss, C_fa); the dict then has ``dcf``, one entry per point in their order:
    ``min_dcf`` (the minimum over the candidate thresholds, exact like the other metrics), ``min_dcf_threshold`` (the smallest that
    reaches it) and ``far_at_min_dcf`` / ``frr_at_min_dcf``.  Without points neither the keys nor the passes change."""
    points = as_dcf_points(dcf_points)
    dcf_w = [_dcf_weights(pt) for pt in points]
    h1 = hist_fn([pass1], PASS1_BINS)
    n_nan = int(h1[0, 0, -1] + h1[0, 1, -1])
    nT, nN = int(h1[0, 0, :-1].sum()), int(h1[0, 1, :-1].sum())
    cum = _Cumulative(nT, nN)
    cum.add_window(h1[0], pass1[0], pass1[1], PASS1_BINS)
    out = {"n_target": nT, "n_nontarget": nN, "n_nan": n_nan}
    # ROC at the pass-1 edges
    edges = [pass1[0] + (b << pass1[1]) for b in range(PASS1_BINS + 1) if pass1[0] + (b << pass1[1]) <= KEY_POS_INF]
    roc_t = key_values(np.array(edges, dtype=np.int64))
    keep = ~np.isnan(roc_t)
    cs = np.array([cum.c[e] for e in edges], dtype=np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["roc"] = {"threshold": roc_t[keep], "far": (cs[:, 1] / nN)[keep], "frr": ((nT - cs[:, 0]) / nT)[keep]}
    passes = 1
    if nT == 0 or nN == 0:
        nan = float("nan")
        out.update(eer=nan, eer_threshold=nan, best_balanced_accuracy=nan, best_threshold=nan, far_at_eer=nan, frr_at_eer=nan,
                   far_at_best=nan, frr_at_best=nan, auc=nan, auc_bound=nan, passes=passes)
        if points:
            out["dcf"] = [{"p_target": pt[0], "c_miss": pt[1], "c_fa": pt[2], "min_dcf": nan, "min_dcf_threshold": nan,
                           "far_at_min_dcf": nan, "frr_at_min_dcf": nan} for pt in points]
        return out
    while True:
        res, refine = _plan(cum, nT, nN, dcf_w)
        if res is not None:
            break
        wins = _windows_for(refine)
        for c in range(0, len(wins), MAX_WINDOWS):
            if passes >= max_passes:
                raise RuntimeError("verification zoom did not converge in %d passes" % max_passes)
            chunk = wins[c:c + MAX_WINDOWS]
            bins = 1 << (min(PASS1_BINS // len(chunk), LDS_WORDS // (2 * len(chunk)) - 3).bit_length() - 1)
            chunk = [(lo, _ceil_log2(-(-(hi - lo) // bins))) for lo, hi in chunk]
            h = hist_fn(chunk, bins)
            for v, (lo, sh) in enumerate(chunk):
                cum.add_window(h[v], lo, sh, bins)
            passes += 1
    (eer_it, best_it, dcf_its) = res
    rate = lambda c: (c[1] / nN, (nT - c[0]) / nT)
    far_e, frr_e = rate(eer_it[3])
    far_b, frr_b = rate(best_it[3])
    thr = lambda it: math.inf if it[1] == KEY_POS_INF else key_value(it[1])
    # AUC (P(target score < non-target score) + P(tie) / 2) on the final partition; within a multi-key segment the order is unknown
    auc2, bound2 = 0, 0
    for lo, hi, c0, c1 in cum.segments():
        t, n = c1[0] - c0[0], c1[1] - c0[1]
        auc2 += 2 * t * (nN - c1[1]) + t * n
        if hi - lo > 1:
            bound2 += t * n
    out.update(eer=(far_e + frr_e) / 2, eer_threshold=thr(eer_it), far_at_eer=far_e, frr_at_eer=frr_e,
               best_balanced_accuracy=1.0 - (far_b + frr_b) / 2, best_threshold=thr(best_it), far_at_best=far_b, frr_at_best=frr_b,
               auc=auc2 / (2 * nT * nN), auc_bound=bound2 / (2 * nT * nN), passes=passes)
    if points:
        out["dcf"] = []
        for pt, it in zip(points, dcf_its):
            far_d, frr_d = rate(it[3])
            out["dcf"].append({"p_target": pt[0], "c_miss": pt[1], "c_fa": pt[2], "min_dcf": dcf_value(pt, far_d, frr_d),
                               "min_dcf_threshold": thr(it), "far_at_min_dcf": far_d, "frr_at_min_dcf": frr_d})
    return out


def sorted_dcf(scores, target, points) -> List[Dict]:
    """The definition of the minimum detection cost, by a full sort (tests and small sets): per point (P_target, C_miss, C_fa) the
    entry of ``exact_sweep``'s ``dcf``.  The thresholds are the distinct finite scores and +inf, a pair is accepted iff s < t, NaN
    scores are left out, the costs are compared as exact rationals and the smallest threshold wins a tie."""
    s = np.asarray(scores, dtype=np.float32).ravel()
    tg = np.asarray(target, dtype=bool).ravel()
    ok = ~np.isnan(s)
    st, sn = np.sort(s[ok & tg]), np.sort(s[ok & ~tg])
    nT, nN = len(st), len(sn)
    cand = np.concatenate([np.unique(s[ok & np.isfinite(s)]), np.array([np.inf], np.float32)])
    cT = [int(c) for c in np.searchsorted(st, cand, side="left")]
    cN = [int(c) for c in np.searchsorted(sn, cand, side="left")]
    out = []
    nan = float("nan")
    for pt in as_dcf_points(points):
        if nT == 0 or nN == 0:
            out.append({"p_target": pt[0], "c_miss": pt[1], "c_fa": pt[2], "min_dcf": nan, "min_dcf_threshold": nan,
                        "far_at_min_dcf": nan, "frr_at_min_dcf": nan})
            continue
        wa, wb = _dcf_weights(pt)
        cost = [wa * (nT - a) * nN + wb * b * nT for a, b in zip(cT, cN)]   # DCF x nT nN min(wa, wb)
        i = min(range(len(cand)), key=lambda k: (cost[k], k))
        far, frr = cN[i] / nN, (nT - cT[i]) / nT
        out.append({"p_target": pt[0], "c_miss": pt[1], "c_fa": pt[2], "min_dcf": dcf_value(pt, far, frr),
                    "min_dcf_threshold": float(cand[i]), "far_at_min_dcf": far, "frr_at_min_dcf": frr})
    return out


def sorted_metrics(scores, target) -> Dict:
    """The definition, by a full sort (tests and small sets): EER, t*, best balanced accuracy and its threshold, n_nan."""
    s = np.asarray(scores, dtype=np.float32).ravel()
    tg = np.asarray(target, dtype=bool).ravel()
    ok = ~np.isnan(s)
    st, sn = np.sort(s[ok & tg]), np.sort(s[ok & ~tg])
    nT, nN = len(st), len(sn)
    fin = s[ok & np.isfinite(s)]
    cand = np.concatenate([np.unique(fin), np.array([np.inf], np.float32)])
    cT = np.searchsorted(st, cand, side="left").astype(object)
    cN = np.searchsorted(sn, cand, side="left").astype(object)
    d = [int(a) * nT + int(b) * nN - nT * nN for a, b in zip(cN, cT)]
    g = [int(b) * nN - int(a) * nT for a, b in zip(cN, cT)]
    ie = min(range(len(cand)), key=lambda i: (abs(d[i]), i))
    ib = min(range(len(cand)), key=lambda i: (-g[i], i))
    rate = lambda i: (int(cN[i]) / nN, (nT - int(cT[i])) / nT)
    fe, re_ = rate(ie)
    fb, rb = rate(ib)
    return {"eer": (fe + re_) / 2, "eer_threshold": float(cand[ie]), "far_at_eer": fe, "frr_at_eer": re_,
            "best_balanced_accuracy": 1.0 - (fb + rb) / 2, "best_threshold": float(cand[ib]), "far_at_best": fb, "frr_at_best": rb,
            "n_target": nT, "n_nontarget": nN, "n_nan": int((~ok).sum())}


# ---- pass-1 bounds ---------------------------------------------------------------------------------------------------------------
def pass1_window(lo_val: float, hi_val: float, bins: int = PASS1_BINS) -> Tuple[int, int]:
    """A window whose bins cover [lo_val, hi_val] (keys), aligned to its bin width."""
    klo, khi = key_of(lo_val), key_of(hi_val)
    sh = min(31, _ceil_log2(-(-(khi - klo + 1) // bins)))
    while True:
        lo = (klo >> sh) << sh
        if lo + (bins << sh) > khi:
            return lo, sh
        sh += 1


def bounds(cache, kind) -> Tuple[float, float]:
    """Cheap bounds of every pair score of ``cache`` under an embedding score kind, from the largest row norm."""
    if kind == SCORES["cosine"]:
        return 0.0, 2.0
    if kind == VM_SCORE_PLDA:   # s = (h_i + h_j) - w_i . w_j
        h = cache.emb[:, -1].double()
        h = h[torch.isfinite(h)]
        r = float(torch.linalg.vector_norm(cache.emb[:, :-1].double(), dim=1).max().item()) if cache.n else 0.0
        r = r * r * 1.001 + 1e-30
        if h.numel() == 0:
            return -r, r
        lo, hi = 2 * float(h.min().item()), 2 * float(h.max().item())
        pad = 1e-3 * max(abs(lo), abs(hi))
        return lo - pad - r, hi + pad + r
    norms = torch.linalg.vector_norm(cache.emb.double(), dim=1)
    r = float(norms.max().item()) if cache.n else 0.0
    r = r * 1.001 + 1e-30
    if kind == SCORES["euclidean"]:
        return 0.0, 2 * r
    if kind == VM_SCORE_NEG_EUCLIDEAN:
        return -2 * r, 0.0
    return -r * r, r * r   # dot product (and weighted_l1 below)


def sample_scores(a: torch.Tensor, b: torch.Tensor, kind: int, weights=None) -> torch.Tensor:
    """float64 scores of the sampled rows (a, b) under a kernel score kind (torch arithmetic: only a window's place depends on them)."""
    a, b = a.double(), b.double()
    if kind in (SCORES["euclidean"], VM_SCORE_NEG_EUCLIDEAN):
        return torch.linalg.vector_norm(a - b, dim=1) * (1 if kind == SCORES["euclidean"] else -1)
    if kind == SCORES["cosine"]:
        return 1 - (a * b).sum(1) / (torch.linalg.vector_norm(a, dim=1) * torch.linalg.vector_norm(b, dim=1))
    if kind == SCORES["dot_product"]:
        return -(a * b).sum(1)
    if kind == VM_SCORE_PLDA:
        return (a[:, -1] + b[:, -1]) - (a[:, :-1] * b[:, :-1]).sum(1)
    return ((a - b).abs() * weights.double()).sum(1)


def place_window(sample_fn: Callable) -> Tuple[int, int]:
    """Pass 1's window of any evaluator.  ``sample_fn()`` runs on rank 0 only and returns (lo, hi, sample): cheap bounds of every score,
    and a float64 tensor of the scores of a seeded sample of trials (or None).  The window spans the 1e-4 .. 1 - 1e-4 quantiles of the
    finite sampled scores, padded by 5 % and clipped to [lo, hi]; with 100 such scores or fewer, or nothing left after the clip, it
    spans the bounds.  It only places the bins over the bulk of the scores, so that one zoom pass usually reaches single keys: whatever
    falls outside lands in the under / over slots and the counts stay exact.  Under torchrun rank 0's window is broadcast."""
    win = torch.zeros(2, dtype=torch.int64)
    if parallel.rank_world()[0] == 0:
        lo, hi, sc = sample_fn()
        win[0], win[1] = pass1_window(lo, hi)
        sc = sc[torch.isfinite(sc)].cpu().numpy() if sc is not None else ()
        if len(sc) > 100:
            q0, q1 = np.quantile(sc, [1e-4, 1 - 1e-4])
            pad = 0.05 * (q1 - q0) + 1e-6 * max(abs(q0), abs(q1)) + 1e-30
            q0, q1 = max(lo, q0 - pad), min(hi, q1 + pad)
            if q0 < q1:
                win[0], win[1] = pass1_window(float(q0), float(q1))
    win = parallel.sum_ranks(win).cpu()
    return int(win[0]), int(win[1])


def sampled_window(cache, kind, weights, lo: float, hi: float, n_sample: int = 1 << 16, norm=None) -> Tuple[int, int]:
    """``place_window`` for the pair trials of ``cache`` within the bounds [lo, hi]: a seeded sample of pairs, normalised with ``norm``."""
    def sample():
        if cache.n < 2:
            return lo, hi, None
        g = torch.Generator().manual_seed(0)
        i = torch.randint(0, cache.n, (n_sample,), generator=g)
        j = (i + torch.randint(1, cache.n, (n_sample,), generator=g)) % cache.n
        sc = sample_scores(cache.emb[i.to(cache.emb.device)], cache.emb[j.to(cache.emb.device)], kind, weights)
        if norm is not None:
            ii, jj = i.to(norm.mu.device), j.to(norm.mu.device)
            mu, rs = norm.mu.double(), norm.rsig.double()
            sc = 0.5 * ((sc - mu[ii]) * rs[ii] + (sc - mu[jj]) * rs[jj])
        return lo, hi, sc
    return place_window(sample)


def norm_bounds(norm: ScoreNorm, lo: float, hi: float) -> Tuple[float, float]:
    """Bounds of the normalised scores of raw scores in [lo, hi]: each half (s - mu_i) rsig_i lies in [(lo - mu_i) rsig_i, (hi - mu_i)
    rsig_i] (rsig >= 0); rows whose statistics are not finite are left out (their scores are NaN or infinite: the NaN / over slots)."""
    mu, rs = norm.mu.double(), norm.rsig.double()
    a, b = (lo - mu) * rs, (hi - mu) * rs
    ok = torch.isfinite(a) & torch.isfinite(b)
    if not bool(ok.any()):
        return -1.0, 1.0
    lo2, hi2 = float(a[ok].min().item()), float(b[ok].max().item())
    pad = 1e-5 * max(abs(lo2), abs(hi2)) + 1e-30
    lo2, hi2 = lo2 - pad, hi2 + pad
    big = float(np.finfo(np.float32).max)
    return max(lo2, -big), min(hi2, big)


def verification_metrics(cache, score: str = "euclidean", model=None, bins: int = PASS1_BINS, norm: Optional[ScoreNorm] = None,
                         dcf_points: Sequence = ()) -> Dict:
    """All-pairs verification metrics of ``cache`` (module docstring): ``eer``, ``eer_threshold``, ``best_balanced_accuracy``,
    ``best_threshold``, FAR / FRR at both, ``auc`` and ``auc_bound`` (the true AUC lies within it), ``roc`` (pass-1 edges as float
    thresholds with FAR and FRR), ``n_target``, ``n_nontarget``, ``n_nan`` and ``passes``.  score="head": the siamese model's own head
    (a uniform_euclidean head is monotone in the distance; the thresholds are then also reported as head outputs p, ``*_p``).
    ``norm``: the metrics of the cohort-normalised scores (``score_norm``); the thresholds are then in normalised units.
    ``dcf_points``: detection-cost points (P_target, C_miss, C_fa) -- adds ``dcf`` with the exact minimum cost of each (``exact_sweep``)."""
    if bins != PASS1_BINS:
        raise ValueError("pass 1 takes %d bins" % PASS1_BINS)
    kind, weights, head = score_kind(cache, score, model)
    check_norm(cache, score, norm)
    if kind == SCORES["weighted_l1"]:
        wsum = float(weights.abs().double().sum().item())
        amax = float(cache.emb.abs().max().item()) if cache.n else 0.0
        lo, hi = -2 * amax * wsum * 1.001 - 1e-30, 2 * amax * wsum * 1.001 + 1e-30
    else:
        lo, hi = bounds(cache, kind)
    if norm is not None:
        lo, hi = norm_bounds(norm, lo, hi)
    out = exact_sweep(lambda wins, b: histogram(cache, kind, weights, wins, b, norm=norm),
                      sampled_window(cache, kind, weights, lo, hi, norm=norm), dcf_points=dcf_points)
    if head is not None and norm is None:
        w, b = head
        out["eer_threshold_p"] = _head_p(out["eer_threshold"], w, b)
        out["best_threshold_p"] = _head_p(out["best_threshold"], w, b)
    return out


def _head_p(t: float, w: float, b: float) -> float:
    """The uniform_euclidean head's output sigmoid(w d + b) at a threshold t on the head score (d, or -d when w < 0)."""
    if math.isinf(t):
        return 1.0 if w != 0 else 1.0 / (1.0 + math.exp(-b))   # t = +inf: every finite distance is accepted
    a = w * (t if w >= 0 else -t) + b
    return 1.0 / (1.0 + math.exp(-a)) if a > -700 else 0.0


def accuracy_at_threshold(cache, t: float, score: str = "euclidean", model=None, norm: Optional[ScoreNorm] = None) -> Dict:
    """Balanced accuracy, FAR and FRR at a fixed threshold t (in score units; with ``norm``, in normalised units): one pass with key_lo =
    key(t), whose under slot is then exactly {s < t}."""
    kind, weights, _ = score_kind(cache, score, model)
    check_norm(cache, score, norm)
    return counts_at_threshold(lambda wins, b: histogram(cache, kind, weights, wins, b, norm=norm), t)


def bayes_threshold(calibration, point) -> float:
    """The Bayes decision threshold of calibrated scores llr = a s + b at a point (P, C_miss, C_fa), moved into score units: accept iff
    llr > -logit(P~), P~ = P C_miss / (P C_miss + (1 - P) C_fa), which for a < 0 is s < t_s = fp32((-logit(P~) - b) / a).  A fit with
    a >= 0 (scores that do not separate the classes the right way round) has no such threshold and raises."""
    if not calibration.a < 0:
        raise ValueError("the calibration's slope a = %r is not negative: the scores do not separate targets from non-targets" % calibration.a)
    pt, cm, cf = as_dcf_points([point])[0]
    theta = -(math.log(pt * cm) - math.log((1.0 - pt) * cf))
    with np.errstate(over="ignore"):
        return float(np.float32((theta - calibration.b) / calibration.a))


def detection_costs(cache, calibration, points, model=None, norm: Optional[ScoreNorm] = None, metrics: Optional[Dict] = None) -> List[Dict]:
    """Per point (P_target, C_miss, C_fa): the entry of ``verification_metrics``'s ``dcf`` (``min_dcf`` and where it is reached) plus
    ``act_dcf``, the cost at the calibration's Bayes threshold ``act_threshold`` (``bayes_threshold``, in score units) counted by
    ``accuracy_at_threshold``, with ``far_at_act`` / ``frr_at_act``.  ``calibration``: a ``calibration.Calibration`` fitted (on other
    data) for the same score; with ``norm`` it must have been fitted on normalised scores.  ``metrics``: the result of
    ``verification_metrics(cache, ..., dcf_points=points)`` where it has been computed already (the sweep is then not repeated).
    A calibration of speaker-model trials (``trials == "model"``) is refused: ``enrolment.model_detection_costs`` takes those."""
    if getattr(calibration, "trials", "pair") != "pair":
        raise ValueError("the calibration was fitted on %s trials, not pair trials" % calibration.trials)
    if (norm is not None) != bool(calibration.normalised):
        raise ValueError("the calibration was fitted on %s scores" % ("normalised" if calibration.normalised else "raw"))
    points = as_dcf_points(points)
    ts = [bayes_threshold(calibration, pt) for pt in points]   # raises before any pass
    if metrics is None:
        metrics = verification_metrics(cache, calibration.score, model=model, norm=norm, dcf_points=points)
    out = [dict(d) for d in metrics["dcf"]]
    if [(d["p_target"], d["c_miss"], d["c_fa"]) for d in out] != points:
        raise ValueError("``metrics`` was computed for other detection-cost points")
    for d, pt, t in zip(out, points, ts):
        at = accuracy_at_threshold(cache, t, calibration.score, model=model, norm=norm)
        d.update(act_dcf=dcf_value(pt, at["far"], at["frr"]), act_threshold=t, far_at_act=at["far"], frr_at_act=at["frr"])
    return out
