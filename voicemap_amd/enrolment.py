"""Speaker models over a cached embedding matrix: enrol every speaker, name the speaker of every utterance, verify utterances against models.

``retrieval.evaluate_tasks`` answers the reference's sampled question (5-way, at most 20-way tasks drawn at random).  This module answers
the exhaustive ones over a ``retrieval.EmbeddingCache``:

* identification: enrol all S speakers of a corpus, score every utterance against every speaker MODEL, report the rank-1 accuracy, the
  rank-k curve (CMC) and the mean reciprocal rank -- the reference's n-shot k-way metric with k = every speaker and n = every other file
  of the speaker (``leave_one_out``) or a seeded choice of n files (``per_speaker``);
* model-trial verification: a trial is (utterance, speaker model), target iff the model is the utterance's own speaker; EER, thresholds and
  the best balanced accuracy are exact (``verification.exact_sweep`` on the histograms of ``vm_speaker_trial_hist``).

Definitions (include/voicemap_hip.h states the same; the numpy twins below follow them in float64 and the tests hold the kernels to them).
Rows ``emb (N, E)`` fp32, ``label (N)`` int32: the dense speaker index in [0, S) or -1 (the row is not enrolled); ``kind``: euclidean 0,
cosine 1, dot_product 2.

* ``|e_u| = sqrt(sum_e e^2)`` (ascending e).  Per-row contribution ``c_u``: euclidean ``e_u``; cosine ``e_u / |e_u|``; dot_product
  ``e_u / |e_u|`` and the magnitude ``|e_u|``.
* Speaker sums ``sum_s = sum c_u`` and ``msum_s = sum |e_u|`` over the enrolled rows of s in ascending row order, float64; ``count_s``.
  The order is part of the contract: bit-identical from run to run and from rank to rank (no float atomics).
* Model of speaker s as seen by query row m: ``n = count_s``, ``Sigma = sum_s``; with leave-one-out and ``q_label[m] == s``,
  ``n = count_s - 1`` and ``Sigma = sum_s - c_m`` (``msum`` likewise).  ``n == 0``: there is no model and (m, s) is not a trial: it is
  counted nowhere.  euclidean and cosine ``p = Sigma / n``; dot_product ``p = (msum / n) (Sigma / n)``  (the reference's prototype
  rules, voicemap/utils.py:159-206: mean embedding / mean unit vector / mean magnitude x mean unit vector).
* Score of the trial (m, s), float64, rounded to fp32 once: euclidean ``sqrt(sum_e (q_e - p_e)^2)`` in the direct form; cosine
  ``1 - q.p / (|q| |p|)``; dot_product ``-q.p`` -- ``oracle.n_shot_prediction``'s numbers for a task whose support rows are the enrolled
  rows of the speakers.  Lower = more alike, as everywhere in ``verification``.
* Order of the trials of one query: (uint32 key of the fp32 score, speaker index) ascending, the key of ``verification.score_keys``
  (-0.0 as +0.0); NaN scores rank after every number, among themselves by speaker index.  ``best_idx[m]`` is the first speaker in that
  order (-1: the row has no trial) and ``best_val[m]`` its score; ``rank[m]`` the number of speakers before the row's own speaker (0 =
  identified), -1 if ``q_label[m] < 0`` or the own speaker has no model for the row (one file under leave-one-out); ``true_score[m]`` the
  score against the own speaker (NaN where rank is -1).

Multi-session PLDA models (``enrol(projected_cache, plda=model)``).  On a cache projected by a ``plda.PldaModel`` a speaker model is
scored by the book: minus the two-covariance log-likelihood ratio of the row against ALL enrolment rows of the speaker together, which
needs only their sum (``sums`` of the projected rows, euclidean kind) and their number (``plda`` module docstring; include/voicemap_hip.h
vm_plda_speaker_identify; the numpy twin is ``plda.trial_scores_plda_numpy``).  The models then carry ``distance == "plda"`` and the
coefficient tables for 1 .. the largest count rows, and ``identify`` / ``model_trial_metrics`` / ``model_trial_accuracy_at_threshold``
mean what they mean above -- trials, order, leave-one-out, ``per_speaker``, ``rows`` -- with that score.  ``plda=`` is the switch:
"plda" is not one of the ``distance`` names.  The cache must already be projected (its width is ``model.P``); a raw cache is refused.

Score normalisation of model trials: S-norm / AS-norm (``model_score_norm``, ``norm=``; include/voicemap_hip.h and DESIGN 8n state the
same).  ``score(r, model)`` is the fp32 trial score above for the back end in use, NaN where the model has no rows (n == 0; PLDA: n
outside 1..n_max).  The cohort is an ``EmbeddingCache`` other than the query cache and ``models.cache``, used two ways: as C cohort
ROWS, and as S_c cohort MODELS (``enrol(cohort, distance=models.distance)`` / ``enrol(cohort, plda=models.plda)`` over all its rows).
Three sets of statistics, each selected and reduced by exactly ``vm_cohort_topk_stats``'s rules (``verification.cohort_stats_numpy``: NaN
scores skipped, K' = min(K, remaining), the K' smallest by (uint32 key with -0.0 as +0.0, index), mu / sigma the float64 mean and
population standard deviation rounded to fp32 once, rsig = fp32(1 / float64(sigma)), K' = 0: NaN, sigma = 0: rsig = +inf):

1. query side: per query row m over the cohort models, ``score(q_m, cohort model)``: ``mu_q``, ``rsig_q`` (M);
2. model side: per enrolled model s over the cohort rows, ``score(cohort row, model s)``: ``mu_s``, ``rsig_s`` (S);
3. own side, leave-one-out only: row m sees its own speaker's model without itself (Sigma = sum_s - c_m, msum likewise, n = count_s - 1)
   and that virtual model has its own statistics over the cohort rows: ``mu_own``, ``rsig_own`` (M), NaN where the row has no own model.

The trial (m, s) is then scored, in fp32 with every operation rounded on its own, ``a = s - mu_q[m]; b = s - mu_M;
s' = 0.5 (a rsig_q[m] + b rsig_M)`` with (mu_M, rsig_M) = (mu_own[m], rsig_own[m]) for the own speaker's trial under leave-one-out and
(mu_s[s], rsig_s[s]) otherwise (``normalise_trials_numpy``); trials, classes and the exact metrics are unchanged.  ``identify`` ranks by
the raw score: normalised ranking is out of scope.

Calibration of model trials (``fit_model_calibration``, ``model_cllr``, ``model_detection_costs``): the ``calibration`` module's affine
map llr = a s + b, its objective, Newton fit and Cllr, over the model trials above instead of the pair trials -- a target iff the model
is the row's own speaker, s the raw or (``norm=``) normalised fp32 trial score, a NaN or infinite s skipped and counted.  One pass of
``vm_[plda_]speaker_trial_calib_sums`` (``model_calib_sums``; twin ``model_calib_sums_numpy``) gives the (2, 8) float64 sums of
``calibration.SUM_NAMES``: the third output mode of the tile kernel behind ``identify`` and the histograms, so its scores are theirs
bit for bit, reduced in a fixed order without float atomics.  A ``Calibration`` fitted here carries ``trials == "model"``; the pair
evaluators refuse it and these refuse a pair one.

Under torchrun every rank computes the sums over all rows itself (N x E reads; the models are then bit-identical everywhere), takes its
``parallel.shard_range`` of the query rows, and the integer rank histogram / trial histograms -- and the float64 calibration sums,
so that every rank takes the same Newton steps -- are summed over ranks.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, parallel
from . import calibration as CAL
from . import verification as V

KINDS = _lib.DIST
_KEY_NAN = 0xFFFFFFFF


def _kind(kind) -> int:
    k = KINDS.get(kind, kind) if isinstance(kind, str) else int(kind)
    if k not in (0, 1, 2):
        raise ValueError("distance must be one of (euclidean, cosine, dot_product)")
    return k


# ---- numpy twins (float64) ---------------------------------------------------------------------------------------------------------
def _contrib(emb, kind: int):
    e = np.asarray(emb, dtype=np.float64)
    mag = np.sqrt((e * e).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = e if kind == 0 else e / mag[:, None]
    return c, mag


def speaker_sums_numpy(emb, label, S: int, kind) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(sums (S, E), msum (S), count (S) int32) of the definition; rows are added in ascending row order."""
    kind = _kind(kind)
    c, mag = _contrib(emb, kind)
    label = np.asarray(label)
    sums, msum, count = np.zeros((S, c.shape[1])), np.zeros(S), np.zeros(S, dtype=np.int32)
    for s in range(S):
        rows = np.flatnonzero(label == s)
        count[s] = len(rows)
        for u in rows:
            sums[s] += c[u]
            msum[s] += mag[u]
    return sums, msum, count


def _models(sg, ms, n, kind: int) -> np.ndarray:
    """The models of the definition, float64 (S, E), from their sums ``sg`` (S, E), ``ms`` (S) and float64 row numbers ``n`` (S); a row
    means nothing where ``n`` is 0."""
    p = sg / n[:, None]
    return (ms / n)[:, None] * p if kind == 2 else p


def _row_scores(qm, qmag, p, kind: int) -> np.ndarray:
    """The geometric score of the definition, float64 (S): one query row ``qm`` of magnitude ``qmag`` against the models ``p``."""
    if kind == 0:
        return np.sqrt(((qm[None, :] - p) ** 2).sum(axis=1))
    if kind == 1:
        return 1.0 - (p @ qm) / (qmag * np.sqrt((p * p).sum(axis=1)))
    return -(p @ qm)


def trial_scores_numpy(emb, label, q, q_label, kind, leave_one_out: bool, S: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(scores (M, S) float64, trial (M, S) bool): the score of every query row against every speaker model of the enrolled rows
    ``emb`` / ``label``; where ``trial`` is False there is no model (the score there is NaN and means nothing)."""
    kind = _kind(kind)
    label, q_label = np.asarray(label), np.asarray(q_label)
    if S is None:
        S = int(label.max()) + 1
    sums, msum, count = speaker_sums_numpy(emb, label, S, kind)
    q = np.asarray(q, dtype=np.float64)
    M = q.shape[0]
    cq, qmag = _contrib(q, kind)
    out = np.full((M, S), np.nan)
    trial = np.zeros((M, S), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for m in range(M):
            n = count.astype(np.float64).copy()
            sg, ms = sums, msum
            own = int(q_label[m])
            if leave_one_out and 0 <= own < S:
                sg, ms = sums.copy(), msum.copy()
                n[own] -= 1
                sg[own] -= cq[m]
                ms[own] -= qmag[m]
            ok = n > 0
            trial[m] = ok
            out[m, ok] = _row_scores(q[m], qmag[m], _models(sg, ms, n, kind), kind)[ok]
    return out, trial


def trial_keys(scores32) -> np.ndarray:
    """uint64 keys of fp32 scores in the order of the definition: ``verification.score_keys``, NaN after every number."""
    s = np.asarray(scores32, dtype=np.float32)
    return np.where(np.isnan(s), _KEY_NAN, V.score_keys(s)).astype(np.uint64)


def ranks_numpy(scores, trial, q_label) -> Dict[str, np.ndarray]:
    """``rank``, ``best_idx`` (int32), ``best_val``, ``true_score`` (fp32) of the definition from an (M, S) score matrix (rounded to fp32
    here) and its trial mask."""
    s = np.asarray(scores).astype(np.float32)
    trial = np.asarray(trial, dtype=bool)
    q_label = np.asarray(q_label)
    M, S = s.shape
    comp = (trial_keys(s) << np.uint64(32)) | np.arange(S, dtype=np.uint64)[None, :]
    comp = np.where(trial, comp, np.uint64(0xFFFFFFFFFFFFFFFF))
    rows = np.arange(M)
    bi = comp.argmin(axis=1)
    has = trial.any(axis=1)
    best_idx = np.where(has, bi, -1).astype(np.int32)
    best_val = np.where(has, s[rows, bi], np.float32(np.nan)).astype(np.float32)
    own = np.where((q_label >= 0) & (q_label < S), q_label, 0).astype(np.int64)
    ranked = (q_label >= 0) & (q_label < S) & trial[rows, own]
    before = ((comp < comp[rows, own][:, None]) & trial).sum(axis=1)
    rank = np.where(ranked, before, -1).astype(np.int32)
    true_score = np.where(ranked, s[rows, own], np.float32(np.nan)).astype(np.float32)
    return {"rank": rank, "best_idx": best_idx, "best_val": best_val, "true_score": true_score}


def loo_sums_numpy(q, q_label, sums, msum, count, kind) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """numpy twin of ``vm_speaker_loo_sums``: the virtual model of every row -- (sums (M, E), msum (M), count (M) int32) of the row's own
    speaker without the row: one float64 subtraction per component; count 0 and zeros where ``q_label`` is outside [0, S) or the
    speaker has one row or none."""
    kind = _kind(kind)
    c, mag = _contrib(q, kind)
    q_label, count = np.asarray(q_label), np.asarray(count)
    sums, msum = np.asarray(sums, dtype=np.float64), np.asarray(msum, dtype=np.float64)
    S = len(count)
    M = c.shape[0]
    vs, vm, vc = np.zeros((M, c.shape[1])), np.zeros(M), np.zeros(M, dtype=np.int32)
    for m in range(M):
        own = int(q_label[m])
        if 0 <= own < S and count[own] > 1:
            vs[m] = sums[own] - c[m]
            vm[m] = msum[own] - mag[m]
            vc[m] = count[own] - 1
    return vs, vm, vc


def _scores_from_sums(q, sums, msum, count, kind: int, tables=None) -> np.ndarray:
    """fp32 (M, S) scores of rows against models given by their sums (``trial_scores_numpy``'s / ``trial_scores_plda_numpy``'s formulas
    without leave-one-out), NaN where there is no model."""
    count = np.asarray(count).astype(np.int64)
    out = np.full((len(q), len(count)), np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if tables is not None:
            A, beta, C, G = (np.asarray(tables[k], dtype=np.float64) for k in ("A", "beta", "C", "G"))
            D = int(G.shape[0])
            ok = (count >= 1) & (count <= int(A.shape[0]) - 1)
            nn = np.where(ok, count, 0)
            w = np.asarray(q, dtype=np.float32)[:, :D].astype(np.float64)
            for m in range(len(w)):
                t = w[m][None, :] - beta[nn] * np.asarray(sums)[:, :D]
                out[m, ok] = ((((A[nn] * t) * t).sum(1) - (G * (w[m] * w[m])).sum()) - C[nn])[ok]
            return out.astype(np.float32)
        ok = count > 0
        q = np.asarray(q, dtype=np.float64)
        qmag = np.sqrt((q * q).sum(axis=1))
        p = _models(np.asarray(sums), np.asarray(msum), count.astype(np.float64), kind)
        for m in range(len(q)):
            out[m, ok] = _row_scores(q[m], qmag[m], p, kind)[ok]
    return out.astype(np.float32)


def model_norm_stats_numpy(emb, label, q, q_label, cohort, cohort_label, kind, top_k: Optional[int], leave_one_out: bool,
                           S: Optional[int] = None, tables=None, cohort_tables=None) -> Dict[str, np.ndarray]:
    """numpy twin of ``model_score_norm``: the three sets of statistics of the module docstring for the query rows ``q`` / ``q_label``
    against the models of the enrolled rows ``emb`` / ``label``, with the cohort rows ``cohort`` and the cohort models of ``cohort`` /
    ``cohort_label``.  ``tables`` (and ``cohort_tables``, default the same): multi-session PLDA (``kind`` is then not used).  Returns
    ``mu_q``, ``sigma_q``, ``rsig_q``, ``count_q`` (M); ``mu_s``, ... (S); with ``leave_one_out`` ``mu_own``, ... (M), else None."""
    from . import plda as _plda
    label, cohort_label = np.asarray(label), np.asarray(cohort_label)
    S = int(label.max()) + 1 if S is None else S
    Sc = int(cohort_label.max()) + 1
    C = len(cohort)
    none_q, none_c = np.full(len(q), -1), np.full(C, -1)
    if tables is not None:
        kind = 0
        ctab = tables if cohort_tables is None else cohort_tables
        sq = _plda.trial_scores_plda_numpy(cohort, cohort_label, q, none_q, ctab, False, Sc)[0]
        sm = _plda.trial_scores_plda_numpy(emb, label, cohort, none_c, tables, False, S)[0]
    else:
        kind = _kind(kind)
        sq = trial_scores_numpy(cohort, cohort_label, q, none_q, kind, False, Sc)[0]
        sm = trial_scores_numpy(emb, label, cohort, none_c, kind, False, S)[0]
    Kq = Sc if top_k is None else min(int(top_k), Sc)
    Ks = C if top_k is None else min(int(top_k), C)
    out = {}
    for name, sc, K in (("q", sq.astype(np.float32), Kq), ("s", sm.astype(np.float32).T, Ks)):
        st = V.cohort_stats_numpy(sc, K)
        out.update({k + "_" + name: st[k] for k in ("mu", "sigma", "rsig", "count")})
    if leave_one_out:
        sums, msum, count = speaker_sums_numpy(emb, label, S, kind)
        vs, vm, vc = loo_sums_numpy(q, q_label, sums, msum, count, kind)
        st = V.cohort_stats_numpy(_scores_from_sums(cohort, vs, vm, vc, kind, tables).T, Ks)
        out.update({k + "_own": st[k] for k in ("mu", "sigma", "rsig", "count")})
    else:
        out.update({k + "_own": None for k in ("mu", "sigma", "rsig", "count")})
    return out


def normalise_trials_numpy(scores, q_label, mu_q, rsig_q, mu_s, rsig_s, mu_own=None, rsig_own=None) -> np.ndarray:
    """The normalised trial scores of ``vm_speaker_trial_hist_norm`` in fp32 from an (M, S) fp32 score matrix: a = s - mu_q[m];
    b = s - mu_M; 0.5 (a rsig_q[m] + b rsig_M), each operation rounded on its own; (mu_M, rsig_M) is the own pair in the own-speaker
    cell when ``mu_own`` / ``rsig_own`` are given (leave-one-out), the model's everywhere else."""
    s = np.asarray(scores, dtype=np.float32)
    M, S = s.shape
    f = lambda x: np.asarray(x, dtype=np.float32)
    mM, rM = np.broadcast_to(f(mu_s)[None, :], (M, S)).copy(), np.broadcast_to(f(rsig_s)[None, :], (M, S)).copy()
    if mu_own is not None:
        ql = np.asarray(q_label)
        rows = np.flatnonzero((ql >= 0) & (ql < S))
        mM[rows, ql[rows]] = f(mu_own)[rows]
        rM[rows, ql[rows]] = f(rsig_own)[rows]
    with np.errstate(invalid="ignore", over="ignore"):
        a = s - f(mu_q)[:, None]
        b = s - mM
        return np.float32(0.5) * (a * f(rsig_q)[:, None] + b * rM)


# ---- the entry points on device tensors --------------------------------------------------------------------------------------------
def speaker_sums(emb: torch.Tensor, label: torch.Tensor, S: int, kind) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``vm_speaker_sums``: (sums (S, E) float64, msum (S) float64, count (S) int32) on the device."""
    lib = _lib.lib()
    kind = _kind(kind)
    emb = emb.contiguous()
    label = label.to(device=emb.device, dtype=torch.int32).contiguous()
    N, E = emb.shape
    dev = emb.device
    sums = torch.zeros(S, E, dtype=torch.float64, device=dev)
    msum = torch.zeros(S, dtype=torch.float64, device=dev)
    count = torch.zeros(S, dtype=torch.int32, device=dev)
    if N > 0:
        ws = lib.workspace("vm_speaker_sums_workspace_bytes", N, E, S, device=dev)
        lib.call("vm_speaker_sums", emb.data_ptr(), label.data_ptr(), N, E, S, kind, sums.data_ptr(), msum.data_ptr(), count.data_ptr(),
                 ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return sums, msum, count


def plda_tables_to(tables, dev) -> Dict[str, torch.Tensor]:
    """``PldaModel.model_tables``' dict as contiguous float64 tensors on ``dev``."""
    return {k: torch.as_tensor(np.ascontiguousarray(np.asarray(tables[k], dtype=np.float64))).to(dev) for k in ("A", "beta", "C", "G")}


def _binding(q, sums, msum, count, kind, tables):
    """What the geometric entry points (``tables`` None) and the multi-session PLDA ones differ in: (the prefix of their names, the
    model arguments that follow M, the (width, S) that follow M in their workspace queries)."""
    E, S = int(q.shape[1]), int(count.shape[0])
    if tables is None:
        return "vm_speaker_", (E, sums.data_ptr(), msum.data_ptr(), count.data_ptr(), S, _kind(kind)), (E, S)
    D, n_max = int(tables["G"].shape[0]), int(tables["C"].shape[0]) - 1
    if int(sums.shape[1]) != E:
        raise ValueError("the sums are %d wide and the rows %d" % (int(sums.shape[1]), E))
    return "vm_plda_speaker_", (E, D, sums.data_ptr(), count.data_ptr(), S) + tuple(tables[k].data_ptr() for k in ("A", "beta", "C", "G")) + (
        n_max,), (D, S)


def _call(binding, name, q, head, tail, ws_tail=()):
    """``<prefix><name>(q, *head, M, <model arguments>, *tail, workspace, stream)``."""
    prefix, model_args, dims = binding
    lib, dev, M = _lib.lib(), q.device, int(q.shape[0])
    ws = lib.workspace(prefix + name + "_workspace_bytes", M, *dims, *ws_tail, device=dev)
    lib.call(prefix + name, q.data_ptr(), *head, M, *model_args, *tail, ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)


def _rows_labels(q: torch.Tensor, q_label: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Contiguous rows and their int32 labels on the rows' device."""
    q = q.contiguous()
    return q, q_label.to(device=q.device, dtype=torch.int32).contiguous()


def _identify_outputs(M: int, S: int, dev, return_scores: bool) -> Dict[str, torch.Tensor]:
    out = {"true_score": torch.empty(M, dtype=torch.float32, device=dev), "rank": torch.empty(M, dtype=torch.int32, device=dev),
           "best_val": torch.empty(M, dtype=torch.float32, device=dev), "best_idx": torch.empty(M, dtype=torch.int32, device=dev)}
    if return_scores:
        out["scores"] = torch.empty(M, S, dtype=torch.float32, device=dev)
    return out


def _hist_windows(windows, bins: int, hist: Optional[torch.Tensor], dev) -> Tuple[torch.Tensor, np.ndarray]:
    """(the (n_windows, 2, bins + 3) int64 counts on ``dev`` -- ``hist`` if one is given --, the windows as the int64 array the entry
    points read)."""
    if hist is None:
        hist = torch.zeros(len(windows), 2, bins + 3, dtype=torch.int64, device=dev)
    return hist, np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1, 2))


def _identify(q, q_label, sums, msum, count, kind, tables, leave_one_out, return_scores=False) -> Dict[str, torch.Tensor]:
    q, q_label = _rows_labels(q, q_label)
    binding = _binding(q, sums, msum, count, kind, tables)
    out = _identify_outputs(int(q.shape[0]), int(count.shape[0]), q.device, return_scores)
    if q.shape[0] > 0:
        _call(binding, "identify", q, (q_label.data_ptr(),), (1 if leave_one_out else 0, out["scores"].data_ptr() if return_scores else None)
              + tuple(out[k].data_ptr() for k in ("true_score", "rank", "best_val", "best_idx")))
    return out


def _trial_hist(q, q_label, sums, msum, count, kind, tables, leave_one_out, windows, bins, stats=None, hist=None) -> torch.Tensor:
    """The plain trial histogram (``stats`` None) or the normalised one of either back end."""
    V.check_windows(windows, bins)   # refused before anything touches the device
    q, q_label = _rows_labels(q, q_label)
    binding = _binding(q, sums, msum, count, kind, tables)
    hist, win = _hist_windows(windows, bins, hist, q.device)
    M, S = int(q.shape[0]), int(count.shape[0])
    if M > 0:
        ptrs = ()
        if stats is not None:
            stats = [None if t is None else t.to(device=q.device, dtype=torch.float32).contiguous() for t in stats]
            for t, n in zip(stats, (M, M, S, S, M, M)):
                if t is not None and int(t.numel()) != n:
                    raise ValueError("a statistics array holds %d entries, not %d" % (int(t.numel()), n))
            ptrs = tuple(None if t is None else t.data_ptr() for t in stats)
        _call(binding, "trial_hist" if stats is None else "trial_hist_norm", q, (q_label.data_ptr(),),
              (1 if leave_one_out else 0, win.ctypes.data, len(windows), bins) + ptrs + (hist.data_ptr(),))
    return hist


def speaker_identify(q: torch.Tensor, q_label: torch.Tensor, sums, msum, count, kind, leave_one_out: bool,
                     return_scores: bool = False) -> Dict[str, torch.Tensor]:
    """``vm_speaker_identify``: ``true_score``, ``rank``, ``best_val``, ``best_idx`` (M) and, with ``return_scores``, ``scores`` (M, S)
    (NaN where there is no trial)."""
    return _identify(q, q_label, sums, msum, count, kind, None, leave_one_out, return_scores)


def plda_speaker_identify(q: torch.Tensor, q_label: torch.Tensor, sums, count, tables, leave_one_out: bool,
                          return_scores: bool = False) -> Dict[str, torch.Tensor]:
    """``vm_plda_speaker_identify``: the outputs of ``speaker_identify`` for PLDA-space rows ``q`` (M, P) against the models of ``sums``
    (S, P) float64 / ``count`` (``speaker_sums`` of the enrolled PLDA-space rows, euclidean kind); ``tables``: ``plda_tables_to``'s."""
    return _identify(q, q_label, sums, None, count, None, tables, leave_one_out, return_scores)


def speaker_trial_hist(q: torch.Tensor, q_label: torch.Tensor, sums, msum, count, kind, leave_one_out: bool,
                       windows: Sequence[Tuple[int, int]], bins: int, hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``vm_speaker_trial_hist``: (n_windows, 2, bins + 3) int64 counts on the device (class 0 = the own speaker's model), added to
    ``hist`` if one is given."""
    return _trial_hist(q, q_label, sums, msum, count, kind, None, leave_one_out, windows, bins, hist=hist)


def plda_speaker_trial_hist(q: torch.Tensor, q_label: torch.Tensor, sums, count, tables, leave_one_out: bool,
                            windows: Sequence[Tuple[int, int]], bins: int, hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``vm_plda_speaker_trial_hist``: ``speaker_trial_hist`` with the multi-session PLDA score."""
    return _trial_hist(q, q_label, sums, None, count, None, tables, leave_one_out, windows, bins, hist=hist)


def speaker_trial_hist_norm(q: torch.Tensor, q_label: torch.Tensor, sums, msum, count, kind, leave_one_out: bool,
                            windows: Sequence[Tuple[int, int]], bins: int, stats: Sequence[Optional[torch.Tensor]], tables=None,
                            hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``vm_speaker_trial_hist_norm`` (``tables``: ``vm_plda_speaker_trial_hist_norm``): ``speaker_trial_hist`` on the normalised scores.
    ``stats``: (mu_q, rsig_q (M), mu_s, rsig_s (S), mu_own, rsig_own (M) or None, None), fp32 on the device."""
    return _trial_hist(q, q_label, sums, msum, count, kind, tables, leave_one_out, windows, bins, stats, hist)


def speaker_loo_sums(q: torch.Tensor, q_label: torch.Tensor, sums, msum, count, kind) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``vm_speaker_loo_sums``: the virtual models (sums (M, E) / msum (M) float64, count (M) int32) of the rows ``q``."""
    lib = _lib.lib()
    kind = _kind(kind)
    q, q_label = _rows_labels(q, q_label)
    dev = q.device
    M, E = q.shape
    vs = torch.zeros(M, E, dtype=torch.float64, device=dev)
    vm = torch.zeros(M, dtype=torch.float64, device=dev)
    vc = torch.zeros(M, dtype=torch.int32, device=dev)
    if M > 0:
        ws = lib.workspace("vm_speaker_loo_sums_workspace_bytes", M, E, device=dev)
        lib.call("vm_speaker_loo_sums", q.data_ptr(), q_label.data_ptr(), M, E, sums.data_ptr(), msum.data_ptr(), count.data_ptr(),
                 int(count.shape[0]), kind, vs.data_ptr(), vm.data_ptr(), vc.data_ptr(), ws.data_ptr(),
                 torch.cuda.current_stream(dev).cuda_stream)
    return vs, vm, vc


def speaker_cohort_stats(q: torch.Tensor, sums, msum, count, kind, side: int, K: int, tables=None,
                         return_topk: bool = False) -> Dict[str, torch.Tensor]:
    """``vm_speaker_cohort_stats`` (``tables``: ``vm_plda_speaker_cohort_stats``): ``mu``, ``sigma``, ``rsig`` (fp32), ``count`` (int32)
    and, with ``return_topk``, ``topk_idx`` (lines, K) of the scores of the rows ``q`` against the models -- per row over the models
    (``side`` 0) or per model over the rows (``side`` 1)."""
    q = q.contiguous()
    dev = q.device
    binding = _binding(q, sums, msum, count, kind, tables)
    n = int(count.shape[0]) if side == 1 else int(q.shape[0])
    out = {k: torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for k in ("mu", "sigma", "rsig")}
    out["count"] = torch.zeros(n, dtype=torch.int32, device=dev)
    if return_topk:
        out["topk_idx"] = torch.full((n, K), -1, dtype=torch.int32, device=dev)
    _call(binding, "cohort_stats", q, (), (side, K) + tuple(out[k].data_ptr() for k in ("mu", "sigma", "rsig", "count"))
          + (out["topk_idx"].data_ptr() if return_topk else None,), ws_tail=(side,))
    return out


# ---- speaker models of an EmbeddingCache -------------------------------------------------------------------------------------------
class SpeakerModels:
    """The enrolled speakers of a cache: ``sums`` (S, E) / ``msum`` (S) float64 and ``count`` (S) int32 on the device, the ``distance``
    they were summed for, ``speakers`` (dense index -> the cache's speaker code), ``label`` (N) int32 (the dense index of every enrolled
    row of the cache, -1 for the rows left out by ``per_speaker``) and the ``cache`` itself.  Multi-session PLDA models (``distance``
    "plda") also hold the ``plda`` model and its ``tables`` (float64, on the device) for 1 .. ``n_max`` = the largest count rows."""

    def __init__(self, sums, msum, count, distance, speakers, label, cache, per_speaker, plda=None, tables=None):
        self.sums, self.msum, self.count = sums, msum, count
        self.distance, self.speakers, self.label, self.cache, self.per_speaker = distance, speakers, label, cache, per_speaker
        self.plda, self.tables = plda, tables

    @property
    def n_max(self) -> Optional[int]:
        return None if self.tables is None else int(self.tables["C"].shape[0]) - 1

    @property
    def S(self) -> int:
        return int(self.count.shape[0])

    @property
    def backend(self) -> Tuple:
        """(sums, msum, count, kind, tables) as the entry points above take them: the one place that knows which back end scores
        these models (the sums of PLDA models are of the euclidean kind)."""
        return self.sums, self.msum, self.count, _lib.VM_DIST_EUCLIDEAN if self.tables is not None else _kind(self.distance), self.tables

    def labels_of(self, speaker_codes) -> np.ndarray:
        """Dense indices of speaker codes (-1: the speaker is not enrolled)."""
        codes = np.asarray(speaker_codes)
        pos = np.clip(np.searchsorted(self.speakers, codes), 0, len(self.speakers) - 1)
        return np.where(self.speakers[pos] == codes, pos, -1).astype(np.int32)


def enrol(cache, distance: Optional[str] = None, per_speaker: Optional[int] = None, seed: int = 0, plda=None) -> SpeakerModels:
    """Enrol the speakers of ``cache`` (dense labels from ``np.unique(cache.speaker)``).  ``per_speaker=n``: a seeded choice of n rows of
    every speaker is enrolled (a speaker with fewer than n + 1 rows enrols all but one) and the other rows are the queries of
    ``identify`` / ``model_trial_metrics`` -- the exhaustive n-shot S-way task.  Every rank sums all rows itself.  ``distance``
    defaults to "euclidean".  ``plda=model`` (a ``plda.PldaModel``): multi-session PLDA models of a cache that ``model.project`` made
    (module docstring); ``distance`` is then left out.  A cache whose width is not ``model.P`` -- a raw, unprojected one -- is refused."""
    if plda is not None:
        if distance not in (None, "plda"):
            raise ValueError("plda= is the switch: leave distance out (got %r)" % (distance,))
        if cache.emb.dim() != 2 or int(cache.emb.shape[1]) != plda.P:
            raise ValueError("enrol(plda=) takes a cache projected by the model -- rows of width %d, got %d: pass model.project(cache)"
                             % (plda.P, int(cache.emb.shape[-1])))
        kind = _lib.VM_DIST_EUCLIDEAN   # the sums of the projected rows themselves
    else:
        distance = "euclidean" if distance is None else distance
        kind = _kind(distance)
    speakers, dense = np.unique(cache.speaker, return_inverse=True)
    label = dense.astype(np.int32).reshape(-1)
    if per_speaker is not None:
        if per_speaker < 1:
            raise ValueError("per_speaker must be >= 1 (or None: every row)")
        rng = np.random.default_rng(seed)
        keep = np.zeros(len(label), dtype=bool)
        order = np.argsort(label, kind="stable")
        bounds = np.searchsorted(label[order], np.arange(len(speakers) + 1))
        for s in range(len(speakers)):
            rows = order[bounds[s]:bounds[s + 1]]
            take = min(int(per_speaker), len(rows) - 1)
            if take > 0:
                keep[rng.choice(rows, take, replace=False)] = True
        label = np.where(keep, label, -1).astype(np.int32)
    sums, msum, count = speaker_sums(cache.emb, torch.as_tensor(label), len(speakers), kind)
    if plda is not None:
        n_max = max(1, int(count.max().item()))
        return SpeakerModels(sums, msum, count, "plda", speakers, label, cache, per_speaker, plda=plda,
                             tables=plda_tables_to(plda.model_tables(n_max), cache.emb.device))
    return SpeakerModels(sums, msum, count, distance, speakers, label, cache, per_speaker)


def _queries(models: SpeakerModels, cache, leave_one_out: Optional[bool]):
    """(query row indices of ``cache`` or None for all rows, their dense labels, leave_one_out)."""
    same = cache is models.cache
    if leave_one_out is None:
        leave_one_out = same and models.per_speaker is None
    if leave_one_out and not (same and models.per_speaker is None):
        raise ValueError("leave_one_out needs the cache that was enrolled whole (per_speaker=None)")
    q_label = models.labels_of(cache.speaker)
    if same and models.per_speaker is not None:
        idx = np.flatnonzero(models.label < 0)
        return idx, q_label[idx], False
    return None, q_label, bool(leave_one_out)


def _shard(models, cache, leave_one_out, rows):
    idx, q_label, loo = _queries(models, cache, leave_one_out)
    n_q = len(q_label)
    rank, world = parallel.rank_world()
    lo, hi = rows if rows is not None else parallel.shard_range(n_q, rank, world)
    dev = cache.emb.device
    if idx is None:
        q = cache.emb[lo:hi]
    else:
        q = cache.emb[torch.as_tensor(idx[lo:hi], dtype=torch.int64, device=dev)]
    return q.contiguous(), torch.as_tensor(q_label[lo:hi]).to(dev), loo, (lo, hi), n_q, idx


def identify(models: SpeakerModels, cache, leave_one_out: Optional[bool] = None, rows: Optional[Tuple[int, int]] = None) -> Dict:
    """S-way identification of the rows of ``cache`` against ``models``: ``rank1_accuracy``, ``cmc`` (float64, ``cmc[k - 1]`` = the share
    of ranked queries with rank < k, k = 1..S), ``mean_reciprocal_rank``, ``n_queries``, ``n_unranked`` (queries without an enrolled own
    speaker or without a model of it), and of this rank's rows (``rows`` = [lo, hi) of the queries; ``query_index``: their rows in the
    cache) ``rank``, ``pred`` (the best speaker's code; the own code's dtype, -1 / "" where there is no trial) and ``true_score``.
    ``leave_one_out`` defaults to "the cache is the one that was enrolled and per_speaker is None".  With ``per_speaker`` models and
    the enrolled cache, the queries are the rows that were not enrolled.  The ranking is by the raw score: ranking by the normalised
    score of ``model_score_norm`` is out of scope."""
    q, q_label, loo, (lo, hi), n_q, idx = _shard(models, cache, leave_one_out, rows)
    out = _identify(q, q_label, *models.backend, loo)
    S = models.S
    rk = out["rank"].long()
    hist = torch.bincount(torch.where(rk < 0, torch.full_like(rk, S), rk), minlength=S + 1)[:S + 1]
    hist = (parallel.sum_ranks(hist) if rows is None else hist).cpu().numpy().astype(np.int64)
    n_ranked = int(hist[:S].sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        cmc = np.cumsum(hist[:S]).astype(np.float64) / n_ranked
        mrr = float((hist[:S] / np.arange(1, S + 1)).sum() / n_ranked) if n_ranked else float("nan")
    bi = out["best_idx"].cpu().numpy()
    pred = np.where(bi >= 0, models.speakers[np.clip(bi, 0, S - 1)], "" if models.speakers.dtype.kind in "US" else -1)
    return {"rank1_accuracy": float(cmc[0]) if n_ranked else float("nan"), "cmc": cmc, "mean_reciprocal_rank": mrr,
            "n_queries": int(hist.sum()), "n_unranked": int(hist[S]), "rank_histogram": hist, "rows": (lo, hi),
            "query_index": np.arange(lo, hi) if idx is None else idx[lo:hi], "rank": out["rank"].cpu().numpy(), "pred": pred,
            "true_score": out["true_score"].cpu().numpy(), "leave_one_out": loo}


def _prototypes(models: SpeakerModels) -> torch.Tensor:
    """The shared models (S, E) in float64 (torch arithmetic: only the pass-1 window depends on them)."""
    n = models.count.double().clamp_min(1.0)
    p = models.sums / n[:, None]
    if _kind(models.distance) == 2:
        p = (models.msum / n)[:, None] * p
    return p


class _Side:
    """One side's (mu, rsig) as ``verification.norm_bounds`` reads them."""

    def __init__(self, mu, rsig):
        self.mu, self.rsig = mu, rsig


def _normalised_sample(stats, lo, hi, sc=None, i=None, s=None):
    """A pass-1 sample (bounds lo / hi, float64 scores ``sc`` of the (row i, model s) pairs) after normalisation with ``stats`` (the six
    arrays of ``speaker_trial_hist_norm``, the per-row ones of the rows sampled from; None: as it is).  The sample is normalised in
    float64; each half (s - mu) rsig lies within ``verification.norm_bounds`` of its side (the own statistics count as the model
    side's), and s' is the mean of the two halves.  Only the window's place depends on any of it."""
    if stats is None:
        return lo, hi, sc
    mq, rq, ms, rs, mo, ro = stats
    l1, h1 = V.norm_bounds(_Side(mq, rq), lo, hi)
    l2, h2 = V.norm_bounds(_Side(ms if mo is None else torch.cat([ms, mo]), rs if ro is None else torch.cat([rs, ro])), lo, hi)
    if sc is not None:
        sc = 0.5 * ((sc - mq.double()[i]) * rq.double()[i] + (sc - ms.double()[s]) * rs.double()[s])
    return 0.5 * (l1 + l2), 0.5 * (h1 + h2), sc


def _geometric_sampler(models: SpeakerModels, q: torch.Tensor):
    """(lo, hi, ok, score) of the geometric kinds for ``_pass1``: bounds from the largest row and model norms, the models that exist, and
    ``score(i, s)``: the float64 scores of (row, model) index pairs."""
    kind = _kind(models.distance)
    P = _prototypes(models)
    ok = models.count > 0
    pr = float(torch.linalg.vector_norm(P[ok], dim=1).max().item()) if bool(ok.any()) else 0.0
    qr = float(torch.linalg.vector_norm(q.double(), dim=1).max().item()) if q.shape[0] else 0.0
    pr, qr = (x if math.isfinite(x) else 1.0 for x in (pr, qr))
    if kind == 1:
        lo, hi = 0.0, 2.0
    elif kind == 0:
        lo, hi = 0.0, (pr + qr) * 1.001 + 1e-30
    else:
        lo, hi = -pr * qr * 1.001 - 1e-30, pr * qr * 1.001 + 1e-30
    return lo, hi, ok, lambda i, s: V.sample_scores(q[i], P[s], kind)


def _plda_sampler(models: SpeakerModels, q: torch.Tensor):
    """``_geometric_sampler`` for multi-session PLDA models: the shared models' operands in torch float64 (mu = beta[n] Sigma, A[n],
    C[n]) and bounds from the largest terms -- the score is sum A (w - mu)^2 - g - C with g = sum G w^2 >= 0."""
    t, D = models.tables, int(models.tables["G"].shape[0])
    n = models.count.long()
    ok = (n >= 1) & (n <= models.n_max)
    n = torch.where(ok, n, torch.zeros_like(n))
    mu, A, C = t["beta"][n] * models.sums[:, :D], t["A"][n], t["C"][n]
    w = q[:, :D].double()
    g = (w * w) @ t["G"]
    fin = lambda x: x if math.isfinite(x) else 1.0
    qr = fin(float(torch.linalg.vector_norm(w, dim=1).max().item())) if q.shape[0] else 0.0
    mr = fin(float(torch.linalg.vector_norm(mu[ok], dim=1).max().item())) if bool(ok.any()) else 0.0
    cm = fin(float(C.abs().max().item()))
    gm = fin(float(g.abs().max().item())) if q.shape[0] else 0.0
    lo = -(gm + cm) * 1.001 - 1e-30
    hi = (fin(float(A.max().item())) * (qr + mr) ** 2 + gm + cm) * 1.001 + 1e-30

    def score(i, s):
        d = w[i] - mu[s]
        return ((A[s] * d * d).sum(1) - g[i]) - C[s]
    return lo, hi, ok, score


def _pass1(models: SpeakerModels, q: torch.Tensor, n_sample: int = 1 << 16, stats=None) -> Tuple[int, int]:
    """``verification.place_window`` for the model trials of rank 0's rows ``q``: the back end's bounds and a seeded sample of (row,
    model) pairs, those of a speaker without a model left out.  ``stats``: the window of the normalised scores
    (``_normalised_sample``).  Only the window's place depends on any of it."""
    sampler = _geometric_sampler if models.tables is None else _plda_sampler

    def sample():
        lo, hi, ok, score = sampler(models, q)
        if q.shape[0] < 1 or not bool(ok.any()):
            return _normalised_sample(stats, lo, hi)
        g = torch.Generator().manual_seed(0)
        i = torch.randint(0, q.shape[0], (n_sample,), generator=g).to(q.device)
        s = torch.randint(0, models.S, (n_sample,), generator=g).to(q.device)
        sc = score(i, s).masked_fill(~ok[s], float("nan"))   # no model: no trial, dropped as not finite
        return _normalised_sample(stats, lo, hi, sc, i, s)
    return V.place_window(sample)


class ModelScoreNorm:
    """The statistics of ``model_score_norm``: ``mu_q`` / ``rsig_q`` (and ``sigma_q``, ``count_q``) per query row, ``mu_s`` / ``rsig_s``
    (``sigma_s``, ``count_s``) per enrolled model, ``mu_own`` / ``rsig_own`` (``sigma_own``, ``count_own``) per query row under
    leave-one-out (else None) -- fp32 / int32 on the device, every rank holding all of them -- with ``top_k`` (None: S-norm), the
    cohort's sizes ``cohort_rows`` and ``cohort_models``, the ``distance`` of the models and the ``leave_one_out`` flag they were
    computed for."""

    def __init__(self, stats, top_k, cohort_rows, cohort_models, distance, leave_one_out):
        for side in ("q", "s", "own"):
            for k in ("mu", "sigma", "rsig", "count"):
                setattr(self, k + "_" + side, stats.get(k + "_" + side))
        self.top_k, self.cohort_rows, self.cohort_models = top_k, cohort_rows, cohort_models
        self.distance, self.leave_one_out = distance, leave_one_out

    @property
    def n_queries(self) -> int:
        return int(self.mu_q.shape[0])

    @property
    def S(self) -> int:
        return int(self.mu_s.shape[0])

    def stats(self, lo: int = 0, hi: Optional[int] = None):
        """The six arrays of ``speaker_trial_hist_norm`` for the query rows [lo, hi)."""
        cut = lambda t: None if t is None else t[lo:hi].contiguous()
        return (cut(self.mu_q), cut(self.rsig_q), self.mu_s, self.rsig_s, cut(self.mu_own), cut(self.rsig_own))


LOO_CHUNK_BYTES = 64 << 20   # the float64 sums of the virtual models of one chunk of rows


def model_score_norm(models: SpeakerModels, cache, cohort, top_k: Optional[int] = 300, leave_one_out: Optional[bool] = None) -> ModelScoreNorm:
    """The S-norm (``top_k=None``: the whole cohort) or AS-norm (the ``top_k`` most alike, per side ``min(top_k, size)``) statistics of
    the model trials of ``cache`` against ``models`` (module docstring).  ``cohort``: an ``EmbeddingCache`` that is neither ``cache`` nor
    ``models.cache`` (for PLDA models: projected by the same model).  Queries and ``leave_one_out`` resolve as in ``identify``.  Under
    torchrun the per-row statistics are computed on each rank's ``parallel.shard_range`` and all-gathered; the per-model ones on every
    rank.  The virtual models of the own side are formed ``LOO_CHUNK_BYTES`` of float64 sums at a time."""
    if cohort is cache or cohort is models.cache or not hasattr(cohort, "emb"):
        raise ValueError("the cohort must be an EmbeddingCache of its own: neither the query cache nor the enrolled one")
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be >= 1 (or None for S-norm)")
    if cohort.emb.dim() != 2 or cohort.n < 1 or int(cohort.emb.shape[1]) != int(models.sums.shape[1]):
        raise ValueError("the cohort must be a non-empty cache of rows %d wide" % int(models.sums.shape[1]))
    cm = enrol(cohort, distance=models.distance, plda=models.plda)   # PLDA models carry distance "plda", which enrol(plda=) accepts
    sums, msum, count, kind, tables = models.backend
    q, q_label, loo, (lo, hi), n_q, _ = _shard(models, cache, leave_one_out, None)
    ce = cohort.emb.to(device=q.device, dtype=torch.float32).contiguous()
    C, Sc = int(ce.shape[0]), cm.S
    Kq = Sc if top_k is None else min(int(top_k), Sc)
    Ks = C if top_k is None else min(int(top_k), C)
    names = ("mu", "sigma", "rsig", "count")
    sq = speaker_cohort_stats(q, cm.sums, cm.msum, cm.count, kind, 0, Kq, tables=cm.tables)
    ss = speaker_cohort_stats(ce, sums, msum, count, kind, 1, Ks, tables=tables)
    rows = [sq[k] for k in names]
    if loo:
        M, E = q.shape
        own = {k: torch.full((M,), float("nan"), dtype=torch.float32, device=q.device) for k in names[:3]}
        own["count"] = torch.zeros(M, dtype=torch.int32, device=q.device)
        step = max(1, LOO_CHUNK_BYTES // (8 * int(E)))
        for r0 in range(0, M, step):
            vs, vm, vc = speaker_loo_sums(q[r0:r0 + step], q_label[r0:r0 + step], sums, msum, count, kind)
            so = speaker_cohort_stats(ce, vs, vm, vc, kind, 1, Ks, tables=tables)
            for k in names:
                own[k][r0:r0 + step] = so[k]
        rows += [own[k] for k in names]
    if parallel.rank_world()[1] > 1:
        allr = parallel.all_gather_rows(torch.stack([t.double() for t in rows], 1), n_q)
        rows = [allr[:, k].to(torch.int32 if k % 4 == 3 else torch.float32).contiguous() for k in range(len(rows))]
    stats = {k + "_q": t for k, t in zip(names, rows[:4])}
    stats.update({k + "_s": ss[k] for k in names})
    stats.update({k + "_own": t for k, t in zip(names, rows[4:])} if loo else {})
    return ModelScoreNorm(stats, top_k, C, Sc, models.distance, loo)


def check_model_norm(models, n_q: int, loo: bool, norm: Optional[ModelScoreNorm]):
    """``verification.check_norm`` for model trials: the statistics must have been computed for these models, queries and leave-one-out."""
    if norm is None:
        return
    if norm.distance != models.distance:
        raise ValueError("the ModelScoreNorm was computed for %r models, not %r" % (norm.distance, models.distance))
    if norm.S != models.S or norm.n_queries != n_q:
        raise ValueError("the ModelScoreNorm holds %d models and %d query rows, the trials %d and %d" % (norm.S, norm.n_queries, models.S, n_q))
    if bool(norm.leave_one_out) != bool(loo):
        raise ValueError("the ModelScoreNorm was computed with leave_one_out=%r, the trials have %r" % (norm.leave_one_out, loo))


def _hist_source(models, cache, leave_one_out, norm=None):
    q, q_label, loo, (lo, hi), n_q, _ = _shard(models, cache, leave_one_out, None)
    check_model_norm(models, n_q, loo, norm)
    stats = None if norm is None else norm.stats(lo, hi)

    def hist_fn(windows, bins):
        return parallel.sum_ranks(_trial_hist(q, q_label, *models.backend, loo, windows, bins, stats)).cpu().numpy()
    return hist_fn, q, stats


def model_trial_metrics(models: SpeakerModels, cache, leave_one_out: Optional[bool] = None, dcf_points=(),
                        norm: Optional[ModelScoreNorm] = None) -> Dict:
    """Exact verification metrics of the trials (row of ``cache``, speaker model): the dict of ``verification.exact_sweep`` (``eer``,
    ``eer_threshold``, ``best_balanced_accuracy``, ``best_threshold``, FAR / FRR at both, ``auc``, ``roc``, ``n_target``,
    ``n_nontarget``, ``n_nan``, ``passes``).  A trial is a target iff the model is the row's own speaker; queries and
    ``leave_one_out`` as in ``identify``.  ``dcf_points``: detection-cost points (P_target, C_miss, C_fa), adding ``dcf`` as in
    ``verification.exact_sweep``.  ``norm`` (``model_score_norm`` of the same models, cache and leave-one-out): the metrics of the
    normalised scores; the thresholds are then in normalised units."""
    hist_fn, q, stats = _hist_source(models, cache, leave_one_out, norm)
    return V.exact_sweep(hist_fn, _pass1(models, q, stats=stats), dcf_points=dcf_points)


def model_trial_accuracy_at_threshold(models: SpeakerModels, cache, t: float, leave_one_out: Optional[bool] = None,
                                      norm: Optional[ModelScoreNorm] = None) -> Dict:
    """Balanced accuracy, FAR and FRR of the model trials at a fixed threshold t (accept iff score < t; with ``norm`` in normalised
    units): one pass with key_lo = key(t), whose under slot is exactly {s < t} -- a threshold found on a validation set applied to a
    test set."""
    hist_fn, _, _ = _hist_source(models, cache, leave_one_out, norm)
    return V.counts_at_threshold(hist_fn, t)


# ---- calibration of model trials ---------------------------------------------------------------------------------------------------
def model_calib_sums_numpy(scores, trial, q_label, a: float, b: float, tau: float) -> np.ndarray:
    """numpy twin of ``vm_[plda_]speaker_trial_calib_sums`` on an (M, S) fp32 score matrix and its trial mask: ``calibration.
    calib_sums_numpy`` over the cells where ``trial`` is set, a target iff the column is the row's ``q_label``."""
    s = np.asarray(scores, dtype=np.float32)
    trial = np.asarray(trial, dtype=bool)
    target = np.arange(s.shape[1])[None, :] == np.asarray(q_label).reshape(-1, 1)
    return CAL.calib_sums_numpy(s[trial], target[trial], a, b, tau)


def _trial_calib_sums(q, q_label, sums, msum, count, kind, tables, leave_one_out, a, b, tau, stats=None) -> torch.Tensor:
    """One pass of ``vm_speaker_trial_calib_sums`` / ``vm_plda_speaker_trial_calib_sums`` (``tables``): the (2, 8) float64 sums on the
    device.  ``stats``: the six arrays of ``speaker_trial_hist_norm`` (the normalised scores) or None (the raw ones)."""
    q, q_label = _rows_labels(q, q_label)
    binding = _binding(q, sums, msum, count, kind, tables)
    out = torch.zeros(2, 8, dtype=torch.float64, device=q.device)
    M, S = int(q.shape[0]), int(count.shape[0])
    if M > 0:
        ptrs = (None,) * 6
        if stats is not None:
            stats = [None if t is None else t.to(device=q.device, dtype=torch.float32).contiguous() for t in stats]
            for t, n in zip(stats, (M, M, S, S, M, M)):
                if t is not None and int(t.numel()) != n:
                    raise ValueError("a statistics array holds %d entries, not %d" % (int(t.numel()), n))
            ptrs = tuple(None if t is None else t.data_ptr() for t in stats)
        _call(binding, "trial_calib_sums", q, (q_label.data_ptr(),),
              (1 if leave_one_out else 0,) + ptrs + (float(a), float(b), float(tau), out.data_ptr()))
    return out


def speaker_trial_calib_sums(q: torch.Tensor, q_label: torch.Tensor, sums, msum, count, kind, leave_one_out: bool, a: float, b: float,
                             tau: float, stats: Optional[Sequence[Optional[torch.Tensor]]] = None, tables=None) -> torch.Tensor:
    """``vm_speaker_trial_calib_sums`` (``tables``: ``vm_plda_speaker_trial_calib_sums``): the (2, 8) float64 calibration sums
    (``calibration.SUM_NAMES``; class 0 = the own speaker's model) of the trials of ``speaker_trial_hist`` at (a, b, tau), on the
    device.  ``stats``: as ``speaker_trial_hist_norm`` takes them, for the normalised scores."""
    return _trial_calib_sums(q, q_label, sums, msum, count, kind, tables, leave_one_out, a, b, tau, stats)


def _calib_source(models, cache, leave_one_out, norm, rows=None):
    """``sums_fn(a, b, tau)`` -> (2, 8) numpy over the model trials: ``_hist_source``'s queries, leave-one-out and sharding.  ``rows``
    given: that range of the queries alone, no communication; otherwise this rank's shard, summed over the ranks."""
    q, q_label, loo, (lo, hi), n_q, _ = _shard(models, cache, leave_one_out, rows)
    check_model_norm(models, n_q, loo, norm)
    stats = None if norm is None else norm.stats(lo, hi)

    def sums_fn(a, b, tau):
        out = _trial_calib_sums(q, q_label, *models.backend, loo, a, b, tau, stats)
        return (out if rows is not None else parallel.sum_ranks(out)).cpu().numpy()
    return sums_fn


def model_calib_sums(models: SpeakerModels, cache, a: float, b: float, tau: float, leave_one_out: Optional[bool] = None,
                     norm: Optional[ModelScoreNorm] = None, rows: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """The (2, 8) float64 sums (``calibration.SUM_NAMES``; class 0 = target) of the model trials of ``cache`` against ``models`` at
    (a, b, tau): one pass of ``vm_[plda_]speaker_trial_calib_sums``.  Queries and ``leave_one_out`` as in ``identify``.  ``rows``: only
    the queries [lo, hi); by default this rank's ``parallel.shard_range``, and under torchrun the sums of all ranks are added.
    ``norm``: on the normalised scores (``model_score_norm`` of the same models, cache and leave-one-out)."""
    return _calib_source(models, cache, leave_one_out, norm, rows)(a, b, tau)


def fit_model_calibration(models: SpeakerModels, cache, prior: float = 0.5, leave_one_out: Optional[bool] = None,
                          norm: Optional[ModelScoreNorm] = None, max_iter: int = 50) -> CAL.Calibration:
    """``calibration.fit_calibration`` on the model trials of ``cache`` against ``models``: the same objective, starting point, Newton
    steps and stopping rule, one ``vm_[plda_]speaker_trial_calib_sums`` pass per evaluation.  The result carries ``score =
    models.distance``, ``normalised = norm is not None`` and ``trials = "model"``."""
    return CAL._fit(_calib_source(models, cache, leave_one_out, norm), prior, models.distance, norm is not None, max_iter, "model")


def _check_model_calibration(models, calibration, norm):
    if calibration.trials != "model":
        raise ValueError("the calibration was fitted on %s trials, not model trials" % calibration.trials)
    if calibration.score != models.distance:
        raise ValueError("the calibration was fitted on %r scores, the models score %r" % (calibration.score, models.distance))
    if (norm is not None) != bool(calibration.normalised):
        raise ValueError("the calibration was fitted on %s scores" % ("normalised" if calibration.normalised else "raw"))


def model_cllr(models: SpeakerModels, cache, calibration, leave_one_out: Optional[bool] = None,
               norm: Optional[ModelScoreNorm] = None) -> float:
    """Cllr of the calibrated scores of the model trials of ``cache`` (one pass at tau = 0): 0 is perfect, 1 is what a = b = 0 gives.
    ``calibration``: fitted by ``fit_model_calibration`` for the same score, raw or normalised as here."""
    _check_model_calibration(models, calibration, norm)
    return CAL.cllr_of(model_calib_sums(models, cache, calibration.a, calibration.b, 0.0, leave_one_out, norm))


def model_detection_costs(models: SpeakerModels, cache, calibration, points, leave_one_out: Optional[bool] = None,
                          norm: Optional[ModelScoreNorm] = None, metrics: Optional[Dict] = None) -> list:
    """``verification.detection_costs`` for model trials.  Per point (P_target, C_miss, C_fa): the entry of ``model_trial_metrics``'s
    ``dcf`` (``min_dcf`` and where it is reached) plus ``act_dcf``, the cost at the calibration's Bayes threshold ``act_threshold``
    (``verification.bayes_threshold``, in score units) counted by ``model_trial_accuracy_at_threshold``, with ``far_at_act`` /
    ``frr_at_act``.  ``calibration``: fitted (on other data) by ``fit_model_calibration`` for the same score, raw or normalised as here.
    ``metrics``: the result of ``model_trial_metrics(..., dcf_points=points)`` where it has been computed already."""
    _check_model_calibration(models, calibration, norm)
    points = V.as_dcf_points(points)
    ts = [V.bayes_threshold(calibration, pt) for pt in points]   # raises before any pass
    if metrics is None:
        metrics = model_trial_metrics(models, cache, leave_one_out, dcf_points=points, norm=norm)
    out = [dict(d) for d in metrics["dcf"]]
    if [(d["p_target"], d["c_miss"], d["c_fa"]) for d in out] != points:
        raise ValueError("``metrics`` was computed for other detection-cost points")
    for d, pt, t in zip(out, points, ts):
        at = model_trial_accuracy_at_threshold(models, cache, t, leave_one_out, norm=norm)
        d.update(act_dcf=V.dcf_value(pt, at["far"], at["frr"]), act_threshold=t, far_at_act=at["far"], frr_at_act=at["frr"])
    return out
