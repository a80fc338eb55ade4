"""Score calibration for all-pairs speaker verification: an affine map llr = a s + b of the scores (distances, or S-norm units) to
log-likelihood ratios, fitted by prior-weighted logistic regression on the trials of one ``EmbeddingCache`` (the validation set) and
judged on another (the test set) by Cllr and -- ``verification.detection_costs`` -- by the detection cost at the Bayes threshold.

The trials are ``verification``'s: all unordered pairs {i, j}, i < j, a target iff both rows have the same speaker, s the fp32 score
of ``vm_pair_score_hist`` (lower = more alike), or its cohort-normalised form with ``norm=``.  A trial whose s is NaN or infinite is
skipped and counted.  Nothing is stored per trial: every Newton iteration is one pass of ``vm_pair_calib_sums`` (csrc/calib.hip),
which recomputes the scores and reduces, per class c (0 = target, 1 = non-target), eight float64 sums in a fixed order:

    z = a s + b + tau;  t = -z (target) or +z (non-target);  e = exp(-|t|)
    loss = max(t, 0) + log1p(e);  p = 1 / (1 + e) if t >= 0 else e / (1 + e);  w = e / (1 + e)^2
    n, n_skipped, L = sum loss, P0 = sum p, P1 = sum p s, W0 = sum w, W1 = sum w s, W2 = sum (w s) s        (``SUM_NAMES``)

loss is softplus(t), p its derivative sigmoid(t), w the second derivative -- the form e / (1 + e)^2 does not cancel as p (1 - p) does.
With the prior pi and tau = logit(pi):

    C(a, b) = pi / nT L_0 + (1 - pi) / nN L_1                       (nT = n_0, nN = n_1)
    g_a = -pi / nT P1_0 + (1 - pi) / nN P1_1,   g_b likewise with P0
    H   = pi / nT [[W2_0, W1_0], [W1_0, W0_0]] + (1 - pi) / nN [[W2_1, W1_1], [W1_1, W0_1]]
    Cllr = (L_0 / nT + L_1 / nN) / (2 ln 2)  at tau = 0  (1 at a = b = 0: scores that say nothing)

``calib_sums_numpy`` / ``fit_calibration_numpy`` state the same on score arrays (the tests hold the kernel to them).  Under torchrun
every rank takes its ``verification.triangle_shards`` rows and the (2, 8) sums are all-reduced, so every rank takes the same steps.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import verification as V

SUM_NAMES = ("n", "n_skipped", "L", "P0", "P1", "W0", "W1", "W2")
# fit_calibration stops when the squared Newton decrement g' H^-1 g falls to NEWTON_STOP^2 C(a, b): relative to the objective, because
# on separable trials the decrement shrinks WITH the objective (both go to 0 as |a| grows) and an absolute rule would call that converged
NEWTON_STOP = 1e-9
LN2 = math.log(2.0)


def logit(p: float) -> float:
    return math.log(p) - math.log1p(-p)


# ---- the sums ----------------------------------------------------------------------------------------------------------------------
def calib_sums_numpy(scores, target, a: float, b: float, tau: float) -> np.ndarray:
    """numpy twin of ``vm_pair_calib_sums`` on an array of fp32 scores and its target mask: the (2, 8) float64 sums of the module
    docstring, every per-trial operation in float64 as stated (the order of the sums is numpy's)."""
    s32 = np.asarray(scores, dtype=np.float32).ravel()
    tg = np.asarray(target, dtype=bool).ravel()
    fin = np.isfinite(s32)
    out = np.zeros((2, 8), dtype=np.float64)
    a, b, tau = np.float64(a), np.float64(b), np.float64(tau)
    for c, cls in enumerate((tg, ~tg)):
        s = s32[cls & fin].astype(np.float64)
        z = a * s + b + tau
        t = -z if c == 0 else z
        e = np.exp(-np.abs(t))
        d = 1.0 + e
        w = e / (d * d)
        p = np.where(t >= 0.0, 1.0 / d, e / d)
        loss = np.maximum(t, 0.0) + np.log1p(e)
        out[c] = (len(s), int((cls & ~fin).sum()), loss.sum(), p.sum(), (p * s).sum(), w.sum(), (w * s).sum(), ((w * s) * s).sum())
    return out


def plan_splits(n: int, rows: Tuple[int, int]) -> Tuple[int, int, int]:
    """(query blocks, splits, most reference tiles in one split) of the grid ``vm_pair_calib_sums`` launches for the rows [lo, hi) of
    an n-row cache: block k's tiles run from that of row lo + 64 k + 1 to the last, cut into ``splits`` equal runs."""
    lo, hi = rows
    blocks = -(-(hi - lo) // 64)
    splits = int(_lib.lib().query("vm_pair_calib_sums_splits", hi - lo, n))
    n_tiles = -(-n // 128)
    most = max([-(-(n_tiles - (lo + 64 * k + 1) // 128) // splits) for k in range(blocks)] or [0])
    return blocks, splits, most


def _device_sums(cache, kind: int, weights, a: float, b: float, tau: float, rows: Tuple[int, int], norm=None) -> torch.Tensor:
    lib = _lib.lib()
    dev = cache.emb.device
    sums = torch.zeros(2, 8, dtype=torch.float64, device=dev)
    if cache.n > 0:
        emb = cache.emb.contiguous()
        ws = lib.workspace("vm_pair_calib_sums_workspace_bytes", cache.n, cache.E, device=dev)
        lib.call("vm_pair_calib_sums", emb.data_ptr(), cache.speaker_dev.data_ptr(), cache.n, cache.E, kind,
                 None if weights is None else weights.data_ptr(), rows[0], rows[1], None if norm is None else norm.mu.data_ptr(),
                 None if norm is None else norm.rsig.data_ptr(), float(a), float(b), float(tau), sums.data_ptr(), ws.data_ptr(),
                 torch.cuda.current_stream(dev).cuda_stream)
    return sums


def _sums(cache, kind, weights, a, b, tau, rows=None, norm=None) -> np.ndarray:
    return V.triangle_sum(lambda r: _device_sums(cache, kind, weights, a, b, tau, r, norm), cache.n, rows)


def calib_sums(cache, a: float, b: float, tau: float, score: str = "euclidean", model=None, norm=None,
               rows: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """The (2, 8) float64 sums (``SUM_NAMES``; class 0 = target) of all pair trials of ``cache`` at (a, b, tau): one pass of
    ``vm_pair_calib_sums``.  ``rows``: only the pairs with i in [lo, hi); by default this rank's ``triangle_shards`` range, and under
    torchrun the sums of all ranks are added.  ``norm``: on the cohort-normalised scores (``verification.score_norm``)."""
    kind, weights, _ = V.score_kind(cache, score, model)
    V.check_norm(cache, score, norm)
    return _sums(cache, kind, weights, a, b, tau, rows, norm)


# ---- objective, gradient, Hessian --------------------------------------------------------------------------------------------------
def objective_terms(sums: np.ndarray, prior: float):
    """(C, gradient (g_a, g_b), Hessian (h_aa, h_ab, h_bb)) of the module docstring from the sums taken at tau = logit(prior)."""
    S = np.asarray(sums, dtype=np.float64)
    nT, nN = S[0, 0], S[1, 0]
    if nT == 0 or nN == 0:
        raise ValueError("calibration needs target and non-target trials (%d, %d)" % (nT, nN))
    ct, cn = prior / nT, (1.0 - prior) / nN
    C = ct * S[0, 2] + cn * S[1, 2]
    g = (-ct * S[0, 4] + cn * S[1, 4], -ct * S[0, 3] + cn * S[1, 3])
    H = (ct * S[0, 7] + cn * S[1, 7], ct * S[0, 6] + cn * S[1, 6], ct * S[0, 5] + cn * S[1, 5])
    return float(C), (float(g[0]), float(g[1])), tuple(float(h) for h in H)


def newton_decrement2(g, H) -> float:
    """g' H^-1 g (inf if H is not positive definite)."""
    haa, hab, hbb = H
    det = haa * hbb - hab * hab
    if not (haa > 0 and det > 0 and math.isfinite(det)):
        return math.inf
    return (hbb * g[0] * g[0] - 2 * hab * g[0] * g[1] + haa * g[1] * g[1]) / det


def cllr_of(sums: np.ndarray) -> float:
    """Cllr from sums taken at tau = 0."""
    S = np.asarray(sums, dtype=np.float64)
    return float((S[0, 2] / S[0, 0] + S[1, 2] / S[1, 0]) / (2 * LN2))


@dataclass
class Calibration:
    """llr = a s + b, fitted at ``prior`` on the scores ``score`` (``normalised``: cohort-normalised).  ``iterations`` Newton steps
    taken in ``passes`` passes over the trials; ``converged``: the stopping rule of ``fit_calibration`` was met, with ``stop`` its
    constant; ``objective`` = C(a, b) and ``cllr_train`` = Cllr on the trials it was fitted on.  ``trials``: "pair" (the all-pairs
    trials of this module) or "model" (the speaker-model trials of ``enrolment.fit_model_calibration``); the evaluators of either kind
    refuse a calibration of the other."""
    a: float
    b: float
    prior: float
    score: str
    normalised: bool
    iterations: int
    converged: bool
    objective: float
    cllr_train: float
    stop: float = NEWTON_STOP
    passes: int = 0
    trials: str = "pair"


def llr(calibration: Calibration, s) -> np.ndarray:
    """The calibrated log-likelihood ratios a s + b (float64) of scores s."""
    return calibration.a * np.asarray(s, dtype=np.float64) + calibration.b


def _fit(sums_fn: Callable[[float, float, float], np.ndarray], prior: float, score: str, normalised: bool, max_iter: int,
         trials: str = "pair") -> Calibration:
    if not 0.0 < prior < 1.0:
        raise ValueError("the prior must lie in (0, 1)")
    tau = logit(prior)
    passes = 1
    S = sums_fn(0.0, 0.0, tau)
    a = b = 0.0
    C, g, H = objective_terms(S, prior)
    # at a = b = 0 every w of a class is one constant: W1 / W0 and W2 / W0 are the class's mean and second moment of the scores, which
    # give the equal-variance Gaussian model's llr  (m0 - m1) / v s - (m0^2 - m1^2) / (2 v)  as the starting point (kept if it is better)
    with np.errstate(all="ignore"):
        m0, m1 = S[0, 6] / S[0, 5], S[1, 6] / S[1, 5]
        v = 0.5 * ((S[0, 7] / S[0, 5] - m0 * m0) + (S[1, 7] / S[1, 5] - m1 * m1))
        a1, b1 = (m0 - m1) / v, -(m0 * m0 - m1 * m1) / (2 * v)
    if v > 0 and math.isfinite(a1) and math.isfinite(b1) and (a1 != 0 or b1 != 0):
        S1 = sums_fn(float(a1), float(b1), tau)
        passes += 1
        C1, g1, H1 = objective_terms(S1, prior)
        if C1 < C:
            a, b, C, g, H = float(a1), float(b1), C1, g1, H1
    it, converged = 0, False
    while True:
        lam2 = newton_decrement2(g, H)
        if lam2 <= NEWTON_STOP * NEWTON_STOP * C:
            converged = True
            break
        if it >= max_iter or not math.isfinite(lam2):
            break
        haa, hab, hbb = H
        det = haa * hbb - hab * hab
        da, db = -(hbb * g[0] - hab * g[1]) / det, -(haa * g[1] - hab * g[0]) / det
        step, moved = 1.0, False
        for _ in range(30):   # backtracking (Armijo, 1e-4): the slope along the step is -lam2
            S2 = sums_fn(a + step * da, b + step * db, tau)
            passes += 1
            C2, g2, H2 = objective_terms(S2, prior)
            if C2 <= C - 1e-4 * step * lam2:
                a, b, C, g, H, moved = a + step * da, b + step * db, C2, g2, H2, True
                break
            step *= 0.5
        it += 1
        if not moved:   # no descent left at this precision
            break
    S0 = sums_fn(a, b, 0.0)
    passes += 1
    return Calibration(a, b, prior, score, normalised, it, converged, C, cllr_of(S0), NEWTON_STOP, passes, trials)


def fit_calibration_numpy(scores, target, prior: float = 0.5, max_iter: int = 50, score: str = "array") -> Calibration:
    """``fit_calibration`` on an array of scores and its target mask, through ``calib_sums_numpy``."""
    return _fit(lambda a, b, tau: calib_sums_numpy(scores, target, a, b, tau), prior, score, False, max_iter)


def fit_calibration(cache, prior: float = 0.5, score: str = "euclidean", model=None, norm=None, max_iter: int = 50) -> Calibration:
    """Fit llr = a s + b on all pair trials of ``cache`` by minimising C(a, b) (module docstring) at ``prior``: Newton's method with
    backtracking, one ``vm_pair_calib_sums`` pass per evaluation.  The first pass, at a = b = 0, also gives the class means and second
    moments of the scores, hence the equal-variance Gaussian starting point.  It stops when the squared Newton decrement g' H^-1 g is
    at most ``NEWTON_STOP``^2 C(a, b) (``NEWTON_STOP`` = 1e-9; since C <= ln 2 the decrement itself is then below ``NEWTON_STOP``),
    returned as ``stop``.  Perfectly separable trials have no minimiser (C -> 0 as a -> -inf): the fit then returns ``converged=False``
    after ``max_iter`` steps, or earlier when the Hessian underflows."""
    kind, weights, _ = V.score_kind(cache, score, model)
    V.check_norm(cache, score, norm)
    return _fit(lambda a, b, tau: _sums(cache, kind, weights, a, b, tau, None, norm), prior, score, norm is not None, max_iter)


def cllr(cache, calibration: Calibration, model=None, norm=None) -> float:
    """Cllr of the calibrated scores of all pair trials of ``cache`` (one pass at tau = 0): 0 is perfect, 1 is what a = b = 0 gives.
    A calibration of speaker-model trials (``trials == "model"``) is refused: ``enrolment.model_cllr`` takes those."""
    if getattr(calibration, "trials", "pair") != "pair":
        raise ValueError("the calibration was fitted on %s trials, not pair trials" % calibration.trials)
    if (norm is not None) != calibration.normalised:
        raise ValueError("the calibration was fitted on %s scores" % ("normalised" if calibration.normalised else "raw"))
    return cllr_of(calib_sums(cache, calibration.a, calibration.b, 0.0, calibration.score, model, norm))
