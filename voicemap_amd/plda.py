"""A PLDA back end for speaker verification and diarization: mean subtraction, LDA, length normalisation and a two-covariance PLDA
log-likelihood ratio, fitted from statistics made on the chip and scored by the scorers that are already there.

The model.  An embedding is x = mu + y_s + eps with y_s ~ N(0, Phi_b) per speaker and eps ~ N(0, Phi_w).  With z = V^T (x - mu),
V^T Phi_w V = I and V^T Phi_b V = diag(psi), the log-likelihood ratio of "same speaker" against "different speakers" of rows i, j is

    llr = sum_d [ b_d z_id z_jd - a_d (z_id^2 + z_jd^2) / 2 ] + c
    b_d = psi_d / (1 + 2 psi_d),  a_d = psi_d^2 / ((1 + 2 psi_d)(1 + psi_d)),  c = -1/2 sum_d log((1 + 2 psi_d) / (1 + psi_d)^2)

(dimensions with psi_d <= 0 carry nothing and are dropped).  With w = sqrt(b) * z the project's "lower = more alike" score is

    s_ij = -llr = (h_i + h_j) - w_i . w_j,   h_i = sum_d q_d w_id^2 + c0,   q_d = a_d / (2 b_d),   c0 = -c / 2

so a PLDA-SPACE ROW is (w_0 .. w_{D-1}, 0 .., h) of width P = 4 ceil((D + 1) / 4): the last column is the row's own term, the columns
between are zero.  Score kind VM_SCORE_PLDA (include/voicemap_hip.h) of vm_pairdist_argmin, vm_pair_score_hist[_norm],
vm_cohort_topk_stats, vm_pair_calib_sums and vm_ahc scores such rows: ``verification_metrics``, ``score_norm``, ``fit_calibration``,
``detection_costs``, ``pairwise_retrieval``, ``cluster`` and ``diarize`` take score / distance "plda" on a projected cache.

The fit (``fit_plda``).  Stage 1: per-speaker sums (vm_speaker_sums) and the total scatter (vm_scatter_f64) of the raw rows; LDA by the
generalised symmetric eigenproblem S_b v = lambda S_w v in float64 numpy, the top ``lda_dim`` directions scaled so V^T S_w V = I; the
rows are projected on the chip (vm_plda_project), with length normalisation.  Stage 2: the same statistics of the projected rows; EM
for the two-covariance model on the sufficient statistics alone (per-speaker count and mean, the total within scatter); diagonalise.
Rows with a negative label take no part.

Speaker MODELS of several enrolment rows.  The mean of PLDA-space rows is not a PLDA-space row, so the score kind above does not serve
``enrolment``'s speaker models.  By the book, the log-likelihood ratio of a test row against the n enrolment rows of one speaker
TOGETHER ("the n + 1 rows share a speaker" against "the n rows share one and the test row has its own") has a closed form that needs
only the SUM of the enrolment rows and n.  Per component the speaker variable's posterior after the n rows has mean
psi Sz / (1 + n psi) and variance psi / (1 + n psi); stated on w = sqrt(b) z and Sigma = the sum of the enrolment rows' w:

    beta[n][d] = psi_d / (1 + n psi_d)                       A[n][d] = (1 + n psi_d) / (2 b_d (1 + (n + 1) psi_d))
    G[d]       = 1 / (2 b_d (1 + psi_d))                     C[n]    = 1/2 sum_d log((1 + psi_d)(1 + n psi_d) / (1 + (n + 1) psi_d))
    score(m, s) = -llr = sum_d A[n][d] (w_md - beta[n][d] Sigma_sd)^2 - sum_d G[d] w_md^2 - C[n]

(``PldaModel.model_tables``; at n = 1 it is s_ij above).  vm_plda_speaker_identify / vm_plda_speaker_trial_hist (csrc/plda_enrol.hip)
score every row against every model this way from vm_speaker_sums' sums of the projected rows; ``trial_scores_plda_numpy`` is their
numpy twin and ``enrolment.enrol(projected_cache, plda=model)`` the way in.

What is checked: the diagonal form and the multi-session form against the joint Gaussian densities, EM's monotone likelihood and fixed
point, the kernels against the float64 statements here, and a synthetic two-covariance corpus end to end.  NO claim about the EER or
the identification accuracy of a trained encoder on real LibriSpeech is made: that has not been measured.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np


def padded_width(D: int) -> int:
    """P of a PLDA-space row with D score components."""
    return 4 * ((D + 1 + 3) // 4)


# ---- the float64 statements of the two kernels ---------------------------------------------------------------------------------------
def scatter_reference(x, label, mean) -> np.ndarray:
    """vm_scatter_f64 in numpy: sum over the rows with label >= 0 (all rows for ``label`` None) of (x_r - mean)(x_r - mean)^T, the
    difference rounded once in float64.  (The kernel accumulates by fma in chunk order; the two agree bit for bit where every sum is
    exact and otherwise within N 2^-53 sum |d_i| |d_j| per entry.)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    d = x - np.asarray(mean, dtype=np.float64)[None, :]
    if label is not None:
        d = d[np.asarray(label) >= 0]
    return d.T @ d


def project_reference(x, mean, A, length_norm: bool, quad=None, c0: float = 0.0) -> np.ndarray:
    """vm_plda_project in numpy, (N, P) fp32: y = A (x - mean) in float64; with ``length_norm`` y <- (y sqrt(D)) / |y|, |y| the root of the
    ascending sum of squares, a zero row left zero; stored as fp32.  With ``quad`` the row is padded to P = 4 ceil((D + 1) / 4) with
    zeros and its last column is fp32(sum_d quad_d v_d^2 + c0) over the STORED values v, ascending d."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    A = np.asarray(A, dtype=np.float64)
    D = A.shape[0]
    y = (x - np.asarray(mean, dtype=np.float64)[None, :]) @ A.T
    if length_norm:
        ss = np.zeros(len(y))
        for d in range(D):
            ss = ss + y[:, d] * y[:, d]
        nrm = np.sqrt(ss)
        ok = nrm != 0.0
        y[ok] = (y[ok] * np.sqrt(float(D))) / nrm[ok, None]
    v = y.astype(np.float32)
    if quad is None:
        return v
    quad = np.asarray(quad, dtype=np.float64)
    out = np.zeros((len(v), padded_width(D)), dtype=np.float32)
    out[:, :D] = v
    s = np.zeros(len(v))
    v64 = v.astype(np.float64)
    for d in range(D):
        s = s + quad[d] * (v64[:, d] * v64[:, d])
    with np.errstate(over="ignore"):
        out[:, -1] = (s + float(c0)).astype(np.float32)
    return out


def plda_reference(x, mean, A, length_norm: bool, quad=None, c0: float = 0.0, label=None) -> Dict[str, np.ndarray]:
    """Both kernels' float64 statements on one matrix: ``scatter`` (``scatter_reference`` of x about ``mean``) and ``rows``
    (``project_reference``)."""
    return {"scatter": scatter_reference(x, label, mean), "rows": project_reference(x, mean, A, length_norm, quad, c0)}


def plda_scores_numpy(Zq, Zr=None) -> np.ndarray:
    """Score kind VM_SCORE_PLDA in numpy, (M, N) fp32, for PLDA-space rows ``Zq`` (M, P) against ``Zr`` (N, P; default ``Zq``):
    acc = the dot product of the components 0 .. P - 2 rounded to fp32, t = fp32(h_i + h_j), s = fp32(t - acc); a row term that is not
    finite gives NaN.  The kernels form acc as an ascending fmaf chain: the two agree bit for bit where every partial sum is an fp32 number
    (grid rows) and otherwise within (P + 2) 2^-24 (sum |q r| + |h_i| + |h_j|)."""
    Zq = np.asarray(Zq, dtype=np.float32)
    Zr = Zq if Zr is None else np.asarray(Zr, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = (Zq[:, :-1].astype(np.float64) @ Zr[:, :-1].astype(np.float64).T).astype(np.float32)
        hq, hr = Zq[:, -1], Zr[:, -1]
        t = (hq[:, None] + hr[None, :]).astype(np.float32)
        s = (t - acc).astype(np.float32)
    bad = ~np.isfinite(hq)[:, None] | ~np.isfinite(hr)[None, :]
    s[bad] = np.float32(np.nan)
    return s


def trial_scores_plda_numpy(proj, label, q, q_label, tables, leave_one_out: bool, S: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """vm_plda_speaker_identify's score matrix in numpy, with the shape and conventions of ``enrolment.trial_scores_numpy``: (scores
    (M, S) float64, trial (M, S) bool) of the PLDA-space query rows ``q`` (M, P) against the speaker models of the enrolled PLDA-space
    rows ``proj`` (N, P) / ``label`` (N; anything outside [0, S) enrols nowhere).  ``tables``: ``PldaModel.model_tables``' dict (any
    float64 arrays of those shapes do); D = the width of ``G``; only the columns 0 .. D - 1 of the rows are read.  Follows the kernel's
    chain (include/voicemap_hip.h): Sigma = the float64 sum of the speaker's rows in ascending row order, n their number; with
    ``leave_one_out`` and q_label[m] == s, n - 1 and Sigma - w_m; no trial unless 1 <= n <= n_max (the score there is NaN and means
    nothing); mu = beta[n] Sigma, t = w - mu, acc = sum_d (A[n] t) t, g = sum_d G (w w), score = (acc - g) - C[n], every operation
    rounded on its own where the kernel has an fma (so: bit for bit where every value is exact, within the counted roundings
    otherwise)."""
    A, beta, C, G = (np.asarray(tables[k], dtype=np.float64) for k in ("A", "beta", "C", "G"))
    D, n_max = int(G.shape[0]), int(A.shape[0]) - 1
    if A.shape != (n_max + 1, D) or beta.shape != A.shape or C.shape != (n_max + 1,) or n_max < 1:
        raise ValueError("tables: A and beta (n_max + 1, D), C (n_max + 1), G (D), n_max >= 1")
    proj, q = np.asarray(proj, dtype=np.float32), np.asarray(q, dtype=np.float32)
    if proj.ndim != 2 or q.ndim != 2 or proj.shape[1] != q.shape[1] or not D < q.shape[1]:
        raise ValueError("rows must be (N, P) and (M, P) PLDA-space rows with P > D = %d" % D)
    label, q_label = np.asarray(label), np.asarray(q_label)
    if S is None:
        S = int(label.max()) + 1
    sums, count = np.zeros((S, D)), np.zeros(S, dtype=np.int64)
    p64 = proj[:, :D].astype(np.float64)
    for s in range(S):
        rows = np.flatnonzero(label == s)
        count[s] = len(rows)
        for u in rows:
            sums[s] += p64[u]
    w = q[:, :D].astype(np.float64)
    M = len(w)
    out = np.full((M, S), np.nan)
    trial = np.zeros((M, S), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(M):
            n, sg = count.copy(), sums
            own = int(q_label[m])
            if leave_one_out and 0 <= own < S:
                sg = sums.copy()
                n[own] -= 1
                sg[own] -= w[m]
            ok = (n >= 1) & (n <= n_max)
            trial[m] = ok
            nn = np.where(ok, n, 0)
            t = w[m][None, :] - beta[nn] * sg
            acc = ((A[nn] * t) * t).sum(1)
            g = (G * (w[m] * w[m])).sum()
            out[m, ok] = ((acc - g) - C[nn])[ok]
    return out, trial


# ---- the two-covariance model on the host (float64) ----------------------------------------------------------------------------------
def _sym(M):
    return 0.5 * (M + M.T)


def _chol(M, what):
    try:
        return np.linalg.cholesky(_sym(M))
    except np.linalg.LinAlgError:
        raise ValueError("%s is not positive definite (too few rows per dimension?)" % what) from None


def simultaneous_diagonalisation(Phi_b, Phi_w) -> Tuple[np.ndarray, np.ndarray]:
    """(V, psi) with V^T Phi_w V = I and V^T Phi_b V = diag(psi), psi descending; only the columns with psi > 0 are kept."""
    L = _chol(Phi_w, "the within-speaker covariance")
    Li = np.linalg.inv(L)
    psi, U = np.linalg.eigh(_sym(Li @ np.asarray(Phi_b, dtype=np.float64) @ Li.T))
    order = np.argsort(-psi)
    psi, U = psi[order], U[:, order]
    keep = psi > 0.0
    return (Li.T @ U)[:, keep], psi[keep]


def llr_terms(psi) -> Dict[str, np.ndarray]:
    """b, a, c, q = a / (2 b) and c0 = -c / 2 of the module docstring."""
    psi = np.asarray(psi, dtype=np.float64)
    b = psi / (1.0 + 2.0 * psi)
    a = psi * psi / ((1.0 + 2.0 * psi) * (1.0 + psi))
    c = -0.5 * float(np.sum(np.log((1.0 + 2.0 * psi) / ((1.0 + psi) * (1.0 + psi)))))
    return {"b": b, "a": a, "c": c, "q": 0.5 * a / b, "c0": -0.5 * c}


def marginal_loglik(count, dev, W, Phi_b, Phi_w) -> float:
    """The log-likelihood of the corpus under the two-covariance model from its sufficient statistics: per speaker the count n_s and
    d_s = m_s - mu, and the total within scatter W.  A speaker's rows split into their mean, m_s ~ N(mu, Phi_b + Phi_w / n_s), and the
    n_s - 1 deviations from it under Phi_w."""
    count = np.asarray(count, dtype=np.float64)
    D = W.shape[0]
    _, ld_w = np.linalg.slogdet(Phi_w)
    Pw_inv = np.linalg.inv(Phi_w)
    ll = -0.5 * float(np.sum(W * Pw_inv))          # tr(Phi_w^-1 W)
    ll -= 0.5 * float(count.sum()) * D * np.log(2.0 * np.pi)
    ll -= 0.5 * float(np.sum(count - 1.0)) * ld_w
    for n in np.unique(count):
        sel = count == n
        C = Phi_w + n * Phi_b
        _, ld = np.linalg.slogdet(C)
        d = dev[sel]
        quad = np.einsum("sd,sd->s", d, np.linalg.solve(C / n, d.T).T)
        ll -= 0.5 * (sel.sum() * ld + float(quad.sum()))
    return ll


def em_two_covariance(count, dev, W, Phi_b, Phi_w, iters: int) -> Tuple[np.ndarray, np.ndarray, List[float]]:
    """``iters`` EM iterations of the two-covariance model from (Phi_b, Phi_w) on the sufficient statistics (``marginal_loglik``'s).
    E-step: C_s = (Phi_b^-1 + n_s Phi_w^-1)^-1, yhat_s = C_s n_s Phi_w^-1 d_s.  M-step: Phi_b = mean_s (C_s + yhat_s yhat_s^T),
    Phi_w = (W + sum_s n_s ((d_s - yhat_s)(d_s - yhat_s)^T + C_s)) / N.  Returns (Phi_b, Phi_w, the marginal log-likelihood BEFORE every
    iteration and after the last: iters + 1 values, never decreasing)."""
    count = np.asarray(count, dtype=np.float64)
    dev = np.asarray(dev, dtype=np.float64)
    S, N = len(count), float(count.sum())
    Phi_b, Phi_w = _sym(np.array(Phi_b, dtype=np.float64)), _sym(np.array(Phi_w, dtype=np.float64))
    ll = [marginal_loglik(count, dev, W, Phi_b, Phi_w)]
    for _ in range(int(iters)):
        Pb_inv, Pw_inv = np.linalg.inv(Phi_b), np.linalg.inv(Phi_w)
        new_b = np.zeros_like(Phi_b)
        new_w = np.array(W, dtype=np.float64)
        for n in np.unique(count):
            sel = count == n
            k = float(sel.sum())
            C = np.linalg.inv(Pb_inv + n * Pw_inv)
            d = dev[sel]
            yhat = d @ (n * (C @ Pw_inv)).T
            r = d - yhat
            new_b += k * C + yhat.T @ yhat
            new_w += n * (r.T @ r + k * C)
        Phi_b, Phi_w = _sym(new_b / S), _sym(new_w / N)
        ll.append(marginal_loglik(count, dev, W, Phi_b, Phi_w))
    return Phi_b, Phi_w, ll


def moment_estimate(count, dev, W) -> Tuple[np.ndarray, np.ndarray]:
    """(Phi_b, Phi_w) by moments: Phi_w = W / (N - S); Phi_b = the covariance of the speaker means less Phi_w / n (n the mean count), its
    eigenvalues floored at 1e-6 of the largest so that EM starts from a positive definite matrix."""
    count = np.asarray(count, dtype=np.float64)
    S, N = len(count), float(count.sum())
    Phi_w = _sym(W / (N - S))
    B = _sym(dev.T @ dev / S - Phi_w / (N / S))
    lam, U = np.linalg.eigh(B)
    lam = np.maximum(lam, 1e-6 * max(float(lam.max()), 1e-300))
    return (U * lam) @ U.T, Phi_w


class PldaModel:
    """What ``fit_plda`` returns.  Stage 1: ``mean1`` (E), ``A1`` (D1, E), ``length_norm``; stage 2: ``mean2`` (D1), ``A2`` (D, D1) =
    diag(sqrt(b)) V^T, ``quad`` (D) = q, ``c0``, ``psi`` (D); ``loglik``: the marginal log-likelihood per EM iteration; ``Phi_b`` /
    ``Phi_w`` (D1, D1).  All float64 numpy."""

    FIELDS = ("mean1", "A1", "mean2", "A2", "quad", "psi", "Phi_b", "Phi_w", "loglik")

    def __init__(self, mean1, A1, length_norm, mean2, A2, quad, c0, psi, Phi_b=None, Phi_w=None, loglik=()):
        f64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        self.mean1, self.A1, self.mean2, self.A2, self.quad, self.psi = f64(mean1), f64(A1), f64(mean2), f64(A2), f64(quad), f64(psi)
        self.length_norm, self.c0 = bool(length_norm), float(c0)
        D1 = self.A1.shape[0]
        self.Phi_b = f64(Phi_b if Phi_b is not None else np.zeros((D1, D1)))
        self.Phi_w = f64(Phi_w if Phi_w is not None else np.zeros((D1, D1)))
        self.loglik = f64(loglik).reshape(-1)
        if self.A1.ndim != 2 or self.A2.ndim != 2 or self.A2.shape[1] != D1 or self.mean1.shape != (self.A1.shape[1],) \
                or self.mean2.shape != (D1,) or self.quad.shape != (self.A2.shape[0],) or self.psi.shape != self.quad.shape:
            raise ValueError("the model's matrices do not fit together")
        if not (1 <= self.A1.shape[1] <= 255 and 1 <= D1 <= 255 and 1 <= self.A2.shape[0] <= 255):
            raise ValueError("every dimension of the model must be in 1 .. 255")
        self._dev = {}

    @classmethod
    def from_covariances(cls, mu, Phi_b, Phi_w, mean1=None, A1=None, length_norm=False, loglik=()):
        """The model of (mu, Phi_b, Phi_w) in the space behind stage 1 (default: no stage 1 -- identity, no length normalisation)."""
        mu = np.asarray(mu, dtype=np.float64)
        V, psi = simultaneous_diagonalisation(Phi_b, Phi_w)
        if psi.size == 0:
            raise ValueError("the between-speaker covariance has no positive direction")
        t = llr_terms(psi)
        D1 = len(mu)
        return cls(np.zeros(D1) if mean1 is None else mean1, np.eye(D1) if A1 is None else A1, length_norm, mu,
                   np.sqrt(t["b"])[:, None] * V.T, t["q"], t["c0"], psi, Phi_b, Phi_w, loglik)

    # ---- sizes
    @property
    def E(self) -> int:
        return int(self.A1.shape[1])

    @property
    def D(self) -> int:
        return int(self.A2.shape[0])

    @property
    def P(self) -> int:
        return padded_width(self.D)

    # ---- the float64 statements
    def stage1_numpy(self, x) -> np.ndarray:
        """The stage-1 rows (N, D1) as the chip stores them (fp32): ``project_reference``."""
        return project_reference(x, self.mean1, self.A1, self.length_norm)

    def project_numpy(self, x) -> np.ndarray:
        """``project`` in numpy: the two ``project_reference`` calls, (N, P) fp32."""
        return project_reference(self.stage1_numpy(x), self.mean2, self.A2, False, self.quad, self.c0)

    def llr_numpy(self, a, b=None) -> np.ndarray:
        """The (len(a), len(b)) float64 log-likelihood ratios of raw rows ``a`` against ``b`` (default ``a``) through the diagonal form,
        nothing rounded to fp32 on the way: z = V^T (y - mean2) of the float64 stage-1 rows y."""
        t = llr_terms(self.psi)
        za = self.z_numpy(a)
        zb = za if b is None else self.z_numpy(b)
        sq = lambda z: 0.5 * ((z * z) @ t["a"])
        return (za * t["b"][None, :]) @ zb.T - sq(za)[:, None] - sq(zb)[None, :] + t["c"]

    def z_numpy(self, x) -> np.ndarray:
        """z = V^T (y - mean2) of the float64 stage-1 rows y of raw rows ``x``, (N, D) float64: nothing is rounded to fp32."""
        x = np.asarray(x, dtype=np.float64)
        y = (x - self.mean1[None, :]) @ self.A1.T
        if self.length_norm:
            nrm = np.sqrt((y * y).sum(1))
            ok = nrm != 0.0
            y[ok] = y[ok] * np.sqrt(float(y.shape[1])) / nrm[ok, None]
        return ((y - self.mean2[None, :]) @ self.A2.T) / np.sqrt(llr_terms(self.psi)["b"])[None, :]

    # ---- speaker models of several enrolment rows (module docstring)
    def model_tables(self, n_max: int) -> Dict[str, np.ndarray]:
        """The coefficient tables of multi-session scoring for models of 1 .. ``n_max`` rows, float64: ``A`` and ``beta``
        (n_max + 1, D), ``C`` (n_max + 1), ``G`` (D).  Row 0 is unused (zeros)."""
        n_max = int(n_max)
        if n_max < 1:
            raise ValueError("n_max must be >= 1")
        psi = self.psi[None, :]
        b = llr_terms(self.psi)["b"][None, :]
        n = np.arange(n_max + 1, dtype=np.float64)[:, None]
        beta = psi / (1.0 + n * psi)
        A = (1.0 + n * psi) / (2.0 * b * (1.0 + (n + 1.0) * psi))
        C = 0.5 * np.log((1.0 + psi) * (1.0 + n * psi) / (1.0 + (n + 1.0) * psi)).sum(1)
        beta[0], A[0], C[0] = 0.0, 0.0, 0.0
        return {"A": np.ascontiguousarray(A), "beta": np.ascontiguousarray(beta), "C": np.ascontiguousarray(C),
                "G": np.ascontiguousarray(1.0 / (2.0 * b[0] * (1.0 + self.psi)))}

    def model_llr_numpy(self, enrol_rows, test_rows) -> np.ndarray:
        """The float64 log-likelihood ratios (len(test_rows)) of raw rows ``test_rows`` against ONE speaker model enrolled from all the
        raw rows ``enrol_rows`` (n >= 1 of them): per component the predictive density of the test row after the n rows -- mean
        psi Sz / (1 + n psi), variance 1 + psi / (1 + n psi) -- against its marginal density, variance 1 + psi.  Stated in z, with
        nothing rounded to fp32 and none of the tables: the independent statement ``model_tables`` is held to."""
        ze, zt = self.z_numpy(enrol_rows), self.z_numpy(test_rows)
        n = float(len(ze))
        if n < 1:
            raise ValueError("a speaker model needs at least one enrolment row")
        psi = self.psi
        mean = psi * ze.sum(0) / (1.0 + n * psi)
        var = 1.0 + psi / (1.0 + n * psi)
        d = zt - mean[None, :]
        return (-0.5 * (np.log(var) + d * d / var) + 0.5 * (np.log(1.0 + psi) + zt * zt / (1.0 + psi))).sum(1)

    # ---- the device path
    def _on(self, dev):
        import torch
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(dev) for a in (self.mean1, self.A1, self.mean2, self.A2, self.quad))
        return self._dev[key]

    def project(self, emb_or_cache):
        """PLDA-space rows of raw embeddings: an (N, E) fp32 device tensor gives an (N, P) device tensor; a cache (``.emb``, ``.speaker``)
        gives a cache of the same class whose rows are PLDA-space rows.  Two vm_plda_project calls."""
        if hasattr(emb_or_cache, "emb"):
            out = type(emb_or_cache)(self.project(emb_or_cache.emb), emb_or_cache.speaker)
            if hasattr(emb_or_cache, "vad_counts"):   # what embed_corpus(vad=...) noted about the rows' audio stays with the rows
                out.vad_counts = emb_or_cache.vad_counts
            return out
        emb = emb_or_cache
        if emb.dim() != 2 or int(emb.shape[1]) != self.E:
            raise ValueError("the model takes (N, %d) rows" % self.E)
        mean1, A1, mean2, A2, quad = self._on(emb.device)
        y = device_project(emb, mean1, A1, self.length_norm)
        return device_project(y, mean2, A2, False, quad, self.c0)

    # ---- files
    def save(self, path) -> None:
        """Everything into one .npz (float64 arrays, bit for bit)."""
        with open(path, "wb") as f:
            np.savez(f, length_norm=np.array(self.length_norm), c0=np.array(self.c0, dtype=np.float64),
                     **{k: getattr(self, k) for k in self.FIELDS})

    @classmethod
    def load(cls, path) -> "PldaModel":
        with np.load(path) as z:
            return cls(z["mean1"], z["A1"], bool(z["length_norm"]), z["mean2"], z["A2"], z["quad"], float(z["c0"]), z["psi"], z["Phi_b"],
                       z["Phi_w"], z["loglik"])


# ---- the device calls ----------------------------------------------------------------------------------------------------------------
def device_scatter(x, label, mean):
    """``vm_scatter_f64``: the (D, D) float64 device tensor of x (N, D) fp32 about ``mean`` (D) float64 on the device; ``label`` (N) int32 or
    None."""
    import torch
    from . import _lib
    lib = _lib.lib()
    x = x.contiguous()
    N, D = int(x.shape[0]), int(x.shape[1])
    dev = x.device
    out = torch.zeros(D, D, dtype=torch.float64, device=dev)
    if N > 0:
        mean = mean.to(device=dev, dtype=torch.float64).contiguous()
        if label is not None:
            label = label.to(device=dev, dtype=torch.int32).contiguous()
        ws = lib.workspace("vm_scatter_f64_workspace_bytes", N, D, device=dev)
        lib.call("vm_scatter_f64", x.data_ptr(), None if label is None else label.data_ptr(), mean.data_ptr(), N, D, out.data_ptr(),
                 ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return out


def device_project(x, mean, A, length_norm: bool, quad=None, c0: float = 0.0):
    """``vm_plda_project`` on device tensors: x (N, E) fp32; mean (E), A (D, E), quad (D) float64 -> (N, P) fp32."""
    import torch
    from . import _lib
    lib = _lib.lib()
    x = x.contiguous()
    N, E = int(x.shape[0]), int(x.shape[1])
    D = int(A.shape[0])
    P = D if quad is None else padded_width(D)
    out = torch.empty(N, P, dtype=torch.float32, device=x.device)
    if N > 0:
        lib.call("vm_plda_project", x.data_ptr(), mean.contiguous().data_ptr(), A.contiguous().data_ptr(), N, E, D, int(bool(length_norm)),
                 None if quad is None else quad.contiguous().data_ptr(), float(c0), out.data_ptr(), P,
                 torch.cuda.current_stream(x.device).cuda_stream)
    return out


def dense_labels(speaker) -> Tuple[np.ndarray, int]:
    """(label (N) int32: 0 .. S - 1 in ascending order of the speaker code, -1 for a negative code; S)."""
    speaker = np.asarray(speaker).astype(np.int64).reshape(-1)
    codes = np.unique(speaker[speaker >= 0])
    label = np.where(speaker >= 0, np.searchsorted(codes, speaker), -1).astype(np.int32)
    return label, int(len(codes))


def _device_stats(x, label_np, S):
    """(count (S), sums (S, D), mu (D), T (D, D)) of device rows: vm_speaker_sums (euclidean kind) and vm_scatter_f64 about the mean of
    the labelled rows."""
    import torch
    from . import _lib
    from .enrolment import speaker_sums
    label = torch.from_numpy(label_np).to(x.device)
    sums, _, count = speaker_sums(x, label, S, _lib.VM_DIST_EUCLIDEAN)
    count = count.cpu().numpy().astype(np.float64)
    sums = sums.cpu().numpy()
    mu = sums.sum(0) / count.sum()
    T = device_scatter(x, label, torch.from_numpy(mu).to(x.device)).cpu().numpy()
    return count, sums, mu, T


def _numpy_stats(x, label_np, S):
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    count = np.bincount(label_np[label_np >= 0], minlength=S).astype(np.float64)
    sums = np.zeros((S, x64.shape[1]))
    np.add.at(sums, label_np[label_np >= 0], x64[label_np >= 0])
    mu = sums.sum(0) / count.sum()
    return count, sums, mu, scatter_reference(x64, label_np, mu)


def _fit(x, speaker, stats, project, lda_dim, length_norm, em_iters) -> PldaModel:
    """The fit over a pair of back ends: ``stats(rows, label, S)`` and ``project(rows, mean, A, length_norm)``."""
    label, S = dense_labels(speaker)
    count0 = np.bincount(label[label >= 0], minlength=S)
    if S < 2:
        raise ValueError("fit_plda needs at least two speakers (%d found)" % S)
    if count0.max() < 2:
        raise ValueError("fit_plda needs a speaker with at least two rows")
    E = int(x.shape[1])
    if not 1 <= E <= 255:
        raise ValueError("fit_plda takes rows of 1 .. 255 components")
    D1 = E if lda_dim is None else int(lda_dim)
    if not 1 <= D1 <= E:
        raise ValueError("lda_dim must be in 1 .. %d" % E)
    # stage 1: LDA
    count, sums, mu1, T = stats(x, label, S)
    dev = sums / count[:, None] - mu1[None, :]
    Sb = _sym((dev * count[:, None]).T @ dev)
    Sw = _sym(T - Sb)
    L = _chol(Sw, "the within-speaker scatter")
    Li = np.linalg.inv(L)
    lam, U = np.linalg.eigh(_sym(Li @ Sb @ Li.T))
    U = U[:, np.argsort(-lam)[:D1]]
    A1 = np.ascontiguousarray((Li.T @ U).T)          # rows v^T with V^T S_w V = I
    y = project(x, mu1, A1, length_norm)
    # stage 2: the two-covariance model of the projected rows
    count, sums, mu2, T2 = stats(y, label, S)
    dev = sums / count[:, None] - mu2[None, :]
    W = _sym(T2 - (dev * count[:, None]).T @ dev)
    Phi_b, Phi_w = moment_estimate(count, dev, W)
    Phi_b, Phi_w, ll = em_two_covariance(count, dev, W, Phi_b, Phi_w, em_iters)
    return PldaModel.from_covariances(mu2, Phi_b, Phi_w, mu1, A1, length_norm, ll)


def fit_plda(cache, lda_dim: Optional[int] = None, length_norm: bool = True, em_iters: int = 10) -> PldaModel:
    """Fit the back end on the rows of ``cache`` (``.emb`` (N, E) fp32 on the device, ``.speaker`` (N) codes; a negative code leaves the row
    out).  The sums, scatters and projections run on the chip, the (E, E) eigenproblems and EM on the host in float64 (module
    docstring).  Fewer than two speakers, or no speaker with two rows, raises ``ValueError``."""
    import torch

    def project(rows, mean, A, ln):
        return device_project(rows, torch.from_numpy(mean).to(rows.device), torch.from_numpy(A).to(rows.device), ln)

    return _fit(cache.emb, cache.speaker, _device_stats, project, lda_dim, length_norm, em_iters)


def fit_plda_numpy(x, speaker, lda_dim: Optional[int] = None, length_norm: bool = True, em_iters: int = 10) -> PldaModel:
    """``fit_plda`` with the float64 statements in place of the kernels (``scatter_reference``, ``project_reference``)."""
    x = np.asarray(x, dtype=np.float32)
    return _fit(x, speaker, _numpy_stats, lambda rows, mean, A, ln: project_reference(rows, mean, A, ln), lda_dim, length_norm, em_iters)
