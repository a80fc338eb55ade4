"""Cases and independent statements for the PLDA back end (tests/test_plda_cpu.py, tests/test_gpu_plda.py).  Pure numpy: it imports
neither torch nor the library."""
import numpy as np

from voicemap_amd import plda as PL

U32 = 2.0 ** -24   # fp32 unit roundoff


# ---- random models -------------------------------------------------------------------------------------------------------------------
def random_spd(rng, D, lo=0.2, hi=5.0):
    """A symmetric positive definite (D, D) matrix with eigenvalues drawn log-uniformly from [lo, hi] in a random basis."""
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    lam = np.exp(rng.uniform(np.log(lo), np.log(hi), D))
    return (Q * lam) @ Q.T


def log_gauss(x, mu, C):
    """log N(x; mu, C) of the rows of x, through numpy.linalg (slogdet, solve)."""
    d = x - mu[None, :]
    _, ld = np.linalg.slogdet(C)
    return -0.5 * (C.shape[0] * np.log(2.0 * np.pi) + ld + np.einsum("nd,nd->n", d, np.linalg.solve(C, d.T).T))


def direct_llr(a, b, mu, Phi_b, Phi_w):
    """The (len(a), len(b)) log-likelihood ratios by the DIRECT statement: the log of the joint Gaussian density of (x_i, x_j) under "one
    speaker" -- covariance [[Phi_b + Phi_w, Phi_b], [Phi_b, Phi_b + Phi_w]] -- less the two marginal densities, full matrices throughout."""
    T = Phi_b + Phi_w
    J = np.block([[T, Phi_b], [Phi_b, T]])
    mu2 = np.concatenate([mu, mu])
    la, lb = log_gauss(a, mu, T), log_gauss(b, mu, T)
    out = np.empty((len(a), len(b)))
    for i in range(len(a)):
        pair = np.concatenate([np.repeat(a[i:i + 1], len(b), 0), b], axis=1)
        out[i] = log_gauss(pair, mu2, J) - la[i] - lb
    return out


# ---- corpora -------------------------------------------------------------------------------------------------------------------------
def two_covariance_corpus(seed, speakers, rows, E, Phi_b, Phi_w, mu):
    """(x (speakers * rows, E) fp32, speaker codes) drawn from the two-covariance model."""
    rng = np.random.default_rng(seed)
    Lb, Lw = np.linalg.cholesky(Phi_b), np.linalg.cholesky(Phi_w)
    y = rng.normal(size=(speakers, E)) @ Lb.T
    x = mu[None, None, :] + y[:, None, :] + rng.normal(size=(speakers, rows, E)) @ Lw.T
    return x.reshape(-1, E).astype(np.float32), np.repeat(np.arange(speakers), rows)


# The end-to-end corpus: E = 16, a unit between-speaker covariance in every direction, and within-speaker noise that is STRONGLY
# anisotropic in a rotated basis -- four directions with standard deviation 6 (session noise that swamps the speaker there), twelve
# with 0.3 -- around a mean well away from the origin.  Cosine and euclidean scores are dominated by the four loud directions; the
# back end learns to ignore them.  40 training and 40 held-out speakers with 8 rows each.
E2E_E, E2E_SPEAKERS, E2E_ROWS, E2E_SEED = 16, 40, 8, 5


def e2e_model():
    rng = np.random.default_rng(E2E_SEED)
    Q, _ = np.linalg.qr(rng.normal(size=(E2E_E, E2E_E)))
    sd = np.array([6.0] * 4 + [0.3] * 12)
    Phi_w = (Q * sd ** 2) @ Q.T
    return rng.normal(size=E2E_E) * 2.0, np.eye(E2E_E), Phi_w


def e2e_corpora():
    """((train x, train speakers), (held-out x, held-out speakers)): disjoint speakers from one model."""
    mu, Phi_b, Phi_w = e2e_model()
    return (two_covariance_corpus(E2E_SEED + 1, E2E_SPEAKERS, E2E_ROWS, E2E_E, Phi_b, Phi_w, mu),
            two_covariance_corpus(E2E_SEED + 2, E2E_SPEAKERS, E2E_ROWS, E2E_E, Phi_b, Phi_w, mu))


def pair_trials(scores, speaker):
    """(scores, target) of the unordered pairs i < j of a symmetric (N, N) score matrix."""
    iu = np.triu_indices(len(speaker), 1)
    speaker = np.asarray(speaker)
    return np.asarray(scores)[iu], speaker[iu[0]] == speaker[iu[1]]


def cosine_scores(x):
    x = np.asarray(x, dtype=np.float64)
    n = np.linalg.norm(x, axis=1)
    return 1.0 - (x @ x.T) / (n[:, None] * n[None, :])


# ---- grid inputs: every sum exact ----------------------------------------------------------------------------------------------------
def grid_plda_rows(rng, n, P, scale=1.0):
    """PLDA-space rows on a dyadic grid: P - 1 components that are integers in [-8, 8] times ``scale`` and a row term that is an integer in
    [-64, 64] times ``scale``^2.  With P <= 256 every product, every partial sum of the chain in any order, h_i + h_j and the final
    difference is an integer below 2^24 in units of scale^2: an fp32 number (255 * 64 + 128 < 2^15)."""
    z = (rng.integers(-8, 9, (n, P)) * scale).astype(np.float32)
    z[:, -1] = (rng.integers(-64, 65, n) * scale * scale).astype(np.float32)
    return z


def grid_f64(rng, shape, amp=64, scale=2.0 ** -4):
    return rng.integers(-amp, amp + 1, shape) * scale


# ---- the rounding bound of scoring projected rows -------------------------------------------------------------------------------------
def projected_score_bound(model, x):
    """An upper bound, entry by entry, of |plda_scores_numpy(model.project_numpy(x)) - (-model.llr_numpy(x))|, counting the fp32 roundings
    on the way (u = 2^-24; float64 errors are 2^-29 times smaller and covered by the 1.05):
      * the stage-1 row y is stored as fp32: |dy| <= u |y|, which moves w = A2 (y - mean2) by at most |A2| u |y|;
      * w is stored as fp32: u |w| more.  Together dw;
      * the row term h = sum q w^2 + c0 moves by 2 sum q |w| dw, and is stored as fp32: u |h| more.  Together dh;
      * the score (h_i + h_j) - w_i . w_j moves by dh_i + dh_j + sum (dw_i |w_j| + |w_i| dw_j), and its own arithmetic -- the product sum
        rounded once, the sum of the two terms, the difference -- adds u (sum |w_i w_j| + 2 (|h_i| + |h_j|)) at most."""
    y = model.stage1_numpy(x).astype(np.float64)
    w = (y - model.mean2[None, :]) @ model.A2.T
    h = (w * w) @ model.quad + model.c0
    dw = U32 * (np.abs(y) @ np.abs(model.A2).T) + U32 * np.abs(w)
    dh = 2.0 * (np.abs(w) * dw) @ model.quad + U32 * np.abs(h)
    aw = np.abs(w)
    cross = dw @ aw.T + aw @ dw.T
    own = U32 * (aw @ aw.T + 2.0 * (np.abs(h)[:, None] + np.abs(h)[None, :]))
    return 1.05 * (dh[:, None] + dh[None, :] + cross + own) + 1e-30
