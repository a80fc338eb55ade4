"""Case builders, independent statements and the error bound shared by tests/test_vbx_cpu.py and tests/test_gpu_vbx.py (VBx:
voicemap_amd/diarization.py vbx / vbx_reference, csrc/vbx.hip).  Pure numpy: it imports neither torch nor the library.

The error bound (DESIGN section 8m has the derivation; u = 2^-53).  One iteration of the statement from given gamma and pi, carried out
in float64 in ANY order of the sums, with or without fma, with an exp and a log of at most one ulp (2 u relative; what the device
documents for both and what numpy's keep), against the exact result:
  * sums over t of the speaker posteriors:  |dF_kd| <= (2 n + 1) u sum_t gamma |rho|,  N_k within (n - 1) u;
  * invL = 1 / (1 + F N_k psi) is made of positive numbers by five more operations: within e_L = (n + 5) u;
  * alpha = F invL F_kd:  d_alpha = (e_L + 3 u) |alpha| + F invL |dF|;
  * q_k (positive terms):  dq = sum_d (e_L invL + 2 |alpha| d_alpha) psi + (2 D + 3) u q_k;
  * ent_k (mixed signs, so absolute):  sum_d (e_L + 2 u |log invL| + e_L invL + 2 |alpha| d_alpha + 4 u mag_d) + D u sum_d mag_d with
    mag_d = |log invL| + invL + alpha^2 + 1;
  * lp[t][k] = fa (rho . alpha - q_k / 2 + G_t):  d_lp = fa ((2 D + 1) u sum |rho| |alpha| + sum |rho| d_alpha + dq / 2 + (2 D + 3) u |G_t| +
    4 u (|rho . alpha| + q_k / 2 + |G_t|));
  * p[t][k] = exp(lp - m_t) up to the factor every entry of its row shares (gamma, pi and log_pX do not depend on it, whatever
    number m_t is):  theta[t][k] = d_lp + u |lp - m_t| + 2 u, relative.
  * The forward-backward adds and multiplies non-negative numbers only, so relative errors add.  gamma[t][k], pi'_k and the total are
    sums over paths of products of one p per row and one transition per row: the p's move a path's weight by at most
    Theta = sum_t max_k theta[t][k], a ratio of two such sums by 2 Theta.  The recursion's own roundings: a forward step is 5 operations,
    the sum over the speakers at most 6 deep (64 lanes) and a division; a backward step 14 in all; a row of gamma sits behind t + 1
    forward steps, n - 1 - t backward steps and the product of all n scales, itself n sums and divisions away from the total:
    (26 n + 2) u.
      gamma  relative  B_g = 1.05 (2 Theta + (26 n + 2) u)
      pi     relative  B_p = 1.05 (2 (2 Theta + (26 n + 2) u + (n + 5) u) + 8 u)     (n terms summed; numerator and denominator)
      ELBO   absolute  B_e = 1.05 (Theta + 12 n u + 3 u sum_t |log c_t| + (n + 1) u S + fb / 2 (sum_k d_ent_k + (K + 2) u sum_k |ent_k|)
                                   + 2 u (|log_pX| + fb / 2 |sum_k ent_k|)),   S = sum_t (|log c_t| + |m_t|)
  The 1.05 covers the second-order terms and the 2^-64 roundings of the extended-precision run that stands in for the exact result.
  An entry of gamma below 1e-290 has been through numbers within reach of the subnormals, where a rounding is absolute: such entries are
  held to |difference| <= 1e-290 and no relative claim is made."""
import itertools

import numpy as np

from voicemap_amd import diarization as DZ
from voicemap_amd import plda as PL

U = 2.0 ** -53
TINY = 1e-290


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def random_tables(rng, D):
    psi = np.exp(rng.uniform(np.log(0.1), np.log(10.0), D))
    return psi, np.sqrt(1.0 + 2.0 * psi), (1.0 + 2.0 * psi) / psi


def random_case(seed, sizes, Ks, D, chains=None, planted=True):
    """One vm_vbx call: ``sizes`` rows per recording, ``Ks`` speakers each (one number or one per recording), PLDA-space rows of width
    P = padded_width(D) drawn from the model (a speaker mean sqrt(psi) y per turn, unit within noise, w = sqrt(b) z), labels with
    rows of no cluster and out of range, a random warm start gamma / pi.  -> dict."""
    rng = np.random.RandomState(seed)
    psi, r, ib = random_tables(rng, D)
    Ks = np.broadcast_to(np.asarray(Ks, dtype=np.int64), (len(sizes),)).copy()
    P = PL.padded_width(D)
    rows, lab, gam, pi = [], [], [], np.zeros((len(sizes), DZ.MAX_K))
    for i, (n, K) in enumerate(zip(sizes, Ks)):
        S = min(int(K), 3)
        y = rng.randn(S, D)
        who = np.repeat(rng.randint(S, size=n // 4 + 1), 4)[:n]
        z = np.sqrt(psi)[None, :] * y[who] + rng.randn(n, D)
        x = np.zeros((n, P), np.float32)
        x[:, :D] = z / np.sqrt(ib)[None, :]
        x[:, -1] = rng.randn(n)   # the row term: never read
        rows.append(x)
        l = who.astype(np.int32) if planted else rng.randint(0, K, size=n).astype(np.int32)
        u = rng.uniform(size=n)
        l[u < 0.1] = -1
        l[(u >= 0.1) & (u < 0.15)] = K
        lab.append(l)
        g = rng.gamma(0.3, size=(n, K)) + 1e-3
        gam.append((g / g.sum(1, keepdims=True)).ravel())
        v = rng.gamma(1.0, size=K) + 1e-2
        pi[i, :K] = v / v.sum()
    row0 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(row0[-1])
    cs = None
    if chains == "edges":   # a start at the first and the last row of every recording, on two consecutive rows, and at a few others
        cs = (rng.uniform(size=N) < 0.05).astype(np.int32) * 7
        for lo, hi in zip(row0[:-1], row0[1:]):
            if hi > lo:
                cs[lo], cs[hi - 1] = 1, 1
            if hi - lo > 4:
                cs[lo + 2], cs[lo + 3] = 1, 1
    return {"rows": np.concatenate(rows).reshape(N, P) if N else np.zeros((0, P), np.float32), "row0": row0, "n_models": Ks,
            "labels": np.concatenate(lab).astype(np.int32) if N else np.zeros(0, np.int32), "chain_start": cs, "tables": (psi, r, ib),
            "gamma": np.concatenate(gam) if N else np.zeros(0), "pi": pi, "D": D}


# (K, D, n): every value of the three grids once with the others small, plus the two all-maximum corners
GRID = ([(K, 4, 65) for K in (1, 2, 3, 63, 64)] + [(3, D, 65) for D in (1, 3, 5, 63, 64, 65, 255)]
        + [(3, 4, n) for n in (1, 2, 63, 64, 257, 1000)] + [(64, 255, 1000), (63, 255, 1000)])
PARAMS = dict(loop_prob=0.9, fa=0.3, fb=17.0, init_smooth=5.0)


NEVER = -np.inf   # an epsilon that never stops
_CACHE = {}


def grid_case(K, D, n):
    key = ("case", K, D, n)
    if key not in _CACHE:
        _CACHE[key] = random_case(1000 * K + 10 * D + n, [n], K, D, chains="edges" if n > 2 else None)
    return _CACHE[key]


def exact(case, gamma=None, pi=None, dtype=np.longdouble):
    """ONE iteration of the statement from a warm start (default the case's), in extended precision: what stands in for the exact result."""
    return DZ.vbx_reference(case["rows"], case["row0"], case["n_models"], case["labels"], case["chain_start"], case["tables"],
                            PARAMS["loop_prob"], PARAMS["fa"], PARAMS["fb"], PARAMS["init_smooth"], 1, NEVER,
                            gamma=case["gamma"] if gamma is None else gamma, pi=case["pi"] if pi is None else pi, dtype=dtype)


def exact_one_iteration(K, D, n):
    """``exact`` of ``grid_case(K, D, n)``, computed once per process."""
    key = ("exact", K, D, n)
    if key not in _CACHE:
        _CACHE[key] = exact(grid_case(K, D, n))
    return _CACHE[key]


def mixed_case():
    """Several recordings with different K in one call, an empty one, one whose labels are all -1; chain starts at row 0, at the last
    row and on consecutive rows."""
    if "mixed" not in _CACHE:
        case = random_case(21, [150, 0, 70, 33, 1], [5, 4, 9, 2, 64], 12, chains="edges")
        case["labels"][220:253] = -1
        _CACHE["mixed"] = case
    return _CACHE["mixed"]


def degenerate_case():
    """K = 2, rows far apart, a warm start that gives speaker 0 the first half, and pi_in exactly 0 under speaker 0: in row 0 the only
    emission that survives the exp belongs to a speaker of prior 0, so c_0 = 0."""
    psi = np.array([1.0, 2.0, 0.5, 1.5])
    x = np.zeros((20, 8), np.float32)
    x[:10, :4], x[10:, :4] = 40.0, -40.0
    g = np.zeros((20, 2))
    g[:10, 0], g[10:, 1] = 1.0, 1.0
    pi = np.zeros((1, 64))
    pi[0, 1] = 1.0
    lab = np.array([0, 1, -1, 5] * 5, dtype=np.int32)
    return {"rows": x, "row0": np.array([0, 20], dtype=np.int64), "n_models": np.array([2], dtype=np.int64), "labels": lab, "chain_start": None,
            "tables": (psi, np.sqrt(1.0 + 2.0 * psi), (1.0 + 2.0 * psi) / psi), "gamma": g.ravel(), "pi": pi, "D": 4}


# ---- independent statements ----------------------------------------------------------------------------------------------------------
def posterior_terms(w, tables, g, fa, fb):
    """(lp (n, K), ent (K,), alpha, invL, G) of one recording from gamma ``g``, vectorised float64: the speaker posteriors and the
    emissions of the statement with numpy's own sums."""
    psi, r, ib = tables
    Fr = fa / fb
    rho = r[None, :] * w
    invL = 1.0 / (1.0 + Fr * g.sum(0)[:, None] * psi[None, :])
    alpha = Fr * invL * (g.T @ rho)
    q = ((invL + alpha * alpha) * psi[None, :]).sum(1)
    ent = (np.log(invL) - invL - alpha * alpha + 1.0).sum(1)
    G = -0.5 * ((ib[None, :] * w * w).sum(1) + w.shape[1] * np.log(2.0 * np.pi))
    return fa * (rho @ alpha.T - 0.5 * q[None, :] + G[:, None]), ent, alpha, invL, G


def lambdas(chain_start, n, loop_prob):
    start = np.zeros(n, bool) if chain_start is None else np.asarray(chain_start) != 0
    start[0] = True
    return np.where(start, 0.0, loop_prob)


def brute_force(lp, lam, pi):
    """(gamma (n, K), log_pX) by enumeration of all K^n paths: a path's weight is the product of exp(lp) along it, pi_k at a row
    that forgets the past and lam [j == k] + (1 - lam) pi_k elsewhere."""
    n, K = lp.shape
    e = np.exp(lp)
    num, tot = np.zeros((n, K)), 0.0
    for path in itertools.product(range(K), repeat=n):
        wgt = 1.0
        for t, k in enumerate(path):
            tr = pi[k] if lam[t] == 0.0 else lam[t] * (path[t - 1] == k) + (1.0 - lam[t]) * pi[k]
            wgt *= e[t, k] * tr
        tot += wgt
        for t, k in enumerate(path):
            num[t, k] += wgt
    return num / tot, np.log(tot)


def log_forward_backward(lp, lam, pi):
    """(gamma, log_pX) by a plain log-domain forward-backward with the full K x K transition matrix of every row."""
    n, K = lp.shape
    lse = lambda x, axis: np.log(np.exp(x - x.max(axis=axis, keepdims=True)).sum(axis=axis)) + x.max(axis=axis)
    with np.errstate(divide="ignore"):
        ltr = [np.log(lam[t] * np.eye(K) + (1.0 - lam[t]) * np.tile(pi[None, :], (K, 1))) for t in range(n)]   # [t][j][k]
        la, lb = np.zeros((n, K)), np.zeros((n, K))
        la[0] = np.log(pi) + lp[0]
        for t in range(1, n):
            la[t] = lp[t] + lse(la[t - 1][:, None] + ltr[t], 0)
        for t in range(n - 2, -1, -1):
            lb[t] = lse(ltr[t + 1] + (lp[t + 1] + lb[t + 1])[None, :], 1)
    tot = lse(la[n - 1], 0)
    return np.exp(la + lb - tot), float(tot)


# ---- the error bound -------------------------------------------------------------------------------------------------------------------
def one_iteration_bound(w, tables, lam, g, pi, fa, fb):
    """(B_gamma relative, B_pi relative, B_elbo absolute) of ONE iteration of one recording from gamma ``g`` (n, K) and priors ``pi``
    (K,): the module docstring's formulas, evaluated in float64."""
    psi, r, ib = tables
    n, D = w.shape
    K = g.shape[1]
    Fr = fa / fb
    lp, ent, alpha, invL, G = posterior_terms(w, tables, g, fa, fb)
    arho, aal = np.abs(r[None, :] * w), np.abs(alpha)
    dF = (2 * n + 1) * U * (g.T @ arho)
    eL = (n + 5) * U
    dal = (eL + 3 * U) * aal + Fr * invL * dF
    q = ((invL + alpha * alpha) * psi[None, :]).sum(1)
    dq = ((eL * invL + 2 * aal * dal) * psi[None, :]).sum(1) + (2 * D + 3) * U * q
    alog = np.abs(np.log(invL))
    mag = alog + invL + alpha * alpha + 1.0
    dent = (eL + 2 * U * alog + eL * invL + 2 * aal * dal + 4 * U * mag).sum(1) + D * U * mag.sum(1)
    dot = (r[None, :] * w) @ alpha.T
    dlp = fa * ((2 * D + 1) * U * (arho @ aal.T) + arho @ dal.T + 0.5 * dq[None, :] + (2 * D + 3) * U * np.abs(G)[:, None]
                + 4 * U * (np.abs(dot) + 0.5 * q[None, :] + np.abs(G)[:, None]))
    m = lp.max(1)
    theta = dlp + U * np.abs(lp - m[:, None]) + 2 * U
    Theta = float(theta.max(1).sum())
    # the scales of a plain forward pass: |log c_t| enters the ELBO's bound
    p, a, logc = np.exp(lp - m[:, None]), np.zeros(K), np.zeros(n)
    for t in range(n):
        at = p[t] * (lam[t] * a + (1.0 - lam[t]) * pi)
        logc[t] = np.log(at.sum())
        a = at / at.sum()
    fbw = (26 * n + 2) * U
    S = float(np.abs(logc).sum() + np.abs(m).sum())
    lpx = float((logc + m).sum())
    Bg = 1.05 * (2 * Theta + fbw)
    Bp = 1.05 * (2 * (2 * Theta + fbw + (n + 5) * U) + 8 * U)
    Be = 1.05 * (Theta + 12 * n * U + 3 * U * float(np.abs(logc).sum()) + (n + 1) * U * S
                 + 0.5 * fb * (float(dent.sum()) + (K + 2) * U * float(np.abs(ent).sum())) + 2 * U * (abs(lpx) + 0.5 * fb * abs(float(ent.sum()))))
    return Bg, Bp, Be


def within(got, want, rel):
    """got against want under the relative bound ``rel``; entries of ``want`` below TINY absolutely."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    tol = np.where(np.abs(want) < TINY, TINY, rel * np.abs(want))
    return np.abs(got - want) <= tol


def check_one_iteration(case, got, exact, params, it_col=0, gamma=None, pi=None):
    """Holds ``got`` (a Vbx whose column ``it_col`` of elbo is the iteration in question) to the bound around ``exact`` (the
    extended-precision twin's ONE iteration from ``gamma`` / ``pi``, default the case's warm start).  Returns the largest used share of
    the three bounds."""
    row0, Ks = case["row0"], case["n_models"]
    gamma = case["gamma"] if gamma is None else gamma
    pi = case["pi"] if pi is None else pi
    D, used, e0 = case["D"], [0.0, 0.0, 0.0], 0
    for r in range(len(row0) - 1):
        lo, hi, K = int(row0[r]), int(row0[r + 1]), int(Ks[r])
        n = hi - lo
        if n == 0:
            continue
        sl = slice(e0, e0 + n * K)
        e0 += n * K
        lam = lambdas(None if case["chain_start"] is None else case["chain_start"][lo:hi], n, params["loop_prob"])
        Bg, Bp, Be = one_iteration_bound(case["rows"][lo:hi, :D].astype(np.float64), case["tables"], lam,
                                         np.asarray(gamma[sl], dtype=np.float64).reshape(n, K), np.asarray(pi[r, :K], dtype=np.float64),
                                         params["fa"], params["fb"])
        wg = np.asarray(exact.gamma[sl], dtype=np.float64).reshape(n, K)
        gg = np.asarray(got.gamma[sl], dtype=np.float64).reshape(n, K)
        assert exact.iters_run[r] == 1 and got.iters_run[r] >= 1
        assert within(gg, wg, Bg).all(), "gamma of recording %d leaves its bound %g" % (r, Bg)
        assert within(got.pi[r, :K], exact.pi[r, :K], Bp).all() and (np.asarray(got.pi[r, K:]) == 0).all(), "pi of recording %d" % r
        de = abs(float(got.elbo[r, it_col]) - float(exact.elbo[r, 0]))
        assert de <= Be, "elbo of recording %d: off by %g, bound %g" % (r, de, Be)
        # an admissible argmax: a k whose exact posterior is within the bound of the row's maximum
        lab = np.asarray(got.labels[lo:hi])
        assert ((lab >= 0) & (lab < K)).all()
        assert (wg[np.arange(n), lab] >= wg.max(1) * (1.0 - Bg) / (1.0 + Bg)).all(), "labels of recording %d" % r
        big = np.abs(wg) >= TINY
        used[0] = max(used[0], float((np.abs(gg - wg)[big] / (Bg * np.abs(wg)[big])).max()))
        used[1] = max(used[1], float((np.abs(np.asarray(got.pi[r, :K], dtype=np.float64) - np.asarray(exact.pi[r, :K], dtype=np.float64))
                                      / (Bp * np.asarray(exact.pi[r, :K], dtype=np.float64))).max()))
        used[2] = max(used[2], de / Be)
    return used


# ---- the planted corpus ----------------------------------------------------------------------------------------------------------------
PLANTED_E, PLANTED_SPEAKERS = 8, 3


def planted_corpus(seed=3, turns=9, between=4.0):
    """One conversation from the two-covariance generator of tests/plda_cases.py: 3 speakers (between covariance ``between`` I, within
    covariance I around a mean away from the origin), turns of 8 .. 20 windows, never the same speaker twice in a row.  The initial
    labels split every speaker in two (K = 6).  -> (PldaModel, rows (n, P) fp32 as the model projects them, truth (n,), labels (n,))."""
    from tests import plda_cases as PC
    rng = np.random.RandomState(seed)
    mu, Phi_b, Phi_w = np.full(PLANTED_E, 0.5), between * np.eye(PLANTED_E), np.eye(PLANTED_E)
    x, spk = PC.two_covariance_corpus(seed, PLANTED_SPEAKERS, 20 * turns, PLANTED_E, Phi_b, Phi_w, mu)
    pool = [list(np.flatnonzero(spk == s)) for s in range(PLANTED_SPEAKERS)]
    order, truth, prev = [], [], -1
    for _ in range(turns):
        s = int(rng.randint(PLANTED_SPEAKERS))
        if s == prev:
            s = (s + 1 + int(rng.randint(PLANTED_SPEAKERS - 1))) % PLANTED_SPEAKERS
        k = int(rng.randint(8, 21))
        order += [pool[s].pop() for _ in range(k)]
        truth += [s] * k
        prev = s
    truth = np.array(truth, dtype=np.int64)
    labels = (2 * truth + (np.arange(len(truth)) % 2)).astype(np.int32)
    model = PL.PldaModel.from_covariances(mu, Phi_b, Phi_w)
    return model, model.project_numpy(x[order]), truth, labels


def planted_ok(labels, truth):
    """Exactly 3 labels survive and they are the planted speakers up to a permutation."""
    found = np.unique(labels)
    if len(found) != PLANTED_SPEAKERS:
        return False
    return all(len(np.unique(labels[truth == s])) == 1 for s in range(PLANTED_SPEAKERS)) and \
        len({int(labels[truth == s][0]) for s in range(PLANTED_SPEAKERS)}) == PLANTED_SPEAKERS
