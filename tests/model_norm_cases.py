"""Shared builders of the model-trial score-normalisation tests (tests/test_model_norm_cpu.py, tests/test_gpu_model_norm.py): grid corpora
on which every float64 score is exact, random corpora, the planted corpus of the end-to-end claim, and the brute-force restatement of
the definitions (include/voicemap_hip.h, "Score normalisation of speaker-model trials") in Python loops."""
import math

import numpy as np

from voicemap_amd import plda as PL
from voicemap_amd import verification as V

KINDS = ["euclidean", "cosine", "dot_product"]
KIND_ID = {"euclidean": 0, "cosine": 1, "dot_product": 2}
N_MAX = 9


# ---- corpora ---------------------------------------------------------------------------------------------------------------------------
def lattice(sizes, E, seed, twins=False, shuffle=True):
    """Integer embeddings in [-8, 8]; speaker s has sizes[s] rows (0: a speaker without rows).  With dyadic sizes every euclidean model
    is dyadic and every squared distance exact in float64 in any order.  ``twins``: the last speaker holds copies of the rows of the one
    before it, so every foreign row ties between the two."""
    r = np.random.default_rng(seed)
    label = np.repeat(np.arange(len(sizes)), sizes)
    emb = r.integers(-8, 9, (len(label), E)).astype(np.float32)
    if twins:
        assert sizes[-1] == sizes[-2]
        emb[label == len(sizes) - 1] = emb[label == len(sizes) - 2][::-1]
    if shuffle:
        p = r.permutation(len(label))
        emb, label = emb[p], label[p]
    return emb, label.astype(np.int32)


def lattice_rows(n, E, seed, dup=False):
    """n integer rows; ``dup``: every row twice (massive ties: every score of a line comes in equal pairs)."""
    r = np.random.default_rng(seed)
    x = r.integers(-8, 9, (n, E)).astype(np.float32)
    if dup:
        x[1::2] = x[0:2 * (n // 2):2][:len(x[1::2])]
    return x


def random_corpus(N, S, E, seed, noise=1.0):
    """Speaker centre + noise; unequal speaker sizes with a one-file speaker (index 0) and one un-enrolled row (label -1)."""
    r = np.random.default_rng(seed)
    label = np.zeros(N, dtype=np.int64)
    if S > 1 and N > 2:
        label[1:] = r.integers(1, S, N - 1)
        label[-1] = -1
    cent = r.normal(0, 1, (S, E))
    emb = (cent[np.maximum(label, 0)] + r.normal(0, noise, (N, E))).astype(np.float32)
    return emb, label.astype(np.int32)


def plda_grid_tables(rng, D):
    """Dyadic tables: A in {1/4, 1/2, 1, 2}, beta in {1, 1/2, 1/4, 1/8}, G in {1/4, 1/2, 1, 2}, C a multiple of 1/16 in [-8, 8]; row 0
    holds a value that would show if it were read."""
    A = 2.0 ** rng.integers(-2, 2, (N_MAX + 1, D))
    beta = 2.0 ** -rng.integers(0, 4, (N_MAX + 1, D)).astype(np.float64)
    C = rng.integers(-128, 129, N_MAX + 1) / 16.0
    G = 2.0 ** rng.integers(-2, 2, D)
    A[0], beta[0], C[0] = 1e300, 1e300, 1e300
    return {"A": A, "beta": beta, "C": C, "G": G.astype(np.float64)}


def plda_grid_rows(rng, sizes, D, shuffle=True):
    """PLDA-space rows on the grid w = k / 8, |k| <= 16 (every product and sum of the score is then exact in float64 for up to 10 rows
    per model and 255 components); speaker s has sizes[s] rows.  The row term (last column) is never read."""
    P = PL.padded_width(D)
    label = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    x = np.zeros((len(label), P), np.float32)
    x[:, :D] = rng.integers(-16, 17, (len(label), D)) / 8.0
    x[:, -1] = rng.normal(size=len(label))
    if shuffle:
        p = rng.permutation(len(label))
        x, label = x[p], label[p]
    return x, label


def plda_sizes(S):
    """Counts that cycle through no rows, one row, past n_max and n_max."""
    cyc = [3, 0, 1, N_MAX + 1, N_MAX, 2, 5, 4, 1, 7]
    return [cyc[s % len(cyc)] for s in range(S)]


def planted(seed=5, S=24, Sc=30, per=6, E=16):
    """The end-to-end plant: every speaker has its own noise level sigma_s = exp(U(-1.3, 1.3)), so its target and non-target euclidean
    scores carry their own offset and scale (a loud speaker's target scores look like a quiet speaker's non-target scores) -- what
    S-norm / AS-norm remove.  Returns the enrolled rows, the test rows of the same speakers, and a cohort of other speakers drawn the
    same way: (emb, spk), (test, test_spk), (cohort, cohort_spk), speaker codes not dense."""
    r = np.random.default_rng(seed)

    def draw(n_spk, code0, n_per):
        cent = r.normal(0, 1.0, (n_spk, E))
        sig = np.exp(r.uniform(-1.3, 1.3, n_spk))
        spk = np.repeat(np.arange(n_spk), n_per)
        x = (cent[spk] + r.normal(0, 1, (len(spk), E)) * sig[spk, None]).astype(np.float32)
        return x, spk, cent, sig
    emb, spk, cent, sig = draw(S, 0, per)
    tspk = np.repeat(np.arange(S), per)
    test = (cent[tspk] + r.normal(0, 1, (len(tspk), E)) * sig[tspk, None]).astype(np.float32)
    coh, cspk, _, _ = draw(Sc, 0, per)
    return (emb, spk * 3 + 100), (test, tspk * 3 + 100), (coh, cspk * 5 + 7)


# ---- the brute-force restatement ---------------------------------------------------------------------------------------------------------
def _contrib(row, kind):
    v = [float(x) for x in row]
    mag = math.sqrt(sum(x * x for x in v))
    if kind == 0:
        return v, mag
    return [x / mag if mag != 0.0 else (math.nan if x == 0.0 else math.copysign(math.inf, x)) for x in v], mag


def brute_sums(emb, label, S, kind):
    """sum_s, msum_s, count_s: the rows of s added in ascending row order."""
    E = emb.shape[1]
    sums, msum, count = [[0.0] * E for _ in range(S)], [0.0] * S, [0] * S
    for u in range(len(emb)):
        s = int(label[u])
        if 0 <= s < S:
            c, mag = _contrib(emb[u], kind)
            for e in range(E):
                sums[s][e] += c[e]
            msum[s] += mag
            count[s] += 1
    return sums, msum, count


def brute_score(row, Sigma, msum, n, kind, tables=None):
    """score(row, model) of the definitions as an fp32 number; NaN where the model has no rows (PLDA: n outside 1..n_max)."""
    with np.errstate(all="ignore"):
        if tables is not None:
            A, beta, C, G = tables["A"], tables["beta"], tables["C"], tables["G"]
            if not 1 <= n <= len(C) - 1:
                return np.float32(np.nan)
            acc = g = 0.0
            for d in range(len(G)):
                w = float(row[d])
                t = w - float(beta[n][d]) * Sigma[d]
                acc += (float(A[n][d]) * t) * t
                g += float(G[d]) * (w * w)
            return np.float32((acc - g) - float(C[n]))
        if n <= 0:
            return np.float32(np.nan)
        q = [float(x) for x in row]
        p = [x / n for x in Sigma]
        if kind == 2:
            p = [(msum / n) * x for x in p]
        if kind == 0:
            return np.float32(math.sqrt(sum((a - b) ** 2 for a, b in zip(q, p))))
        dot = sum(a * b for a, b in zip(q, p))
        if kind == 2:
            return np.float32(-dot)
        den = math.sqrt(sum(a * a for a in q)) * math.sqrt(sum(b * b for b in p))
        return np.float32(1.0 - np.float64(dot) / np.float64(den))


def brute_line(values, K):
    """(mu, sigma, rsig, count, selected indices) of one line of fp32 scores by vm_cohort_topk_stats' rules."""
    v = np.asarray(values, dtype=np.float32)
    keys = V.score_keys(v)
    order = sorted((int(keys[i]), i) for i in range(len(v)) if not np.isnan(v[i]))[:K]
    if not order:
        return np.float32(np.nan), np.float32(np.nan), np.float32(np.nan), 0, []
    sel = [float(v[i]) for _, i in order]
    mean = sum(sel) / len(sel)
    sig = np.float32(math.sqrt(sum((x - mean) ** 2 for x in sel) / len(sel)))
    with np.errstate(divide="ignore"):
        rsig = np.float32(np.float64(1.0) / np.float64(sig))
    return np.float32(mean), sig, rsig, len(sel), [i for _, i in order]


def brute_norm_stats(emb, label, q, q_label, cohort, cohort_label, kind, top_k, loo, S, tables=None):
    """The three sets of statistics, every score and every line in Python loops.  Also returns the three score matrices (lists)."""
    kind = 0 if tables is not None else KIND_ID.get(kind, kind)
    Sc = int(np.max(cohort_label)) + 1
    C = len(cohort)
    Kq = Sc if top_k is None else min(top_k, Sc)
    Ks = C if top_k is None else min(top_k, C)
    sums, msum, count = brute_sums(emb, label, S, kind)
    csums, cmsum, ccount = brute_sums(cohort, cohort_label, Sc, kind)
    out = {}
    lines_q = [[brute_score(q[m], csums[s], cmsum[s], ccount[s], kind, tables) for s in range(Sc)] for m in range(len(q))]
    lines_s = [[brute_score(cohort[c], sums[s], msum[s], count[s], kind, tables) for c in range(C)] for s in range(S)]
    sets = [("q", lines_q, Kq), ("s", lines_s, Ks)]
    if loo:
        lines_o = []
        for m in range(len(q)):
            s = int(q_label[m])
            if 0 <= s < S and count[s] > 1:
                c, mag = _contrib(q[m], kind)
                Sig = [a - b for a, b in zip(sums[s], c)]
                lines_o.append([brute_score(cohort[k], Sig, msum[s] - mag, count[s] - 1, kind, tables) for k in range(C)])
            else:
                lines_o.append([np.float32(np.nan)] * C)
        sets.append(("own", lines_o, Ks))
    for name, lines, K in sets:
        st = [brute_line(ln, K) for ln in lines]
        out["mu_" + name] = np.array([x[0] for x in st], np.float32)
        out["sigma_" + name] = np.array([x[1] for x in st], np.float32)
        out["rsig_" + name] = np.array([x[2] for x in st], np.float32)
        out["count_" + name] = np.array([x[3] for x in st], np.int32)
        out["lines_" + name] = np.array(lines, np.float32).reshape(len(lines), -1)
    return out


def brute_normalise(scores, q_label, st, loo):
    """s' of every cell of an (M, S) fp32 matrix, one np.float32 operation at a time."""
    M, S = scores.shape
    out = np.zeros((M, S), np.float32)
    h = np.float32(0.5)
    with np.errstate(all="ignore"):
        for m in range(M):
            for s in range(S):
                own = loo and int(q_label[m]) == s
                muM, rsM = (st["mu_own"][m], st["rsig_own"][m]) if own else (st["mu_s"][s], st["rsig_s"][s])
                a = np.float32(scores[m, s] - st["mu_q"][m])
                b = np.float32(scores[m, s] - muM)
                out[m, s] = h * np.float32(np.float32(a * st["rsig_q"][m]) + np.float32(b * rsM))
    return out
