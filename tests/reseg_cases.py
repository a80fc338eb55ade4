"""Case builders shared by tests/test_reseg_cpu.py and tests/test_gpu_reseg.py (resegmentation: voicemap_amd/diarization.py
resegment / reseg_reference, csrc/reseg.hip).

Grid embeddings.  Every speaker is ONE point, every row of the speaker is that point, so a model whose rows all belong to one speaker
is that point exactly (a sum of n equal dyadic vectors, divided by n) and its emissions are exact in every summation order:
  euclidean    integer points on the axes, magnitudes 3 and 4 on neighbouring axes: the distances between pure models are integers
               or roots of integer sums (3-4-5 among them), the squares summed are integers;
  cosine       unit axis vectors +-e_a: every dot product has one non-zero term, every norm is 1;
  dot_product  the same rows times 1/2.
With more speakers than 2 E (cosine, dot_product) two speakers share a point: their models tie, which is wanted.  The planted label
sequences carry isolated flips (a model then mixes two points: its emissions are no longer exact numbers, but both sides round the
same float64 sums of a few dyadic terms), rows of no model (-1), labels out of range, and -- where K exceeds the speakers present --
clusters that are dead from the start.
"""
import itertools

import numpy as np

U = 2.0 ** -53
KINDS = ("euclidean", "cosine", "dot_product")


def speaker_points(kind, S, E):
    """(S, E) fp32: the point of every speaker."""
    pts = np.zeros((S, E), np.float32)
    for s in range(S):
        a, rnd = s % E, s // E
        if kind == "euclidean":
            pts[s, a] = (3 if a % 2 == 0 else 4) + rnd
        else:
            pts[s, a] = (1.0 if rnd % 2 == 0 else -1.0) * (1.0 if kind == "cosine" else 0.5)
    return pts


def planted_sequence(rng, n, S):
    """n speaker indices in turns of 1 .. 6 rows, never the same speaker twice in a row (when S > 1)."""
    out, prev = [], -1
    while len(out) < n:
        s = int(rng.randint(S))
        if S > 1 and s == prev:
            s = (s + 1 + int(rng.randint(S - 1))) % S
        out += [s] * int(rng.randint(1, 7))
        prev = s
    return np.array(out[:n], dtype=np.int64)


def spoiled_labels(rng, truth, K, flip=0.1, none=0.1, wild=0.05):
    """The planted labels with isolated flips to another model, rows of no model (-1) and labels out of range (K, 99, -7)."""
    lab = truth.astype(np.int32).copy()
    n = len(lab)
    u = rng.uniform(size=n)
    f = u < flip
    lab[f] = rng.randint(0, K, size=int(f.sum()))
    lab[(u >= flip) & (u < flip + none)] = -1
    w = (u >= flip + none) & (u < flip + none + wild)
    lab[w] = rng.choice([K, 99, -7], size=int(w.sum()))
    return lab


def chain_table(rng, sizes, mode):
    """None | "edges": a start at the first and the last row of every recording and at a few rows between | "all": every row."""
    N = int(np.sum(sizes))
    if mode is None:
        return None
    if mode == "all":
        return np.ones(N, np.int32)
    cs = (rng.uniform(size=N) < 0.05).astype(np.int32) * 7   # any non-zero value starts a chain
    lo = 0
    for n in sizes:
        if n:
            cs[lo], cs[lo + n - 1] = 1, 1
        lo += n
    return cs


def grid_case(seed, sizes, K, E, kind, chains=None, speakers=None):
    """One vm_reseg call on grid rows: ``sizes`` rows per recording, K models each, ``speakers`` (default min(K, 3)) speakers present
    per recording.  -> dict(emb, row0, n_models, labels, chain_start, truth)."""
    rng = np.random.RandomState(seed)
    S = min(K, 3) if speakers is None else speakers
    pts = speaker_points(kind, S, E)
    emb, lab, truth = [], [], []
    for n in sizes:
        t = planted_sequence(rng, n, S)
        truth.append(t)
        emb.append(pts[t])
        lab.append(spoiled_labels(rng, t, K))
    row0 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return {"emb": np.concatenate(emb).astype(np.float32).reshape(-1, E), "row0": row0, "n_models": np.full(len(sizes), K, np.int64),
            "labels": np.concatenate(lab).astype(np.int32), "chain_start": chain_table(rng, sizes, chains),
            "truth": np.concatenate(truth)}


def general_case(seed, sizes, K, E, chains=None):
    """Random normal rows around K centres per recording, labels = the centre with a tenth flipped."""
    rng = np.random.RandomState(seed)
    emb, lab = [], []
    for n in sizes:
        centres = 2.0 * rng.randn(K, E)
        t = planted_sequence(rng, n, K)
        emb.append(centres[t] + rng.randn(n, E))
        lab.append(spoiled_labels(rng, t, K, none=0.05, wild=0.0))
    row0 = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return {"emb": np.concatenate(emb).astype(np.float32).reshape(-1, E), "row0": row0, "n_models": np.full(len(sizes), K, np.int64),
            "labels": np.concatenate(lab).astype(np.int32), "chain_start": chain_table(rng, sizes, chains)}


def emission_tolerance(emb, label, sc, kind, K):
    """The tolerance of a device emission against the float64 twin ``sc`` (n, K) of ONE recording: one fp32 ulp of fp32(sc) plus an
    absolute floor for the float64 rounding of the sums, which the two sides add in different orders -- the reasoning of
    tests/test_gpu_enrolment.py without its leave-one-out term.  With u = 2^-53, n the largest model size and E components, a model
    component carries at most ~n u of relative rounding from its sum (plus a few u from the divisions), the E-term score sum another
    ~E u, so with g = 8 (n + E) u:
      euclidean   |d sqrt(sum (q - p)^2)| <= g (|q| + |p|) <= g 2 R                       (R = the largest row norm; |p| <= R)
      dot_product |d q.p| <= g |q| |p| <= g R^2
      cosine      the models are means of unit vectors: |d p| <= g against |p| >= p_min (the smallest model norm), so
                  |d cos| <= 2 g / p_min"""
    from voicemap_amd import enrolment as EN
    label = np.asarray(label)
    ok = (label >= 0) & (label < K)
    n = int(np.bincount(label[ok], minlength=K).max())
    g = 8.0 * (n + emb.shape[1]) * U
    R = float(np.linalg.norm(emb.astype(np.float64), axis=1).max())
    if kind == "euclidean":
        floor = g * 2 * R
    elif kind == "dot_product":
        floor = g * R * R
    else:
        sm, _, count = EN.speaker_sums_numpy(emb, label, K, 1)
        pn = np.linalg.norm(sm[count > 0] / count[count > 0, None], axis=1)
        floor = 2 * g / float(np.nanmin(pn))
    with np.errstate(invalid="ignore"):
        return np.spacing(np.abs(sc.astype(np.float32))).astype(np.float64) + floor


def brute_force(emis, chain_start, switch_cost):
    """The smallest cost over ALL K^n label sequences of ONE recording, in float64: the emissions of the labels plus ``switch_cost`` per
    change of label inside a chain.  On dyadic emissions and costs every sum is exact, so the order of the additions does not matter."""
    e = np.asarray(emis, dtype=np.float64)
    n, K = e.shape
    start = np.zeros(n, bool) if chain_start is None else np.asarray(chain_start) != 0
    start[0] = True
    best = np.inf
    for seq in itertools.product(range(K), repeat=n):
        c = 0.0
        for t, k in enumerate(seq):
            c += e[t, k]
            if not start[t] and seq[t - 1] != k:
                c += switch_cost
        best = min(best, c)
    return best


def path_cost(emis, chain_start, switch_cost, labels):
    """The cost of one label sequence, as ``brute_force`` counts it."""
    e = np.asarray(emis, dtype=np.float64)
    start = np.zeros(len(e), bool) if chain_start is None else np.asarray(chain_start) != 0
    start[0] = True
    return float(sum(e[t, k] for t, k in enumerate(labels)) + switch_cost * sum(1 for t in range(1, len(e))
                                                                                  if not start[t] and labels[t] != labels[t - 1]))
