"""Exact references for the embedding scorers (tests/test_gpu_score_exact.py; checked on the host by tests/test_score_exact_cpu.py).

The four kernels that score cached embeddings -- pairdist_kernel (eval.hip), pair_hist_kernel (verif.hip), cohort_score_kernel
(cohort.hip) and mine_kernel (mine.hip) -- run one tile loop (score_tile_loop, csrc/score_tile.hpp; pair_hist_kernel holds a copy of it), and the
rest of the suite checks three of them against the fourth.  This module is the anchor outside that loop: pure numpy, it imports neither the library nor torch.

Method (that of gemm_exact.py / bn_exact.py / spectro_exact.py).  Embeddings are integers in [-8, 8] times one power of two per case
(2^-3, 2^0, 2^2).  With E <= 256 every (a - b)^2, a * b and w * |a - b| (w a signed power of two) and every partial sum IN ANY ORDER
is an fp32 number: at most 256 * 16^2 = 2^16 grid units, far below 2^24 (``headroom`` computes the figure of a case; the host test asserts
it for every case).  So the accumulator a kernel holds before its epilogue is known exactly, whatever its summation order, and the
score is that exact sum followed by the kernel's stated single fp32 operations:

    euclidean       float32(sqrt(float64(sum)))     (for every integer 0 .. 65 536 this equals the fp32 square root bit for bit)
    neg_euclidean   its negation
    dot_product     -acc; a zero sum is -0.0 and the sign bit is compared
    weighted_l1     acc
    cosine          rsq exact, then sqrtf, qn * rn, acc / (.), 1 - (.) as fp32 operations one by one (pairdist_kernel's order)

The cosine is held to bit equality like the others.  The library is built without a fast-math flag (voicemap_amd/build.py), so the
device's fp32 sqrtf and division are correctly rounded and the five-operation chain above reproduces bit for bit: on the MI355X every
cosine case of the device file came out equal, 0 / 0 = NaN of a zero row included.  (``cosine_bound`` counts the chain's roundings
against float64; the host test holds ``pair_scores`` to it, the device test does not need it.)

The argmin reference is the contract as the code has it: first minimum, the query's own row q_row0 + m excluded, NaN never chosen, a
row with nothing below +inf gives (+inf, -1).  ``plant_ties`` copies one reference row to several indices after asserting that it is
the strict nearest of its queries, so the expected answer is the smallest surviving index; TIE_CLASSES names where the copies sit
relative to the kernel's five places of "first minimum wins" (a lane's two references, the shuffle butterfly, the tiles of a split, the
splits, the excluded own row).

The n-shot part restates voicemap/utils.py:159-206 in float64 with exact per-class means (n in 1, 2, 4, 8: dyadic), duplicated
classes (bit-identical arithmetic under every distance: the lower class must win) and NaN classes (numpy.argmin's order: the first
NaN wins)."""
import numpy as np

KINDS = {"euclidean": 0, "cosine": 1, "dot_product": 2, "weighted_l1": 3, "neg_euclidean": 4}
PAIRDIST_KINDS = ("euclidean", "cosine", "dot_product")
LIMIT = 1 << 24                    # integers below it are fp32 numbers
SCALES = (2.0 ** -3, 1.0, 4.0)
PD_T, PD_RT, PD_MAX_E = 64, 128, 256   # csrc/score_tile.hpp's ST_*: queries per workgroup, references per stage, the widest embedding
U = 2.0 ** -24                     # fp32 unit roundoff

# every side of the 4-wide vector, of the 64-component chunk and of PD_MAX_E
E_TABLE = (1, 2, 3, 4, 5, 7, 32, 60, 63, 64, 65, 67, 68, 100, 127, 128, 129, 130, 192, 193, 253, 255, 256)
M_VALUES = (1, 7, 8, 9, 63, 64, 65, 130)
N_VALUES = (1, 63, 64, 65, 127, 128, 129, 257)
# (M, N, q_row0); q_row0 >= 0: the queries are rows q_row0 .. q_row0 + M of the reference matrix (a row shard against the whole)
SHAPES = (
    (1, 1, -1), (1, 1, 0), (1, 63, -1), (1, 64, 31), (1, 257, 256),
    (7, 1, -1), (7, 63, -1), (7, 64, 0), (7, 65, 29), (7, 257, 250),
    (8, 64, -1), (8, 65, 57), (8, 127, 0), (8, 128, 60),
    (9, 1, -1), (9, 63, 54), (9, 129, -1), (9, 128, 0), (9, 257, 124),
    (63, 63, 0), (63, 64, -1), (63, 65, 2), (63, 127, 64), (63, 257, -1),
    (64, 64, 0), (64, 65, -1), (64, 128, 64), (64, 129, 33), (64, 257, 193),
    (65, 65, 0), (65, 63, -1), (65, 127, -1), (65, 128, 63), (65, 129, 64), (65, 257, 96),
    (130, 1, -1), (130, 64, -1), (130, 129, -1), (130, 257, 0), (130, 257, 60), (130, 257, 127),
)
# (M, N) -> (splits, tiles_per_split, empty trailing splits) of pd_splits: the plans no other test runs
SPLIT_PLANS = {(16384, 1100): (8, 2, 3), (8192, 2200): (16, 2, 7), (4096, 8320): (32, 3, 10)}
SPLIT_E = (3, 4, 5)
TIE_CLASSES = ("same_lane", "two_lanes", "two_tiles_one_split", "two_splits", "last_partial_tile", "own_before", "own_after")
# the copies: widths on the scalar fetch path, and a row shard that is a multiple of neither 8 nor 64 at either end
COPY_E = (1, 2, 3, 5, 63, 65, 67, 130, 253)
COPY_N, COPY_ROWS = 257, (37, 203)


# ---- grid inputs --------------------------------------------------------------------------------------------------------------------
def grid(rng, shape, scale, amp=8):
    """Integers in [-amp, amp] times ``scale`` (a power of two), fp32."""
    return (rng.integers(-amp, amp + 1, shape) * scale).astype(np.float32)


def lattice_weights(rng, E):
    """Signed powers of two 2^-3 .. 2^2, a fifth of them negative (test_weighted_l1_on_a_lattice_is_exact's)."""
    return (2.0 ** rng.integers(-3, 3, E) * np.where(rng.random(E) < 0.2, -1, 1)).astype(np.float32)


def grid_unit(x):
    """The largest power of two that divides every finite non-zero entry of x (1.0 for an all-zero array)."""
    x = np.asarray(x, dtype=np.float64)
    x = np.abs(x[np.isfinite(x) & (x != 0)])
    if x.size == 0:
        return 1.0
    for k in range(12, -31, -1):
        if np.all(x / 2.0 ** k == np.round(x / 2.0 ** k)):
            return 2.0 ** k
    raise AssertionError("not on a dyadic grid")


def headroom(q, ref, kind, weights=None):
    """An upper bound, in grid units, of sum_e |term_e| for every (query, reference) pair: below LIMIT every partial sum in any order
    is an fp32 number."""
    amax = max(float(np.abs(q).max()), float(np.abs(ref).max()))
    u = min(grid_unit(q), grid_unit(ref))
    E = q.shape[1]
    if kind == "weighted_l1":
        return float(np.abs(weights).sum()) * 2.0 * amax / (u * grid_unit(weights))
    if kind in ("euclidean", "neg_euclidean"):
        return E * (2.0 * amax / u) ** 2
    return E * (amax / u) ** 2


# ---- reference scores ---------------------------------------------------------------------------------------------------------------
def exact_sums(q, ref, kind, weights=None):
    """float64 (M, N): sum (a - b)^2, sum a * b or sum w |a - b|, exact on grid inputs (every term and partial sum is a float64 number)."""
    q64, r64 = np.asarray(q, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "weighted_l1":
            w = np.asarray(weights, dtype=np.float64)
            out = np.empty((len(q64), len(r64)))
            for m0 in range(0, len(q64), 16):
                out[m0:m0 + 16] = np.abs(q64[m0:m0 + 16, None, :] - r64[None, :, :]) @ w
            return out
        g = q64 @ r64.T
        if kind in ("euclidean", "neg_euclidean"):
            return (q64 * q64).sum(1)[:, None] + (r64 * r64).sum(1)[None, :] - 2.0 * g
        return g


def pair_scores(q, ref, kind, weights=None):
    """The fp32 (M, N) score matrix of ``kind``: exact sums, then the kernel's single fp32 operations."""
    f32 = np.float32
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind == "cosine":
            acc = exact_sums(q, ref, "dot_product").astype(f32)
            q64, r64 = np.asarray(q, dtype=np.float64), np.asarray(ref, dtype=np.float64)
            qn = np.sqrt((q64 * q64).sum(1).astype(f32))          # fp32 sqrt of the exact fp32 squared norm
            rn = np.sqrt((r64 * r64).sum(1).astype(f32))
            den = qn[:, None] * rn[None, :]
            return (f32(1.0) - acc / den).astype(f32)
        s = exact_sums(q, ref, kind, weights)
        if kind == "euclidean":
            return np.sqrt(s).astype(f32)
        if kind == "neg_euclidean":
            return -(np.sqrt(s).astype(f32))
        if kind == "dot_product":
            return -(s.astype(f32))
        return s.astype(f32)


def cosine_float64(q, ref):
    q64, r64 = np.asarray(q, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (q64 @ r64.T) / (np.sqrt((q64 * q64).sum(1))[:, None] * np.sqrt((r64 * r64).sum(1))[None, :])


def cosine_bound(c):
    """|d - (1 - c)| for d = 1 - acc / (sqrtf(qsq) * sqrtf(rsq)) with exact acc, qsq, rsq and c their float64 quotient: two square roots,
    one product and one quotient each put a relative 2^-24 on the quotient (4 u |c|, second-order terms in the 1.01), the difference
    rounds once more (u |1 - c|)."""
    return 1.01 * U * (4.0 * np.abs(c) + np.abs(1.0 - c)) + 1e-45


# ---- argmin reference ---------------------------------------------------------------------------------------------------------------
def first_argmin(scores, q_row0=-1):
    """(best_val fp32 (M), best_idx int32 (M)) of vm_pairdist_argmin's contract: the FIRST minimum of row m over the reference rows other
    than q_row0 + m; NaN is never chosen; a row with nothing below +inf gives (+inf, -1)."""
    s = np.asarray(scores, dtype=np.float32)
    M, N = s.shape
    c = np.where(np.isnan(s), np.float32(np.inf), s)
    if q_row0 >= 0:
        own = q_row0 + np.arange(M)
        ok = own < N
        c[np.arange(M)[ok], own[ok]] = np.inf
    idx = c.argmin(1).astype(np.int32)
    val = c[np.arange(M), idx].astype(np.float32)
    none = ~(val < np.inf)
    idx[none] = -1
    val[none] = np.inf
    return val, idx


def split_plan(M, N):
    """pd_splits (csrc/eval.hip) and what follows from it: (splits, tiles_per_split, empty trailing splits)."""
    mt, nt = -(-M // PD_T), -(-N // PD_RT)
    s = max(1, min(-(-2048 // mt), nt))
    tps = -(-nt // s)
    return s, tps, s - -(-nt // tps)


def splits_from_workspace(nbytes, M, N):
    """The split count inside vm_pairdist_workspace_bytes(M, N): minus the two squared-norm vectors, the scalar-path copy of the queries
    (8-row groups x PD_MAX_E) and their two 256-byte paddings, over the 8 bytes of a partial minimum per split and query."""
    fixed = (M + N) * 4 + 256 + -(-M // 8) * 8 * PD_MAX_E * 4 + 256
    rest = nbytes - fixed
    assert rest > 0 and rest % (8 * M) == 0, (nbytes, M, N)
    return rest // (8 * M)


def locate(m, n, M, N, splits):
    """Where the kernel computes entry (m, n): for a mismatch report."""
    tps = -(-(-(-N // PD_RT)) // splits)
    t = n // PD_RT
    return "query row %d (workgroup %d, wave %d, slot %d), reference row %d (lane %d, half %d, tile %d, split %d)" % (
        m, m // PD_T, (m % PD_T) // 8, m % 8, n, n % 64, (n % PD_RT) // 64, t, t // tps)


# ---- planted ties -------------------------------------------------------------------------------------------------------------------
def plant_ties(ref, rows, positions, src, q=None, kind=None, q_row0=-1):
    """A copy of ``ref`` with row ``src`` copied to every index of ``positions``.  With ``q``: first asserts that before the copy row
    ``src`` is the strict nearest (under ``kind``, own rows excluded) of every query of ``rows``, so that afterwards the expected
    argmin of those queries is the smallest index of ``positions`` that is not the query's own row."""
    if q is not None:
        s = pair_scores(q[list(rows)], ref, kind)
        for k, m in enumerate(rows):
            row = np.where(np.isnan(s[k]), np.inf, s[k].astype(np.float64))
            if q_row0 >= 0 and q_row0 + m < len(ref):
                row[q_row0 + m] = np.inf
            assert src != q_row0 + m or q_row0 < 0
            assert row[src] < np.delete(row, src).min(), (kind, m, src)
    out = ref.copy()
    out[list(positions)] = ref[src]
    return out


def tie_positions(M, N, q_row0, tps):
    """TIE_CLASSES that fit the shape -> (query rows or None: assigned by the builder, positions).  Reference index n sits in tile
    n // 128 (split tile // tps), half (n % 128) // 64, lane n % 64."""
    nt = -(-N // PD_RT)
    last0 = (nt - 1) * PD_RT
    out = {}
    if N > 69:
        out["same_lane"] = (None, (5, 69))                                        # lane 5's two references
    if nt > 1 and PD_RT + 41 < N:
        out["two_lanes"] = (None, (PD_RT + 9, PD_RT + 41))                        # two lanes of the first half of tile 1
    if tps >= 2 and (tps + 1) * PD_RT + 3 < N:
        out["two_tiles_one_split"] = (None, (tps * PD_RT + 17, (tps + 1) * PD_RT + 3))   # split 1: the later tile has the lower lane
    if tps * PD_RT + 50 < N:
        out["two_splits"] = (None, (100, tps * PD_RT + 50))                       # split 0 and split 1
    if N % PD_RT != 0 and nt > 1:
        out["last_partial_tile"] = (None, (last0, N - 1) if N - 1 > last0 else (last0 - 3, last0))
    if q_row0 >= 0:
        a, b = 10, (200 if M > 200 else M - 25)
        if q_row0 + a + 64 < N and M > a:
            out["own_before"] = ((a,), (q_row0 + a, q_row0 + a + 64))             # the own row first, the other copy in the same lane
        if 0 < q_row0 + b < N and b > a:
            out["own_after"] = ((b,), (q_row0 + b - 1, q_row0 + b))               # the other copy first, in the neighbouring lane
    return out


class TieCase:
    """One (M, N, E, q_row0) problem with every tie class of ``tie_positions`` planted: base rows are integers in [-4, 4]; class c has
    its own vector v_c (+-8 at the even components, +-7 at the odd ones, its sign pattern the bits of c: no base row is parallel to
    it) and its queries are v_c with one even component one unit nearer to zero.  ``expected[m]`` = the argmin every kind must return
    for the planted queries."""

    def __init__(self, M, N, E, q_row0, scale, seed):
        assert E >= 3
        self.M, self.N, self.E, self.q_row0, self.scale = M, N, E, q_row0, scale
        self.plan = split_plan(M, N)
        rng = np.random.default_rng(seed)
        self.q = grid(rng, (M, E), scale, 4)
        base = grid(rng, (N, E), scale, 4)
        self.classes = tie_positions(M, N, q_row0, self.plan[1])
        taken_rows = {r for rows, _ in self.classes.values() if rows for r in rows}
        used_pos = [p for _, pos in self.classes.values() for p in pos]
        assert len(set(used_pos)) == len(used_pos) and max(used_pos) < N
        self.groups = []       # (class, rows, positions, src)
        for c, (name, (rows, pos)) in enumerate(self.classes.items()):
            if rows is None:
                rows = []
                for r in ((8 * c + 1) % M, (64 * (c + 1) + c) % M, M - 1 - c):
                    if r not in taken_rows:
                        taken_rows.add(r)
                        rows.append(r)
                assert rows
            v = np.array([(-1.0 if (e < 3 and (c >> e) & 1) else 1.0) * (8 if e % 2 == 0 else 7) for e in range(E)]) * scale
            for r in rows:
                j = 2 * (r % ((E + 1) // 2))
                self.q[r] = v
                self.q[r, j] -= np.sign(v[j]) * scale
            own = {q_row0 + r for r in rows} if q_row0 >= 0 else set()
            src = next(p for p in pos if p not in own)
            base[src] = v
            self.groups.append((name, tuple(rows), tuple(pos), src))
        self.before = base

    def build(self, kind):
        """(q, ref with every class planted, {query row: expected best_idx}); asserts the strict-nearest precondition under ``kind``."""
        ref = self.before
        expected = {}
        for name, rows, pos, src in self.groups:
            ref = plant_ties(ref, rows, pos, src, self.q, kind, self.q_row0)
            for r in rows:
                expected[r] = min(p for p in pos if self.q_row0 < 0 or p != self.q_row0 + r)
        return self.q, ref, expected


TIE_CASES = (
    (65, 257, 5, 96, 1.0),               # one tile per split: everything but two_tiles_one_split
    (16384, 1100, 3, 0, 2.0 ** -3), (16384, 1100, 4, 0, 1.0), (16384, 1100, 5, 0, 4.0),
    (8192, 2200, 3, 0, 1.0), (8192, 2200, 4, 0, 4.0), (8192, 2200, 5, 0, 2.0 ** -3),
    (4096, 8320, 3, 0, 4.0), (4096, 8320, 4, 0, 2.0 ** -3), (4096, 8320, 5, 0, 1.0),
)
FULL_MATRIX_SHAPE = (16384, 1100)        # the split-plan shape whose whole dist matrix is compared (72 MB); the others: argmin only


def tie_case(M, N, E, q_row0, scale):
    return TieCase(M, N, E, q_row0, scale, seed=M + 3 * N + E)


def tie_kind(M, N, E):
    """The kind a split-plan case runs under: every shape and every E meets all three."""
    return PAIRDIST_KINDS[(list(SPLIT_PLANS).index((M, N)) + E) % 3]


# ---- the small-shape cases ----------------------------------------------------------------------------------------------------------
def shape_pools(E):
    """(query pool (130, E), reference pool (257, E)) of width E: a shape (M, N, q_row0) takes ref = pool[:N] and q = qpool[:M], or with
    q_row0 >= 0 the rows q_row0 .. q_row0 + M of ref."""
    rng = np.random.default_rng(1000 + E)
    scale = SCALES[E_TABLE.index(E) % 3] if E in E_TABLE else SCALES[E % 3]
    return grid(rng, (max(M_VALUES), E), scale), grid(rng, (max(N_VALUES), E), scale)


def shape_reference(E, kind):
    """The two full reference matrices every shape of width E is a corner of: pool queries x pool references, and references x
    references (for q_row0 >= 0)."""
    qp, rp = shape_pools(E)
    return pair_scores(qp, rp, kind), pair_scores(rp, rp, kind)


def shape_scores(full_q, full_r, M, N, q_row0):
    return full_q[:M, :N] if q_row0 < 0 else full_r[q_row0:q_row0 + M, :N]


def copy_inputs(E):
    """(emb (257, E), speaker labels, lattice weights) for the three other kernels that run the tile loop."""
    rng = np.random.default_rng(5000 + E)
    emb = grid(rng, (COPY_N, E), SCALES[E % 3])
    return emb, rng.integers(0, 6, COPY_N).astype(np.int32), lattice_weights(rng, E)


# ---- n-shot -------------------------------------------------------------------------------------------------------------------------
NSHOT_DIST_CASES = ((1, 1, 1), (2, 2, 5), (64, 4, 7), (65, 8, 3), (70, 1, 16), (129, 2, 5))          # (k, n, E), 12 tasks each
NSHOT_DIST_TASKS = 12
NSHOT_IDX_CASES = ((1, 1, 3, 1), (3, 63, 5, 2), (4, 64, 4, 4), (5, 65, 6, 8), (257, 200, 5, 1), (257, 256, 3, 2),
                   (5, 1, 70, 2), (4, 256, 129, 4))                                                   # (tasks, E, k, n)


def _nshot_plan(k, t):
    """(classes that hold the nearest support set, classes that hold a NaN row) of task t; the kernels take 64 classes per pass."""
    last = k - 1
    what = t % 6
    if what == 0:
        return (), ()                                              # a plain random task
    if what == 1:
        return ((3, 67) if k > 67 else (0, last)), ()              # a tie across two passes (or the first and the last class)
    if what == 2:
        return (last,), ()                                         # the minimum only in the last pass
    if what == 3:
        return ((3,) if k > 3 else (0,)), ((66,) if k > 66 else (last,))      # a NaN in pass 1 against the minimum in pass 0
    if what == 4:
        return (0,), tuple(sorted({min(5, last), last}))           # two NaNs: the first wins
    return (min(63, last), min(64, last), last), ()                # a tie on both sides of the pass boundary


class NshotCase:
    """tasks x k x n index sets into a pool of grid rows.  Pool row 0 is u (+-8), row 1 is NaN, the others are integers in [-4, 4]
    whose first component has the sign opposite to u's (no other row is parallel to u, whatever E).  A task's query is u and its nearest
    classes hold n copies of u (planted tasks), or everything is random (plain tasks)."""

    def __init__(self, tasks, E, k, n, seed):
        self.tasks, self.E, self.k, self.n = tasks, E, k, n
        rng = np.random.default_rng(seed)
        scale = self.scale = SCALES[seed % 3]
        rows = 48
        emb = grid(rng, (rows, E), scale, 4)
        u = np.where(rng.random(E) < 0.5, -8.0, 8.0) * scale
        first = -np.sign(u[0]) * rng.integers(1, 5, rows) * scale
        emb[:, 0] = first
        emb[0], emb[1] = u, np.nan
        self.emb = emb.astype(np.float32)
        self.query_idx = np.zeros(tasks, np.int32)
        self.support_idx = rng.integers(2, rows, (tasks, k, n)).astype(np.int32)
        for t in range(tasks):
            near, nans = _nshot_plan(k, t)
            if not near:
                self.query_idx[t] = rng.integers(2, rows)
            for c in near:
                self.support_idx[t, c] = 0
            for c in nans:
                self.support_idx[t, c, rng.integers(0, n)] = 1
        self.support_idx = self.support_idx.reshape(tasks, k * n)

    @property
    def query(self):
        return self.emb[self.query_idx]

    @property
    def support(self):
        return self.emb[self.support_idx]          # (tasks, k * n, E)

    def groups(self, t):
        """class -> the lowest class of task t with the same support rows in the same order (bit-identical arithmetic)."""
        s = self.support_idx[t].reshape(self.k, self.n)
        first = {}
        return np.array([first.setdefault(tuple(s[c]), c) for c in range(self.k)])


def nshot_case(tasks, E, k, n):
    return NshotCase(tasks, E, k, n, seed=7 * tasks + 3 * E + 11 * k + n)


def nshot_pred(query, support, n, k, kind):
    """float64 (k) distances of one task, voicemap/utils.py:159-206.  euclidean: the class mean is exact (n a power of two, grid rows),
    so is the sum of squares, and the square root rounds once."""
    q = np.asarray(query, dtype=np.float64)
    s = np.asarray(support, dtype=np.float64).reshape(k, n, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "euclidean":
            d = q[None, :] - s.sum(1) / n
            return np.sqrt((d * d).sum(1))
        mag = np.sqrt((s * s).sum(2))                       # (k, n)
        mu = (s / mag[:, :, None]).sum(1) / n               # mean unit vector
        if kind == "cosine":
            return 1.0 - (mu @ q) / (np.sqrt(q @ q) * np.sqrt((mu * mu).sum(1)))
        return -((mu @ q) * (mag.sum(1) / n))


def nshot_expected(pred, groups, kind):
    """The argmin a correct kernel must return, or None where float64 cannot decide it.  A NaN distance comes first (numpy.argmin).
    euclidean is exact, so ties are ties.  cosine / dot_product round: classes with the same support rows tie bit for bit in any
    implementation, and the nearest group must lead every other class by 1e-6 (relative to max(1, |d|)) to count as decided."""
    pred = np.asarray(pred, dtype=np.float64)
    if np.isnan(pred).any():
        return int(np.argmax(np.isnan(pred)))
    a = int(np.argmin(pred))
    if kind == "euclidean":
        return a
    others = pred[groups != groups[a]]
    if others.size and others.min() - pred[a] <= 1e-6 * max(1.0, abs(pred[a])):
        return None
    return int(groups[a])
