"""Host-side checks of tests/score_exact.py (the helper of tests/test_gpu_score_exact.py): every case is fp32-exact, the reference
scores equal a slow fp32 emulation of the kernels' ascending-component fmaf chain, the square-root statement holds, every tie class and
split plan is among the cases with its strict-nearest precondition, and the argmin / n-shot references agree with numpy and the oracle."""
import numpy as np
import pytest

from tests import score_exact as S

ALL_KINDS = tuple(S.KINDS)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


def _fma(a, b, c):
    """fp32 fmaf(a, b, c) through float64: the product of two fp32 numbers is a float64 number, and on grid inputs so is the sum, so the
    one rounding to fp32 is fmaf's."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate(q, ref, kind, weights=None):
    """The tile loop's arithmetic in fp32, component by component in ascending order, then the epilogue's single operations -- nothing
    shared with ``pair_scores`` (no float64 sums, no matrix product, fp32 square roots)."""
    f32 = np.float32
    M, E = q.shape
    acc = np.zeros((M, len(ref)), f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for e in range(E):
            a, b = q[:, None, e].astype(f32), ref[None, :, e].astype(f32)
            if kind in ("euclidean", "neg_euclidean"):
                d = a - b
                acc = _fma(d, d, acc)
            elif kind == "weighted_l1":
                acc = _fma(np.full_like(acc, weights[e]), np.abs(a - b), acc)
            else:
                acc = _fma(np.broadcast_to(a, acc.shape), np.broadcast_to(b, acc.shape), acc)
        if kind == "euclidean":
            return np.sqrt(acc)
        if kind == "neg_euclidean":
            return -np.sqrt(acc)
        if kind == "dot_product":
            return -acc
        if kind == "weighted_l1":
            return acc

        def rowsq(x):    # rowsq_kernel: lane l chains its components l, l + 64, ..., then the shuffle tree
            lanes = np.zeros((len(x), 64), f32)
            for e in range(E):
                lanes[:, e % 64] = _fma(x[:, e], x[:, e], lanes[:, e % 64])
            o = 32
            while o:
                lanes = lanes + lanes[:, np.arange(64) ^ o]
                o >>= 1
            return lanes[:, 0]
        qn, rn = np.sqrt(rowsq(q.astype(f32))), np.sqrt(rowsq(ref.astype(f32)))
        return f32(1.0) - acc / (qn[:, None] * rn[None, :])


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", S.E_TABLE)
def test_shape_cases_are_fp32_exact(E):
    qp, rp = S.shape_pools(E)
    assert S.grid_unit(qp) in S.SCALES and np.abs(qp / S.grid_unit(qp)).max() <= 8 and np.abs(rp / S.grid_unit(rp)).max() <= 8
    for kind in S.PAIRDIST_KINDS:
        assert S.headroom(qp, rp, kind) <= 256 * 16 ** 2 < S.LIMIT
        assert S.headroom(rp, rp, kind) <= 256 * 16 ** 2


@pytest.mark.parametrize("E", S.COPY_E)
def test_copy_cases_are_fp32_exact(E):
    emb, label, w = S.copy_inputs(E)
    for kind in ALL_KINDS:
        assert S.headroom(emb, emb, kind, w) <= 2 * 256 * 16 ** 2 < S.LIMIT     # weighted_l1: 256 * 4 * 16 in units of 2^-3
    assert set(np.abs(w)) <= {2.0 ** k for k in range(-3, 3)} and (E < 60 or (w < 0).any())
    lo, hi = S.COPY_ROWS
    assert lo % 8 and lo % 64 and hi % 8 and hi % 64 and (hi - lo) % 8 and 0 < lo < hi < S.COPY_N


def test_tables_cover_what_the_issue_lists():
    assert {m for m, _, _ in S.SHAPES} == set(S.M_VALUES) and {n for _, n, _ in S.SHAPES} == set(S.N_VALUES)
    assert 38 <= len(S.SHAPES) <= 44 and len(set(S.SHAPES)) == len(S.SHAPES)
    rows0 = [(r, m, n) for m, n, r in S.SHAPES]
    assert any(r < 0 for r, _, _ in rows0) and any(r == 0 for r, _, _ in rows0)
    assert any(0 < r < n - m for r, m, n in rows0) and any(r == n - m and r > 0 for r, m, n in rows0)
    assert all(r < 0 or r + m <= n for r, m, n in rows0)
    for E in S.E_TABLE:
        assert 1 <= E <= S.PD_MAX_E
    assert {E % 4 for E in S.E_TABLE} == {0, 1, 2, 3} and {63, 64, 65, 127, 128, 129, 255, 256} <= set(S.E_TABLE)
    assert all(E % 4 for E in S.COPY_E)


# ---- the reference scores ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("E", [1, 3, 5, 63, 64, 65, 130, 256])
def test_pair_scores_equal_the_fp32_fmaf_chain(E, kind):
    qp, rp = S.shape_pools(E)
    q, ref = qp[:9], rp[:65]
    ref[7] = 0.0                                       # a zero row: -0.0 dot products, 0 / 0 cosines
    q[2] = ref[11]                                     # a zero distance
    w = S.lattice_weights(np.random.default_rng(E), E)
    got, want = S.pair_scores(q, ref, kind, w), emulate(q, ref, kind, w)
    assert got.dtype == np.float32 and _same_bits(got, want)
    if kind == "dot_product":
        assert (_bits(got[:, 7]) == 0x80000000).all()   # -0.0, sign and all
    if kind == "cosine":
        zero = ~q.any(1)[:, None] | ~ref.any(1)[None, :]    # 0 / 0 exactly where a norm is zero (E = 1, 3: some grid rows are)
        assert zero[:, 7].all() and np.array_equal(np.isnan(got), zero)
        c = S.cosine_float64(q, ref)
        assert (np.abs(got - (1.0 - c))[~zero] <= S.cosine_bound(c)[~zero]).all()
    if kind == "euclidean":
        assert got[2, 11] == 0.0 and (got >= 0).all()


def test_float32_of_the_float64_square_root_is_the_fp32_square_root():
    i = np.arange(65537)
    for scale in S.SCALES:
        x = i * scale * scale
        assert np.array_equal(_bits(np.sqrt(x.astype(np.float64)).astype(np.float32)), _bits(np.sqrt(x.astype(np.float32))))


# ---- ties and plans ------------------------------------------------------------------------------------------------------------------
def test_split_plans_are_the_stated_ones():
    assert set(S.SPLIT_PLANS) == {(16384, 1100), (8192, 2200), (4096, 8320)}
    for (M, N), plan in S.SPLIT_PLANS.items():
        assert S.split_plan(M, N) == plan and plan[1] >= 2 and plan[2] >= 1
        nbytes = plan[0] * M * 8 + (M + N) * 4 + 256 + -(-M // 8) * 8 * 256 * 4 + 256      # vm_pairdist_workspace_bytes
        assert S.splits_from_workspace(nbytes, M, N) == plan[0]
    assert {(M, N) for M, N, *_ in S.TIE_CASES if (M, N) in S.SPLIT_PLANS} == set(S.SPLIT_PLANS)
    for MN in S.SPLIT_PLANS:
        assert {E for M, N, E, *_ in S.TIE_CASES if (M, N) == MN} == set(S.SPLIT_E)
        assert {S.tie_kind(*MN, E) for E in S.SPLIT_E} == set(S.PAIRDIST_KINDS)
    assert S.FULL_MATRIX_SHAPE in S.SPLIT_PLANS
    assert all(S.split_plan(m, n)[1:] == (1, 0) for m, n, _ in S.SHAPES)    # the small shapes: one tile per split, none empty


def test_every_tie_class_is_among_the_cases():
    per_shape = {}
    for case in S.TIE_CASES:
        per_shape.setdefault(case[:2], set()).update(S.tie_case(*case).classes)
    assert set().union(*per_shape.values()) == set(S.TIE_CLASSES)
    assert sum(v == set(S.TIE_CLASSES) for mn, v in per_shape.items() if mn in S.SPLIT_PLANS) >= 2   # with several tiles per split


@pytest.mark.parametrize("case", S.TIE_CASES)
def test_tie_cases_hold_every_class_and_their_precondition(case):
    M, N, E, q_row0, scale = case
    tc = S.tie_case(*case)
    # one tile per split has no second tile; 8 320 = 65 x 128 has no partial tile
    want = set(S.TIE_CLASSES) - ({"two_tiles_one_split"} if tc.plan[1] < 2 else set()) - ({"last_partial_tile"} if N % 128 == 0 else set())
    assert set(tc.classes) == want and len(want) >= 6
    tps = tc.plan[1]
    tile, lane, half = (lambda n: n // 128), (lambda n: n % 64), (lambda n: (n % 128) // 64)
    for name, rows, pos, src in tc.groups:
        a, b = pos
        assert a < b < N and src in pos
        if name == "same_lane":
            assert tile(a) == tile(b) and lane(a) == lane(b) and half(a) != half(b)
        if name == "two_lanes":
            assert tile(a) == tile(b) and half(a) == half(b) and lane(a) != lane(b)
        if name == "two_tiles_one_split":
            assert tile(a) != tile(b) and tile(a) // tps == tile(b) // tps and lane(b) < lane(a)
        if name == "two_splits":
            assert tile(a) // tps != tile(b) // tps
        if name == "last_partial_tile":
            assert tile(b) == (N - 1) // 128 and N % 128
        if name == "own_before":
            assert a == q_row0 + rows[0] and len(rows) == 1
        if name == "own_after":
            assert b == q_row0 + rows[0] and len(rows) == 1
    for kind in S.PAIRDIST_KINDS:
        q, ref, expected = tc.build(kind)               # asserts: the planted row is the strict nearest before planting
        assert S.headroom(q, ref, kind) <= 256 * 16 ** 2
        s = S.pair_scores(q[sorted(expected)], ref, kind)
        for k, m in enumerate(sorted(expected)):
            val, idx = S.first_argmin(s[k:k + 1], q_row0 + m if q_row0 >= 0 else -1)
            assert idx[0] == expected[m], (kind, m)
            name, rows, pos, src = next(g for g in tc.groups if m in g[1])
            assert (_bits(s[k, list(pos)]) == _bits(s[k, pos[0]])).all()      # the copies tie bit for bit


def test_first_argmin_is_numpy_argmin_without_nan_inf_or_exclusion():
    s = np.random.default_rng(1).normal(0, 1, (50, 300)).astype(np.float32)
    s[:, 100] = s[:, 7]                                    # ties
    val, idx = S.first_argmin(s)
    assert np.array_equal(idx, s.argmin(1)) and np.array_equal(val, s.min(1)) and idx.dtype == np.int32


def test_first_argmin_contract_edges():
    inf, nan = np.inf, np.nan
    s = np.array([[3, 1, 1, 2], [nan, nan, nan, nan], [inf, inf, inf, inf], [nan, 5, inf, 5], [0.0, -0.0, 1, 1], [2, 2, nan, 0]], np.float32)
    val, idx = S.first_argmin(s)
    assert idx.tolist() == [1, -1, -1, 1, 0, 3] and _same_bits(val, np.array([1, inf, inf, 5, 0.0, 0], np.float32))
    val, idx = S.first_argmin(s[:4], 1)                   # rows 0 .. 3 are reference rows 1 .. 4: entry (m, 1 + m) is excluded
    assert idx.tolist() == [2, -1, -1, 1] and val.tolist()[0] == 1 and val[3] == 5
    val, idx = S.first_argmin(np.zeros((1, 1), np.float32), 0)
    assert idx.tolist() == [-1] and np.isposinf(val).all()


# ---- n-shot --------------------------------------------------------------------------------------------------------------------------
def _nshot_cases():
    return [S.nshot_case(S.NSHOT_DIST_TASKS, E, k, n) for k, n, E in S.NSHOT_DIST_CASES] + [S.nshot_case(*c) for c in S.NSHOT_IDX_CASES]


def test_nshot_tables_cover_what_the_issue_lists():
    assert {k for k, _, _ in S.NSHOT_DIST_CASES} == {1, 2, 64, 65, 70, 129}
    assert {t for t, *_ in S.NSHOT_IDX_CASES} >= {1, 3, 4, 5, 257} and {E for _, E, *_ in S.NSHOT_IDX_CASES} == {1, 63, 64, 65, 200, 256}
    assert {c.n for c in _nshot_cases()} == {1, 2, 4, 8}


@pytest.mark.parametrize("kind", S.PAIRDIST_KINDS)
def test_nshot_references_equal_the_oracle_and_the_planted_tasks_are_decided(kind):
    from oracle import voicemap_oracle as O
    seen = set()
    decided = total = 0
    for c in _nshot_cases():
        q, s = c.query, c.support
        for t in range(min(c.tasks, 24)):
            pred = S.nshot_pred(q[t], s[t], c.n, c.k, kind)
            with np.errstate(all="ignore"):
                ref = O.n_shot_prediction(q[t], s[t], c.n, c.k, kind)
            if kind == "euclidean":
                assert np.array_equal(pred, ref, equal_nan=True)
                # the same through integers: n q - sum s in grid units, an int64 sum of squares, one square root
                u = c.scale
                ok = ~np.isnan(pred)
                si = np.round(s[t].astype(np.float64).reshape(c.k, c.n, -1)[ok] / u).astype(np.int64)
                d = c.n * np.round(q[t].astype(np.float64) / u).astype(np.int64)[None, :] - si.sum(1)
                assert np.array_equal(pred[ok], np.sqrt((d * d).sum(1).astype(np.float64)) * (u / c.n))
            else:
                assert np.array_equal(np.isnan(pred), np.isnan(ref))
                ok = ~np.isnan(ref)
                assert np.abs(pred[ok] - ref[ok]).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(ref[ok]).max(initial=0.0))
            exp = S.nshot_expected(pred, c.groups(t), kind)
            near, nans = S._nshot_plan(c.k, t)
            total += 1
            decided += exp is not None
            if near:                                             # a planted task is decided under every kind, and as planned
                assert exp == (min(nans) if nans else min(near)), (c.k, t, kind)
            if c.k > 67 and not nans and pred[3] == pred[67] == pred.min():
                seen.add("tie 3 / 67")
            if c.k == 129 and exp == 128:
                seen.add("minimum only in pass 2")
            if nans and min(nans) >= 64 and near and max(near) < 64 and exp == min(nans):
                seen.add("NaN in pass 1 against a minimum in pass 0")
            if len(nans) == 2 and exp == min(nans):
                seen.add("first of two NaNs")
    assert seen == {"tie 3 / 67", "minimum only in pass 2", "NaN in pass 1 against a minimum in pass 0", "first of two NaNs"}
    assert decided >= 0.8 * total
