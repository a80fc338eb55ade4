"""-m gpu: the embedding scorers against tests/score_exact.py -- an independent exact reference, not vm_pairdist_argmin's own matrix.

vm_pairdist_argmin: the dist matrix as uint32 bits and best_val / best_idx against ``first_argmin`` of the REFERENCE over every
embedding width around the 4-wide vector, the 64-component chunk and PD_MAX_E x some forty (M, N, q_row0) shapes x the three kinds (grid
inputs: ties everywhere), planted ties of every position class on three shapes whose split plan has several tiles per split and empty
trailing splits (the plan is read back from the workspace size), the contract's edges ((+inf, -1) rows, NaN never wins), every output
and the workspace between guard words; vm_nshot_distances / vm_nshot_indexed with duplicated and NaN classes on both sides of the
64-class pass; and the three other kernels that run the tile loop (vm_pair_score_hist, vm_cohort_topk_stats, vm_mine_pairs) against the same
reference at widths on the scalar fetch path.  A mismatch is reported by query row, reference row, lane, tile and split."""
import numpy as np
import pytest
import torch

from tests import score_exact as S
from tests.gpu_util import L, dev, p, stream
from voicemap_amd import mining as MN
from voicemap_amd import verification as V
from voicemap_amd.retrieval import EmbeddingCache

pytestmark = pytest.mark.gpu
PATTERN = 0x7FC5A5A5      # the guard word (as fp32: a NaN with a payload no kernel produces)
GUARD = 64                # words on either side: the inner buffer stays 256-byte aligned


class Guarded:
    """n 4-byte words between two runs of guard words; the inner words start as the pattern too, so an entry the kernel never wrote
    shows.  ``fetch`` copies everything back, asserts the guards and returns the inner words."""

    def __init__(self, n, np_dtype=np.float32):
        self.n, self.np_dtype = int(n), np_dtype
        self.raw = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.int32, device="cuda")

    def ptr(self):
        return self.raw.data_ptr() + 4 * GUARD

    def fetch(self, what):
        h = self.raw.cpu().numpy()
        assert (h[:GUARD] == PATTERN).all(), "%s: written in front of the buffer" % what
        assert (h[GUARD + self.n:] == PATTERN).all(), "%s: written behind the buffer" % what
        return h[GUARD:GUARD + self.n].view(self.np_dtype)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _first_bad(got, want):
    """Index of the first entry whose bits differ (NaN: any NaN but the guard pattern matches a NaN), or None."""
    want = np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got) | (_u32(got) == PATTERN), _u32(got) != _u32(want))
    if not bad.any():
        return None
    return tuple(int(i) for i in np.argwhere(bad)[0]), int(bad.sum())


def pairdist(q_t, ref_t, M, N, E, kind, q_row0, want_dist=True):
    """One guarded vm_pairdist_argmin launch -> (dist (M, N) or None, best_val, best_idx, splits)."""
    nbytes = L().query("vm_pairdist_workspace_bytes", M, N)
    assert nbytes % 4 == 0
    ws = Guarded(nbytes // 4)                      # exactly the size the library asks for
    d = Guarded(M * N) if want_dist else None
    bv, bi = Guarded(M), Guarded(M, np.int32)
    L().call("vm_pairdist_argmin", p(q_t), p(ref_t), M, N, E, S.KINDS[kind], q_row0, d.ptr() if want_dist else None, bv.ptr(), bi.ptr(),
             ws.ptr(), stream())
    torch.cuda.synchronize()
    ws.fetch("workspace")
    dist = d.fetch("dist").reshape(M, N) if want_dist else None
    return dist, bv.fetch("best_val"), bi.fetch("best_idx"), S.splits_from_workspace(nbytes, M, N)


def check_dist(dist, want, splits, what):
    M, N = want.shape
    bad = _first_bad(dist, want)
    if bad is not None:
        (m, n), count = bad
        pytest.fail("%s: %d of %d scores differ; first: got %r (0x%08x), want %r (0x%08x) at %s" % (
            what, count, M * N, dist[m, n], _u32(dist)[m, n], want[m, n], _u32(want)[m, n], S.locate(m, n, M, N, splits)))


def check_argmin(bv, bi, want, q_row0, splits, what):
    """best_* against first_argmin of the REFERENCE matrix ``want``."""
    M, N = want.shape
    wv, wi = S.first_argmin(want, q_row0)
    bad = np.flatnonzero(bi != wi)
    if bad.size:
        m = int(bad[0])
        pytest.fail("%s: %d argmins differ; query row %d: got %d, want %d (score %r)\n  got:  %s\n  want: %s" % (
            what, bad.size, m, bi[m], wi[m], wv[m], S.locate(m, bi[m], M, N, splits) if bi[m] >= 0 else "none",
            S.locate(m, wi[m], M, N, splits) if wi[m] >= 0 else "none"))
    badv = _first_bad(bv, wv)
    assert badv is None, "%s: best_val differs at query row %d: got %r, want %r" % (what, badv[0][0], bv[badv[0][0]], wv[badv[0][0]])


def check_pairdist(q, ref, kind, q_row0, want, what, q_t=None, ref_t=None, full=True):
    """dist (if ``full``) and argmin of a launch against the reference ``want``; then the dist = NULL launch: identical best_*."""
    M, N, E = len(q), len(ref), q.shape[1]
    q_t = dev(q) if q_t is None else q_t
    ref_t = dev(ref) if ref_t is None else ref_t
    if full:
        dist, bv, bi, splits = pairdist(q_t, ref_t, M, N, E, kind, q_row0)
        check_dist(dist, want, splits, what)
        check_argmin(bv, bi, want, q_row0, splits, what)
    bv2, bi2, splits = pairdist(q_t, ref_t, M, N, E, kind, q_row0, want_dist=False)[1:]
    if full:
        assert np.array_equal(bi, bi2) and np.array_equal(_u32(bv), _u32(bv2)), what + ": the dist = NULL launch differs"
    else:
        check_argmin(bv2, bi2, want, q_row0, splits, what + " (dist = NULL)")
    return bv2, bi2, splits


# ---- vm_pairdist_argmin: widths x shapes x kinds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.PAIRDIST_KINDS)
@pytest.mark.parametrize("E", S.E_TABLE)
def test_pairdist_equals_the_reference_bit_for_bit(E, kind):
    qp, rp = S.shape_pools(E)
    full_q, full_r = S.shape_reference(E, kind)
    qp_t, rp_t = dev(qp), dev(rp)
    for M, N, q_row0 in S.SHAPES:
        want = np.ascontiguousarray(S.shape_scores(full_q, full_r, M, N, q_row0))
        q = qp[:M] if q_row0 < 0 else rp[q_row0:q_row0 + M]
        q_t = qp_t if q_row0 < 0 else rp_t[q_row0:q_row0 + M]
        _, _, splits = check_pairdist(q, rp[:N], kind, q_row0, want, "E=%d %s M=%d N=%d q_row0=%d" % (E, kind, M, N, q_row0), q_t, rp_t)
        assert splits == S.split_plan(M, N)[0]


# ---- planted ties, split plans ------------------------------------------------------------------------------------------------------
def _scores_blocked(q, ref, kind, block=1024):
    return np.concatenate([S.pair_scores(q[m0:m0 + block], ref, kind) for m0 in range(0, len(q), block)])


@pytest.mark.parametrize("case", S.TIE_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def test_planted_ties_in_every_position_class(case):
    M, N, E, q_row0, scale = case
    tc = S.tie_case(*case)
    in_plan = (M, N) in S.SPLIT_PLANS
    for kind in ((S.tie_kind(M, N, E),) if in_plan else S.PAIRDIST_KINDS):
        q, ref, expected = tc.build(kind)
        want = _scores_blocked(q, ref, kind)
        what = "ties %dx%dx%d %s" % (M, N, E, kind)
        full = not in_plan or (M, N) == S.FULL_MATRIX_SHAPE
        bv, bi, splits = check_pairdist(q, ref, kind, q_row0, want, what, full=full)
        # the plan this case exists for: a later change of the heuristic cannot silently take it out of coverage
        assert (splits,) + S.split_plan(M, N)[1:] == tc.plan and (not in_plan or tc.plan == S.SPLIT_PLANS[(M, N)])
        for name, rows, pos, src in tc.groups:
            for m in rows:
                assert bi[m] == expected[m], "%s: class %s, query row %d: got %d, want %d of %s\n  got:  %s\n  want: %s" % (
                    what, name, m, bi[m], expected[m], pos, S.locate(m, max(int(bi[m]), 0), M, N, splits),
                    S.locate(m, expected[m], M, N, splits))


# ---- the contract's edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.PAIRDIST_KINDS)
def test_rows_with_nothing_below_inf_give_inf_and_minus_one(kind):
    rng = np.random.default_rng(17)
    E = 5
    q, ref = S.grid(rng, (9, E), 1.0), S.grid(rng, (70, E), 1.0)
    q[q.any(1) == 0] = 1.0
    ref[ref.any(1) == 0] = 1.0
    inf = np.float32(np.inf)
    # an all-NaN query row
    qn = q.copy()
    qn[3] = np.nan
    want = S.pair_scores(qn, ref, kind)
    assert np.isnan(want[3]).all() and not np.isnan(np.delete(want, 3, 0)).any()
    bv, bi, _ = check_pairdist(qn, ref, kind, -1, want, "NaN query row " + kind)
    assert bi[3] == -1 and bv[3] == inf and (np.delete(bi, 3) >= 0).all()
    # an all-NaN reference matrix
    rn = np.full_like(ref, np.nan)
    bv, bi, _ = check_pairdist(q, rn, kind, -1, np.full((9, 70), np.nan, np.float32), "NaN references " + kind)
    assert (bi == -1).all() and (bv == inf).all()
    # M = N = 1 and the only reference is the query's own row
    bv, bi, _ = check_pairdist(ref[:1], ref[:1], kind, 0, S.pair_scores(ref[:1], ref[:1], kind), "M=N=1 " + kind)
    assert bi.tolist() == [-1] and bv.tolist() == [inf]
    # a NaN reference row never wins, wherever it sits
    for at in (0, 64, 69):
        rr = ref.copy()
        rr[at] = np.nan
        bv, bi, _ = check_pairdist(q, rr, kind, -1, S.pair_scores(q, rr, kind), "NaN reference row %d %s" % (at, kind))
        assert (bi != at).all() and (bi >= 0).all() and np.isfinite(bv).all()


def test_euclidean_overflow_to_inf_gives_minus_one():
    q, ref = np.full((9, 5), 2e19, np.float32), np.full((70, 5), -2e19, np.float32)     # (a - b)^2 = 1.6e39 > FLT_MAX
    want = np.full((9, 70), np.inf, np.float32)
    dist, bv, bi, splits = pairdist(dev(q), dev(ref), 9, 70, 5, "euclidean", -1)
    check_dist(dist, want, splits, "overflow")
    assert (bi == -1).all() and (bv == np.float32(np.inf)).all()


# ---- n-shot -------------------------------------------------------------------------------------------------------------------------
def _check_nshot(c, kind, pred, am, what):
    q, s = c.query, c.support
    pred = pred.reshape(c.tasks, c.k)
    decided = 0
    for t in range(c.tasks):
        ref = S.nshot_pred(q[t], s[t], c.n, c.k, kind)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(pred[t]), nan), (what, t)
        if kind == "euclidean":    # exact class means and sums: the float64 reference rounded once
            assert np.array_equal(_u32(pred[t])[~nan], _u32(ref.astype(np.float32))[~nan]), (what, t, pred[t], ref)
        elif (~nan).any():
            assert np.abs(pred[t] - ref)[~nan].max() < 2e-6 * max(1.0, np.abs(ref[~nan]).max()), (what, t)
        exp = S.nshot_expected(ref, c.groups(t), kind)
        if exp is not None:
            decided += 1
            assert am[t] == exp, "%s: task %d: argmin %d, want %d (plan %s)" % (what, t, am[t], exp, S._nshot_plan(c.k, t))
    assert kind != "euclidean" or decided == c.tasks


@pytest.mark.parametrize("kind", S.PAIRDIST_KINDS)
@pytest.mark.parametrize("k,n,E", S.NSHOT_DIST_CASES)
def test_nshot_distances_ties_and_nans_across_the_class_passes(k, n, E, kind):
    c = S.nshot_case(S.NSHOT_DIST_TASKS, E, k, n)
    pred, am = Guarded(c.tasks * k), Guarded(c.tasks, np.int32)
    L().call("vm_nshot_distances", p(dev(c.query)), p(dev(c.support)), c.tasks, k, n, E, S.KINDS[kind], pred.ptr(), am.ptr(), stream())
    torch.cuda.synchronize()
    _check_nshot(c, kind, pred.fetch("pred"), am.fetch("argmin"), "nshot_distances k=%d n=%d E=%d %s" % (k, n, E, kind))


@pytest.mark.parametrize("kind", S.PAIRDIST_KINDS)
@pytest.mark.parametrize("tasks,E,k,n", S.NSHOT_IDX_CASES)
def test_nshot_indexed_ties_and_nans(tasks, E, k, n, kind):
    c = S.nshot_case(tasks, E, k, n)
    emb, qi, si = dev(c.emb), dev(c.query_idx, torch.int32), dev(c.support_idx, torch.int32)
    pred, am, am2 = Guarded(tasks * k), Guarded(tasks, np.int32), Guarded(tasks, np.int32)
    L().call("vm_nshot_indexed", p(emb), len(c.emb), p(qi), p(si), tasks, k, n, E, S.KINDS[kind], pred.ptr(), am.ptr(), stream())
    L().call("vm_nshot_indexed", p(emb), len(c.emb), p(qi), p(si), tasks, k, n, E, S.KINDS[kind], None, am2.ptr(), stream())
    torch.cuda.synchronize()
    a = am.fetch("argmin")
    _check_nshot(c, kind, pred.fetch("pred"), a, "nshot_indexed tasks=%d E=%d k=%d n=%d %s" % (tasks, E, k, n, kind))
    assert np.array_equal(a, am2.fetch("argmin without pred"))


# ---- the other kernels that run the tile loop, against the independent reference ------------------------------------------------------


@pytest.mark.parametrize("E", S.COPY_E)
def test_pair_score_hist_bins_the_reference_scores(E):
    emb, label, w = S.copy_inputs(E)
    lo, hi = S.COPY_ROWS
    cache = EmbeddingCache(dev(emb), label)
    w_t = dev(w)
    i, j = np.triu_indices(S.COPY_N, 1)
    keep = (i >= lo) & (i < hi)
    i, j = i[keep], j[keep]
    tg = label[i] == label[j]
    for kind in S.KINDS:
        s = S.pair_scores(emb[lo:hi], emb, kind, w)[i - lo, j]
        f = s[np.isfinite(s)]
        a, b = float(f.min()), float(f.max())
        wt = w_t if kind == "weighted_l1" else None
        coarse = [V.pass1_window(a, 0.5 * (a + b))]           # the top half of the scores lands in the over slot
        got = V.histogram(cache, S.KINDS[kind], wt, coarse, 4096, rows=(lo, hi))
        assert got.sum() == len(s) and np.array_equal(got, V.bin_scores(s, tg, coarse, 4096)), (E, kind)
        u = np.unique(f)
        single = [(V.key_of(float(v)), 0) for v in u[sorted({0, len(u) // 2, len(u) - 1})]]      # single-key windows
        got = V.histogram(cache, S.KINDS[kind], wt, single, 1024, rows=(lo, hi))
        assert np.array_equal(got, V.bin_scores(s, tg, single, 1024)), (E, kind)


@pytest.mark.parametrize("E", S.COPY_E)
def test_cohort_selection_is_that_of_the_reference_scores(E):
    emb, label, w = S.copy_inputs(E)
    lo, hi = S.COPY_ROWS
    emb_t, w_t = dev(emb), dev(w)
    for kind in ("euclidean", "dot_product", "weighted_l1", "cosine"):
        s = S.pair_scores(emb[lo:hi], emb, kind, w)
        for K in (1, 7, S.COPY_N):
            out = V.cohort_topk_stats(emb_t[lo:hi], emb_t, S.KINDS[kind], w_t if kind == "weighted_l1" else None, K, lo, return_topk=True)
            idx, cnt = V.cohort_select_numpy(s, K, lo)
            assert np.array_equal(out[3].cpu().numpy(), cnt), (E, kind, K)
            assert np.array_equal(out[4].cpu().numpy(), idx), (E, kind, K)


@pytest.mark.parametrize("E", S.COPY_E)
def test_mined_lists_are_those_of_the_reference_scores(E):
    emb, label, w = S.copy_inputs(E)
    lo, hi = S.COPY_ROWS
    emb_t, label_t = dev(emb), dev(label, torch.int32)
    for kind in S.PAIRDIST_KINDS:
        s = S.pair_scores(emb[lo:hi], emb, kind)
        for K in (1, 8, 64):
            ref = MN.mine_pairs_numpy(s, label, K, K, row0=lo)
            got = tuple(t.cpu().numpy() for t in MN.mine_rows(emb_t, label_t, S.KINDS[kind], (lo, hi), K, K))
            for g, r, name in zip(got, ref, ("neg_idx", "neg_val", "pos_idx", "pos_val")):
                if g.dtype == np.float32:
                    nan = np.isnan(r)
                    assert np.array_equal(np.isnan(g), nan) and np.array_equal(_u32(g)[~nan], _u32(r)[~nan]), (E, kind, K, name)
                else:
                    assert np.array_equal(g, r), (E, kind, K, name, np.argwhere(g != r)[:5])
