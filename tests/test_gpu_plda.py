"""-m gpu tests of the PLDA back end: score kind VM_SCORE_PLDA in the six scorers, vm_scatter_f64, vm_plda_project, and the fit end to
end (voicemap_amd/plda.py, csrc/plda.hip, csrc/score_tile.hpp).

The score kind is held to bit equality on grid rows (tests/plda_cases.py grid_plda_rows: every product, partial sum, h_i + h_j and
final difference is an fp32 number, so the score is known whatever the order of the chain), with ``plda_scores_numpy`` as the one
reference matrix that the histogram, the cohort statistics, the calibration sums and the clustering are then fed.  The two new
kernels are held to bit equality on dyadic-grid inputs and to counted bounds elsewhere, with guard words around their outputs."""
import numpy as np
import pytest
import torch

from tests import calib_refs as R
from tests import plda_cases as PC
from tests import score_exact as SE
from tests.gpu_util import L, p, stream
from voicemap_amd import diarization as DZ
from voicemap_amd import plda as PL
from voicemap_amd import verification as V
from voicemap_amd.retrieval import EmbeddingCache

pytestmark = pytest.mark.gpu

PLDA, DOT = 6, 2
WIDTHS = (4, 8, 64, 68, 132, 256)   # the vector width; 68 and 132: a last chunk that holds only zeros and h; ST_MAX_E
# (M, N, q_row0) around the 64-query block and the 128-reference tile: M in {1, 8, 9, 64, 65}, N in {1, 64, 127, 128, 129, 257}
SHAPES = ((1, 1, 0), (1, 64, 31), (1, 257, -1), (8, 127, 0), (8, 128, 60), (9, 129, -1), (9, 257, 124), (64, 64, 0), (64, 128, 64),
          (64, 257, 193), (65, 1, -1), (65, 127, -1), (65, 128, 63), (65, 129, 64), (65, 257, 96))
GUARD = 64


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def cuda(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def pairdist(q, ref, kind, q_row0=-1):
    """(dist (M, N), best_val, best_idx) of vm_pairdist_argmin on host arrays."""
    M, E = q.shape
    N = ref.shape[0]
    x, y = cuda(q), cuda(ref)
    ws = L().workspace("vm_pairdist_workspace_bytes", M, N, device="cuda")
    d = torch.empty(M, N, device="cuda")
    bv, bi = torch.empty(M, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda")
    L().call("vm_pairdist_argmin", p(x), p(y), M, N, E, kind, q_row0, p(d), p(bv), p(bi), p(ws), stream())
    torch.cuda.synchronize()
    return d.cpu().numpy(), bv.cpu().numpy(), bi.cpu().numpy()


_POOL = {}


def pool(P):
    """(reference rows (257, P), foreign query rows (65, P), speaker codes, the (257, 257) score matrix of the statement): grid rows,
    made once per width and never modified."""
    if P not in _POOL:
        rng = np.random.default_rng(1000 + P)
        scale = (2.0 ** -2, 1.0, 2.0)[P % 3]
        ref, q = PC.grid_plda_rows(rng, 257, P, scale), PC.grid_plda_rows(rng, 65, P, scale)
        spk = rng.integers(0, 6, 257)
        s = PL.plda_scores_numpy(ref)
        for a in (ref, q, spk, s):
            a.setflags(write=False)
        _POOL[P] = (ref, q, spk, s)
    return _POOL[P]


# ---- the score kind ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", WIDTHS)
def test_pairdist_matrix_and_argmin_equal_the_statement_bit_for_bit(P):
    ref_all, q_all, _, _ = pool(P)
    for M, N, q_row0 in SHAPES:
        ref = ref_all[:N]
        q = ref[q_row0:q_row0 + M] if q_row0 >= 0 else q_all[:M]
        if len(q) < M:   # a shard that would run past the matrix: shorten it
            M = len(q)
        want = PL.plda_scores_numpy(q, ref)
        assert np.abs(want).max() < 2 ** 24 * SE.grid_unit(want)   # every score is an fp32 number on the grid
        d, bv, bi = pairdist(q, ref, PLDA, q_row0)
        assert np.array_equal(bits(d), bits(want)), (P, M, N, q_row0)
        wv, wi = SE.first_argmin(want, q_row0)
        assert np.array_equal(bi, wi) and np.array_equal(bits(bv), bits(wv)), (P, M, N, q_row0)


@pytest.mark.parametrize("P", WIDTHS)
def test_histogram_counts_equal_bin_scores_of_the_statement(P):
    ref, _, spk, s = pool(P)
    cache = EmbeddingCache(cuda(ref), spk)
    i, j = np.triu_indices(257, 1)
    tgt = spk[i] == spk[j]
    lo, hi = float(s.min()), float(s.max())
    wins = [V.pass1_window(lo, hi, 1024), (V.key_of(0.0), 8), (0, 22)]
    for rows in ((0, 257), (9, 130), (200, 257)):
        keep = (i >= rows[0]) & (i < rows[1])
        got = V.histogram(cache, PLDA, None, wins, 1024, rows)
        assert np.array_equal(got, V.bin_scores(s[i[keep], j[keep]], tgt[keep], wins, 1024)), (P, rows)
    assert V.histogram(cache, PLDA, None, wins, 1024, (0, 257))[:, :, :1024].sum() > 0


@pytest.mark.parametrize("P", (8, 68, 256))
def test_cohort_statistics_and_normalised_histogram_follow_their_statements(P):
    ref, q, spk, s = pool(P)
    i, j = np.triu_indices(257, 1)
    tgt = spk[i] == spk[j]
    for K, self_row0 in ((7, 0), (257, 0), (300, -1)):
        K = min(K, 257)
        rows = ref if self_row0 >= 0 else q
        sc = s if self_row0 >= 0 else PL.plda_scores_numpy(q, ref)
        mu, sig, rsig, cnt, topk = (t.cpu().numpy() for t in V.cohort_topk_stats(cuda(rows), cuda(ref), PLDA, None, K, self_row0, return_topk=True))
        want = V.cohort_stats_numpy(sc, K, self_row0 if self_row0 >= 0 else None)
        assert np.array_equal(cnt, want["count"]) and np.array_equal(topk, want["topk_idx"])
        for got, name in ((mu, "mu"), (sig, "sigma")):   # float64 sums of at most 257 fp32 numbers, rounded once: the neighbour at most
            assert np.all(np.abs(got.astype(np.float64) - want[name]) <= np.spacing(np.abs(want[name]))), name
        with np.errstate(divide="ignore"):
            assert np.array_equal((1.0 / sig.astype(np.float64)).astype(np.float32), rsig)
        if self_row0 >= 0:
            cache = EmbeddingCache(cuda(ref), spk)
            norm = V.ScoreNorm(cuda(mu), cuda(sig), cuda(rsig), cuda(cnt), "plda", K, 257)
            sn = V.normalise_scores_numpy(s[i, j], i, j, mu, rsig)
            wins = [V.pass1_window(float(np.nanmin(sn)), float(np.nanmax(sn)), 1024)]
            assert np.array_equal(V.histogram(cache, PLDA, None, wins, 1024, (0, 257), norm=norm), V.bin_scores(sn, tgt, wins, 1024))


@pytest.mark.skipif(not R.have_extended(), reason="np.longdouble is not wider than float64 here")
@pytest.mark.parametrize("P", (4, 68, 256))
def test_calibration_sums_follow_the_extended_precision_statement(P):
    from voicemap_amd import calibration as C
    ref, _, spk, s = pool(P)
    cache = EmbeddingCache(cuda(ref), spk)
    i, j = np.triu_indices(257, 1)
    tgt = spk[i] == spk[j]
    scale = 1.0 / max(1.0, float(np.abs(s).max()))
    for rows, abt in (((0, 257), (0.0, 0.0, 0.0)), ((0, 257), (-3.0 * scale, 0.5, -0.25)), ((70, 201), (-40.0 * scale, 2.0, 1.5))):
        keep = (i >= rows[0]) & (i < rows[1])
        got = C._device_sums(cache, PLDA, None, *abt, rows).cpu().numpy().reshape(2, 8)
        R.assert_sums_close(got, s[i[keep], j[keep]], tgt[keep], *abt, what="plda P=%d rows=%r" % (P, rows))


@pytest.mark.parametrize("linkage", DZ.LINKAGES)
def test_ahc_equals_the_reference_on_the_statement_matrix(linkage):
    lens = [1, 65, 0, 130, 40]
    for P in (8, 68):
        ref = pool(P)[0][:sum(lens)]
        row0 = np.concatenate([[0], np.cumsum(lens)])
        res = DZ.cluster(cuda(ref), row0, "plda", linkage)
        for r, n in enumerate(lens):
            got = res.recording(r)
            if n == 0:
                assert got.n_clusters == 0
                continue
            want = DZ.ahc_reference(PL.plda_scores_numpy(ref[row0[r]:row0[r + 1]]), linkage)
            assert np.array_equal(got.merge_a, want.merge_a) and np.array_equal(got.merge_b, want.merge_b), (P, r)
            assert np.array_equal(bits(got.merge_h), bits(want.merge_h)) and np.array_equal(got.merge_size, want.merge_size), (P, r)
            assert np.array_equal(got.labels, want.labels) and got.n_clusters == want.n_clusters == 1


def test_a_zero_row_term_gives_the_dot_kinds_keys():
    """Arbitrary rows, not on a grid, last column zero: the PLDA kind runs the dot kind's chain (the zeroed query component adds nothing) and
    finishes with (0 + 0) - acc, which is -acc up to the sign of a zero -- and the key takes -0.0 for +0.0."""
    rng = np.random.default_rng(5)
    for P, M, N in ((4, 9, 64), (68, 65, 257), (256, 64, 129)):
        q, ref = rng.normal(size=(M, P)).astype(np.float32), rng.normal(size=(N, P)).astype(np.float32)
        q[:, -1] = ref[:, -1] = 0.0
        q[0, :] = 0.0   # a zero row: the dot kind gives -0.0, the PLDA kind +0.0
        a, av, ai = pairdist(q, ref, PLDA)
        b, bv, bi = pairdist(q, ref, DOT)
        assert np.array_equal(V.score_keys(a), V.score_keys(b)) and np.array_equal(ai, bi) and np.array_equal(V.score_keys(av), V.score_keys(bv))
        assert (bits(a[0]) == 0).all() and (bits(b[0]) == 0x80000000).all()


def test_general_rows_lie_within_the_counted_bound_and_a_bad_row_term_gives_nan():
    """|s - s64| <= (E + 2) 2^-24 (sum |q r| + |h_i| + |h_j|): E - 1 fmaf roundings, the sum of the row terms and the difference."""
    rng = np.random.default_rng(6)
    for P, M, N in ((8, 65, 129), (132, 9, 257), (256, 64, 128)):
        q, ref = (rng.normal(size=(M, P)) * 3).astype(np.float32), (rng.normal(size=(N, P)) * 3).astype(np.float32)
        ref[3, -1], ref[N - 1, -1], q[M - 1, -1] = np.inf, np.nan, -np.inf
        s, _, bi = pairdist(q, ref, PLDA)
        q64, r64 = q.astype(np.float64), ref.astype(np.float64)
        bad = np.zeros((M, N), bool)
        bad[M - 1, :] = bad[:, 3] = bad[:, N - 1] = True
        assert np.array_equal(np.isnan(s), bad) and np.array_equal(np.isnan(PL.plda_scores_numpy(q, ref)), bad)
        with np.errstate(invalid="ignore"):
            s64 = (q64[:, -1][:, None] + r64[:, -1][None, :]) - q64[:, :-1] @ r64[:, :-1].T
            bound = (P + 2) * SE.U * (np.abs(q64[:, :-1]) @ np.abs(r64[:, :-1]).T + np.abs(q64[:, -1])[:, None] + np.abs(r64[:, -1])[None, :])
        err = np.abs(s.astype(np.float64) - s64)[~bad]
        print("P=%d: largest error / bound %.3f" % (P, (err / bound[~bad]).max()))
        assert (err <= bound[~bad]).all()
        assert bi[M - 1] == -1 and (bi[:M - 1] >= 0).all()


def test_every_scorer_refuses_a_width_that_cannot_hold_plda_rows():
    from voicemap_amd._lib import VoicemapHipError
    rng = np.random.default_rng(0)
    for E in (1, 2, 3, 6, 67):
        x = cuda(rng.normal(size=(16, E)).astype(np.float32))
        cache = EmbeddingCache(x, np.arange(16) % 3)
        calls = {
            "vm_pairdist_argmin": lambda: pairdist(x.cpu().numpy(), x.cpu().numpy(), PLDA),
            "vm_pair_score_hist": lambda: V.histogram(cache, PLDA, None, [(0, 22)], 1024, (0, 16)),
            "vm_pair_score_hist_norm": lambda: V.histogram(cache, PLDA, None, [(0, 22)], 1024, (0, 16),
                                                           norm=V.ScoreNorm(x[:, 0].contiguous(), None, x[:, 0].contiguous(), None, "plda", 1, 1)),
            "vm_cohort_topk_stats": lambda: V.cohort_topk_stats(x, x, PLDA, None, 3),
            "vm_pair_calib_sums": lambda: __import__("voicemap_amd.calibration", fromlist=["x"])._device_sums(cache, PLDA, None, 0.0, 0.0, 0.0, (0, 16)),
            "vm_ahc": lambda: DZ.cluster(x, [0, 16], "plda", "average"),
        }
        for name, call in calls.items():
            with pytest.raises(VoicemapHipError, match=name + r".* failed \(-1\).*VM_SCORE_PLDA needs E % 4 == 0"):
                call()
    torch.cuda.synchronize()


# ---- vm_scatter_f64 ------------------------------------------------------------------------------------------------------------------
def scatter(x, label, mean):
    """One guarded vm_scatter_f64 call on host arrays -> (D, D) float64."""
    N, D = x.shape
    out = torch.full((GUARD + D * D + GUARD,), -1.25e300, dtype=torch.float64, device="cuda")
    nbytes = L().query("vm_scatter_f64_workspace_bytes", N, D)
    ws = torch.full((GUARD + nbytes // 8 + GUARD,), -7.5e299, dtype=torch.float64, device="cuda")
    xd, md = cuda(x), cuda(mean, torch.float64)
    ld = None if label is None else cuda(label, torch.int32)
    L().call("vm_scatter_f64", p(xd), p(ld), p(md), N, D, out.data_ptr() + GUARD * 8, ws.data_ptr() + GUARD * 8, stream())
    torch.cuda.synchronize()
    o, w = out.cpu().numpy(), ws.cpu().numpy()
    assert (o[:GUARD] == -1.25e300).all() and (o[GUARD + D * D:] == -1.25e300).all(), "words around out were written"
    assert (w[:GUARD] == -7.5e299).all() and (w[GUARD + nbytes // 8:] == -7.5e299).all(), "words around the workspace were written"
    return o[GUARD:GUARD + D * D].reshape(D, D).copy()


def chunk_rows():
    return L().query("vm_scatter_f64_chunk_rows")


@pytest.mark.parametrize("D", (1, 3, 4, 64, 65, 255))
def test_scatter_on_a_dyadic_grid_equals_numpy_bit_for_bit(D):
    """Rows: integers in [-64, 64] / 16 (fp32), means on the same grid: every difference, product and partial sum is a multiple of 2^-8
    below 2^53 of them -- exact in float64 in any order.  Rows with a negative label are skipped; the result is exactly symmetric and
    the same on a second run."""
    c = chunk_rows()
    assert c >= 2
    rng = np.random.default_rng(D)
    for N in (1, c - 1, c, c + 1, 3 * c + 5):
        x = PC.grid_f64(rng, (N, D)).astype(np.float32)
        mean = PC.grid_f64(rng, D, amp=16)
        label = rng.integers(-2, 4, N).astype(np.int32)
        for lab in (None, label):
            got = scatter(x, lab, mean)
            want = PL.scatter_reference(x, lab, mean)
            assert np.array_equal(got.view(np.uint64), (want + 0.0).view(np.uint64)), (D, N, lab is None)
            assert np.array_equal(got, got.T)
        assert np.array_equal(scatter(x, label, mean).view(np.uint64), got.view(np.uint64))
    if D == 4:
        assert not scatter(x, np.full(N, -1, np.int32), mean).any()   # nobody takes part: zeros, not what the buffer held


@pytest.mark.parametrize("D", (3, 64, 255))
def test_scatter_of_general_rows_lies_within_the_summation_bound(D):
    """Per entry |got - ref| <= N 2^-53 sum_r |d_ri| |d_rj|: N - 1 additions (fewer with the fma chain) against an extended-precision or
    float64 pairwise reference; exactly symmetric, bit-identical from run to run."""
    c = chunk_rows()
    rng = np.random.default_rng(50 + D)
    N = 3 * c + 5
    x = (rng.normal(size=(N, D)) * 2 + 1).astype(np.float32)
    label = rng.integers(-1, 5, N).astype(np.int32)
    mean = x[label >= 0].astype(np.float64).mean(0)
    got = scatter(x, label, mean)
    d = (x.astype(np.float64) - mean[None, :])[label >= 0]
    ref = np.asarray((d.astype(np.longdouble).T @ d.astype(np.longdouble)), dtype=np.float64)
    bound = N * 2.0 ** -53 * (np.abs(d).T @ np.abs(d))
    print("D=%d: largest error / bound %.3g" % (D, (np.abs(got - ref) / bound).max()))
    assert (np.abs(got - ref) <= bound).all()
    assert np.array_equal(got, got.T) and np.array_equal(scatter(x, label, mean).view(np.uint64), got.view(np.uint64))


# ---- vm_plda_project -----------------------------------------------------------------------------------------------------------------
def project(x, mean, A, length_norm, quad=None, c0=0.0):
    """One guarded vm_plda_project call on host arrays -> (N, P) fp32."""
    N, E = x.shape
    D = A.shape[0]
    P = D if quad is None else PL.padded_width(D)
    out = torch.full((GUARD + N * P + GUARD,), -7.75e30, dtype=torch.float32, device="cuda")
    xd, md, Ad = cuda(x), cuda(mean, torch.float64), cuda(A, torch.float64)
    qd = None if quad is None else cuda(quad, torch.float64)
    L().call("vm_plda_project", p(xd), p(md), p(Ad), N, E, D, int(length_norm), p(qd), float(c0), out.data_ptr() + GUARD * 4, P, stream())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:GUARD] == np.float32(-7.75e30)).all() and (o[GUARD + N * P:] == np.float32(-7.75e30)).all(), "words around out were written"
    return o[GUARD:GUARD + N * P].reshape(N, P).copy()


DIMS = (1, 3, 4, 63, 64, 255)
ROWS = (1, 63, 64, 65)


@pytest.mark.parametrize("E", DIMS)
def test_projection_on_a_grid_equals_the_statement_bit_for_bit(E):
    """Without length normalisation, on grid inputs (x: integers / 16, mean: integers / 4, A: integers in [-4, 4] / 8, quad: integers in
    [0, 8] / 4, c0 on the grid): every y_d is a multiple of 2^-7 below 2^24 of them and every sum of the row term is exact in float64, so
    the stored fp32 row, the h column included, is the statement's."""
    rng = np.random.default_rng(E)
    for D in DIMS:
        N = ROWS[(DIMS.index(D) + DIMS.index(E)) % 4]
        x = PC.grid_f64(rng, (N, E)).astype(np.float32)
        mean, A = PC.grid_f64(rng, E, amp=8, scale=0.25), PC.grid_f64(rng, (D, E), amp=4, scale=0.125)
        quad, c0 = PC.grid_f64(rng, D, amp=4, scale=0.25) + 1.0, -3.25
        assert np.array_equal(bits(project(x, mean, A, False)), bits(PL.project_reference(x, mean, A, False))), (E, D, N)
        got = project(x, mean, A, False, quad, c0)
        assert got.shape == (N, PL.padded_width(D)) and np.array_equal(bits(got), bits(PL.project_reference(x, mean, A, False, quad, c0))), (E, D, N)


def _one_ulp(got, want64):
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize("E", DIMS)
def test_projection_of_general_rows_is_the_neighbour_of_the_statement_at_most(E):
    """General inputs, with and without length normalisation: every entry within 1 fp32 ulp of the float64 statement rounded to fp32 (the
    float64 error is far below half an fp32 ulp, so only a tie can move it, and then only to the neighbour); the row term is the
    statement applied to the kernel's OWN stored columns, at 1 ulp (it is a float64 sum rounded once); the padding is exactly zero; a
    zero row stays zero under length normalisation."""
    rng = np.random.default_rng(100 + E)
    for D in DIMS:
        N = ROWS[(DIMS.index(D) + DIMS.index(E) + 1) % 4]
        x = rng.normal(size=(N, E)).astype(np.float32)
        mean = rng.normal(size=E) * 0.1
        x[N // 2] = mean.astype(np.float32)
        mean[:] = mean.astype(np.float32)     # so that row N // 2 is exactly the mean: a zero row
        A, quad, c0 = rng.normal(size=(D, E)) / np.sqrt(E), rng.uniform(0.1, 2.0, D), 0.625
        for ln in (False, True):
            got = project(x, mean, A, ln, quad, c0)
            y = (x.astype(np.float64) - mean[None, :]) @ A.T
            if ln:
                nrm = np.sqrt((y * y).sum(1))
                y[nrm > 0] = y[nrm > 0] * np.sqrt(float(D)) / nrm[nrm > 0, None]
            assert _one_ulp(got[:, :D], y).all(), (E, D, N, ln)
            assert not got[:, D:-1].any() and not got[N // 2, :D].any()
            v = got[:, :D].astype(np.float64)
            assert _one_ulp(got[:, -1], (v * v) @ quad + c0).all(), (E, D, N, ln)
            assert np.array_equal(bits(project(x, mean, A, ln)), bits(got[:, :D]))   # the same columns without quad


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    (tx, ts), (hx, hs) = PC.e2e_corpora()
    train = EmbeddingCache(cuda(tx), ts)
    held = EmbeddingCache(cuda(hx), hs)
    return train, held, PL.fit_plda(train), PL.fit_plda_numpy(tx, ts)


def test_the_fit_on_the_chip_agrees_with_the_numpy_fit(fitted):
    train, held, model, ref = fitted
    assert model.D == ref.D == 16 and model.P == 20 and len(model.loglik) == 11
    assert np.max(np.abs(model.psi - ref.psi) / ref.psi) < 1e-6
    assert (np.diff(model.loglik) >= -1e-10 * np.abs(model.loglik[:-1])).all()
    proj = model.project(held)
    assert isinstance(proj, EmbeddingCache) and proj.emb.shape == (320, 20) and np.array_equal(proj.speaker, held.speaker)
    got = proj.emb.cpu().numpy()
    want = model.project_numpy(held.emb.cpu().numpy())
    assert np.all(np.abs(got[:, :16].astype(np.float64) - want[:, :16]) <= 2 * np.spacing(np.abs(want[:, :16])))   # two roundings to fp32
    assert not got[:, 16:19].any()
    with pytest.raises(ValueError, match=r"\(N, 16\) rows"):
        model.project(proj.emb)


def test_verification_on_projected_rows_end_to_end(fitted):
    """``verification_metrics(score="plda")`` equals ``sorted_metrics`` of the pair-distance matrix; S-norm and the calibration fit run
    on the projected cache and match their host statements; and on the held-out speakers the PLDA EER is at most half the cosine EER
    (the corpus was chosen on the host so that the float64 statement alone satisfies this: tests/plda_cases.py)."""
    from voicemap_amd import calibration as C
    from voicemap_amd import retrieval
    train, held, model, _ = fitted
    proj = model.project(held)
    out = retrieval.pairwise_retrieval(proj, "plda", return_matrix=True, rows=(0, proj.n))
    s = out["matrix"].cpu().numpy()
    Z = proj.emb.cpu().numpy()
    z64 = Z.astype(np.float64)
    s64 = (z64[:, -1][:, None] + z64[:, -1][None, :]) - z64[:, :-1] @ z64[:, :-1].T
    assert (np.abs(s - s64) <= 22 * SE.U * (np.abs(z64[:, :-1]) @ np.abs(z64[:, :-1]).T + np.abs(z64[:, -1])[:, None] + np.abs(z64[:, -1])[None, :])).all()
    assert (np.abs(s - (-model.llr_numpy(held.emb.cpu().numpy()))) <= 2 * PC.projected_score_bound(model, held.emb.cpu().numpy())).all()
    sc, tgt = PC.pair_trials(s, held.speaker)
    want = V.sorted_metrics(sc, tgt)
    got = V.verification_metrics(proj, "plda")
    for k in ("eer", "eer_threshold", "best_balanced_accuracy", "best_threshold", "n_target", "n_nontarget", "n_nan"):
        assert got[k] == want[k], k
    cos = V.verification_metrics(held, "cosine")
    print("held-out EER: plda %.4f, cosine %.4f; nearest-neighbour accuracy %.3f" % (got["eer"], cos["eer"], out["accuracy"]))
    assert got["eer"] <= 0.5 * cos["eer"]
    # S-norm against the training rows, projected by the same model
    norm = V.score_norm(proj, model.project(train), "plda", top_k=None)
    stats = V.cohort_stats_numpy(pairdist(Z, model.project(train).emb.cpu().numpy(), PLDA)[0], train.n)
    mu = norm.mu.cpu().numpy()
    assert np.all(np.abs(mu.astype(np.float64) - stats["mu"]) <= np.spacing(np.abs(stats["mu"])))
    i, j = np.triu_indices(proj.n, 1)
    sn = V.normalise_scores_numpy(s[i, j], i, j, mu, norm.rsig.cpu().numpy())
    got_n, want_n = V.verification_metrics(proj, "plda", norm=norm), V.sorted_metrics(sn, tgt)
    assert got_n["eer"] == want_n["eer"] and got_n["eer_threshold"] == want_n["eer_threshold"]
    # calibration: the device fit against the numpy fit on the matrix's trials
    cal, ref = C.fit_calibration(proj, score="plda"), C.fit_calibration_numpy(sc, tgt)
    assert cal.converged and ref.converged and cal.a < 0
    assert abs(cal.a - ref.a) < 1e-6 and abs(cal.b - ref.b) < 1e-6   # (the tolerance of the calibration tests: two Newton runs on sums in two orders)


def test_diarize_with_the_plda_distance_matches_cut_on_the_host(tmp_path_factory):
    from tests import vad_cases as VC
    from voicemap_amd import models, utils
    ds = VC.pause_corpus(tmp_path_factory.mktemp("plda_diar_shards"), seconds=0.15)
    ds.to_device("cuda")
    enc = models.get_baseline_convolutional_encoder(16, 24, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (600, 1), distance_metric="uniform_euclidean")
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    conv = DZ.make_conversations(ds, 2, speakers=(2, 2), turns=(3, 4), turn_seconds=(0.2, 0.4), seed=3)
    _, plain = DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075)
    # the back end is fitted on 240 generated rows of 6 "speakers" spread like the windows' embeddings: any labelled rows do for a check
    # of the plumbing (an untrained encoder, a handful of windows: no claim about the error)
    rng = np.random.default_rng(9)
    e = plain.emb.cpu().numpy().astype(np.float64)
    lab = np.arange(240) % 6
    rows = e.mean(0) + (rng.normal(size=(6, 24))[lab] + 0.5 * rng.normal(size=(240, 24))) * (e.std(0) + 1e-3)
    model = PL.fit_plda(EmbeddingCache(cuda(rows.astype(np.float32)), lab), lda_dim=6)
    segments, res = DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075, distance="plda", plda=model)
    assert torch.equal(res.emb, plain.emb) and res.rows.shape == (len(plain.emb), model.P) and torch.equal(res.rows, model.project(res.emb))
    thr = float(np.nanmedian(res.host().merge_h))
    seg_t, res_t = DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075, distance="plda", plda=model, threshold=thr)
    for r in range(2):
        lo, hi = int(res.row0[r]), int(res.row0[r + 1])
        full = res.recording(r)
        want = DZ.ahc_reference(pairdist(res.rows[lo:hi].cpu().numpy(), res.rows[lo:hi].cpu().numpy(), PLDA)[0], "average")
        assert np.array_equal(full.merge_a, want.merge_a) and np.array_equal(bits(full.merge_h), bits(want.merge_h))
        labels, c = DZ.cut(full.merge_a, full.merge_b, full.merge_h, hi - lo, threshold=thr)
        got = res_t.recording(r)
        assert np.array_equal(got.labels, labels) and got.n_clusters == c
        assert np.array_equal(seg_t[r], DZ.window_segments(res.starts[r], res.window, int(conv.lens[r]), labels))
    with pytest.raises(ValueError, match="come together"):
        DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075, distance="plda")
    with pytest.raises(ValueError, match="come together"):
        DZ.diarize(net, conv.audio, conv.offsets, conv.lens, bp, 0.15, 0.075, plda=model)
