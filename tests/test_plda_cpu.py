"""Host checks of the PLDA back end (voicemap_amd/plda.py): the diagonal form against the joint Gaussian densities, the fp32 score of
projected rows against the float64 log-likelihood ratio inside a counted bound, EM's monotone likelihood and its fixed point, the
error paths and the file round trip.  No GPU: the float64 statements stand in for the kernels (tests/test_gpu_plda.py holds the
kernels to these statements)."""
import numpy as np
import pytest

from tests import plda_cases as PC
from voicemap_amd import plda as PL


@pytest.mark.parametrize("D", (1, 2, 5, 16))
def test_llr_numpy_is_the_direct_statement(D):
    """The log of the joint density of (x_i, x_j) under "one speaker" less the two marginals, with full Phi_b and Phi_w through
    numpy.linalg, against the diagonal form: 1e-9 relative."""
    rng = np.random.default_rng(100 + D)
    for _ in range(3):
        Phi_b, Phi_w, mu = PC.random_spd(rng, D), PC.random_spd(rng, D), rng.normal(size=D)
        model = PL.PldaModel.from_covariances(mu, Phi_b, Phi_w)
        assert model.D == D and model.P == 4 * ((D + 4) // 4) and (np.diff(model.psi) <= 0).all()
        a, b = mu + 2.0 * rng.normal(size=(9, D)), mu + 2.0 * rng.normal(size=(6, D))
        got, want = model.llr_numpy(a, b), PC.direct_llr(a, b, mu, Phi_b, Phi_w)
        assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-3)) < 1e-9
        assert np.array_equal(model.llr_numpy(a), model.llr_numpy(a, a)) and np.allclose(model.llr_numpy(a), model.llr_numpy(a).T, rtol=0, atol=1e-12)


def test_a_direction_without_between_speaker_variance_is_dropped():
    rng = np.random.default_rng(3)
    Phi_w = PC.random_spd(rng, 4)
    v = rng.normal(size=(4, 2))
    model = PL.PldaModel.from_covariances(np.zeros(4), v @ v.T - 1e-3 * np.eye(4), Phi_w)   # two positive, two negative directions
    assert model.D == 2 and model.P == 4 and (model.psi > 0).all()
    with pytest.raises(ValueError, match="no positive direction"):
        PL.PldaModel.from_covariances(np.zeros(4), -np.eye(4), Phi_w)


@pytest.mark.parametrize("length_norm,lda_dim", ((True, None), (False, None), (True, 7)))
def test_scores_of_projected_rows_are_minus_the_llr_within_the_counted_bound(length_norm, lda_dim):
    (tx, ts), (hx, _) = PC.e2e_corpora()
    model = PL.fit_plda_numpy(tx, ts, lda_dim=lda_dim, length_norm=length_norm)
    Z = model.project_numpy(hx)
    assert Z.dtype == np.float32 and Z.shape == (len(hx), model.P) and not Z[:, model.D:-1].any()
    got = PL.plda_scores_numpy(Z).astype(np.float64)
    want = -model.llr_numpy(hx)
    bound = PC.projected_score_bound(model, hx)
    ratio = np.abs(got - want) / bound
    print("largest error / bound: %.3f; largest error %.3g at scores up to %.3g" % (ratio.max(), np.abs(got - want).max(), np.abs(want).max()))
    assert (ratio <= 1.0).all()
    assert bound.max() < 1e-3 * np.abs(want).max()   # the bound says something


def test_plda_scores_numpy_handles_a_row_term_that_is_not_finite():
    rng = np.random.default_rng(0)
    Z = PC.grid_plda_rows(rng, 5, 8)
    Z[1, -1], Z[3, -1] = np.inf, np.nan
    s = PL.plda_scores_numpy(Z)
    bad = np.zeros((5, 5), bool)
    bad[[1, 3], :] = bad[:, [1, 3]] = True
    assert np.array_equal(np.isnan(s), bad)
    z64 = Z.astype(np.float64)
    want = (z64[:, -1][:, None] + z64[:, -1][None, :]) - z64[:, :-1] @ z64[:, :-1].T
    assert np.array_equal(s[~bad], want[~bad].astype(np.float32))


def _stats(x, speaker):
    label, S = PL.dense_labels(speaker)
    count, sums, mu, T = PL._numpy_stats(x, label, S)
    dev = sums / count[:, None] - mu[None, :]
    return count, dev, T - (dev * count[:, None]).T @ dev, mu


def test_em_never_lowers_the_marginal_likelihood():
    """From the moment estimate and from a poor start, balanced and unbalanced: every step's likelihood is at least the last one's, up to
    1e-10 relative."""
    mu, Phi_b, Phi_w = PC.e2e_model()
    x, spk = PC.two_covariance_corpus(11, 30, 6, PC.E2E_E, Phi_b, Phi_w, mu)
    keep = np.ones(len(x), bool)
    keep[np.random.default_rng(1).choice(len(x), 50, replace=False)] = False      # unbalanced: speakers keep 2 .. 6 rows
    for xs, ss in ((x, spk), (x[keep], spk[keep])):
        count, dev, W, _ = _stats(xs, ss)
        for start in (PL.moment_estimate(count, dev, W), (np.eye(PC.E2E_E) * 7.0, np.eye(PC.E2E_E) * 0.01)):
            _, _, ll = PL.em_two_covariance(count, dev, W, *start, iters=12)
            ll = np.asarray(ll)
            assert len(ll) == 13 and np.isfinite(ll).all()
            assert (np.diff(ll) >= -1e-10 * np.abs(ll[:-1])).all(), np.diff(ll)
            assert ll[-1] > ll[0]


def test_em_holds_the_closed_form_solution_of_a_balanced_design():
    """Balanced data, S speakers of n rows: the likelihood's maximum is Phi_w = SSW / (S (n - 1)), Phi_b = SSB / (S n) - Phi_w / n where
    that is positive definite, and one EM iteration started there moves neither matrix by 1e-9 relative."""
    rng = np.random.default_rng(7)
    D, S, n = 5, 400, 4
    Phi_b, Phi_w = PC.random_spd(rng, D, 0.5, 4.0), PC.random_spd(rng, D, 0.5, 4.0)
    x, spk = PC.two_covariance_corpus(8, S, n, D, Phi_b, Phi_w, rng.normal(size=D))
    count, dev, W, _ = _stats(x, spk)
    ssb = (dev * count[:, None]).T @ dev
    w0 = W / (S * (n - 1))
    b0 = ssb / (S * n) - w0 / n
    assert np.linalg.eigvalsh(b0).min() > 0
    b1, w1, ll = PL.em_two_covariance(count, dev, W, b0, w0, iters=1)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    assert rel(b1, b0) < 1e-9 and rel(w1, w0) < 1e-9, (rel(b1, b0), rel(w1, w0))
    assert abs(ll[1] - ll[0]) <= 1e-10 * abs(ll[0])
    # ... and it is where EM from the moment estimate is heading
    b9, w9, ll9 = PL.em_two_covariance(count, dev, W, *PL.moment_estimate(count, dev, W), iters=200)
    assert ll9[-1] <= ll[0] + 1e-9 * abs(ll[0]) and rel(w9, w0) < 1e-3


def test_fit_ignores_rows_with_a_negative_label_and_refuses_what_it_cannot_fit():
    (tx, ts), _ = PC.e2e_corpora()
    rng = np.random.default_rng(2)
    extra = rng.normal(size=(9, PC.E2E_E)).astype(np.float32) * 50
    a = PL.fit_plda_numpy(tx, ts, em_iters=3)
    b = PL.fit_plda_numpy(np.concatenate([extra[:4], tx, extra[4:]]), np.concatenate([-np.ones(4, int), ts, -np.arange(1, 6)]), em_iters=3)
    assert np.allclose(a.psi, b.psi, rtol=1e-9, atol=0) and np.allclose(a.mean1, b.mean1, rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="at least two speakers"):
        PL.fit_plda_numpy(tx[:8], ts[:8])
    with pytest.raises(ValueError, match="at least two speakers"):
        PL.fit_plda_numpy(tx, -np.ones(len(tx), int))
    with pytest.raises(ValueError, match="two rows"):
        PL.fit_plda_numpy(tx[::8], ts[::8])
    with pytest.raises(ValueError, match="lda_dim"):
        PL.fit_plda_numpy(tx, ts, lda_dim=17)
    with pytest.raises(ValueError, match="lda_dim"):
        PL.fit_plda_numpy(tx, ts, lda_dim=0)
    flat = tx.copy()
    flat[:, 3] = 0.0                                 # a component that never varies: the within scatter has a zero row
    with pytest.raises(ValueError, match="not positive definite"):
        PL.fit_plda_numpy(flat, ts)
    with pytest.raises(ValueError, match="do not fit together"):
        PL.PldaModel(np.zeros(3), np.eye(3), True, np.zeros(2), np.eye(3), np.ones(3), 0.0, np.ones(3))
    with pytest.raises(ValueError, match="1 .. 255"):
        PL.PldaModel(np.zeros(256), np.eye(256), True, np.zeros(256), np.eye(256), np.ones(256), 0.0, np.ones(256))


def test_the_score_name_is_wired_without_touching_the_other_tables():
    from voicemap_amd import _lib, verification as V
    assert _lib.VM_SCORE_PLDA == 6 and _lib.PAIR_DIST == {**_lib.DIST, "plda": 6} and "plda" not in _lib.DIST and "plda" not in V.SCORES

    class Cache:
        def __init__(self, E):
            self.E = E
    assert V.score_kind(Cache(68), "plda", None) == (6, None, None)
    for E in (0, 2, 67):
        with pytest.raises(ValueError, match="multiple of 4"):
            V.score_kind(Cache(E), "plda", None)
    with pytest.raises(ValueError, match="plda"):
        V.score_kind(Cache(8), "plda2", None)


def test_save_and_load_round_trip_bit_for_bit(tmp_path):
    (tx, ts), (hx, _) = PC.e2e_corpora()
    model = PL.fit_plda_numpy(tx, ts, lda_dim=9, length_norm=True, em_iters=4)
    path = tmp_path / "model.npz"
    model.save(path)
    back = PL.PldaModel.load(path)
    for k in PL.PldaModel.FIELDS:
        a, b = getattr(model, k), getattr(back, k)
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), k
    assert back.length_norm is True and back.c0 == model.c0 and len(back.loglik) == 5
    assert np.array_equal(back.project_numpy(hx).view(np.uint32), model.project_numpy(hx).view(np.uint32))
    other = PL.fit_plda_numpy(tx, ts, length_norm=False, em_iters=1)
    other.save(path)
    assert PL.PldaModel.load(path).length_norm is False


def test_the_statements_of_the_kernels_on_a_hand_case():
    x = np.array([[1.0, 2.0], [3.0, -2.0], [5.0, 0.0]], dtype=np.float32)
    mean = np.array([3.0, 0.0])
    assert np.array_equal(PL.scatter_reference(x, None, mean), [[8.0, -4.0], [-4.0, 8.0]])
    assert np.array_equal(PL.scatter_reference(x, np.array([0, -1, 4]), mean), [[8.0, -4.0], [-4.0, 4.0]])
    A = np.array([[1.0, 0.0], [0.0, 0.5], [1.0, 1.0]])
    rows = PL.project_reference(x, mean, A, False)
    assert rows.dtype == np.float32 and np.array_equal(rows, [[-2.0, 1.0, 0.0], [0.0, -1.0, -2.0], [2.0, 0.0, 2.0]])
    z = PL.project_reference(x, mean, A, False, quad=np.array([1.0, 2.0, 0.25]), c0=-1.0)
    assert z.shape == (3, 4) and np.array_equal(z[:, :3], rows) and np.array_equal(z[:, 3], [5.0, 2.0, 4.0])
    n = PL.project_reference(np.array([[3.0, 0.0], [6.0, 4.0]], np.float32), mean, np.eye(2), True)
    assert np.array_equal(n[0], [0.0, 0.0]) and np.allclose(n[1], np.array([3.0, 4.0]) * np.sqrt(2.0) / 5.0, rtol=1e-7)
    both = PL.plda_reference(x, mean, A, False)
    assert np.array_equal(both["rows"], rows) and np.array_equal(both["scatter"], [[8.0, -4.0], [-4.0, 8.0]])
    assert [PL.padded_width(d) for d in (1, 2, 3, 4, 63, 64, 255)] == [4, 4, 4, 8, 64, 68, 256]
