"""No-GPU tests of the VBx statement, voicemap_amd/diarization.py vbx_reference (the numpy twin of vm_vbx): its posteriors and bound
against enumeration of all paths and against a log-domain forward-backward, its structure (chain starts, K = 1, normalisation), the
monotone bound, a planted conversation, and the rounding bound of tests/vbx_cases.py between its float64 and its extended-precision
run on every case the device tests use."""
import numpy as np
import pytest

from tests import vbx_cases as VC
from voicemap_amd import diarization as DZ

NEVER = -np.inf


def one_iteration(case, loop_prob, fa, fb, dtype=np.float64, **kw):
    return DZ.vbx_reference(case["rows"], case["row0"], case["n_models"], case["labels"], case["chain_start"], case["tables"], loop_prob,
                            fa, fb, 5.0, 1, NEVER, gamma=case["gamma"], pi=case["pi"], dtype=dtype, **kw)


def independent(case, fa, fb):
    """(lp, ent) of the one recording of ``case`` from its warm start, by tests/vbx_cases.py's vectorised statement."""
    n, K, D = len(case["rows"]), int(case["n_models"][0]), case["D"]
    lp, ent, _, _, _ = VC.posterior_terms(case["rows"][:, :D].astype(np.float64), case["tables"], case["gamma"].reshape(n, K), fa, fb)
    return lp, ent


@pytest.mark.parametrize("loop_prob", [0.0, 0.5, 0.99])
@pytest.mark.parametrize("n,K", [(1, 3), (4, 3), (6, 2), (6, 3), (5, 1)])
def test_posteriors_and_log_px_against_all_paths(n, K, loop_prob):
    case = VC.random_case(7 * n + K, [n], K, 3)
    if n >= 4:
        case["chain_start"] = np.zeros(n, np.int32)
        case["chain_start"][n // 2] = 1   # a chain start in the middle
    fa, fb = 0.7, 3.0
    got = one_iteration(case, loop_prob, fa, fb)
    lp, ent = independent(case, fa, fb)
    gamma, log_px = VC.brute_force(lp, VC.lambdas(case["chain_start"], n, loop_prob), case["pi"][0, :K])
    assert np.allclose(got.gamma.reshape(n, K), gamma, rtol=1e-10, atol=1e-300)
    assert abs(got.elbo[0, 0] - (log_px + 0.5 * fb * ent.sum())) <= 1e-10 * (abs(log_px) + 0.5 * fb * np.abs(ent).sum())
    # row by row: the label is a speaker whose enumerated posterior is within 1e-9 of the row's maximum
    assert (gamma[np.arange(n), got.labels] >= gamma.max(1) - 1e-9).all()


@pytest.mark.parametrize("n,K,D", [(40, 5, 6), (130, 7, 20), (64, 64, 4)])
def test_posteriors_and_log_px_against_a_log_domain_forward_backward(n, K, D):
    case = VC.random_case(n + K, [n], K, D, chains="edges")
    fa, fb = 0.3, 17.0
    got = one_iteration(case, 0.9, fa, fb)
    lp, ent = independent(case, fa, fb)
    gamma, log_px = VC.log_forward_backward(lp, VC.lambdas(case["chain_start"], n, 0.9), case["pi"][0, :K])
    assert np.allclose(got.gamma.reshape(n, K), gamma, rtol=1e-8, atol=1e-300)
    assert abs(got.elbo[0, 0] - (log_px + 0.5 * fb * ent.sum())) <= 1e-9 * (abs(log_px) + 0.5 * fb * np.abs(ent).sum())


def test_a_chain_start_is_two_recordings_that_share_pi():
    """The posteriors of a recording with a chain start at row s, under FIXED speaker models and priors, are those of its two halves as
    recordings of their own: compared through the independent forward-backward on the twin's emissions, and on the twin itself where
    the halves are given the whole's models (a warm start whose sums are the whole's is not expressible, so the halves go through
    the forward-backward statement)."""
    n, K, s = 30, 4, 13
    case = VC.random_case(5, [n], K, 5)
    case["chain_start"] = np.zeros(n, np.int32)
    case["chain_start"][s] = 1
    got = one_iteration(case, 0.8, 0.5, 2.0).gamma.reshape(n, K)
    lp, _ = independent(case, 0.5, 2.0)
    pi = case["pi"][0, :K]
    first, _ = VC.log_forward_backward(lp[:s], VC.lambdas(None, s, 0.8), pi)
    second, _ = VC.log_forward_backward(lp[s:], VC.lambdas(None, n - s, 0.8), pi)
    assert np.allclose(got, np.concatenate([first, second]), rtol=1e-9, atol=1e-300)


def test_a_chain_start_through_the_twin_itself_on_two_recordings():
    """Two recordings that share pi, through the twin alone.  The whole is the rows X twice, with the same posteriors twice and a
    chain start at the seam: its sums are N_k = 2 N_k(X) and F_kd = 2 F_kd(X).  The halves are two recordings X with fb halved, so that
    F = fa / fb doubles: F N_k and F F_kd, hence invL, alpha and every emission, are the whole's (fa, which scales the emissions, is
    the same).  The posteriors do not depend on fb otherwise, and the new priors of the whole are the mean of the halves'."""
    n, K, D = 23, 4, 5
    half = VC.random_case(8, [n], K, D, chains="edges")
    args = dict(loop_prob=0.8, fa=0.5, init_smooth=5.0, iters=1, epsilon=NEVER)
    cs = np.concatenate([half["chain_start"], [1], half["chain_start"][1:]]).astype(np.int32)
    whole = DZ.vbx_reference(np.concatenate([half["rows"]] * 2), [0, 2 * n], K, np.concatenate([half["labels"]] * 2), cs, half["tables"],
                             fb=2.0, gamma=np.concatenate([half["gamma"]] * 2), pi=half["pi"], **args)
    two = DZ.vbx_reference(np.concatenate([half["rows"]] * 2), [0, n, 2 * n], K, np.concatenate([half["labels"]] * 2),
                           np.concatenate([half["chain_start"]] * 2), half["tables"], fb=1.0, gamma=np.concatenate([half["gamma"]] * 2),
                           pi=np.concatenate([half["pi"]] * 2), **args)
    assert list(whole.iters_run) == [1] and list(two.iters_run) == [1, 1]
    assert np.allclose(whole.gamma, two.gamma, rtol=1e-10, atol=1e-300) and np.array_equal(whole.labels, two.labels)
    assert np.allclose(two.pi[0], two.pi[1], rtol=1e-12) and np.allclose(whole.pi[0], two.pi[0], rtol=1e-10)


def test_a_degenerate_recording_stops_with_its_labels():
    case = VC.degenerate_case()
    got = one_iteration(case, 0.9, 0.3, 17.0)
    assert got.iters_run[0] == -2 and np.array_equal(got.labels, case["labels"]) and np.isnan(got.elbo).all()
    assert np.array_equal(got.gamma, case["gamma"]) and np.array_equal(got.pi, case["pi"])   # as the start left them
    # after a complete iteration: a prior that is exactly 0 only from the second iteration on
    late = dict(case, pi=np.pad(np.array([[0.5, 0.5]]), ((0, 0), (0, 62))))
    one = one_iteration(late, 0.9, 0.3, 17.0)
    assert one.iters_run[0] == 1
    zero = one.pi.copy()
    zero[0, :2] = [0.0, 1.0]
    two = DZ.vbx_reference(late["rows"], late["row0"], 2, late["labels"], None, late["tables"], 0.9, 0.3, 17.0, 5.0, 1, NEVER,
                           gamma=one.gamma, pi=zero)
    assert two.iters_run[0] == -2 and np.array_equal(two.gamma, one.gamma)


def test_one_speaker_is_trivial_and_everything_is_normalised():
    one = VC.random_case(1, [17], 1, 4)
    got = one_iteration(one, 0.9, 0.3, 17.0)
    assert (got.gamma == 1.0).all() and got.pi[0, 0] == 1.0 and (got.pi[0, 1:] == 0).all() and (got.labels == 0).all()
    case = VC.random_case(2, [50, 0, 21], [5, 3, 64], 6, chains="edges")
    got = DZ.vbx_reference(case["rows"], case["row0"], case["n_models"], case["labels"], case["chain_start"], case["tables"], 0.9, 0.3,
                           17.0, 5.0, 4, NEVER)
    assert list(got.iters_run) == [4, 0, 4] and np.isnan(got.elbo[1]).all() and (got.pi[1] == 0).all()
    assert np.allclose(got.gamma[:250].reshape(50, 5).sum(1), 1.0, atol=1e-13) and np.allclose(got.gamma[250:].reshape(21, 64).sum(1), 1.0, atol=1e-13)
    assert np.allclose(got.pi[[0, 2]].sum(1), 1.0, atol=1e-13) and (got.pi[0, 5:] == 0).all()


def test_the_start_from_labels_and_the_stop_rule():
    case = VC.random_case(3, [40], 3, 4)
    case["labels"][:3] = [-1, 3, 1]
    got = DZ.vbx_reference(case["rows"], case["row0"], 3, case["labels"], None, case["tables"], 0.9, 0.3, 17.0, 2.0, 1, NEVER)
    # one iteration from the labels = one iteration from the softmax of the smoothed one-hot rows, uniform where there is no cluster
    q = np.exp(-2.0)
    g = np.where(case["labels"][:, None] == np.arange(3)[None, :], 1.0, q) / (1.0 + 2.0 * q)
    g[(case["labels"] < 0) | (case["labels"] >= 3)] = 1.0 / 3.0
    assert np.allclose(g.sum(1), 1.0)
    warm = DZ.vbx_reference(case["rows"], case["row0"], 3, case["labels"], None, case["tables"], 0.9, 0.3, 17.0, 2.0, 1, NEVER,
                            gamma=g.ravel(), pi=np.pad(np.full((1, 3), 1.0 / 3.0), ((0, 0), (0, 61))))
    assert np.allclose(got.gamma, warm.gamma, rtol=1e-12) and np.allclose(got.elbo, warm.elbo, rtol=1e-12)
    # a huge epsilon stops at the second iteration, which is counted and kept; elbo is NaN past it
    full = DZ.vbx_reference(case["rows"], case["row0"], 3, case["labels"], None, case["tables"], 0.9, 0.3, 17.0, 2.0, 6, NEVER)
    stop = DZ.vbx_reference(case["rows"], case["row0"], 3, case["labels"], None, case["tables"], 0.9, 0.3, 17.0, 2.0, 6, 1e30)
    assert stop.iters_run[0] == 2 and np.isnan(stop.elbo[0, 2:]).all() and np.array_equal(stop.elbo[0, :2], full.elbo[0, :2])
    assert full.iters_run[0] == 6 and np.isfinite(full.elbo).all()
    with pytest.raises(ValueError):
        DZ.vbx_reference(case["rows"], case["row0"], 65, case["labels"], None, case["tables"], 0.9, 0.3, 17.0, 2.0, 1, NEVER)
    for bad in (dict(loop_prob=1.0), dict(fa=0.0), dict(fb=np.inf), dict(init_smooth=-1.0), dict(iters=0), dict(iters=65),
                dict(epsilon=np.nan)):
        kw = dict(loop_prob=0.9, fa=0.3, fb=17.0, init_smooth=2.0, iters=1, epsilon=NEVER)
        kw.update(bad)
        with pytest.raises(ValueError):
            DZ.vbx_reference(case["rows"], case["row0"], 3, case["labels"], None, case["tables"], **kw)


def test_the_elbo_never_decreases():
    """fa = fb = 1 is the exact variational bound: 20 iterations, no drop larger than the float64 spread measured against the
    extended-precision run."""
    case = VC.random_case(11, [120], 6, 8, chains="edges")
    args = (case["rows"], case["row0"], 6, case["labels"], case["chain_start"], case["tables"], 0.9, 1.0, 1.0, 5.0, 20, NEVER)
    f64, ext = DZ.vbx_reference(*args), DZ.vbx_reference(*args, dtype=np.longdouble)
    assert f64.iters_run[0] == ext.iters_run[0] == 20
    spread = float(np.abs(f64.elbo[0].astype(np.longdouble) - ext.elbo[0]).max())
    print("float64 spread of the ELBO:", spread, "first and last:", float(f64.elbo[0, 0]), float(f64.elbo[0, -1]))
    assert (np.diff(f64.elbo[0]) >= -spread).all()
    assert f64.elbo[0, -1] > f64.elbo[0, 0]


def test_a_planted_conversation_ends_with_its_speakers():
    model, rows, truth, labels = VC.planted_corpus()
    assert len(np.unique(labels)) == 6 and len(truth) >= 72
    args = (rows, [0, len(rows)], 6, labels, None, DZ.vbx_tables(model), 0.9, 0.3, 17.0, 5.0, 20, 1e-4)
    f64, ext = DZ.vbx_reference(*args), DZ.vbx_reference(*args, dtype=np.longdouble)
    assert VC.planted_ok(f64.labels, truth) and VC.planted_ok(ext.labels, truth)
    assert np.array_equal(f64.labels, ext.labels) and f64.iters_run[0] == ext.iters_run[0] >= 2
    # three priors carry the conversation, three have shrunk away
    assert (np.sort(f64.pi[0, :6])[:3] < 1e-3).all() and (np.sort(f64.pi[0, :6])[3:] > 0.1).all()


@pytest.mark.parametrize("it", [1, 2, 5])
def test_the_float64_twin_stays_inside_the_bound_on_the_mixed_case(it):
    """The case of the device's iteration tests: the float64 twin's iteration ``it`` from its own state after ``it - 1``."""
    case = VC.mixed_case()
    gamma, pi = case["gamma"], case["pi"]
    if it > 1:
        state = DZ.vbx_reference(case["rows"], case["row0"], case["n_models"], case["labels"], case["chain_start"], case["tables"],
                                 VC.PARAMS["loop_prob"], VC.PARAMS["fa"], VC.PARAMS["fb"], 5.0, it - 1, NEVER, gamma=gamma, pi=pi)
        assert list(state.iters_run) == [it - 1, 0, it - 1, it - 1, it - 1]
        gamma, pi = state.gamma, state.pi
    used = VC.check_one_iteration(case, VC.exact(case, gamma, pi, dtype=np.float64), VC.exact(case, gamma, pi), VC.PARAMS, gamma=gamma, pi=pi)
    print("iteration", it, "used shares of the gamma, pi, elbo bounds:", used)


@pytest.mark.parametrize("K,D,n", VC.GRID)
def test_the_float64_twin_stays_inside_the_bound(K, D, n):
    case = VC.grid_case(K, D, n)
    f64 = one_iteration(case, VC.PARAMS["loop_prob"], VC.PARAMS["fa"], VC.PARAMS["fb"])
    used = VC.check_one_iteration(case, f64, VC.exact_one_iteration(K, D, n), VC.PARAMS)
    print("K", K, "D", D, "n", n, "used shares of the gamma, pi, elbo bounds:", used)
