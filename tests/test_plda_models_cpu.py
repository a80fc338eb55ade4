"""CPU checks of multi-session PLDA speaker models (voicemap_amd/plda.py model_tables / model_llr_numpy / trial_scores_plda_numpy,
voicemap_amd/enrolment.py enrol(plda=...)): the closed form against the joint Gaussian densities with full matrices, the coefficient
tables against the closed form, the numpy twin of the kernel's contract against a loop that re-enrols every model by hand, and the
error paths.  No GPU."""
import numpy as np
import pytest

from tests import plda_cases as PC
from voicemap_amd import _lib
from voicemap_amd import enrolment as EN
from voicemap_amd import plda as PL


def _model(D, seed):
    rng = np.random.default_rng(seed)
    return PL.PldaModel.from_covariances(rng.normal(size=D), PC.random_spd(rng, D), PC.random_spd(rng, D)), rng


def _joint(rows, mu, Phi_b, Phi_w):
    """log density of k rows of ONE speaker: covariance Phi_b in every block plus Phi_w on the diagonal blocks, full matrices."""
    k = len(rows)
    J = np.kron(np.ones((k, k)), Phi_b) + np.kron(np.eye(k), Phi_w)
    return PC.log_gauss(rows.reshape(1, -1), np.tile(mu, k), J)[0]


def _close(a, b, rel=1e-9):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= rel * np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("n", (1, 2, 5))
@pytest.mark.parametrize("D", (1, 2, 5, 16))
def test_model_llr_equals_the_log_ratio_of_the_joint_densities(D, n):
    """llr = log p(e_1 .. e_n, t | one speaker) - log p(e_1 .. e_n | one speaker) - log p(t), every density a Gaussian with its full
    (k D, k D) covariance through numpy.linalg; at n = 1 it is also ``llr_numpy`` of the two rows; and the table form on w is the same."""
    model, rng = _model(D, 100 * D + n)
    mu, Phi_b, Phi_w = model.mean2, model.Phi_b, model.Phi_w
    e = rng.normal(size=(n, D)) * 2.0 + mu
    t = rng.normal(size=(7, D)) * 2.0 + mu
    got = model.model_llr_numpy(e, t)
    want = np.array([_joint(np.vstack([e, t[i:i + 1]]), mu, Phi_b, Phi_w) - _joint(e, mu, Phi_b, Phi_w)
                     - PC.log_gauss(t[i:i + 1], mu, Phi_b + Phi_w)[0] for i in range(len(t))])
    assert _close(got, want)
    if n == 1:
        assert _close(got, model.llr_numpy(e, t)[0])
    tab = model.model_tables(max(n, 3))
    b = PL.llr_terms(model.psi)["b"]
    w, sigma = model.z_numpy(t) * np.sqrt(b), (model.z_numpy(e) * np.sqrt(b)).sum(0)
    score = (tab["A"][n] * (w - tab["beta"][n] * sigma) ** 2).sum(1) - (tab["G"] * w * w).sum(1) - tab["C"][n]
    assert _close(-score, got)


def test_tables_have_the_stated_shapes_and_row_zero_is_unused():
    model, _ = _model(5, 3)
    tab = model.model_tables(4)
    assert tab["A"].shape == tab["beta"].shape == (5, 5) and tab["C"].shape == (5,) and tab["G"].shape == (5,)
    assert all(v.dtype == np.float64 and v.flags.c_contiguous for v in tab.values())
    assert not tab["A"][0].any() and not tab["beta"][0].any() and tab["C"][0] == 0.0
    t = PL.llr_terms(model.psi)
    # n = 1 is the row-against-row score of the module docstring: sum A (w_i - beta w_j)^2 - G w_i^2 - C == (h_i + h_j) - w_i . w_j
    rng = np.random.default_rng(0)
    wi, wj = rng.normal(size=5), rng.normal(size=5)
    h = lambda w: (t["q"] * w * w).sum() + t["c0"]
    assert _close((tab["A"][1] * (wi - tab["beta"][1] * wj) ** 2).sum() - (tab["G"] * wi * wi).sum() - tab["C"][1], h(wi) + h(wj) - wi @ wj)


def _by_hand(model, proj, label, q, q_label, loo, S, n_max):
    """Every cell from scratch: gather the enrolment rows of the speaker (without the query row itself under leave-one-out, which is
    then the row of the same index), and score the query by the predictive densities in z -- no sums, no tables."""
    D = model.D
    sb = np.sqrt(PL.llr_terms(model.psi)["b"])
    psi = model.psi
    out = np.full((len(q), S), np.nan)
    trial = np.zeros((len(q), S), bool)
    for m in range(len(q)):
        for s in range(S):
            rows = np.flatnonzero(label == s)
            if loo and q_label[m] == s:
                rows = rows[rows != m]
            n = len(rows)
            if not 1 <= n <= n_max:
                continue
            ze = proj[rows, :D].astype(np.float64) / sb
            zt = q[m, :D].astype(np.float64) / sb
            mean, var = psi * ze.sum(0) / (1 + n * psi), 1 + psi / (1 + n * psi)
            llr = (-0.5 * (np.log(var) + (zt - mean) ** 2 / var) + 0.5 * (np.log(1 + psi) + zt * zt / (1 + psi))).sum()
            out[m, s], trial[m, s] = -llr, True
    return out, trial


@pytest.mark.parametrize("loo", (True, False))
def test_twin_equals_a_loop_that_re_enrols_by_hand(loo):
    model, rng = _model(6, 11)
    S, sizes = 5, [1, 4, 0, 7, 3]
    label = np.repeat(np.arange(S), sizes)
    rng.shuffle(label)
    label = np.concatenate([label, [-1]]).astype(np.int32)        # one row is not enrolled
    raw = rng.normal(size=(len(label), 6)) * 2.0 + model.mean2
    proj = model.project_numpy(raw)
    assert proj.shape == (len(label), 8) and proj.dtype == np.float32
    tab = model.model_tables(6)                                   # the speaker with 7 rows has no shared model: 7 > n_max
    got, trial = PL.trial_scores_plda_numpy(proj, label, proj, label, tab, loo, S)
    want, want_trial = _by_hand(model, proj, label, proj, label, loo, S, 6)
    assert np.array_equal(trial, want_trial)
    assert _close(got[trial], want[trial]) and np.isnan(got[~trial]).all()
    one = int(np.flatnonzero(label == 0)[0])
    assert trial[one, 0] == (not loo)                             # a speaker with one row: under leave-one-out its own trial is gone
    assert not trial[:, 2].any()                                  # nobody enrolled
    big = label == 3
    assert not trial[~big, 3].any() and trial[big, 3].all() == loo   # 7 rows: only the own rows' leave-one-out models (6 rows) exist
    ranks = EN.ranks_numpy(got, trial, label)
    assert ranks["rank"][one] == (-1 if loo else ranks["rank"][one]) and ranks["rank"][-1] == -1
    # the default S and foreign queries
    g2, t2 = PL.trial_scores_plda_numpy(proj, label, proj[:3], [-1, 9, 1], tab, loo)
    assert g2.shape == (3, 5) and np.array_equal(t2[0], t2[1])


def test_error_paths():
    model, rng = _model(4, 5)
    with pytest.raises(ValueError, match="n_max"):
        model.model_tables(0)
    with pytest.raises(ValueError, match="at least one"):
        model.model_llr_numpy(np.zeros((0, 4)), np.zeros((2, 4)))
    tab = model.model_tables(3)
    rows = model.project_numpy(rng.normal(size=(6, 4)))
    lab = np.array([0, 0, 1, 1, 1, -1])
    with pytest.raises(ValueError, match="tables"):
        PL.trial_scores_plda_numpy(rows, lab, rows, lab, dict(tab, C=tab["C"][:2]), False)
    with pytest.raises(ValueError, match="P > D"):
        PL.trial_scores_plda_numpy(rows[:, :4], lab, rows[:, :4], lab, tab, False)


def test_enrol_refuses_a_cache_that_is_not_projected_and_a_distance_beside_plda():
    import torch
    from voicemap_amd.retrieval import EmbeddingCache
    model, rng = _model(4, 6)
    raw = EmbeddingCache(torch.zeros(6, 4), np.arange(6) % 2)       # the model's own input width: a raw cache
    with pytest.raises(ValueError, match=r"projected by the model.*width 8, got 4"):
        EN.enrol(raw, plda=model)
    with pytest.raises(ValueError, match="leave distance out"):
        EN.enrol(EmbeddingCache(torch.zeros(6, 8), np.arange(6) % 2), "cosine", plda=model)
    assert "plda" not in _lib.DIST and "plda" not in EN.KINDS           # plda= is the switch, not a distance name
    with pytest.raises(ValueError, match="distance must be one of"):
        EN.enrol(raw, "plda")


def test_the_entry_points_are_declared_and_refuse_bad_arguments_before_any_launch():
    P, I, L_ = _lib.P, _lib.I, _lib.L
    names = ("vm_plda_speaker_identify", "vm_plda_speaker_identify_workspace_bytes", "vm_plda_speaker_trial_hist",
             "vm_plda_speaker_trial_hist_workspace_bytes")
    for n in names:
        assert n in _lib.header_functions() and n in _lib.SIGNATURES
    assert _lib.SIGNATURES[names[0]] == (I, [P, P, L_, I, I, P, P, L_, P, P, P, P, I, I, P, P, P, P, P, P, P])
    assert _lib.SIGNATURES[names[2]] == (I, [P, P, L_, I, I, P, P, L_, P, P, P, P, I, I, P, I, I, P, P, P])
    assert _lib.SIGNATURES[names[1]] == (L_, [L_, I, L_])
    lib = _lib.lib()
    assert lib.query(names[1], 10, 3, 4) >= 2 * 4 * 3 * 8 + 4 * 8 + 10 * 12 and lib.query(names[1], 10, 0, 4) == 0
    x = 0x10000   # a pointer-like value that is never dereferenced: every call below fails its argument check first
    win = np.array([0, 22], dtype=np.int64)

    def ident(M=4, P_=8, D=5, S=3, n_max=2, q=x, A=x, ws=x, rank=x):
        return lib.cdll.vm_plda_speaker_identify(q, x, M, P_, D, x, x, S, A, x, x, x, n_max, 0, None, x, rank, x, x, ws, None)

    def hist(P_=8, D=5, n_max=2, wins=win.ctypes.data, n_win=1, bins=16, h=x):
        return lib.cdll.vm_plda_speaker_trial_hist(x, x, 4, P_, D, x, x, 3, x, x, x, x, n_max, 0, wins, n_win, bins, h, x, None)

    for call, what in ((lambda: ident(q=None), "null pointer"), (lambda: ident(A=None), "null pointer"), (lambda: ident(ws=None), "null pointer"),
                       (lambda: ident(rank=None), "null pointer"), (lambda: ident(D=8), "D < P"), (lambda: ident(D=0), "D < P"),
                       (lambda: ident(P_=6, D=5), "P % 4 == 0"), (lambda: ident(P_=260, D=5), "P <= 256"), (lambda: ident(n_max=0), "n_max"),
                       (lambda: ident(S=0), "bad sizes"), (lambda: ident(M=-1), "bad sizes"), (lambda: ident(q=x + 4), "16-byte"),
                       (lambda: hist(D=8), "D < P"), (lambda: hist(n_max=0), "n_max"), (lambda: hist(h=None), "null pointer"),
                       (lambda: hist(wins=None), "null pointer"), (lambda: hist(n_win=5), "windows"), (lambda: hist(bins=0), "bins"),
                       (lambda: hist(n_win=4, bins=2048), "LDS words")):
        assert call() == -1
        assert what in lib.cdll.vm_last_error().decode(), (what, lib.cdll.vm_last_error())
