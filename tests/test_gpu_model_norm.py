"""-m gpu checks of model-trial score normalisation (csrc/enrol_norm.hip, voicemap_amd/enrolment.py model_score_norm / norm=): the virtual
leave-one-out models bit for bit, the three statistics in two stages against vm_[plda_]speaker_identify's own score matrix (selection
exact, mu / sigma within one fp32 ulp of float64, rsig exact), the normalised histograms as integers against numpy's binning of
normalise_trials_numpy, the exact metrics against the sort-based definition, determinism, bad arguments, and the planted end-to-end
claim -- on one rank, on two, and through the experiment script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import model_norm_cases as MC
from tests.gpu_util import L, p, stream
from voicemap_amd import enrolment as EN
from voicemap_amd import plda as PL
from voicemap_amd import verification as V
from voicemap_amd._lib import VoicemapHipError
from voicemap_amd.retrieval import EmbeddingCache

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
GUARD = 64
F_GUARD, I_GUARD, H_GUARD, D_GUARD = np.float32(-7.75e30), np.int32(-123456789), np.int64(-0x0123456789ABCDEF), np.float64(-3.25e200)
SIZES = (1, 63, 64, 65, 130)
MS = [(1, 1), (63, 64), (64, 65), (65, 63), (130, 130), (1, 130), (130, 1)]


def cuda(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    """Bit for bit; NaN matches NaN (numpy's 0 / 0 carries the sign bit, the chip's does not)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


class Guarded:
    """A device buffer of ``n`` elements between GUARD sentinel words on either side."""

    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.t = torch.full((GUARD + n + GUARD,), fill.item(), dtype=dtype, device="cuda")

    def ptr(self):
        return self.t.data_ptr() + GUARD * self.t.element_size()

    def get(self, what="a buffer"):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == self.fill).all() and (a[GUARD + self.n:] == self.fill).all(), "words around %s were written" % what
        return a[GUARD:GUARD + self.n].copy()


def _cache(emb, codes):
    return EmbeddingCache(cuda(np.asarray(emb, np.float32)), np.asarray(codes))


# ---- 1. vm_speaker_loo_sums ----------------------------------------------------------------------------------------------------------------
def _loo_case(M, E, seed):
    """M integer rows: speakers of 1, 2, 3, 4, ... rows in turn, the last rows labelled -1 and past S."""
    sizes, left = [], M
    while left > 0:
        sizes.append(min(left, 1 + len(sizes) % 5))
        left -= sizes[-1]
    emb, label = MC.lattice(sizes, E, seed)
    emb[(emb == 0).all(1)] = 1.0                            # no zero row: its unit vector is 0 / 0
    ql = label.copy()
    if M > 3:
        ql[-1], ql[-2] = -1, len(sizes) + 4
    return emb, label, ql, len(sizes)


@pytest.mark.parametrize("kind", MC.KINDS)
def test_loo_sums_equal_the_twin_bit_for_bit_and_score_like_leave_one_out(kind):
    """Grid rows (integers: every |e| is a correctly rounded root of an exact sum, every c a correctly rounded quotient), the device's
    own sums: one float64 subtraction per component, so the twin's bits; and vm_speaker_identify against the virtual models gives, on
    the diagonal, the bits of true_score of the leave-one-out call."""
    for E in (1, 31, 32, 33, 50, 64, 256):
        for M in SIZES if E in (50, 64) else (65,):
            emb, label, ql, S = _loo_case(M, E, 100 * E + M)
            e, lab, qld = cuda(emb), cuda(label), cuda(ql)
            sums, msum, count = EN.speaker_sums(e, lab, S, kind)
            vs, vm, vc = EN.speaker_loo_sums(e, qld, sums, msum, count, kind)
            ws, wm, wc = EN.loo_sums_numpy(emb, ql, sums.cpu().numpy(), msum.cpu().numpy(), count.cpu().numpy(), kind)
            assert _same(vs.cpu().numpy(), ws) and _same(vm.cpu().numpy(), wm) and np.array_equal(vc.cpu().numpy(), wc), (E, M)
            cnt = count.cpu().numpy()
            gone = (ql < 0) | (ql >= S) | (cnt[np.clip(ql, 0, S - 1)] <= 1)
            assert np.all(wc[gone] == 0) and not ws[gone].any() and np.all(wc[~gone] == cnt[ql[~gone]] - 1)
            loo = EN.speaker_identify(e, qld, sums, msum, count, kind, True)
            virt = EN.speaker_identify(e, cuda(np.full(M, -1, np.int32)), vs, vm, vc, kind, False, return_scores=True)
            diag = virt["scores"].cpu().numpy()[np.arange(M), np.arange(M)]
            assert _same(diag, loo["true_score"].cpu().numpy()), (E, M)
            assert np.isnan(diag[gone]).all() and (kind != "euclidean" or not np.isnan(diag[~gone]).any())


def _tolerance(rows, q, sc, kind, n, p_min):
    """tests/test_gpu_enrolment.py's rule: one fp32 ulp of fp32(twin) plus a floor for the float64 rounding of the sums, g = 8 (n + E) u:
    euclidean g 2 R, dot_product g R^2, cosine 2 g / p_min (R: the largest row norm; p_min: the smallest model norm)."""
    g = 8.0 * (n + rows.shape[1]) * U
    R = float(np.linalg.norm(np.concatenate([rows, q]).astype(np.float64), axis=1).max())
    floor = {"euclidean": g * 2 * R, "dot_product": g * R * R, "cosine": 2 * g / p_min}[kind]
    with np.errstate(invalid="ignore"):
        return np.spacing(np.abs(sc.astype(np.float32))).astype(np.float64) + floor


@pytest.mark.parametrize("kind", MC.KINDS)
def test_scores_against_the_virtual_models_lie_within_one_ulp_of_the_twin(kind):
    emb, label = MC.random_corpus(400, 12, 50, 7)
    coh, _ = MC.random_corpus(130, 5, 50, 8)
    e, lab = cuda(emb), cuda(label)
    sums, msum, count = EN.speaker_sums(e, lab, 12, kind)
    vs, vm, vc = EN.speaker_loo_sums(e, lab, sums, msum, count, kind)
    got = EN.speaker_identify(cuda(coh), cuda(np.full(len(coh), -1, np.int32)), vs, vm, vc, kind, False, return_scores=True)["scores"].cpu().numpy()
    s64, m64, c64 = EN.speaker_sums_numpy(emb, label, 12, kind)
    ws, wm, wc = EN.loo_sums_numpy(emb, label, s64, m64, c64, kind)
    k = MC.KIND_ID[kind]
    with np.errstate(divide="ignore", invalid="ignore"):
        pm = ws / wc[:, None]
        ref = _twin64(coh, ws, wm, wc, k)
        p_min = float(np.nanmin(np.where(wc > 0, np.linalg.norm(pm, axis=1), np.nan)))
    tol = _tolerance(emb, coh, ref, kind, int(c64.max()), p_min)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref[:, wc == 0]).all() and (wc == 0).sum() == 2
    ok = ~np.isnan(ref)
    assert np.all(np.abs(got.astype(np.float64) - ref)[ok] <= tol[ok])


def _twin64(q, sums, msum, count, kind):
    """float64 scores of rows against models given by their sums (the twin's formulas, not rounded)."""
    q = q.astype(np.float64)
    n = count.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = sums / n[:, None]
        if kind == 2:
            P = (msum / n)[:, None] * P
        if kind == 0:
            sc = np.sqrt(((q[:, None, :] - P[None]) ** 2).sum(-1))
        elif kind == 1:
            sc = 1.0 - (q @ P.T) / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(P, axis=1)[None, :])
        else:
            sc = -(q @ P.T)
    sc[:, count <= 0] = np.nan
    return sc


# ---- 2. the statistics, in two stages ------------------------------------------------------------------------------------------------------
def _ulp_close(got, ref64):
    """|got - fp32(ref64)| <= 1 fp32 ulp at every finite entry; NaN where the reference is NaN (tests/test_gpu_score_norm.py)."""
    ref = ref64.astype(np.float32)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    sp = np.spacing(np.abs(ref[~nan])).astype(np.float64)
    assert np.all(np.abs(got[~nan].astype(np.float64) - ref64[~nan]) <= sp)


def _check_lines(s, st, K):
    """The device statistics ``st`` of the lines (rows) of the fp32 matrix ``s``."""
    got = {k: v.cpu().numpy() for k, v in st.items()}
    idx, c = V.cohort_select_numpy(s, K)
    assert np.array_equal(got["count"], c)
    assert "topk_idx" not in got or np.array_equal(got["topk_idx"], idx)
    m64, s64 = np.full(len(s), np.nan), np.full(len(s), np.nan)
    for m in range(len(s)):
        if c[m]:
            v = s[m, idx[m, :c[m]]].astype(np.float64)
            m64[m] = v.mean()
            s64[m] = np.sqrt(((v - v.mean()) ** 2).mean())
    _ulp_close(got["mu"], m64)
    _ulp_close(got["sigma"], s64)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal((1.0 / got["sigma"].astype(np.float64)).astype(np.float32), got["rsig"], equal_nan=True)
    return got


def _ks(n_avail):
    return sorted({1, max(1, n_avail // 2), n_avail, n_avail + 5})


def _stats_both_sides(q, models, kind, tables=None):
    """Both sides at every K of ``_ks`` against the identify matrix of the same operands; returns that matrix."""
    sums, msum, count = models
    none = cuda(np.full(len(q), -1, np.int32))
    if tables is None:
        s = EN.speaker_identify(q, none, sums, msum, count, kind, False, return_scores=True)["scores"].cpu().numpy()
    else:
        s = EN.plda_speaker_identify(q, none, sums, count, tables, False, return_scores=True)["scores"].cpu().numpy()
    for side, mat in ((0, s), (1, np.ascontiguousarray(s.T))):
        avail = int((~np.isnan(mat)).sum(1).max())
        for K in _ks(max(avail, 1)):
            st = EN.speaker_cohort_stats(q, sums, msum, count, kind, side, K, tables=tables, return_topk=True)
            _check_lines(mat, st, K)
    return s


@pytest.mark.parametrize("kind", MC.KINDS)
def test_statistics_equal_numpy_on_the_identify_matrix(kind):
    """Random rows.  (M, S) around the 64 x 64 tile at E = 50 and 64; E around the 32-component chunk, and 256, at (65, 130)."""
    for E, shapes in ((50, MS), (64, MS), (1, [(65, 130)]), (31, [(65, 130)]), (32, [(65, 130)]), (33, [(65, 130)]), (256, [(65, 130)])):
        for M, S in shapes:
            emb, label = MC.random_corpus(max(3 * S, 8), S, E, 1000 * E + 10 * M + S)
            if S > 2:
                label[label == S - 1] = -1                 # the last model has no rows: NaN against every row
            rows, _ = MC.random_corpus(M, 3, E, 7 + M + S)
            if kind == "cosine" and M > 2:
                rows[1] = 0.0                               # a zero row: NaN against every model under cosine
            models = EN.speaker_sums(cuda(emb), cuda(label), S, kind)
            _stats_both_sides(cuda(rows), models, kind)


@pytest.mark.parametrize("D", (1, 15, 16, 17, 33, 255))
def test_plda_statistics_equal_numpy_on_the_identify_matrix(D):
    rng = np.random.default_rng(D)
    tables = MC.plda_grid_tables(rng, D)
    tdev = EN.plda_tables_to(tables, "cuda")
    for M, S in [(65, 130), (64, 63), (1, 1), (130, 65)] if D in (16, 17) else [(65, 130)]:
        emb, label = MC.plda_grid_rows(rng, MC.plda_sizes(S), D)
        rows, _ = MC.plda_grid_rows(rng, [M], D)
        rows[:, :D] += rng.normal(0, 0.3, (M, D)).astype(np.float32)   # off the grid: no planted ties
        if M > 2:
            rows[2, :D] = np.nan
        sums, msum, count = EN.speaker_sums(cuda(emb), cuda(label), S, "euclidean") if len(emb) else (
            torch.zeros(S, emb.shape[1], dtype=torch.float64, device="cuda"), torch.zeros(S, dtype=torch.float64, device="cuda"),
            torch.zeros(S, dtype=torch.int32, device="cuda"))
        s = _stats_both_sides(cuda(rows), (sums, msum, count), "euclidean", tables=tdev)
        sizes = np.asarray(MC.plda_sizes(S))
        assert np.isnan(s[:, (sizes < 1) | (sizes > MC.N_MAX)]).all()


def test_lattice_case_massive_ties_an_all_nan_line_and_a_zero_sigma_line():
    """Integer rows in equal pairs against dyadic models: every score comes at least twice, so every odd K cuts a tie by index; a model
    without rows (side 1) and a NaN row (side 0) give all-NaN lines: count 0 and NaN statistics; K = 1 and K = 2 give sigma = 0 and
    rsig = +inf."""
    sizes = [1, 2, 4, 0, 8, 2, 4, 4] * 9
    emb, label = MC.lattice(sizes, 6, 5)
    rows = MC.lattice_rows(130, 6, 6, dup=True)
    rows[6:8] = np.nan
    S = len(sizes)
    models = EN.speaker_sums(cuda(emb), cuda(label), S, "euclidean")
    q = cuda(rows)
    s = EN.speaker_identify(q, cuda(np.full(130, -1, np.int32)), *models, "euclidean", False, return_scores=True)["scores"].cpu().numpy()
    for side, mat in ((0, s), (1, np.ascontiguousarray(s.T))):
        for K in (1, 2, 3, 17, 64, 65, 200):
            got = _check_lines(mat, EN.speaker_cohort_stats(q, *models, "euclidean", side, K, return_topk=True), K)
            dead = np.isnan(mat).all(1)
            assert dead.sum() == (9 if side else 2) and np.all(got["count"][dead] == 0) and np.isnan(got["rsig"][dead]).all()
            assert np.all(got["topk_idx"][dead] == -1)
            if K == 1 or (K == 2 and side == 1):   # down a column the two smallest are an equal pair of rows
                assert np.all(got["sigma"][~dead] == 0) and np.isposinf(got["rsig"][~dead]).all()
    keys = V.score_keys(s.T[0])
    order = np.lexsort((np.arange(130), keys))
    assert keys[order[2]] == keys[order[3]] or keys[order[0]] == keys[order[1]]   # the ties are there


@pytest.mark.parametrize("side", [0, 1])
def test_long_selection_past_the_lds_capacity(side):
    """33 000 entries per line against 3 counterparts: the keys no longer fit LDS and every radix pass re-reads the tile."""
    r = np.random.default_rng(9)
    n, E = 33000, 8
    if side == 0:   # 3 rows against 33 000 one-row models
        emb, label = r.normal(0, 1, (n, E)).astype(np.float32), np.arange(n, dtype=np.int32)
        rows = r.normal(0, 1, (3, E)).astype(np.float32)
    else:           # 33 000 rows against 3 models
        emb, label = r.normal(0, 1, (30, E)).astype(np.float32), np.repeat(np.arange(3), 10).astype(np.int32)
        rows = r.normal(0, 1, (n, E)).astype(np.float32)
        rows[5] = np.nan
    models = EN.speaker_sums(cuda(emb), cuda(label), int(label.max()) + 1, "euclidean")
    q = cuda(rows)
    s = EN.speaker_identify(q, cuda(np.full(len(rows), -1, np.int32)), *models, "euclidean", False, return_scores=True)["scores"].cpu().numpy()
    mat = np.ascontiguousarray(s.T) if side else s
    assert mat.shape == (3, n)
    for K in (300, n):   # (the index list of all 33 000 is quadratic work: the statistics alone there)
        _check_lines(mat, EN.speaker_cohort_stats(q, *models, "euclidean", side, K, return_topk=K == 300), K)


# ---- 3. the normalised histograms ----------------------------------------------------------------------------------------------------------
def _planted_stats(r, M, S, loo):
    """Planted fp32 statistics, independent of section 2: negative and positive mu, +inf rsig, NaN mu; under leave-one-out an own pair
    that differs from every model's."""
    st = {"mu_q": r.normal(0, 2, M).astype(np.float32), "rsig_q": r.uniform(0.2, 4, M).astype(np.float32),
          "mu_s": r.normal(0, 2, S).astype(np.float32), "rsig_s": r.uniform(0.2, 4, S).astype(np.float32)}
    st["mu_q"][0] = -abs(st["mu_q"][0]) - 1
    if M > 4:
        st["rsig_q"][3], st["mu_q"][4] = np.inf, np.nan
    if S > 3:
        st["rsig_s"][1], st["mu_s"][2] = np.inf, np.nan
    if loo:
        st["mu_own"] = (r.normal(0, 2, M) + 40).astype(np.float32)
        st["rsig_own"] = r.uniform(0.2, 4, M).astype(np.float32)
        if M > 6:
            st["rsig_own"][5], st["mu_own"][6] = np.inf, np.nan
    return st


def _trial_mask(count, q_label, loo, n_max=None):
    c = np.asarray(count).astype(np.int64)
    n = np.tile(c, (len(q_label), 1))
    if loo:
        n = n - (q_label[:, None] == np.arange(len(c))[None, :])
    return (n > 0) if n_max is None else (n >= 1) & (n <= n_max)


def _hist_checks(q, ql, models, kind, loo, st, s, trial, tables=None, coarse_only=False):
    """The device histogram of the normalised scores against numpy's binning of normalise_trials_numpy(device matrix, planted arrays):
    a coarse 4096-bin window and four zoomed 1024-bin windows, counts exactly equal."""
    sums, msum, count = models
    S = s.shape[1]
    target = ql[:, None] == np.arange(S)[None, :]
    sn = EN.normalise_trials_numpy(s, ql, st["mu_q"], st["rsig_q"], st["mu_s"], st["rsig_s"], st.get("mu_own"), st.get("rsig_own"))
    sv, tv = sn[trial], target[trial]
    stats = [cuda(st[k]) if k in st else None for k in ("mu_q", "rsig_q", "mu_s", "rsig_s", "mu_own", "rsig_own")]
    f = sv[np.isfinite(sv)]
    lo, hi = (float(f.min()), float(f.max())) if len(f) else (-1.0, 1.0)
    one = [V.pass1_window(lo, 0.5 * (lo + hi) if hi > lo else lo + 1.0)]
    call = lambda wins, bins: EN.speaker_trial_hist_norm(cuda(q), cuda(ql), sums, msum, count, kind, loo, wins, bins, stats,
                                                         tables=tables).cpu().numpy()
    h = call(one, 4096)
    assert np.array_equal(h, V.bin_scores(sv, tv, one, 4096))
    assert h.sum() == trial.sum()
    if coarse_only:
        return h, one
    b = int(np.argmax(h[0, 0, :4096] + h[0, 1, :4096]))
    k0, sh0 = one[0]
    med = float(np.median(f)) if len(f) else 0.0
    four = [(k0 + (b << sh0), max(0, sh0 - 10)), (V.key_of(med), 0), (V.key_of(0.5 * (lo + hi)), 31), (0, 22)]
    assert np.array_equal(call(four, 1024), V.bin_scores(sv, tv, four, 1024))
    return h, one


@pytest.mark.parametrize("loo", [True, False])
@pytest.mark.parametrize("kind", MC.KINDS)
def test_normalised_histogram_equals_numpy_binning_of_the_normalised_device_matrix(kind, loo):
    r = np.random.default_rng(17)
    for E, N, S in ((50, 130, 65), (64, 64, 5), (33, 63, 64), (1, 65, 3), (256, 65, 130)):
        emb, label = MC.random_corpus(N, S, E, 30 + E)
        if kind == "cosine":
            emb[np.flatnonzero(label == -1)[:1]] = 0.0       # an un-enrolled zero row: NaN against every model
        e, lab = cuda(emb), cuda(label)
        models = EN.speaker_sums(e, lab, S, kind)
        s = EN.speaker_identify(e, lab, *models, kind, loo, return_scores=True)["scores"].cpu().numpy()
        trial = _trial_mask(models[2].cpu().numpy(), label, loo)
        st = _planted_stats(r, N, S, loo)
        h, one = _hist_checks(emb, label, models, kind, loo, st, s, trial)
        assert h[0, :, -1].sum() > 0                        # the NaN slot is used: NaN mu, or inf - inf
        if loo:   # the own cells really took the own pair: with the model's pair in their place numpy's target counts are others
            sn2 = EN.normalise_trials_numpy(s, label, st["mu_q"], st["rsig_q"], st["mu_s"], st["rsig_s"])
            tgt = label[:, None] == np.arange(S)[None, :]
            assert not np.array_equal(V.bin_scores(sn2[trial], tgt[trial], one, 4096)[0, 0], h[0, 0])


@pytest.mark.parametrize("loo", [True, False])
def test_plda_normalised_histogram_equals_numpy_binning(loo):
    r = np.random.default_rng(23)
    for D, S in ((15, 65), (16, 130), (17, 64), (33, 10), (255, 10), (1, 3)):
        tables = MC.plda_grid_tables(r, D)
        tdev = EN.plda_tables_to(tables, "cuda")
        emb, label = MC.plda_grid_rows(r, MC.plda_sizes(S), D)
        extra, _ = MC.plda_grid_rows(r, [3], D)
        q, ql = np.concatenate([emb, extra]), np.concatenate([label, [-1, S, 0]]).astype(np.int32)
        sums, msum, count = EN.speaker_sums(cuda(emb), cuda(label), S, "euclidean")
        s = EN.plda_speaker_identify(cuda(q), cuda(ql), sums, count, tdev, loo, return_scores=True)["scores"].cpu().numpy()
        trial = _trial_mask(count.cpu().numpy(), ql, loo, MC.N_MAX)
        assert np.array_equal(~np.isnan(s), trial)
        _hist_checks(q, ql, (sums, msum, count), "euclidean", loo, _planted_stats(r, len(q), S, loo), s, trial, tables=tdev)


def test_normalised_histogram_over_several_splits_with_an_empty_trailing_one():
    """M = 8 256 rows (129 row tiles) x S = 1 088 models (17 model tiles): 16 splits of 2 tiles, of which the last seven hold none."""
    r = np.random.default_rng(29)
    M, S, E = 8256, 1088, 8
    lab = r.integers(0, S, M).astype(np.int32)
    lab[:S] = np.arange(S)
    emb = (r.normal(0, 1, (S, E))[lab] + r.normal(0, 0.7, (M, E))).astype(np.float32)
    e, ld = cuda(emb), cuda(lab)
    models = EN.speaker_sums(e, ld, S, "euclidean")
    s = EN.speaker_identify(e, ld, *models, "euclidean", True, return_scores=True)["scores"].cpu().numpy()
    trial = _trial_mask(models[2].cpu().numpy(), lab, True)
    _hist_checks(emb, lab, models, "euclidean", True, _planted_stats(r, M, S, True), s, trial, coarse_only=True)


# ---- 4. model_trial_metrics(norm=) ---------------------------------------------------------------------------------------------------------
def _assert_metrics_equal(got, ref):
    for k in ("eer", "eer_threshold", "far_at_eer", "frr_at_eer", "best_balanced_accuracy", "best_threshold", "n_target", "n_nontarget",
              "n_nan"):
        assert got[k] == ref[k], (k, got[k], ref[k])


def _norm_arrays(norm):
    f = lambda t: None if t is None else t.cpu().numpy()
    return f(norm.mu_q), f(norm.rsig_q), f(norm.mu_s), f(norm.rsig_s), f(norm.mu_own), f(norm.rsig_own)


@pytest.mark.parametrize("kind", MC.KINDS + ["plda"])
def test_model_trial_metrics_with_norm_equal_the_sorted_definition(kind):
    r = np.random.default_rng(31)
    S, E = 20, 32
    emb, label = MC.random_corpus(400, S, E, 33, noise=1.5)
    label = np.where(label < 0, 5, label)
    coh, cl = MC.random_corpus(260, 13, E, 34, noise=1.5)
    cl = np.where(cl < 0, 3, cl)
    cache, cohort = _cache(emb, label * 7 + 100), _cache(coh, cl)
    model = None
    if kind == "plda":
        model = PL.fit_plda(_cache(*[x for x in _train(E)]))
        cache, cohort = model.project(cache), model.project(cohort)
    for loo in (True, False):
        models = EN.enrol(cache, plda=model) if model is not None else EN.enrol(cache, kind)
        for top_k in (None, 40):
            norm = EN.model_score_norm(models, cache, cohort, top_k=top_k, leave_one_out=loo)
            assert norm.leave_one_out is loo and norm.cohort_rows == 260 and norm.cohort_models == 13 and (norm.mu_own is not None) == loo
            ql = cuda(label)
            if model is not None:
                s = EN.plda_speaker_identify(cache.emb, ql, models.sums, models.count, models.tables, loo, return_scores=True)["scores"]
            else:
                s = EN.speaker_identify(cache.emb, ql, models.sums, models.msum, models.count, kind, loo, return_scores=True)["scores"]
            s = s.cpu().numpy()
            trial = _trial_mask(models.count.cpu().numpy(), label, loo, models.n_max)
            target = label[:, None] == np.arange(S)[None, :]
            sn = EN.normalise_trials_numpy(s, label, *_norm_arrays(norm))
            m = EN.model_trial_metrics(models, cache, leave_one_out=loo, norm=norm)
            _assert_metrics_equal(m, V.sorted_metrics(sn[trial], target[trial]))
            at = EN.model_trial_accuracy_at_threshold(models, cache, m["best_threshold"], leave_one_out=loo, norm=norm)
            assert at["balanced_accuracy"] == m["best_balanced_accuracy"]
            if loo:   # the one-file speaker has no own model: NaN own statistics, and its own cell is no trial
                one = np.flatnonzero(label == 0)
                assert np.isnan(norm.mu_own.cpu().numpy()[one]).all() and not trial[one, 0].any()
        with pytest.raises(ValueError, match="leave_one_out"):
            EN.model_trial_metrics(models, cache, leave_one_out=not loo, norm=norm)
    with pytest.raises(ValueError, match="cohort must be"):
        EN.model_score_norm(models, cache, cache)
    with pytest.raises(ValueError, match="top_k"):
        EN.model_score_norm(models, cache, cohort, top_k=0)


def _train(E):
    emb, label = MC.random_corpus(600, 30, E, 35, noise=1.5)
    return emb, np.where(label < 0, 1, label)


# ---- 5. byte identity ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes():
    emb, label = MC.random_corpus(700, 40, 50, 41)
    coh, _ = MC.random_corpus(300, 5, 50, 42)
    r = np.random.default_rng(43)
    st = _planted_stats(r, 700, 40, True)
    stats = [cuda(st[k]) for k in ("mu_q", "rsig_q", "mu_s", "rsig_s", "mu_own", "rsig_own")]
    for kind in MC.KINDS:
        runs = []
        for _ in range(2):
            e, lab, c = cuda(emb), cuda(label), cuda(coh)
            models = EN.speaker_sums(e, lab, 40, kind)
            virt = EN.speaker_loo_sums(e, lab, *models, kind)
            out = [t.cpu().numpy().tobytes() for t in virt]
            for side in (0, 1):
                sd = EN.speaker_cohort_stats(c, *models, kind, side, 37, return_topk=True)
                out += [sd[k].cpu().numpy().tobytes() for k in sorted(sd)]
            so = EN.speaker_cohort_stats(c, *virt, kind, 1, 37)
            out += [so[k].cpu().numpy().tobytes() for k in sorted(so)]
            out.append(EN.speaker_trial_hist_norm(e, lab, *models, kind, True, [V.pass1_window(-20.0, 20.0)], 4096, stats).cpu().numpy().tobytes())
            runs.append(out)
        assert runs[0] == runs[1], kind


# ---- 6. bad arguments ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_errors_and_leave_the_outputs_untouched():
    rng = np.random.default_rng(3)
    D, M, S = 5, 9, 4
    tables = EN.plda_tables_to(MC.plda_grid_tables(rng, D), "cuda")
    proj, label = MC.plda_grid_rows(rng, [3, 2, 1, 3], D)
    M = len(proj)
    qd, ld = cuda(proj), cuda(label)
    sums, msum, count = EN.speaker_sums(qd, ld, S, "euclidean")
    n = max(M, S)
    fl = [Guarded(n, torch.float32, F_GUARD) for _ in range(3)]
    cnt, topk = Guarded(n, torch.int32, I_GUARD), Guarded(n * 3, torch.int32, I_GUARD)
    vs, vm, vc = Guarded(M * 8, torch.float64, D_GUARD), Guarded(M, torch.float64, D_GUARD), Guarded(M, torch.int32, I_GUARD)
    hist = Guarded(4 * 2 * 1027, torch.int64, H_GUARD)
    ws = Guarded(1 << 16, torch.int64, H_GUARD)
    stat = [cuda(np.ones(n, np.float32)) for _ in range(6)]
    win = np.array([0, 22, 0, 22, 0, 22, 0, 22], dtype=np.int64)
    good = dict(q=p(qd), ql=p(ld), M=M, E=8, D=D, sums=p(sums), msum=p(msum), count=p(count), S=S, A=p(tables["A"]), beta=p(tables["beta"]),
                C=p(tables["C"]), G=p(tables["G"]), n_max=MC.N_MAX, kind=0, side=0, K=3, mu=fl[0].ptr(), sigma=fl[1].ptr(), rsig=fl[2].ptr(),
                cnt=cnt.ptr(), ws=ws.ptr(), loo=1, wins=win.ctypes.data, n_win=1, bins=16, hist=hist.ptr(), mu_q=p(stat[0]), rsig_q=p(stat[1]),
                mu_s=p(stat[2]), rsig_s=p(stat[3]), mu_own=p(stat[4]), rsig_own=p(stat[5]), vs=vs.ptr())

    def call(which, **bad):
        a = dict(good, **bad)
        ptab = (a["A"], a["beta"], a["C"], a["G"], a["n_max"])
        stats = (a["side"], a["K"], a["mu"], a["sigma"], a["rsig"], a["cnt"], topk.ptr(), a["ws"], stream())
        hn = (a["loo"], a["wins"], a["n_win"], a["bins"], a["mu_q"], a["rsig_q"], a["mu_s"], a["rsig_s"], a["mu_own"], a["rsig_own"], a["hist"],
              a["ws"], stream())
        if which == "loo":
            L().call("vm_speaker_loo_sums", a["q"], a["ql"], a["M"], a["E"], a["sums"], a["msum"], a["count"], a["S"], a["kind"], a["vs"],
                     vm.ptr(), vc.ptr(), a["ws"], stream())
        elif which == "stats":
            L().call("vm_speaker_cohort_stats", a["q"], a["M"], a["E"], a["sums"], a["msum"], a["count"], a["S"], a["kind"], *stats)
        elif which == "plda_stats":
            L().call("vm_plda_speaker_cohort_stats", a["q"], a["M"], a["E"], a["D"], a["sums"], a["count"], a["S"], *ptab, *stats)
        elif which == "hist":
            L().call("vm_speaker_trial_hist_norm", a["q"], a["ql"], a["M"], a["E"], a["sums"], a["msum"], a["count"], a["S"], a["kind"], *hn)
        else:
            L().call("vm_plda_speaker_trial_hist_norm", a["q"], a["ql"], a["M"], a["E"], a["D"], a["sums"], a["count"], a["S"], *ptab, *hn)

    null = "null pointer"
    cases = {
        "loo": [(dict(q=None), null), (dict(ql=None), null), (dict(vs=None), null), (dict(ws=None), null), (dict(kind=3), "unknown kind"),
                (dict(E=0), "E must be"), (dict(S=0), "bad sizes")],
        "stats": [(dict(q=None), null), (dict(msum=None), null), (dict(mu=None), null), (dict(cnt=None), null), (dict(ws=None), null),
                  (dict(K=0), "K must be"), (dict(side=2), "side must be"), (dict(side=-1), "side must be"), (dict(kind=6), "unknown kind"),
                  (dict(q=p(qd) + 4), "16-byte")],
        "plda_stats": [(dict(G=None), null), (dict(rsig=None), null), (dict(K=0), "K must be"), (dict(side=2), "side must be"),
                       (dict(D=8), "D < P"), (dict(n_max=0), "n_max")],
        "hist": [(dict(mu_q=None), null), (dict(rsig_s=None), null), (dict(hist=None), null), (dict(mu_own=None), "go together"),
                 (dict(rsig_own=None), "go together"), (dict(loo=0), "must be NULL without leave_one_out"),
                 (dict(mu_own=None, rsig_own=None), "needs mu_own"), (dict(n_win=4, bins=1025), "LDS words"), (dict(n_win=5), "windows")],
        "plda_hist": [(dict(rsig_q=None), null), (dict(mu_own=None), "go together"), (dict(loo=0), "must be NULL without leave_one_out"),
                      (dict(n_win=4, bins=1025), "LDS words"), (dict(beta=None), null)],
    }
    for which, lst in cases.items():
        for bad, msg in lst:
            with pytest.raises(VoicemapHipError, match=r"failed \(-1\).*" + msg):
                call(which, **bad)
    torch.cuda.synchronize()
    for g_, fill in [(x, F_GUARD) for x in fl] + [(cnt, I_GUARD), (topk, I_GUARD), (vs, D_GUARD), (vm, D_GUARD), (vc, I_GUARD), (hist, H_GUARD),
                                                  (ws, H_GUARD)]:
        assert (g_.get() == fill).all()
    hist.t[GUARD:GUARD + 38] = 0
    for which in cases:                  # ... and the same arguments without a fault run
        call(which)
    torch.cuda.synchronize()
    assert (vc.get("out_count") != I_GUARD).all() and (cnt.get("count")[:M] != I_GUARD).all()
    cn = count.cpu().numpy()              # both histogram calls accumulated their trials
    assert hist.get("hist")[:38].sum() == int(_trial_mask(cn, label, True).sum() + _trial_mask(cn, label, True, MC.N_MAX).sum())
    call("stats", M=0)                   # M == 0: no launch, nothing written
    call("hist", M=0)
    torch.cuda.synchronize()
    for x in fl + [ws, topk]:
        x.get()


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------------------
def _planted_caches():
    (emb, spk), (test, tspk), (coh, cspk) = MC.planted()
    return _cache(emb, spk), _cache(test, tspk), _cache(coh, cspk)


def test_as_norm_lowers_the_eer_of_the_planted_corpus_on_the_device():
    """The plant of tests/test_model_norm_cpu.py through model_score_norm and model_trial_metrics: AS-norm strictly below raw, at the
    values the float64 twins give (raw 0.263889, AS-norm 0.222222; the device's fp32 scores differ from the twins' in the last place,
    which can move a trial across a threshold: within 0.01)."""
    from tests.test_model_norm_cpu import PLANTED_ASNORM_EER, PLANTED_RAW_EER
    enrolled, test, cohort = _planted_caches()
    models = EN.enrol(enrolled, "euclidean")
    raw = EN.model_trial_metrics(models, test)
    norm = EN.model_score_norm(models, test, cohort, top_k=20)
    asn = EN.model_trial_metrics(models, test, norm=norm)
    print("planted corpus on the device: raw EER %.6f, AS-norm EER %.6f" % (raw["eer"], asn["eer"]))
    assert norm.leave_one_out is False and norm.mu_own is None and norm.top_k == 20
    assert asn["eer"] < raw["eer"]
    assert abs(raw["eer"] - PLANTED_RAW_EER) < 0.01 and abs(asn["eer"] - PLANTED_ASNORM_EER) < 0.01
    assert asn["n_target"] == raw["n_target"] == test.n and asn["n_nontarget"] == raw["n_nontarget"]


_TWO_RANK = r"""
import json, sys
sys.path.insert(0, {root!r})
import numpy as np, torch
from voicemap_amd import parallel, enrolment as EN
from voicemap_amd.retrieval import EmbeddingCache
rank, world, _ = parallel.init_distributed(timeout_s=120)
torch.cuda.set_device(0)
r = np.random.default_rng(4)
spk = r.integers(0, 13, 1001)
emb = (r.normal(0, 1, (13, 32))[spk] + r.normal(0, 1.5, (1001, 32))).astype(np.float32)
cs = r.integers(0, 9, 301)
coh = (r.normal(0, 1, (9, 32))[cs] + r.normal(0, 1.5, (301, 32))).astype(np.float32)
cache, cohort = EmbeddingCache(torch.as_tensor(emb).cuda(), spk), EmbeddingCache(torch.as_tensor(coh).cuda(), cs)
models = EN.enrol(cache, "cosine")
norm = EN.model_score_norm(models, cache, cohort, top_k=50)
m = EN.model_trial_metrics(models, cache, norm=norm)
m.pop("roc")
stats = [t.cpu().numpy().view(np.uint32).tolist() for t in (norm.mu_q, norm.rsig_q, norm.mu_s, norm.rsig_s, norm.mu_own, norm.rsig_own)]
if rank == 0:
    print("RESULT " + json.dumps(dict(m, stats=stats)))
"""


def test_two_rank_gloo_run_gives_the_same_metrics(tmp_path):
    script = tmp_path / "two_rank.py"
    script.write_text(_TWO_RANK.format(root=ROOT))
    env = dict(os.environ, VOICEMAP_DIST_BACKEND="gloo", MASTER_PORT="29747")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", str(script)], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    two = json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    r = np.random.default_rng(4)
    spk = r.integers(0, 13, 1001)
    emb = (r.normal(0, 1, (13, 32))[spk] + r.normal(0, 1.5, (1001, 32))).astype(np.float32)
    cs = r.integers(0, 9, 301)
    coh = (r.normal(0, 1, (9, 32))[cs] + r.normal(0, 1.5, (301, 32))).astype(np.float32)
    cache, cohort = _cache(emb, spk), _cache(coh, cs)
    models = EN.enrol(cache, "cosine")
    norm = EN.model_score_norm(models, cache, cohort, top_k=50)
    one = EN.model_trial_metrics(models, cache, norm=norm)
    stats = two.pop("stats")
    for got, t in zip(stats, (norm.mu_q, norm.rsig_q, norm.mu_s, norm.rsig_s, norm.mu_own, norm.rsig_own)):
        assert got == t.cpu().numpy().view(np.uint32).tolist()
    for k, v in two.items():
        assert v == one[k] or (v != v and one[k] != one[k]), k


PARENT_KEYS = ["distance", "speakers", "per_speaker", "leave_one_out", "queries", "unranked", "rank1_accuracy", "rank5_accuracy",
               "mean_reciprocal_rank", "trial_eer", "trial_eer_threshold", "trial_best_balanced_accuracy", "trial_best_threshold",
               "target_trials", "nontarget_trials", "whole_utterance", "enrol_set", "test_set"]


def _script(*extra):
    out = subprocess.run([sys.executable, "-m", "experiments.speaker_identification", "--synthetic", "--n-seconds", "1", *extra], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def test_experiment_script_with_and_without_score_norm():
    """--score-norm as-norm --top-k 50 prints a parsable line whose trial fields equal a hand call of the API on the same seeded model
    and sets; without --score-norm the line has exactly the fields it had before the option existed, with the raw values."""
    from experiments import speaker_identification as SI
    from experiments._common import setup
    from experiments.verification_accuracy import cohort_subset
    from voicemap_amd import models as VM, retrieval
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    from voicemap_amd.utils import BatchPreProcessor, preprocess_instances
    row = _script("--score-norm", "as-norm", "--top-k", "50")
    plain = _script()
    assert list(plain) == PARENT_KEYS
    assert list(row) == PARENT_KEYS[:-2] + ["score_norm", "top_k", "cohort_size"] + PARENT_KEYS[-2:]
    assert (row["score_norm"], row["top_k"], row["cohort_size"]) == ("as-norm", 50, 160)
    for k in PARENT_KEYS:
        if not k.startswith("trial_"):
            assert row[k] == plain[k], k
    # the hand call: the script's own seeded model and generated sets
    setup()
    mk = lambda seed, name: SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=1.0, stochastic=False, seed=seed, subset=name)
    enrol_set = mk(1, "synthetic-enrol")                   # the script's order: the enrolled set, the model, the cohort
    enc = VM.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
    net = VM.build_siamese_net(enc, (16000 // 4, 1), distance_metric="uniform_euclidean")
    pre = BatchPreProcessor("siamese", preprocess_instances(4))
    ce = retrieval.embed_corpus(net, enrol_set, pre, "siamese")
    cc = retrieval.embed_corpus(net, cohort_subset(mk(3, "synthetic-cohort"), 5000), pre, "siamese")
    models = EN.enrol(ce, "euclidean")
    raw = EN.model_trial_metrics(models, ce)
    asn = EN.model_trial_metrics(models, ce, norm=EN.model_score_norm(models, ce, cc, top_k=50))
    for m, got in ((raw, plain), (asn, row)):
        assert (got["trial_eer"], got["trial_eer_threshold"], got["trial_best_balanced_accuracy"], got["trial_best_threshold"]) == (
            m["eer"], m["eer_threshold"], m["best_balanced_accuracy"], m["best_threshold"])
    assert row["trial_eer_threshold"] != plain["trial_eer_threshold"]
    assert SI._parser().parse_args([]).score_norm == "none"
