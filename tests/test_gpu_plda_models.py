"""-m gpu tests of multi-session PLDA speaker models: vm_plda_speaker_identify / vm_plda_speaker_trial_hist (csrc/plda_enrol.hip) and
``enrolment.enrol(plda=...)`` on top of them.

On grid inputs every intermediate of the stated chain is exact in float64 (the sizes are worked out at ``_grid_case``), so the fp32
score is the single rounding of a known number whatever the order: scores, true_score, rank and best_* are held to the bits of the numpy
twin (``plda.trial_scores_plda_numpy`` + ``enrolment.ranks_numpy``) and the histogram to ``verification.bin_scores`` of that matrix.
General rows are held to a bound that counts the roundings of the chain (``_counted_bound``).  Every output and the workspace sit
between guard words."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import plda_cases as PC
from tests.gpu_util import L, p, stream
from voicemap_amd import enrolment as EN
from voicemap_amd import plda as PL
from voicemap_amd import verification as V
from voicemap_amd._lib import VoicemapHipError
from voicemap_amd.retrieval import EmbeddingCache

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
N_MAX = 9
U = 2.0 ** -53
F_GUARD, I_GUARD, H_GUARD = np.float32(-7.75e30), np.int32(-123456789), np.int64(-0x0123456789ABCDEF)


def cuda(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Guarded:
    """A device buffer of ``n`` elements between GUARD sentinel words on either side."""

    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.t = torch.full((GUARD + n + GUARD,), fill.item(), dtype=dtype, device="cuda")

    def ptr(self):
        return self.t.data_ptr() + GUARD * self.t.element_size()

    def get(self, what):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == self.fill).all() and (a[GUARD + self.n:] == self.fill).all(), "words around %s were written" % what
        return a[GUARD:GUARD + self.n].copy()


def _tables_dev(tables):
    return EN.plda_tables_to(tables, "cuda")


def identify(q, q_label, sums, count, tables, loo, with_scores=True):
    """One guarded vm_plda_speaker_identify call: host rows / labels, device sums / count / tables -> dict of host arrays."""
    M, P = q.shape
    S, D, n_max = int(count.shape[0]), int(tables["G"].shape[0]), int(tables["C"].shape[0]) - 1
    qd, ld = cuda(q), cuda(q_label, torch.int32)
    out = {"scores": Guarded(M * S, torch.float32, F_GUARD), "true_score": Guarded(M, torch.float32, F_GUARD),
           "rank": Guarded(M, torch.int32, I_GUARD), "best_val": Guarded(M, torch.float32, F_GUARD), "best_idx": Guarded(M, torch.int32, I_GUARD)}
    nbytes = L().query("vm_plda_speaker_identify_workspace_bytes", M, D, S)
    ws = Guarded((nbytes + 7) // 8, torch.int64, H_GUARD)
    L().call("vm_plda_speaker_identify", p(qd), p(ld), M, P, D, p(sums), p(count), S, p(tables["A"]), p(tables["beta"]), p(tables["C"]),
             p(tables["G"]), n_max, int(loo), out["scores"].ptr() if with_scores else None, out["true_score"].ptr(), out["rank"].ptr(),
             out["best_val"].ptr(), out["best_idx"].ptr(), ws.ptr(), stream())
    torch.cuda.synchronize()
    ws.get("the workspace")
    res = {k: v.get(k) for k, v in out.items()}
    if not with_scores:
        assert (res.pop("scores") == F_GUARD).all()
    else:
        res["scores"] = res["scores"].reshape(M, S)
    return res


def trial_hist(q, q_label, sums, count, tables, loo, windows, bins, acc=None):
    """One guarded vm_plda_speaker_trial_hist call -> (n_windows, 2, bins + 3) int64, added to ``acc`` on the device side."""
    M, P = q.shape
    S, D, n_max = int(count.shape[0]), int(tables["G"].shape[0]), int(tables["C"].shape[0]) - 1
    n = len(windows) * 2 * (bins + 3)
    h = Guarded(n, torch.int64, H_GUARD)
    h.t[GUARD:GUARD + n] = 0 if acc is None else cuda(acc.reshape(-1))
    nbytes = L().query("vm_plda_speaker_trial_hist_workspace_bytes", M, D, S)
    ws = Guarded((nbytes + 7) // 8, torch.int64, H_GUARD)
    qd, ld = cuda(q), cuda(q_label, torch.int32)
    win = np.ascontiguousarray(np.asarray(windows, dtype=np.int64).reshape(-1, 2))
    L().call("vm_plda_speaker_trial_hist", p(qd), p(ld), M, P, D, p(sums), p(count), S, p(tables["A"]), p(tables["beta"]), p(tables["C"]),
             p(tables["G"]), n_max, int(loo), win.ctypes.data, len(windows), bins, h.ptr(), ws.ptr(), stream())
    torch.cuda.synchronize()
    ws.get("the workspace")
    return h.get("hist").reshape(len(windows), 2, bins + 3)


# ---- grid inputs: bit equality ---------------------------------------------------------------------------------------------------------
def _grid_tables(rng, D):
    """Dyadic tables that need not come from a psi: A in {1/4, 1/2, 1, 2}, beta in {1, 1/2, 1/4, 1/8}, G in {1/4, 1/2, 1, 2}, C a multiple
    of 1/16 in [-8, 8].  Row 0 holds a value that would show if it were read."""
    A = 2.0 ** rng.integers(-2, 2, (N_MAX + 1, D))
    beta = 2.0 ** -rng.integers(0, 4, (N_MAX + 1, D)).astype(np.float64)
    C = rng.integers(-128, 129, N_MAX + 1) / 16.0
    G = 2.0 ** rng.integers(-2, 2, D)
    A[0], beta[0], C[0] = 1e300, 1e300, 1e300
    return {"A": A, "beta": beta, "C": C, "G": G.astype(np.float64)}


def _grid_case(rng, M, S, D):
    """Enrolled rows, labels, query rows and query labels on the grid w = k / 8, |k| <= 16.
    Exactness (units of 2^-14): a sum of at most 10 rows is a multiple of 1/8 below 20; mu = beta Sigma a multiple of 2^-6 below 20;
    t = w - mu a multiple of 2^-6 below 22; u = A t a multiple of 2^-8 below 44; u t a multiple of 2^-14 below 968; 255 of them stay
    below 2^18: 32 significant bits.  G w^2 is a multiple of 2^-8 below 8 and C one of 2^-4 below 8.  So every partial sum in any order,
    with or without fma, is exact in float64, and the score is a float64 number rounded to fp32 once.
    Speakers: counts cycle through 3, 0, 1, N_MAX + 1, N_MAX, 2, 5, ...; the last speaker is a twin of the one before it (the same rows
    in another order: every foreign query ties between them and the lower index must win).  Queries: the enrolled rows first (their own
    labels: what leave-one-out means), then foreign rows labelled -1, S and S + 5, and one all-NaN row labelled with a real speaker."""
    P = PL.padded_width(D)
    cyc = [3, 0, 1, N_MAX + 1, N_MAX, 2, 5, 4, 1, 7]
    sizes = [cyc[s % len(cyc)] for s in range(S)]
    if S >= 2:
        sizes[-1] = sizes[-2] = 3 if sizes[-2] == 0 else sizes[-2]
    label = np.repeat(np.arange(S), sizes).astype(np.int32)
    N = len(label)
    proj = np.zeros((N, P), np.float32)
    proj[:, :D] = rng.integers(-16, 17, (N, D)) / 8.0
    proj[:, -1] = rng.normal(size=N)          # the row term h: never read by these entry points
    if S >= 2:
        proj[label == S - 1] = proj[label == S - 2][::-1]
    perm = rng.permutation(N)
    proj, label = proj[perm], label[perm]
    q = np.zeros((M, P), np.float32)
    q[:, :D] = rng.integers(-16, 17, (M, D)) / 8.0
    q[:, -1] = np.inf                          # ... not even when it is not finite
    ql = np.array([(-1, S, S + 5)[i % 3] for i in range(M)], dtype=np.int32)
    k = min(N, max(M - 4, M // 2)) if M > 1 else min(N, M)
    q[:k], ql[:k] = proj[:k], label[:k]
    if M >= 2:
        q[M - 1, :D], ql[M - 1] = np.nan, max(0, S - 3)
    return proj, label, q, ql, sizes


MS = [(M, S) for M in (1, 63, 64, 65, 130) for S in (1, 2, 63, 64, 65, 130)]


@pytest.mark.parametrize("D", (1, 3, 15, 16, 17, 31, 32, 33, 63, 64, 100, 255))
def test_grid_inputs_equal_the_twin_bit_for_bit(D):
    """Every (M, S) around the 64 x 64 tile, with and without leave-one-out, at component counts around the 16-component stage (and the
    32- and 64-component marks)."""
    rng = np.random.default_rng(7000 + D)
    tables = _grid_tables(rng, D)
    tdev = _tables_dev(tables)
    seen = {"tie": 0, "nan": 0, "non_trial": 0, "over": 0}
    for M, S in MS:
        proj, label, q, ql, sizes = _grid_case(rng, M, S, D)
        sums, _, count = EN.speaker_sums(cuda(proj), cuda(label), S, "euclidean")
        assert np.array_equal(count.cpu().numpy(), sizes)
        for loo in (False, True):
            sc, trial = PL.trial_scores_plda_numpy(proj, label, q, ql, tables, loo, S)
            s32 = sc.astype(np.float32)
            fin = sc[trial & ~np.isnan(sc)]
            assert not (fin * 2 ** 14 % 1).any() and (np.abs(fin) < 2 ** 19).all()   # the twin's numbers lie on the grid the docstring derives
            want = EN.ranks_numpy(sc, trial, ql)
            got = identify(q, ql, sums, count, tdev, loo)
            where = (D, M, S, loo)
            assert np.array_equal(np.isnan(got["scores"]), ~trial | np.isnan(sc)), where
            assert np.array_equal(bits(got["scores"])[trial], bits(s32)[trial]), where
            for k in ("rank", "best_idx"):
                assert np.array_equal(got[k], want[k]), (k,) + where
            for k in ("true_score", "best_val"):
                ok = ~np.isnan(want[k])
                assert np.array_equal(np.isnan(got[k]), ~ok) and np.array_equal(bits(got[k])[ok], bits(want[k])[ok]), (k,) + where
            # the speakers that must be non-trials, and the planted ties
            cnt = np.asarray(sizes)
            shared_ok = (cnt >= 1) & (cnt <= N_MAX)
            foreign = (ql < 0) | (ql >= S)
            assert np.array_equal(trial[foreign], np.tile(shared_ok, (foreign.sum(), 1))), where
            seen["non_trial"] += int((~shared_ok).sum())
            seen["over"] += int((cnt == N_MAX + 1).sum())
            if S >= 2 and foreign.any():
                fr = np.flatnonzero(foreign & ~np.isnan(q[:, 0]))
                assert np.array_equal(bits(got["scores"][fr, S - 2]), bits(got["scores"][fr, S - 1])) and not (got["best_idx"][fr] == S - 1).any(), where
                seen["tie"] += int((got["best_idx"][fr] == S - 2).sum())
            seen["nan"] += int(np.isnan(sc[trial]).sum())
            # the histogram of the same trials: one window over the finite scores, then four, then two row ranges accumulated
            sv, tv = s32[trial], (ql[:, None] == np.arange(S)[None, :])[trial]
            f = sv[np.isfinite(sv)]
            one = [V.pass1_window(float(f.min()), float(f.max()), 1024)] if len(f) else [(0, 22)]
            h = trial_hist(q, ql, sums, count, tdev, loo, one, 1024)
            assert np.array_equal(h, V.bin_scores(sv, tv, one, 1024)), where
            assert h.sum() == trial.sum() and h[0, :, -1].sum() == np.isnan(sv).sum()
            if (M, S) in ((130, 130), (65, 63), (63, 65)):
                four = [one[0], (V.key_of(float(np.median(f))), 0), (V.key_of(0.0), 31), (0, 22)]
                assert np.array_equal(trial_hist(q, ql, sums, count, tdev, loo, four, 1024), V.bin_scores(sv, tv, four, 1024)), where
                cut = M // 3 + 1
                acc = trial_hist(q[:cut], ql[:cut], sums, count, tdev, loo, one, 1024)
                acc = trial_hist(q[cut:], ql[cut:], sums, count, tdev, loo, one, 1024, acc=acc)
                assert np.array_equal(acc, h), where
    assert seen["tie"] > 0 and seen["nan"] > 0 and seen["non_trial"] > 0 and seen["over"] > 0, seen
    # scores == NULL: the other outputs are the same and nothing is written in its place
    lean = identify(q, ql, sums, count, tdev, True, with_scores=False)
    for k in ("rank", "best_idx"):
        assert np.array_equal(lean[k], got[k])


# ---- general rows: the counted bound -----------------------------------------------------------------------------------------------------
def _counted_bound(w, sums, count, q_label, tables, loo):
    """(reference (M, S), bound (M, S), trial) for device sums and general rows.  The reference is the stated formula on the float64
    inputs in extended precision (numpy.longdouble; where that is no wider than float64 the bound is doubled: the reference then
    carries the same roundings).  The bound counts the kernel's float64 roundings, u = 2^-53, to first order:
      mu = fl(beta Sigma): |d mu| <= u |mu|, and u |mu| more under leave-one-out, where Sigma = fl(sum - w) is rounded first;
      t = fl(w - mu): |dt| <= u |t| + 2 u |mu|;
      A t t, two roundings (the product A t and the fma's sum are counted below): |d term| <= A (2 |t| |dt|) + u A t^2
                                                                                            <= u (3 A t^2 + 4 A |t| |mu|);
      the D fma roundings of acc: at most u acc each (every term is >= 0, so a partial sum is at most acc): D u acc;
      the D fma roundings of g (G w^2 is exact inside the fma, the terms are >= 0): D u g;
      acc - g and the difference with C: u (acc + g) and u (acc + g + |C|).
    Total: u ((D + 5) acc + (D + 2) g + |C| + 4 sum A |t| |mu|) <= (D + 5) u T with T = acc + g + |C| + sum_d A |t| |mu|; 1.001 covers
    the second-order terms.  The fp32 rounding adds half an ulp of the result (added by the caller)."""
    A, beta, C, G = (tables[k] for k in ("A", "beta", "C", "G"))
    D, n_max = len(G), len(C) - 1
    ld = np.longdouble
    wide = np.finfo(ld).eps < np.finfo(np.float64).eps
    M, S = len(w), len(count)
    ref, bound = np.full((M, S), np.nan), np.full((M, S), np.nan)
    trial = np.zeros((M, S), bool)
    wl = w.astype(ld)
    for m in range(M):
        n = count.astype(np.int64).copy()
        sg = sums[:, :D].astype(ld)
        own = int(q_label[m])
        if loo and 0 <= own < S:
            n[own] -= 1
            sg[own] = sums[own, :D].astype(ld) - wl[m]    # exact here; the kernel's float64 difference is a rounding counted above
        ok = (n >= 1) & (n <= n_max)
        trial[m] = ok
        nn = np.where(ok, n, 1)
        mu = beta[nn].astype(ld) * sg
        t = wl[m][None, :] - mu
        At = A[nn].astype(ld)
        acc = (At * t * t).sum(1)
        g = (G.astype(ld) * wl[m] * wl[m]).sum()
        ref[m] = np.where(ok, (acc - g - C[nn].astype(ld)).astype(np.float64), np.nan)
        T = acc + g + np.abs(C[nn]) + (At * np.abs(t) * np.abs(mu)).sum(1)
        bound[m] = (1.001 * (D + 5) * U * T * (1.0 if wide else 2.0)).astype(np.float64)
    return ref, bound, trial


def _general_cases():
    """(name, tables, enrolled PLDA-space rows, labels): the fitted end-to-end model of tests/plda_cases.py on its held-out rows, and a
    wider model (D = 100) drawn at random, its rows drawn from its own two covariances."""
    (tx, ts), (hx, hs) = PC.e2e_corpora()
    model = PL.fit_plda_numpy(tx, ts)
    yield "fitted D=16", model, model.project_numpy(hx), hs.astype(np.int32)
    rng = np.random.default_rng(77)
    D = 100
    mu, Phi_b, Phi_w = rng.normal(size=D), PC.random_spd(rng, D), PC.random_spd(rng, D)
    x, spk = PC.two_covariance_corpus(78, 30, 7, D, Phi_b, Phi_w, mu)
    wide = PL.PldaModel.from_covariances(mu, Phi_b, Phi_w)
    yield "random D=100", wide, wide.project_numpy(x), spk.astype(np.int32)


def test_general_rows_lie_within_the_counted_bound():
    worst = 0.0
    for name, model, rows, label in _general_cases():
        label = label.copy()
        label[::17] = -1                      # some rows are not enrolled: uneven counts
        S = int(label.max()) + 1
        sums, _, count = EN.speaker_sums(cuda(rows), cuda(label), S, "euclidean")
        n_max = int(count.max().item()) - 1   # the largest speakers have no shared model, only leave-one-out ones
        tables = model.model_tables(n_max)
        tdev = _tables_dev(tables)
        for loo in (False, True):
            got = identify(rows, label, sums, count, tdev, loo)
            ref, bound, trial = _counted_bound(rows[:, :model.D].astype(np.float64), sums.cpu().numpy(), count.cpu().numpy(), label, tables, loo)
            assert trial.any() and (~trial).any()
            assert np.array_equal(np.isnan(got["scores"]), ~trial)
            g = got["scores"].astype(np.float64)
            tol = bound + 0.5 * np.spacing(np.abs(got["scores"])).astype(np.float64)
            err = np.abs(g - ref)
            ratio = float((err[trial] / tol[trial]).max())
            f64 = float((np.maximum(err - 0.5 * np.spacing(np.abs(got["scores"])).astype(np.float64), 0.0)[trial] / bound[trial]).max())
            same = float((bits(got["scores"])[trial] == bits(ref.astype(np.float32))[trial]).mean())
            print("%s loo=%d: largest error / (bound + half an fp32 ulp) %.4f; beyond the half ulp / bound %.3g; equal to the rounded "
                  "reference %.6f of the trials; largest bound / half an fp32 ulp %.3g" %
                  (name, loo, ratio, f64, same, float((bound[trial] / (0.5 * np.spacing(np.abs(got["scores"][trial])))).max())))
            worst = max(worst, ratio)
            assert (err[trial] <= tol[trial]).all(), (name, loo, ratio)
            # the twin is within the same bound of the reference, and the device's own outputs agree with each other exactly
            sc, t2 = PL.trial_scores_plda_numpy(rows, label, rows, label, tables, loo, S)
            assert np.array_equal(t2, trial) and (np.abs(sc - ref)[trial] <= bound[trial]).all()
            dev = EN.ranks_numpy(got["scores"], trial, label)
            for k in ("rank", "best_idx"):
                assert np.array_equal(got[k], dev[k])
            for k in ("true_score", "best_val"):
                assert np.array_equal(bits(got[k]), bits(dev[k])) or np.array_equal(got[k], dev[k], equal_nan=True)
    assert worst <= 1.0


# ---- determinism and argument checks -----------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes():
    name, model, rows, label = next(_general_cases())
    S = int(label.max()) + 1
    sums, _, count = EN.speaker_sums(cuda(rows), cuda(label), S, "euclidean")
    tdev = _tables_dev(model.model_tables(int(count.max().item())))
    runs = []
    for _ in range(2):
        got = identify(rows, label, sums, count, tdev, True)
        h = trial_hist(rows, label, sums, count, tdev, True, [(0, 22), (V.key_of(0.0), 12)], 1024)
        runs.append([got[k].tobytes() for k in sorted(got)] + [h.tobytes()])
    assert runs[0] == runs[1]


def test_bad_arguments_are_errors_and_leave_the_outputs_untouched():
    rng = np.random.default_rng(3)
    D, M, S = 5, 9, 4
    tables = _grid_tables(rng, D)
    tdev = _tables_dev(tables)
    proj, label, q, ql, _ = _grid_case(rng, M, S, D)
    sums, _, count = EN.speaker_sums(cuda(proj), cuda(label), S, "euclidean")
    qd, ld = cuda(q), cuda(ql, torch.int32)
    outs = [Guarded(M * S, torch.float32, F_GUARD), Guarded(M, torch.float32, F_GUARD), Guarded(M, torch.int32, I_GUARD),
            Guarded(M, torch.float32, F_GUARD), Guarded(M, torch.int32, I_GUARD)]
    hist = Guarded(2 * 19, torch.int64, H_GUARD)
    ws = Guarded(1 << 14, torch.int64, H_GUARD)
    win = np.array([0, 22], dtype=np.int64)
    good = dict(q=p(qd), ql=p(ld), M=M, P=8, D=D, sums=p(sums), count=p(count), S=S, A=p(tdev["A"]), beta=p(tdev["beta"]), C=p(tdev["C"]),
                G=p(tdev["G"]), n_max=N_MAX, ws=ws.ptr(), rank=outs[2].ptr(), hist=hist.ptr(), wins=win.ctypes.data)

    def call(which, **bad):
        a = dict(good, **bad)
        head = (a["q"], a["ql"], a["M"], a["P"], a["D"], a["sums"], a["count"], a["S"], a["A"], a["beta"], a["C"], a["G"], a["n_max"], 1)
        if which == "identify":
            L().call("vm_plda_speaker_identify", *head, outs[0].ptr(), outs[1].ptr(), a["rank"], outs[3].ptr(), outs[4].ptr(), a["ws"], stream())
        else:
            L().call("vm_plda_speaker_trial_hist", *head, a["wins"], 1, 16, a["hist"], a["ws"], stream())

    cases = [(dict(D=8), "D < P"), (dict(D=9), "D < P"), (dict(P=6), r"P % 4 == 0"), (dict(n_max=0), "n_max"), (dict(q=None), "null pointer"),
             (dict(sums=None), "null pointer"), (dict(beta=None), "null pointer"), (dict(G=None), "null pointer"), (dict(ws=None), "null pointer"),
             (dict(S=0), "bad sizes"), (dict(q=p(qd) + 4), "16-byte")]
    for which in ("identify", "hist"):
        for bad, msg in cases + [((dict(rank=None), "null pointer") if which == "identify" else (dict(hist=None), "null pointer"))]:
            with pytest.raises(VoicemapHipError, match=r"failed \(-1\).*" + msg):
                call(which, **bad)
    torch.cuda.synchronize()
    for o, fill in zip(outs, (F_GUARD, F_GUARD, I_GUARD, F_GUARD, I_GUARD)):
        assert (o.get("an output") == fill).all()
    assert (hist.get("hist") == H_GUARD).all() and (ws.get("the workspace") == H_GUARD).all()
    call("identify")                     # ... and the same arguments without a fault run
    torch.cuda.synchronize()
    assert (outs[2].get("rank") != I_GUARD).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
PER_SPEAKER, SEED = 3, 1


@pytest.fixture(scope="module")
def e2e():
    (tx, ts), (hx, hs) = PC.e2e_corpora()
    held = EmbeddingCache(cuda(hx), hs)
    model = PL.fit_plda(EmbeddingCache(cuda(tx), ts))
    return model, held, model.project(held), hx, hs


def _rank1(sc, trial, label):
    r = EN.ranks_numpy(sc, trial, label)["rank"]
    return float((r[r >= 0] == 0).mean())


def test_enrol_identify_and_metrics_end_to_end(e2e):
    """Held-out speakers of the anisotropic two-covariance corpus, 3 enrolment rows per speaker and the other 5 as queries: identify
    equals the twin (scores within the counted bound, ranks inside the interval the bound allows and exactly those of the device's own
    matrix), model_trial_metrics equals sorted_metrics of that matrix, leave-one-out and row shards work, and rank-1 accuracy with
    multi-session PLDA models is at least that of cosine models on the same rows -- first on the host, by the float64 statements alone."""
    model, held, proj, hx, hs = e2e
    models = EN.enrol(proj, plda=model, per_speaker=PER_SPEAKER, seed=SEED)
    cos = EN.enrol(held, "cosine", per_speaker=PER_SPEAKER, seed=SEED)
    assert models.distance == "plda" and models.n_max == PER_SPEAKER and models.S == 40 and np.array_equal(models.label, cos.label)
    assert models.tables["A"].shape == (PER_SPEAKER + 1, model.D) and models.sums.shape == (40, model.P)
    enrolled = models.label >= 0
    qi = np.flatnonzero(~enrolled)
    dense = np.searchsorted(models.speakers, hs).astype(np.int32)
    # the host statements: float64 twins on the host projection / the raw rows
    rows64 = model.project_numpy(hx)
    sc_p, tr_p = PL.trial_scores_plda_numpy(rows64, models.label, rows64[qi], dense[qi], model.model_tables(PER_SPEAKER), False, 40)
    sc_c, tr_c = EN.trial_scores_numpy(hx, cos.label, hx[qi], dense[qi], "cosine", False, S=40)
    host_p, host_c = _rank1(sc_p, tr_p, dense[qi]), _rank1(sc_c, tr_c, dense[qi])
    print("host rank-1: multi-session plda %.4f, cosine %.4f" % (host_p, host_c))
    assert host_p >= host_c and host_p > 0.5
    res, res_c = EN.identify(models, proj), EN.identify(cos, held)
    print("device rank-1: multi-session plda %.4f, cosine %.4f" % (res["rank1_accuracy"], res_c["rank1_accuracy"]))
    assert res["rank1_accuracy"] >= res_c["rank1_accuracy"]
    assert res["leave_one_out"] is False and res["n_queries"] == len(qi) and res["n_unranked"] == 0 and np.array_equal(res["query_index"], qi)
    # identify against the twin on the DEVICE's rows
    rows = proj.emb.cpu().numpy()
    out = EN.plda_speaker_identify(proj.emb[cuda(qi)], cuda(dense[qi]), models.sums, models.count, models.tables, False, return_scores=True)
    g = out["scores"].cpu().numpy()
    tables = {k: v.cpu().numpy() for k, v in models.tables.items()}
    ref, bound, trial = _counted_bound(rows[qi, :model.D].astype(np.float64), models.sums.cpu().numpy(), models.count.cpu().numpy(), dense[qi],
                                       tables, False)
    tol = bound + 0.5 * np.spacing(np.abs(g)).astype(np.float64)
    assert trial.all() and (np.abs(g - ref) <= tol).all()
    sc, _ = PL.trial_scores_plda_numpy(rows, models.label, rows[qi], dense[qi], tables, False, 40)
    assert (np.abs(sc - ref) <= bound).all()
    own = ref[np.arange(len(qi)), dense[qi]][:, None]
    own_tol = tol[np.arange(len(qi)), dense[qi]][:, None]
    lo, hi = (ref + tol < own - own_tol).sum(1), (ref - tol <= own + own_tol).sum(1) - 1
    assert (lo == hi).mean() >= 0.99 and ((res["rank"] >= lo) & (res["rank"] <= hi)).all()
    dev = EN.ranks_numpy(g, trial, dense[qi])
    assert np.array_equal(res["rank"], dev["rank"]) and np.array_equal(res["pred"], models.speakers[dev["best_idx"]])
    assert np.array_equal(bits(res["true_score"]), bits(dev["true_score"]))
    part = EN.identify(models, proj, rows=(50, 120))
    assert np.array_equal(part["rank"], res["rank"][50:120]) and part["n_queries"] == 70
    # model-trial metrics: the sorted definition on the device's matrix, with detection costs, and a fixed threshold
    tgt = dense[qi][:, None] == np.arange(40)[None, :]
    m = EN.model_trial_metrics(models, proj, dcf_points=[0.01])
    want = V.sorted_metrics(g[trial], tgt[trial])
    for k in ("eer", "eer_threshold", "best_balanced_accuracy", "best_threshold", "n_target", "n_nontarget", "n_nan"):
        assert m[k] == want[k], (k, m[k], want[k])
    assert m["n_target"] == len(qi) and len(m["dcf"]) == 1 and 0.0 <= m["dcf"][0]["min_dcf"] <= 1.0
    at = EN.model_trial_accuracy_at_threshold(models, proj, m["best_threshold"])
    assert at["balanced_accuracy"] == m["best_balanced_accuracy"]
    t = float(np.median(g))
    at = EN.model_trial_accuracy_at_threshold(models, proj, t)
    assert (at["far"], at["frr"]) == (float((g[~tgt] < t).mean()), float((g[tgt] >= t).mean()))
    # leave-one-out on the whole cache: n_max = 8 and every own model has 7 rows
    full = EN.enrol(proj, plda=model)
    assert full.n_max == 8
    loo = EN.identify(full, proj)
    assert loo["leave_one_out"] is True and loo["n_queries"] == 320 and loo["n_unranked"] == 0
    out = EN.plda_speaker_identify(proj.emb, cuda(dense), full.sums, full.count, full.tables, True, return_scores=True)
    assert np.array_equal(loo["rank"], EN.ranks_numpy(out["scores"].cpu().numpy(), np.ones((320, 40), bool), dense)["rank"])
    ml = EN.model_trial_metrics(full, proj)
    wl = V.sorted_metrics(out["scores"].cpu().numpy(), dense[:, None] == np.arange(40)[None, :])
    assert ml["eer"] == wl["eer"] and ml["best_threshold"] == wl["best_threshold"] and ml["n_target"] == 320
    # what is refused
    with pytest.raises(ValueError, match="projected by the model"):
        EN.enrol(held, plda=model)


def test_experiment_script_runs_the_plda_backend_once():
    out = subprocess.run([sys.executable, "-m", "experiments.speaker_identification", "--synthetic", "--n-seconds", "1", "--backend", "plda",
                          "--lda-dim", "8"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    row = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert row["distance"] == "plda" and row["backend"] == "plda" and row["plda_train"] == "train" and row["lda_dim"] == 8
    assert row["speakers"] == 20 and row["queries"] == 160 and row["leave_one_out"] is True and row["model_rows_max"] == 8
    assert 0.0 <= row["rank1_accuracy"] <= row["rank5_accuracy"] <= 1.0 and 0.0 <= row["trial_eer"] <= 1.0
    assert row["target_trials"] == 160 and row["nontarget_trials"] == 160 * 19
