"""-m gpu tests of vm_reseg (csrc/reseg.hip) against its numpy statement, voicemap_amd/diarization.py reseg_reference: grid cases at bit
equality (labels, path cost bits, iteration counts, changed rows, emissions), general embeddings in two stages (the emissions within the
derived tolerance of the enrolment scores; the decode of the device's OWN emissions bit for bit), a recording longer than vm_ahc
could cluster, run-to-run identity, argument errors and tables the kernel must refuse.  Every output and the workspace sit between guard
words that must survive the call."""
import numpy as np
import pytest
import torch

from tests import reseg_cases as RC
from voicemap_amd import _lib
from voicemap_amd import diarization as DZ

pytestmark = pytest.mark.gpu

GUARD = 64   # bytes on either side of every buffer


class Guarded:
    """A device buffer of ``n`` elements of ``dtype`` filled with ``fill`` between two runs of guard bytes."""

    def __init__(self, n, dtype, fill):
        item = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((2 * GUARD + n * item,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.raw[GUARD:GUARD + n * item].view(dtype)
        self.view.fill_(fill)

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all().item()) and bool((self.raw[-GUARD:] == 0xA5).all().item())


def tables(case):
    row0 = np.asarray(case["row0"], dtype=np.int64)
    K = np.asarray(case["n_models"], dtype=np.int64)
    em0 = np.concatenate([[0], np.cumsum(np.diff(row0) * K)]).astype(np.int64)
    return row0, K, em0


def run(case, kind, switch_cost, iters, want_emis=True, em0=None):
    """One vm_reseg call through the C entry point.  -> Reseg of numpy arrays (outputs the call left alone hold their fill: -9 / NaN)."""
    lib = _lib.lib()
    row0, K, em0_ = tables(case)
    em0 = em0_ if em0 is None else em0
    emb = torch.from_numpy(case["emb"]).cuda()
    N, E, R, total = emb.shape[0], emb.shape[1], len(row0) - 1, int(em0[-1])
    tab = torch.from_numpy(np.concatenate([row0, em0])).cuda()
    km = torch.from_numpy(K.astype(np.int32)).cuda()
    lab = torch.from_numpy(case["labels"].astype(np.int32)).cuda()
    cs = None if case["chain_start"] is None else torch.from_numpy(case["chain_start"].astype(np.int32)).cuda()
    out = {"labels": Guarded(N, torch.int32, -9), "path_cost": Guarded(R, torch.float64, float("nan")),
           "iters_run": Guarded(R, torch.int32, -9), "n_changed": Guarded(R, torch.int32, -9),
           "emis": Guarded(total, torch.float32, float("nan"))}
    ws = Guarded(lib.query("vm_reseg_workspace_bytes", N, E, R, total), torch.uint8, 0)
    lib.call("vm_reseg", emb.data_ptr(), N, E, tab.data_ptr(), tab[R + 1:].data_ptr(), R, total, km.data_ptr(), lab.data_ptr(),
             None if cs is None else cs.data_ptr(), _lib.DIST[kind], float(switch_cost), int(iters), out["labels"].ptr(),
             out["path_cost"].ptr(), out["iters_run"].ptr(), out["n_changed"].ptr(), out["emis"].ptr() if want_emis else None, ws.ptr(),
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ws.intact() and all(g.intact() for g in out.values()), "a guard word was overwritten"
    return DZ.Reseg(*(out[k].view.cpu().numpy() for k in ("labels", "path_cost", "iters_run", "n_changed", "emis")))


def assert_equals_reference(case, kind, switch_cost, iters, got):
    want = DZ.reseg_reference(case["emb"], case["row0"], case["n_models"], case["labels"], case["chain_start"], kind, switch_cost, iters)
    live = np.diff(case["row0"]) > 0   # an empty recording: nothing written but iters_run
    assert np.array_equal(got.iters_run, want.iters_run)
    assert np.array_equal(got.labels, want.labels)
    assert np.array_equal(got.n_changed[live], want.n_changed[live]) and (got.n_changed[~live] == -9).all()
    assert np.array_equal(got.path_cost[live].view(np.uint64), want.path_cost[live].view(np.uint64)) and np.isnan(got.path_cost[~live]).all()
    assert np.array_equal(got.emis.view(np.uint32), want.emis.view(np.uint32))
    return want


SIZES = [0, 1, 2, 63, 64, 65, 257]


@pytest.mark.parametrize("kind", RC.KINDS)
@pytest.mark.parametrize("E", [1, 3, 64, 100, 256])
@pytest.mark.parametrize("K", [1, 2, 3, 63, 64])
def test_grid_cases_equal_the_statement_bit_for_bit(kind, K, E):
    case = RC.grid_case(11 * K + E, SIZES, K, E, kind)
    got = run(case, kind, 0.25, 4)
    want = assert_equals_reference(case, kind, 0.25, 4, got)
    assert want.iters_run.max() >= 1 and (want.iters_run[0] == 0)


@pytest.mark.parametrize("chains", ["edges", "all"])
@pytest.mark.parametrize("kind", RC.KINDS)
def test_grid_cases_with_chain_breaks(kind, chains):
    case = RC.grid_case(5, SIZES, 3, 8, kind, chains=chains)
    got = run(case, kind, 0.5, 3)
    assert_equals_reference(case, kind, 0.5, 3, got)
    if chains == "all":   # every row alone: the row-wise first minimum of the emissions, whatever the switch cost
        lo = 0
        for r, n in enumerate(SIZES):
            if got.iters_run[r] >= 1:
                e = got.emis[lo * 3:(lo + n) * 3].reshape(n, 3)
                assert np.array_equal(got.labels[lo:lo + n], e.argmin(axis=1))
                assert got.path_cost[r] == e.min(axis=1).astype(np.float64).cumsum()[-1]
            lo += n


def test_dead_clusters_ties_and_no_model_at_all():
    """K = 6 models over 2 speakers: models 2 .. 5 start empty unless a flip enters them; a recording whose labels are all out of range
    has no model: -1 labels, NaN cost, 0 iterations, +inf emissions.  K = 3 speakers on E = 1 under cosine share points: ties."""
    case = RC.grid_case(3, [40, 17, 30], 6, 4, "euclidean", speakers=2)
    case["labels"][40:57] = np.where(np.arange(17) % 2 == 0, -1, 6)
    got = run(case, "euclidean", 1.0, 5)
    assert_equals_reference(case, "euclidean", 1.0, 5, got)
    assert (got.labels[40:57] == -1).all() and np.isnan(got.path_cost[1]) and got.iters_run[1] == 0 and got.n_changed[1] == 0
    assert np.isinf(got.emis[40 * 6:57 * 6]).all()
    tie = RC.grid_case(4, [50], 3, 1, "cosine", speakers=3)
    assert_equals_reference(tie, "cosine", 0.0, 3, run(tie, "cosine", 0.0, 3))


@pytest.mark.parametrize("kind", RC.KINDS)
def test_general_embeddings_in_two_stages(kind):
    """(a) one iteration: the device's emissions against trial_scores_numpy on the same labels, inside the enrolment tolerance.  (b) the
    numpy decode of the device's own emissions gives the device's labels and path cost bit for bit -- after one iteration and after
    several (the emissions returned are the last iteration's)."""
    from voicemap_amd.enrolment import trial_scores_numpy
    sizes, K, E = [130, 0, 65, 300], 5, 24
    case = RC.general_case(7, sizes, K, E, chains="edges")
    row0 = case["row0"]
    one = run(case, kind, 0.3, 1)
    for r, n in enumerate(sizes):
        if n == 0:
            continue
        lo, hi = int(row0[r]), int(row0[r + 1])
        x, lab = case["emb"][lo:hi], case["labels"][lo:hi]
        sc, trial = trial_scores_numpy(x, lab, x, np.full(n, -1), kind, False, S=K)
        got = one.emis[lo * K:hi * K].reshape(n, K).astype(np.float64)
        tol = RC.emission_tolerance(x, lab, sc, kind, K)
        assert trial.any() and np.isinf(got[~trial]).all()
        print(kind, r, "largest error / tolerance:", float((np.abs(got - sc)[trial] / tol[trial]).max()))
        assert np.all(np.abs(got - sc)[trial] <= tol[trial])
    for res in (one, run(case, kind, 0.3, 6)):
        for r, n in enumerate(sizes):
            if n == 0:
                continue
            lo, hi = int(row0[r]), int(row0[r + 1])
            labels, cost = DZ.viterbi_reference(res.emis[lo * K:hi * K].reshape(n, K), case["chain_start"][lo:hi], 0.3)
            assert np.array_equal(labels, res.labels[lo:hi])
            assert np.float64(cost).view(np.uint64) == res.path_cost[r:r + 1].view(np.uint64)[0]
            assert 1 <= res.iters_run[r] <= 6


def test_one_recording_longer_than_the_clustering_cap():
    n, K = 5000, 4
    assert n > DZ.MAX_N
    case = RC.grid_case(9, [n], K, 16, "cosine")
    got = run(case, "cosine", 0.5, 3)
    assert_equals_reference(case, "cosine", 0.5, 3, got)
    # the Python call gives the same
    res = DZ.resegment(torch.from_numpy(case["emb"]).cuda(), case["row0"], case["labels"], K, distance="cosine", switch_cost=0.5, iters=3)
    assert np.array_equal(res.host().labels, got.labels) and res.recording(0).emis.shape == (n, K)


def test_two_runs_are_identical_and_the_emissions_are_optional():
    case = RC.general_case(1, [200, 90], 7, 33)
    a, b = run(case, "euclidean", 0.7, 4), run(case, "euclidean", 0.7, 4)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    c = run(case, "euclidean", 0.7, 4, want_emis=False)
    assert np.isnan(c.emis).all()
    for x, y in zip(a[:4], c[:4]):
        assert x.tobytes() == y.tobytes()


def test_argument_errors_come_before_any_launch():
    case = RC.grid_case(0, [10, 5], 2, 4, "cosine")
    lib = _lib.lib()
    emb = torch.from_numpy(case["emb"]).cuda()
    row0, K, em0 = tables(case)
    tab = torch.from_numpy(np.concatenate([row0, em0])).cuda()
    km, lab = torch.from_numpy(K.astype(np.int32)).cuda(), torch.from_numpy(case["labels"]).cuda()
    outs = [Guarded(15, torch.int32, -9), Guarded(2, torch.float64, float("nan")), Guarded(2, torch.int32, -9), Guarded(2, torch.int32, -9)]
    ws = Guarded(lib.query("vm_reseg_workspace_bytes", 15, 4, 2, int(em0[-1])), torch.uint8, 0)

    def call(kind=_lib.VM_DIST_COSINE, sc=0.5, iters=3, emb_p=emb.data_ptr(), lab_p=lab.data_ptr(), out_p=outs[0].ptr(), ws_p=ws.ptr(),
             tab_p=tab.data_ptr()):
        lib.call("vm_reseg", emb_p, 15, 4, tab_p, tab[3:].data_ptr(), 2, int(em0[-1]), km.data_ptr(), lab_p, None, kind, sc, iters, out_p,
                 outs[1].ptr(), outs[2].ptr(), outs[3].ptr(), None, ws_p, torch.cuda.current_stream().cuda_stream)

    with pytest.raises(_lib.VoicemapHipError, match="PLDA-space row"):
        call(kind=_lib.VM_SCORE_PLDA)
    for bad in (dict(iters=0), dict(iters=17), dict(sc=-0.5), dict(sc=float("nan")), dict(sc=float("inf")), dict(kind=7),
                dict(emb_p=None), dict(lab_p=None), dict(out_p=None), dict(ws_p=None), dict(tab_p=None)):
        with pytest.raises(_lib.VoicemapHipError):
            call(**bad)
    torch.cuda.synchronize()
    assert all((g.view.cpu() == -9).all() for g in (outs[0], outs[2], outs[3])) and ws.intact()
    call()
    torch.cuda.synchronize()
    assert (outs[2].view.cpu() >= 1).all()
    # the Python caller refuses what the launcher cannot see, and PLDA with the reason
    with pytest.raises(ValueError, match="not a PLDA-space row"):
        DZ.resegment(emb, row0, case["labels"], 2, distance="plda")
    with pytest.raises(ValueError, match="recording 0 has 65 models"):
        DZ.resegment(emb, row0, case["labels"], [65, 2])
    with pytest.raises(ValueError, match="recording 1 has 0 models"):
        DZ.resegment(emb, row0, case["labels"], [2, 0])
    with pytest.raises(ValueError, match="labels must hold one value per row"):
        DZ.resegment(emb, row0, case["labels"][:-1], 2)
    with pytest.raises(ValueError, match="row0 must run from 0"):
        DZ.resegment(emb, [0, 10, 14], case["labels"], 2)
    with pytest.raises(ValueError, match="iters"):
        DZ.resegment(emb, row0, case["labels"], 2, iters=17)


@pytest.mark.parametrize("bad_k", [0, 65])
def test_a_model_count_out_of_range_leaves_minus_one_and_nothing_else(bad_k):
    """The launcher cannot see n_models: the kernel marks the recording and writes nothing for it; its neighbours are decoded."""
    case = RC.grid_case(2, [20, 30, 10], 2, 4, "dot_product")
    good = run(case, "dot_product", 0.25, 3)
    _, _, em0 = tables(case)
    case["n_models"] = np.array([2, bad_k, 2], dtype=np.int64)
    got = run(case, "dot_product", 0.25, 3, em0=em0)   # the emission table of the good call: the bad recording's range stays its own
    assert got.iters_run[1] == -1 and (got.labels[20:50] == -9).all() and np.isnan(got.path_cost[1]) and got.n_changed[1] == -9
    assert np.isnan(got.emis[40:100]).all()
    for lo, hi, r in ((0, 20, 0), (50, 60, 2)):
        assert np.array_equal(got.labels[lo:hi], good.labels[lo:hi]) and got.iters_run[r] == good.iters_run[r] >= 1
        assert got.path_cost[r] == good.path_cost[r]
