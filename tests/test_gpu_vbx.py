"""-m gpu tests of vm_vbx (csrc/vbx.hip) against its numpy statement, voicemap_amd/diarization.py vbx_reference: one iteration from a warm
start inside the rounding bound of tests/vbx_cases.py on a grid of sizes, several iterations without compounding error (the prefix of a
longer run is the shorter run bit for bit, and its last iteration is held to the one-iteration bound from the shorter run's state),
the stop rule, mixed tables and edges, a degenerate recording, argument errors, run-to-run identity and a planted conversation.  Every output and the workspace
sit between guard words that must survive the call."""
import numpy as np
import pytest
import torch

from tests import vbx_cases as VC
from voicemap_amd import _lib
from voicemap_amd import diarization as DZ

pytestmark = pytest.mark.gpu

GUARD = 64   # bytes on either side of every buffer
NEVER = VC.NEVER


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


def run(case, iters, epsilon=NEVER, warm=True, gamma=None, pi=None, em0=None, **over):
    """One vm_vbx call through the C entry point.  -> Vbx of numpy arrays (outputs the call left alone hold their fill: -9 / NaN)."""
    lib = _lib.lib()
    par = dict(VC.PARAMS)
    par.update(over)
    row0, K, em0_ = tables(case)
    em0 = em0_ if em0 is None else em0
    rows = torch.from_numpy(case["rows"]).cuda()
    N, P, D, R, total = rows.shape[0], rows.shape[1], case["D"], len(row0) - 1, int(em0[-1])
    tab = torch.from_numpy(np.concatenate([row0, em0])).cuda()
    mod = torch.from_numpy(np.concatenate(case["tables"])).cuda()
    km = torch.from_numpy(K.astype(np.int32)).cuda()
    lab = torch.from_numpy(case["labels"].astype(np.int32)).cuda()
    cs = None if case["chain_start"] is None else torch.from_numpy(case["chain_start"].astype(np.int32)).cuda()
    g_in = p_in = None
    if warm:
        g_in = torch.from_numpy(np.ascontiguousarray(case["gamma"] if gamma is None else gamma, dtype=np.float64)).cuda()
        p_in = torch.from_numpy(np.ascontiguousarray(case["pi"] if pi is None else pi, dtype=np.float64)).cuda()
    out = {"labels": Guarded(N, torch.int32, -9), "gamma": Guarded(total, torch.float64, float("nan")),
           "pi": Guarded(R * 64, torch.float64, float("nan")), "elbo": Guarded(R * iters, torch.float64, -7.0),
           "iters_run": Guarded(R, torch.int32, -9)}
    ws = Guarded(lib.query("vm_vbx_workspace_bytes", N, D, R, total), torch.uint8, 0)
    lib.call("vm_vbx", rows.data_ptr(), N, P, D, tab.data_ptr(), tab[R + 1:].data_ptr(), R, total, km.data_ptr(), lab.data_ptr(),
             None if cs is None else cs.data_ptr(), mod.data_ptr(), mod[D:].data_ptr(), mod[2 * D:].data_ptr(), par["loop_prob"], par["fa"],
             par["fb"], par["init_smooth"], float(epsilon), int(iters), None if g_in is None else g_in.data_ptr(),
             None if p_in is None else p_in.data_ptr(), out["labels"].ptr(), out["gamma"].ptr(), out["pi"].ptr(), out["elbo"].ptr(),
             out["iters_run"].ptr(), ws.ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ws.intact() and all(g.intact() for g in out.values()), "a guard word was overwritten"
    return DZ.Vbx(out["labels"].view.cpu().numpy(), out["gamma"].view.cpu().numpy(), out["pi"].view.cpu().numpy().reshape(R, 64),
                  out["elbo"].view.cpu().numpy().reshape(R, iters), out["iters_run"].view.cpu().numpy())


@pytest.mark.parametrize("K,D,n", VC.GRID)
def test_one_iteration_is_inside_the_counted_bound(K, D, n):
    case = VC.grid_case(K, D, n)
    got = run(case, 1)
    assert got.iters_run[0] == 1
    used = VC.check_one_iteration(case, got, VC.exact_one_iteration(K, D, n), VC.PARAMS)
    print("K", K, "D", D, "n", n, "used shares of the gamma, pi, elbo bounds:", used)


@pytest.mark.parametrize("it", [2, 5])
def test_many_iterations_do_not_compound(it):
    case = VC.mixed_case()
    short, full = run(case, it - 1), run(case, it)
    live = np.diff(case["row0"]) > 0
    assert (short.iters_run[live] == it - 1).all() and (full.iters_run[live] == it).all()
    assert full.elbo[live, :it - 1].tobytes() == short.elbo[live].tobytes()   # the prefix, bit for bit
    exact = VC.exact(case, gamma=short.gamma, pi=short.pi)
    used = VC.check_one_iteration(case, full, exact, VC.PARAMS, it_col=it - 1, gamma=short.gamma, pi=short.pi)
    print("iteration", it, "used shares of the gamma, pi, elbo bounds:", used)


def test_the_stop_rule_and_the_elbo_past_it():
    case = VC.mixed_case()
    full, stop = run(case, 6), run(case, 6, epsilon=1e30)
    live = np.diff(case["row0"]) > 0
    assert (stop.iters_run[live] == 2).all() and (full.iters_run[live] == 6).all() and np.isfinite(full.elbo[live]).all()
    assert np.isnan(stop.elbo[live, 2:]).all() and stop.elbo[live, :2].tobytes() == full.elbo[live, :2].tobytes()
    two = run(case, 2)   # the iteration that stops is counted and its results are kept
    for x, y in zip(stop[:3], two[:3]):
        assert x.tobytes() == y.tobytes()


def test_mixed_tables_edges_and_the_start_from_labels():
    """Different K in one call, an empty recording (nothing written but iters_run = 0), a recording whose labels are all -1 (a uniform
    start), a one-row recording with 64 speakers, chain starts at row 0, at the last row and on consecutive rows -- from the labels,
    not from a warm start: the start itself is checked against the statement through one iteration."""
    case = VC.mixed_case()
    row0, K, em0 = tables(case)
    got = run(case, 1, warm=False)
    want = DZ.vbx_reference(case["rows"], row0, K, case["labels"], case["chain_start"], case["tables"], VC.PARAMS["loop_prob"],
                            VC.PARAMS["fa"], VC.PARAMS["fb"], VC.PARAMS["init_smooth"], 1, NEVER, dtype=np.longdouble)
    assert list(got.iters_run) == [1, 0, 1, 1, 1]
    assert np.isnan(got.pi[1]).all() and (got.elbo[1] == -7.0).all()   # the empty recording: nothing written
    # the start the kernel made = the start of the statement: exp(-init_smooth) is taken once on the host on both sides
    q = np.exp(-VC.PARAMS["init_smooth"])
    starts, pis = [], np.zeros((5, 64))
    for r in range(5):
        lo, hi, k = int(row0[r]), int(row0[r + 1]), int(K[r])
        lab = case["labels"][lo:hi]
        g = np.where(lab[:, None] == np.arange(k)[None, :], 1.0, q) / (1.0 + (k - 1) * q)
        g[(lab < 0) | (lab >= k)] = 1.0 / k
        starts.append(g.ravel())
        pis[r, :k] = 1.0 / k
    used = VC.check_one_iteration(case, got, want, VC.PARAMS, gamma=np.concatenate(starts), pi=pis)   # skips the empty recording
    print("from the labels: used shares of the gamma, pi, elbo bounds:", used)
    lo, hi = int(em0[3]), int(em0[4])   # all labels -1: the uniform start
    assert np.allclose(got.gamma[lo:hi].reshape(-1, 2).sum(1), 1.0, atol=1e-12)


def test_a_degenerate_recording_stops_with_its_labels():
    """A prior of exactly 0 under the only speaker whose emission survives the exp in row 0: c_0 = 0, a number the forward pass tests
    for.  The recording stops with iters_run = -2 and its input labels; gamma and pi are the start's, elbo stays NaN; its neighbour in
    the same call runs as it does alone."""
    bad, good = VC.degenerate_case(), VC.random_case(4, [30], 2, 4)
    both = {"rows": np.concatenate([bad["rows"], good["rows"]]), "row0": np.array([0, 20, 50], dtype=np.int64),
            "n_models": np.array([2, 2], dtype=np.int64), "labels": np.concatenate([bad["labels"], good["labels"]]), "chain_start": None,
            "tables": bad["tables"], "gamma": np.concatenate([bad["gamma"], good["gamma"]]), "pi": np.concatenate([bad["pi"], good["pi"]]),
            "D": 4}
    got = run(both, 3)
    want = DZ.vbx_reference(both["rows"], both["row0"], 2, both["labels"], None, both["tables"], VC.PARAMS["loop_prob"], VC.PARAMS["fa"],
                            VC.PARAMS["fb"], VC.PARAMS["init_smooth"], 3, NEVER, gamma=both["gamma"], pi=both["pi"])
    assert list(want.iters_run) == [-2, 3] and list(got.iters_run) == [-2, 3]
    assert np.array_equal(got.labels[:20], bad["labels"]) and np.isnan(got.elbo[0]).all()
    assert got.gamma[:40].tobytes() == bad["gamma"].tobytes() and got.pi[0].tobytes() == bad["pi"][0].tobytes()
    alone = run(dict(good, tables=bad["tables"]), 3)
    assert got.gamma[40:].tobytes() == alone.gamma.tobytes() and got.elbo[1].tobytes() == alone.elbo[0].tobytes()
    assert np.array_equal(got.labels[20:], alone.labels) and got.pi[1].tobytes() == alone.pi[0].tobytes()


def test_two_runs_are_identical():
    case = VC.mixed_case()
    a, b = run(case, 4, warm=False), run(case, 4, warm=False)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("bad_k", [0, 65])
def test_a_speaker_count_out_of_range_leaves_minus_one_and_nothing_else(bad_k):
    case = VC.random_case(2, [20, 30, 10], 2, 4)
    good = run(case, 2)
    _, _, em0 = tables(case)
    bad = dict(case, n_models=np.array([2, bad_k, 2], dtype=np.int64))
    got = run(bad, 2, em0=em0)
    assert got.iters_run[1] == -1 and (got.labels[20:50] == -9).all() and np.isnan(got.gamma[40:100]).all()
    assert np.isnan(got.pi[1]).all() and (got.elbo[1] == -7.0).all()
    for lo, hi, r in ((0, 20, 0), (50, 60, 2)):
        assert np.array_equal(got.labels[lo:hi], good.labels[lo:hi]) and got.iters_run[r] == good.iters_run[r] == 2
        assert got.elbo[r].tobytes() == good.elbo[r].tobytes() and got.pi[r].tobytes() == good.pi[r].tobytes()


def test_argument_errors_come_before_any_launch():
    case = VC.random_case(0, [10, 5], 2, 4)
    lib = _lib.lib()
    rows = torch.from_numpy(case["rows"]).cuda()
    row0, K, em0 = tables(case)
    tab = torch.from_numpy(np.concatenate([row0, em0])).cuda()
    mod = torch.from_numpy(np.concatenate(case["tables"])).cuda()
    km, lab = torch.from_numpy(K.astype(np.int32)).cuda(), torch.from_numpy(case["labels"]).cuda()
    outs = [Guarded(15, torch.int32, -9), Guarded(30, torch.float64, -9.0), Guarded(128, torch.float64, -9.0), Guarded(6, torch.float64, -9.0),
            Guarded(2, torch.int32, -9)]
    ws = Guarded(lib.query("vm_vbx_workspace_bytes", 15, 4, 2, 30), torch.uint8, 0)

    def call(D=4, P=8, lp=0.9, fa=0.3, fb=17.0, sm=5.0, eps=1e-4, iters=3, rows_p=rows.data_ptr(), lab_p=lab.data_ptr(),
             out_p=outs[0].ptr(), ws_p=ws.ptr(), tab_p=tab.data_ptr(), mod_p=mod.data_ptr(), g_in=None):
        lib.call("vm_vbx", rows_p, 15, P, D, tab_p, tab[3:].data_ptr(), 2, 30, km.data_ptr(), lab_p, None, mod_p, mod[4:].data_ptr(),
                 mod[8:].data_ptr(), lp, fa, fb, sm, eps, iters, g_in, None, out_p, outs[1].ptr(), outs[2].ptr(), outs[3].ptr(),
                 outs[4].ptr(), ws_p, torch.cuda.current_stream().cuda_stream)

    for bad in (dict(iters=0), dict(iters=65), dict(lp=1.0), dict(lp=-0.1), dict(lp=float("nan")), dict(fa=0.0), dict(fb=float("inf")),
                dict(sm=-1.0), dict(eps=float("nan")), dict(D=0), dict(D=256), dict(D=9), dict(rows_p=None), dict(lab_p=None),
                dict(out_p=None), dict(ws_p=None), dict(tab_p=None), dict(mod_p=None), dict(g_in=outs[1].ptr())):
        with pytest.raises(_lib.VoicemapHipError):
            call(**bad)
    torch.cuda.synchronize()
    assert all((g.view.cpu() == -9).all() for g in outs) and ws.intact()
    call()
    torch.cuda.synchronize()
    assert (outs[4].view.cpu() >= 1).all()
    # the Python caller refuses what the launcher cannot see
    with pytest.raises(ValueError, match="recording 0 has 65 speakers"):
        DZ.vbx(rows, row0, case["labels"], [65, 2], case["tables"])
    with pytest.raises(ValueError, match="recording 1 has 0 speakers"):
        DZ.vbx(rows, row0, case["labels"], [2, 0], case["tables"])
    with pytest.raises(ValueError, match="labels must hold one value per row"):
        DZ.vbx(rows, row0, case["labels"][:-1], 2, case["tables"])
    with pytest.raises(ValueError, match="row0 must run from 0"):
        DZ.vbx(rows, [0, 10, 14], case["labels"], 2, case["tables"])
    with pytest.raises(ValueError, match="iters"):
        DZ.vbx(rows, row0, case["labels"], 2, case["tables"], iters=65)
    with pytest.raises(ValueError, match="tables"):
        DZ.vbx(rows, row0, case["labels"], 2, tuple(np.ones(9) for _ in range(3)))
    with pytest.raises(ValueError, match="gamma must hold 30 values"):
        DZ.vbx(rows, row0, case["labels"], 2, case["tables"], gamma=np.ones(29))


def test_the_python_call_gives_what_the_entry_point_gives():
    case = VC.mixed_case()
    got = run(case, 3, warm=False)
    res = DZ.vbx(torch.from_numpy(case["rows"]).cuda(), case["row0"], case["labels"], case["n_models"], case["tables"], case["chain_start"],
                 iters=3, epsilon=NEVER, **VC.PARAMS)
    h = res.host()
    live = np.diff(case["row0"]) > 0
    assert np.array_equal(h.labels, got.labels) and h.gamma.tobytes() == got.gamma.tobytes() and np.array_equal(h.iters_run, got.iters_run)
    assert h.pi[live].tobytes() == got.pi[live].tobytes() and h.elbo[live].tobytes() == got.elbo[live].tobytes()
    assert (h.pi[~live] == 0).all() and np.isnan(h.elbo[~live]).all()
    rec = res.recording(2)
    assert rec.gamma.shape == (70, 9) and rec.pi.shape == (9,) and rec.iters_run == 3 and res.recording(1).gamma.shape == (0, 0)
    warm = DZ.vbx(torch.from_numpy(case["rows"]).cuda(), case["row0"], case["labels"], case["n_models"], case["tables"], case["chain_start"],
                  iters=1, epsilon=NEVER, gamma=case["gamma"], pi=case["pi"], **VC.PARAMS).host()
    assert warm.gamma.tobytes() == run(case, 1).gamma.tobytes()


def test_a_planted_conversation_ends_with_its_speakers():
    model, rows, truth, labels = VC.planted_corpus()
    res = DZ.vbx(torch.from_numpy(rows).cuda(), [0, len(rows)], labels, 6, model, loop_prob=0.9).host()
    assert VC.planted_ok(res.labels, truth) and 2 <= res.iters_run[0] <= 20
    assert (np.sort(res.pi[0, :6])[:3] < 1e-3).all() and (np.sort(res.pi[0, :6])[3:] > 0.1).all()
