"""-m gpu tests of vm_ahc (voicemap_amd/csrc/cluster.hip) against the statement ``diarization.ahc_reference`` (and its fast form in
tests/ahc_cases.py, which the CPU tests hold to the statement).  Every comparison is equality -- floats as uint32 bit patterns, ints
exactly -- and guard words lie around every output and around the workspace, which has exactly the size the library asks for."""
import numpy as np
import pytest
import torch

from tests import ahc_cases as AC
from voicemap_amd import diarization as DZ

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = {torch.int32: -7, torch.float32: 12345.0, torch.uint8: 0xAB}
MIXED = [1, 2, 0, 63, 65, 1, 130, 200, 129]   # straddles the 64-row groups and the 128-row tiles; an empty and two single-window recordings


class Guarded:
    """n elements between two runs of GUARD sentinel words."""

    def __init__(self, n, dtype):
        self.n, self.sent = int(n), SENT[dtype]
        self.buf = torch.full((GUARD + self.n + GUARD,), self.sent, dtype=dtype, device="cuda")

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def host(self):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == self.sent).all() and (h[GUARD + self.n:] == self.sent).all(), "a guard word was overwritten"
        return h[GUARD:GUARD + self.n].copy()

    def untouched(self):
        return bool((self.buf.cpu().numpy() == self.sent).all())


def lib():
    from voicemap_amd import _lib
    return _lib.lib()


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def tables(lens):
    lens = np.asarray(lens, np.int64)
    row0 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mat0 = np.concatenate([[0], np.cumsum(lens ** 2)]).astype(np.int64)
    return row0, mat0


def run_ahc(emb, lens, kind, linkage, threshold=None, target=None):
    """One guarded vm_ahc call.  ``emb``: (N, E) float32 numpy or device tensor; ``target``: None (NULL), or one value per recording.
    -> dict of the six outputs on the host plus ``D``: the matrices of the workspace, one (n, n) array per recording."""
    from voicemap_amd import _lib
    emb_t = emb if torch.is_tensor(emb) else torch.from_numpy(np.ascontiguousarray(emb, np.float32)).cuda()
    N, E = emb_t.shape
    row0, mat0 = tables(lens)
    R, sq = len(lens), int(mat0[-1])
    assert row0[-1] == N
    tab = torch.from_numpy(np.concatenate([row0, mat0])).cuda()
    tgt = None if target is None else torch.tensor(list(target), dtype=torch.int32, device="cuda")
    nbytes = lib().query("vm_ahc_workspace_bytes", N, E, R, sq)
    ws = Guarded(nbytes, torch.uint8)
    g = {"merge_a": Guarded(N, torch.int32), "merge_b": Guarded(N, torch.int32), "merge_h": Guarded(N, torch.float32),
         "merge_size": Guarded(N, torch.int32), "labels": Guarded(N, torch.int32), "n_clusters": Guarded(R, torch.int32)}
    lib().call("vm_ahc", emb_t.data_ptr(), N, E, tab.data_ptr(), tab.data_ptr() + (R + 1) * 8, R, sq, _lib.DIST[kind],
               AC.LINKAGES.index(linkage), float("nan") if threshold is None else float(threshold), None if tgt is None else tgt.data_ptr(),
               g["merge_a"].ptr, g["merge_b"].ptr, g["merge_h"].ptr, g["merge_size"].ptr, g["labels"].ptr, g["n_clusters"].ptr, ws.ptr,
               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {k: v.host() for k, v in g.items()}
    mats = ws.host()[:sq * 4].view(np.float32)
    out["D"] = [mats[mat0[r]:mat0[r + 1]].reshape(int(lens[r]), int(lens[r])) for r in range(R)]
    out["row0"] = row0
    return out


_D = {}


def distances(name, emb, lens, kind):
    """The recordings' distance matrices as the kernel computes them: the workspace after a call in which nothing merges (target = n_r),
    one call per (case, kind) of a module run.  That call's other outputs are checked here too."""
    if (name, kind) not in _D:
        out = run_ahc(emb, lens, kind, "average", target=[max(int(n), 1) for n in lens])
        assert np.array_equal(out["n_clusters"], np.asarray(lens, np.int32))
        assert (out["merge_a"] == -1).all() and (out["merge_b"] == -1).all() and (out["merge_size"] == -1).all()
        assert (bits(out["merge_h"]) == 0x7FC00000).all()
        assert np.array_equal(out["labels"], np.concatenate([np.arange(n, dtype=np.int32) for n in lens]))
        _D[name, kind] = out["D"]
    return _D[name, kind]


def expect(D, linkage, threshold=None, target=1):
    """The statement; above 70 windows its fast form (held to it bit for bit by the CPU tests, up to 150 windows), which takes a
    tenth of the time."""
    return AC.ahc_fast(D, linkage, threshold, target) if len(D) > 70 else DZ.ahc_reference(D, linkage, threshold, target)


def check(out, Ds, linkage, threshold=None, target=None, what=""):
    for r, D in enumerate(Ds):
        lo, hi = int(out["row0"][r]), int(out["row0"][r + 1])
        want = expect(D, linkage, threshold, 1 if target is None else target[r])
        for k in ("merge_a", "merge_b", "merge_size", "labels"):
            assert np.array_equal(out[k][lo:hi], getattr(want, k)), (what, r, k, np.flatnonzero(out[k][lo:hi] != getattr(want, k))[:8])
        assert np.array_equal(bits(out["merge_h"][lo:hi]), bits(want.merge_h)), (what, r, "merge_h")
        assert out["n_clusters"][r] == want.n_clusters, (what, r, "n_clusters")


# ---- distances -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("E", [1, 3, 64, 100, 256])
def test_matrices_equal_pairdist_bit_for_bit(E, kind):
    lens = [5, 0, 70, 131, 1, 64]
    emb = torch.from_numpy(AC.random_points(sum(lens), E, 10 + E)).cuda()
    Ds = distances("dist-%d" % E, emb, lens, kind)
    row0, _ = tables(lens)
    for r, n in enumerate(lens):
        if n == 0:
            assert Ds[r].size == 0
            continue
        want = AC.pairdist(emb[row0[r]:row0[r + 1]], kind)
        off = ~np.eye(n, dtype=bool)
        assert np.array_equal(bits(Ds[r])[off], bits(want)[off]), (r, np.argwhere((bits(Ds[r]) != bits(want)) & off)[:4])
        assert (bits(np.diagonal(Ds[r])) == 0x7FC00000).all()
        assert np.array_equal(bits(Ds[r]), bits(Ds[r].T))   # symmetric bit for bit: the merge loop relies on it


# ---- several recordings in one call ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("linkage", AC.LINKAGES)
def test_recordings_of_every_size_in_one_call(linkage, kind):
    emb = AC.random_points(sum(MIXED), 24, 7)
    Ds = distances("mixed", emb, MIXED, kind)
    out = run_ahc(emb, MIXED, kind, linkage)
    assert out["n_clusters"].tolist() == [min(n, 1) for n in MIXED]
    check(out, Ds, linkage, what=(linkage, kind))


@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("linkage", AC.LINKAGES)
def test_ties_are_decided_by_slot_order(linkage, kind):
    """Integer-grid embeddings with duplicated rows: most distances are shared by many pairs, so nearly every choice is made by (a, b)."""
    lens = [150, 97]
    emb = np.concatenate([AC.grid_points(150, 3, 2), AC.grid_points(97, 3, 5, levels=2)])
    Ds = distances("grid", emb, lens, kind)
    assert len(np.unique(bits(Ds[0])[~np.eye(150, dtype=bool)])) < 500   # of 22 350 entries
    check(run_ahc(emb, lens, kind, linkage), Ds, linkage, what=(linkage, kind))
    h = np.float32(np.median(Ds[0][~np.isnan(Ds[0])]))
    check(run_ahc(emb, lens, kind, linkage, threshold=h), Ds, linkage, threshold=h, what=(linkage, kind, "threshold"))


@pytest.mark.parametrize("kind", ["euclidean", "cosine", "dot_product"])
@pytest.mark.parametrize("linkage", AC.LINKAGES)
def test_a_nan_row(linkage, kind):
    """A NaN window: its distances are NaN, last in the order.  With a threshold the run stops when only NaN heights are left; without
    one the NaN merges are recorded (and, under average linkage, spread as the canonical NaN)."""
    lens = [61, 20]
    emb = np.concatenate([AC.nan_points(61, 4, 3), AC.random_points(20, 4, 8)])
    Ds = distances("nan", emb, lens, kind)
    assert np.isnan(Ds[0][20]).all() and np.isnan(Ds[0][:, 20]).all()
    out = run_ahc(emb, lens, kind, linkage)
    check(out, Ds, linkage, what=(linkage, kind))
    assert out["n_clusters"].tolist() == [1, 1] and np.isnan(out["merge_h"][59])
    out = run_ahc(emb, lens, kind, linkage, threshold=1e30)
    check(out, Ds, linkage, threshold=1e30, what=(linkage, kind, "threshold"))
    assert out["n_clusters"].tolist() == [2, 1]


# ---- the stop rules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linkage", AC.LINKAGES)
def test_stop_rules(linkage):
    lens = [40, 33, 50, 7]
    emb = AC.random_points(sum(lens), 16, 21)
    Ds = distances("stop", emb, lens, "cosine")
    full = run_ahc(emb, lens, "cosine", linkage)
    check(full, Ds, linkage, what="full")
    h = full["merge_h"][20]                       # a height of recording 0 (tie-free data: it is reached exactly once there)
    at = run_ahc(emb, lens, "cosine", linkage, threshold=h)
    check(at, Ds, linkage, threshold=h, what="at a height")
    below = np.nextafter(h, np.float32(-np.inf))
    under = run_ahc(emb, lens, "cosine", linkage, threshold=below)
    check(under, Ds, linkage, threshold=below, what="just below it")
    if linkage != "average":                      # monotone linkages: merge 20 is the last one at h, and the first one missing below it
        assert at["merge_a"][20] >= 0 and at["merge_a"][21] == -1 and under["merge_a"][20] == -1 and under["merge_a"][19] >= 0
    target = [0, -2, 60, 3]                       # 0 and negative mean 1; more than n_r: nothing merges
    out = run_ahc(emb, lens, "cosine", linkage, target=target)
    check(out, Ds, linkage, target=target, what="targets")
    assert out["n_clusters"].tolist() == [1, 1, 50, 3]
    both = run_ahc(emb, lens, "cosine", linkage, threshold=h, target=[30, 2, 2, 2])
    check(both, Ds, linkage, threshold=h, target=[30, 2, 2, 2], what="threshold and targets")
    assert np.array_equal(run_ahc(emb, lens, "cosine", linkage, target=None)["labels"], full["labels"])   # NULL target = 1


# ---- capacity ------------------------------------------------------------------------------------------------------------------------------
def test_capacity_2048_windows_single_linkage():
    """The largest recording: gaps 1 .. 2047 in a random order along a line.  Merge t must close the gap of size t + 1, at exactly that
    height, between the two clusters a union-find on the host says lie on either side of it."""
    emb, ma, mb, mh, ms = AC.gap_line(2048)
    out = run_ahc(emb, [2048], "euclidean", "single")
    assert np.array_equal(out["merge_a"], ma) and np.array_equal(out["merge_b"], mb) and np.array_equal(out["merge_size"], ms)
    assert np.array_equal(bits(out["merge_h"]), bits(mh))
    assert out["n_clusters"].tolist() == [1] and (out["labels"] == 0).all()
    # the same line stopped at 100 clusters: the 99 widest gaps stay open
    out = run_ahc(emb, [2048], "euclidean", "single", target=[100])
    assert np.array_equal(out["merge_a"][:1948], ma[:1948]) and (out["merge_a"][1948:] == -1).all() and out["n_clusters"].tolist() == [100]
    gaps = np.diff(emb[:, 0])
    want = np.concatenate([[0], np.cumsum(gaps > 1948)]).astype(np.int32)
    assert np.array_equal(out["labels"], want)


def test_1024_windows_average_linkage_against_the_fast_form():
    emb = AC.gap_line(1024, seed=1)[0]
    lens = [1024, 3]
    emb = np.concatenate([emb, AC.random_points(3, 1, 0)])
    Ds = distances("line-1024", emb, lens, "euclidean")
    check(run_ahc(emb, lens, "euclidean", "average"), Ds, "average", what="n = 1024")


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    from voicemap_amd import _lib
    lens = [6, 4]
    row0, mat0 = tables(lens)
    tab = torch.from_numpy(np.concatenate([row0, mat0])).cuda()
    emb = torch.zeros(11, 4, device="cuda")   # one row more: a view one float in is misaligned
    wide = torch.zeros(10, 257, device="cuda")
    ws = Guarded(lib().query("vm_ahc_workspace_bytes", 10, 256, 2, int(mat0[-1])), torch.uint8)
    g = [Guarded(10, torch.int32), Guarded(10, torch.int32), Guarded(10, torch.float32), Guarded(10, torch.int32), Guarded(10, torch.int32),
         Guarded(2, torch.int32)]

    def call(emb_ptr, E, linkage, outs, kind=0):
        return lib().cdll.vm_ahc(emb_ptr, 10, E, tab.data_ptr(), tab.data_ptr() + 3 * 8, 2, int(mat0[-1]), kind, linkage, float("nan"), None,
                                 *outs, ws.ptr, torch.cuda.current_stream().cuda_stream)
    ptrs = [x.ptr for x in g]
    cases = {"E = 257": (wide.data_ptr(), 257, 2, ptrs), "an unknown linkage": (emb.data_ptr(), 4, 3, ptrs),
             "a NULL output": (emb.data_ptr(), 4, 2, ptrs[:4] + [None] + ptrs[5:]),
             "a misaligned emb": (emb.data_ptr() + 4, 4, 2, ptrs)}
    for what, args in cases.items():
        assert call(*args) == -1, what
        assert lib().cdll.vm_last_error().decode().startswith("vm_ahc:"), what
    assert call(emb.data_ptr(), 4, 2, ptrs, kind=3) == -1
    torch.cuda.synchronize()
    assert ws.untouched() and all(x.untouched() for x in g)
    assert lib().query("vm_ahc_workspace_bytes", 0, 4, 0, 0) == 0
    # no recordings, no rows: nothing to do, no pointer is read
    lib().call("vm_ahc", None, 0, 4, None, None, 0, 0, 0, 0, float("nan"), None, None, None, None, None, None, None, None, None)
    # an unaligned emb is fine when E % 4 != 0
    assert call(emb.data_ptr() + 4, 3, 2, ptrs) == 0
    torch.cuda.synchronize()
    assert g[5].host().tolist() == [1, 1]


def test_the_wrapper_validates_what_the_launcher_cannot_see():
    with pytest.raises(ValueError, match="recording 1 holds 2049 windows"):
        DZ.cluster(torch.zeros(2052, 4, device="cuda"), [0, 3, 2052])
    with pytest.raises(ValueError, match="must not decrease"):
        DZ.cluster(torch.zeros(8, 4, device="cuda"), [0, 6, 4, 8])
    with pytest.raises(ValueError, match="from 0 to the number of rows"):
        DZ.cluster(torch.zeros(8, 4, device="cuda"), [0, 4, 7])
    with pytest.raises(ValueError):
        DZ.cluster(torch.zeros(8, 4, device="cuda"), [0, 8], linkage="ward")
    with pytest.raises(ValueError):
        DZ.cluster(torch.zeros(8, 4, device="cuda"), [0, 8], distance="manhattan")
    empty = DZ.cluster(torch.zeros(0, 4, device="cuda"), [0, 0, 0])
    assert empty.host().n_clusters.tolist() == [0, 0] and empty.host().labels.size == 0


def test_the_wrapper_is_the_entry_point():
    emb = AC.random_points(sum(MIXED), 24, 7)
    Ds = distances("mixed", emb, MIXED, "cosine")
    res = DZ.cluster(torch.from_numpy(emb).cuda(), tables(MIXED)[0], "cosine", "complete", threshold=0.9, n_speakers=2)
    h = res.host()
    out = {k: getattr(h, k) for k in ("merge_a", "merge_b", "merge_h", "merge_size", "labels", "n_clusters")}
    out["row0"] = res.row0
    check(out, Ds, "complete", threshold=0.9, target=[2] * len(MIXED), what="cluster()")
    one = res.recording(7)
    assert len(one.labels) == 200 and one.n_clusters == h.n_clusters[7] and one.merge_a[-1] == -1


def test_two_calls_give_identical_bytes():
    emb = AC.random_points(sum(MIXED), 24, 7)
    for linkage, kind in (("average", "cosine"), ("single", "euclidean")):
        a, b = run_ahc(emb, MIXED, kind, linkage), run_ahc(emb, MIXED, kind, linkage)
        for k in ("merge_a", "merge_b", "merge_h", "merge_size", "labels", "n_clusters"):
            assert a[k].tobytes() == b[k].tobytes(), (linkage, kind, k)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a["D"], b["D"]))
