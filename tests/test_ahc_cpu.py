"""CPU checks of the clustering contract (voicemap_amd/diarization.py): the statement ``ahc_reference`` against scipy's linkage in
float64, the fast form of tests/ahc_cases.py against the statement at bit equality in float32, ``cut`` against stopped runs,
``to_linkage``, the label numbering and the unused-slot fills."""
import numpy as np
import pytest

from tests import ahc_cases as AC
from voicemap_amd import diarization as DZ


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def same(a, b):
    """Two Ahc results agree: ints exactly, heights as bit patterns."""
    return (np.array_equal(a.merge_a, b.merge_a) and np.array_equal(a.merge_b, b.merge_b) and np.array_equal(bits(a.merge_h), bits(b.merge_h))
            and np.array_equal(a.merge_size, b.merge_size) and np.array_equal(a.labels, b.labels) and a.n_clusters == b.n_clusters)


@pytest.mark.parametrize("n", [2, 3, 17, 60])
@pytest.mark.parametrize("method", ["single", "complete", "average"])
def test_statement_against_scipy(method, n):
    """Tie-free random points: after ``to_linkage`` the id columns and the sizes are scipy's and the heights agree within 1e-12."""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    distance = pytest.importorskip("scipy.spatial.distance")
    x = np.random.RandomState(100 + n).randn(n, 5)
    cond = distance.pdist(x)
    D = distance.squareform(cond)
    got = DZ.ahc_reference(D, method, dtype=np.float64)
    assert got.n_clusters == 1 and (got.merge_a[:n - 1] >= 0).all()
    Z = DZ.to_linkage(got.merge_a, got.merge_b, got.merge_h, got.merge_size, n)
    want = hierarchy.linkage(cond, method=method)
    assert Z.shape == want.shape == (n - 1, 4)
    assert np.array_equal(Z[:, :2], want[:, :2]) and np.array_equal(Z[:, 3], want[:, 3])
    np.testing.assert_allclose(Z[:, 2], want[:, 2], rtol=1e-12, atol=0)


def _inputs():
    out = []
    for kind in AC.KINDS:
        out.append(("random-%s" % kind, AC.host_distances(AC.random_points(97, 7, 1), kind)))
        out.append(("grid-%s" % kind, AC.host_distances(AC.grid_points(150, 3, 2), kind)))
    out.append(("nan-row", AC.host_distances(AC.nan_points(61, 4, 3), "euclidean")))
    out.append(("two", AC.host_distances(AC.random_points(2, 3, 4), "euclidean")))
    out.append(("one", AC.host_distances(AC.random_points(1, 3, 5), "euclidean")))
    return out


INPUTS = _inputs()
_FULL = {}


def full(name, D, linkage):
    """The statement's full dendrogram of an input, computed once."""
    if (name, linkage) not in _FULL:
        _FULL[name, linkage] = DZ.ahc_reference(D, linkage)
    return _FULL[name, linkage]


@pytest.mark.parametrize("linkage", AC.LINKAGES)
@pytest.mark.parametrize("name,D", INPUTS, ids=[n for n, _ in INPUTS])
def test_fast_form_is_the_statement_bit_for_bit(name, D, linkage):
    n = len(D)
    ref = full(name, D, linkage)
    assert same(AC.ahc_fast(D, linkage), ref)
    heights = ref.merge_h[:max(n - 1, 0)]
    heights = heights[~np.isnan(heights)]
    if len(heights):
        h = np.float32(np.sort(heights)[len(heights) // 2])
        for thr, tgt in ((h, 1), (np.nextafter(h, np.float32(-np.inf)), 1), (None, 5), (h, 3), (np.float32(np.nan), 2)):
            assert same(AC.ahc_fast(D, linkage, thr, tgt), DZ.ahc_reference(D, linkage, thr, tgt)), (thr, tgt)


@pytest.mark.parametrize("linkage", AC.LINKAGES)
@pytest.mark.parametrize("name,D", INPUTS[:6:2] + INPUTS[1:6:4] + INPUTS[6:7], ids=[n for n, _ in INPUTS[:6:2] + INPUTS[1:6:4] + INPUTS[6:7]])
def test_cut_reproduces_a_stopped_run(name, D, linkage):
    """From the FULL dendrogram, ``cut`` gives the labels and the cluster count of a run stopped by a threshold at, just below and just
    above a recorded height, and by every cluster count 1 .. n."""
    n = len(D)
    ref = full(name, D, linkage)
    fin = ref.merge_h[:n - 1][~np.isnan(ref.merge_h[:n - 1])]
    picks = fin[np.linspace(0, len(fin) - 1, 4).astype(int)]
    for h in picks:
        for thr in (h, np.nextafter(h, np.float32(-np.inf)), np.nextafter(h, np.float32(np.inf))):
            want = AC.ahc_fast(D, linkage, thr, 1)
            labels, c = DZ.cut(ref.merge_a, ref.merge_b, ref.merge_h, n, threshold=thr)
            assert c == want.n_clusters and np.array_equal(labels, want.labels), (h, thr)
    for k in range(1, n + 1):
        want = AC.ahc_fast(D, linkage, None, k)
        labels, c = DZ.cut(ref.merge_a, ref.merge_b, ref.merge_h, n, n_clusters=k)
        assert c == want.n_clusters == k and np.array_equal(labels, want.labels), k
    # both at once: whichever stops first
    want = AC.ahc_fast(D, linkage, picks[1], n // 2)
    labels, c = DZ.cut(ref.merge_a, ref.merge_b, ref.merge_h, n, threshold=picks[1], n_clusters=n // 2)
    assert c == want.n_clusters and np.array_equal(labels, want.labels)


def test_to_linkage_on_four_points():
    """Points at 0, 1, 3, 7 under single linkage: (0, 1) at 1; then slot 0 (now cluster 4) with 2 at 2; then cluster 5 with 3 at 4."""
    pos = np.array([0.0, 1.0, 3.0, 7.0])
    D = np.abs(pos[:, None] - pos[None, :])
    r = DZ.ahc_reference(D, "single")
    assert r.merge_a.tolist() == [0, 0, 0, -1] and r.merge_b.tolist() == [1, 2, 3, -1] and r.merge_size.tolist() == [2, 3, 4, -1]
    assert r.merge_h[:3].tolist() == [1.0, 2.0, 4.0] and np.isnan(r.merge_h[3])
    Z = DZ.to_linkage(r.merge_a, r.merge_b, r.merge_h, r.merge_size, 4)
    assert Z.tolist() == [[0, 1, 1, 2], [2, 4, 2, 3], [3, 5, 4, 4]]
    # a stopped run gives a shorter Z
    s = DZ.ahc_reference(D, "single", threshold=2.0)
    assert DZ.to_linkage(s.merge_a, s.merge_b, s.merge_h, s.merge_size, 4).tolist() == [[0, 1, 1, 2], [2, 4, 2, 3]]


def test_label_numbering_and_unused_slots():
    """Clusters are numbered in ascending order of their slot -- a cluster's slot is its lowest member, because a merge keeps a < b --
    and the merge lists hold -1 / NaN (the canonical quiet NaN) wherever no merge was recorded: always in the last entry."""
    pos = np.array([10.0, 0.0, 11.0, 1.0, 20.0, 0.5])     # {0, 2} {1, 3, 5} {4}
    D = np.abs(pos[:, None] - pos[None, :]).astype(np.float32)
    r = DZ.ahc_reference(D, "complete", threshold=2.0)
    assert r.n_clusters == 3 and r.labels.tolist() == [0, 1, 0, 1, 2, 1] and r.labels.dtype == np.int32
    assert r.merge_a.tolist() == [1, 0, 1, -1, -1, -1] and r.merge_b.tolist() == [5, 2, 3, -1, -1, -1]
    assert r.merge_size.tolist() == [2, 2, 3, -1, -1, -1]
    assert bits(r.merge_h).tolist() == bits([0.5, 1.0, 1.0]).tolist() + [0x7FC00000] * 3
    # target = n and target > n: nothing merges; target 0 and negative mean 1
    for tgt in (6, 9):
        s = DZ.ahc_reference(D, "average", target=tgt)
        assert s.n_clusters == 6 and s.labels.tolist() == list(range(6)) and (s.merge_a == -1).all() and np.isnan(s.merge_h).all()
    for tgt in (0, -3):
        assert same(DZ.ahc_reference(D, "average", target=tgt), DZ.ahc_reference(D, "average", target=1))
    # an empty recording
    e = DZ.ahc_reference(np.zeros((0, 0), np.float32), "single")
    assert e.n_clusters == 0 and e.labels.size == 0 and e.merge_a.size == 0
    # a NaN height stops a run with a threshold and merges without one
    D[0, :] = D[:, 0] = np.nan
    assert DZ.ahc_reference(D, "single", threshold=1e9).n_clusters == 2
    full_run = DZ.ahc_reference(D, "single")
    assert full_run.n_clusters == 1 and np.isnan(full_run.merge_h[4]) and full_run.merge_a[4] == 0


def test_average_update_rounds_every_operation_on_its_own():
    """The statement's average update is the chain of four separately rounded fp32 operations -- two products, their sum, the
    quotient -- with the sizes converted exactly."""
    f32 = np.float32
    d01, d02, d12, d03, d13, d23 = (f32(v) for v in (0.1, 1.1000001, 1.3, 5.1, 6.3, 7.7))
    D = np.array([[0, d01, d02, d03], [d01, 0, d12, d13], [d02, d12, 0, d23], [d03, d13, d23, 0]], np.float32)
    r = DZ.ahc_reference(D, "average")
    assert (r.merge_a[0], r.merge_b[0], r.merge_a[1], r.merge_b[1]) == (0, 1, 0, 2)
    assert bits(r.merge_h[1]) == bits((f32(1) * d02 + f32(1) * d12) / f32(2))
    d03b = (f32(1) * d03 + f32(1) * d13) / f32(2)
    assert bits(r.merge_h[2]) == bits((f32(2) * d03b + f32(1) * d23) / f32(3))
