"""The host side of resegmentation and speech gating (voicemap_amd/diarization.py), without a GPU: reseg_reference's decode against
brute force and its planted tie rules, the iteration rule, make_conversations with and without pauses, and the numpy helpers diarize
gates windows, breaks chains, cuts segments and picks the coarse lattice with."""
import hashlib

import numpy as np
import pytest

from tests import reseg_cases as RC
from voicemap_amd import diarization as DZ


# ---- the decode -------------------------------------------------------------------------------------------------------------------------
def dyadic_emissions(rng, n, K):
    """Multiples of 1/8 in [0, 4): every sum of them and of dyadic switch costs is exact in float64."""
    return (rng.randint(0, 32, size=(n, K)) / 8.0).astype(np.float32)


@pytest.mark.parametrize("switch_cost", [0.0, 0.125, 0.5, 1.0, 3.75, 100.0])
def test_the_decode_finds_the_brute_force_minimum_exactly(switch_cost):
    rng = np.random.RandomState(int(switch_cost * 8))
    for n, K, chains in ((1, 1, None), (1, 3, None), (4, 1, None), (5, 2, None), (7, 3, None), (6, 3, [0, 0, 1, 0, 0, 1]), (7, 2, [1] * 7),
                         (7, 3, [0, 0, 0, 5, 0, 0, 0])):
        for _ in range(3):
            e = dyadic_emissions(rng, n, K)
            labels, cost = DZ.viterbi_reference(e, chains, switch_cost)
            assert cost == RC.brute_force(e, chains, switch_cost)             # exact doubles
            assert RC.path_cost(e, chains, switch_cost, labels) == cost     # and the labels are a sequence that costs it


def test_grid_emissions_are_what_the_points_say_and_decode_like_brute_force():
    """Pure models on the grid: the euclidean emission of a row against a model is the distance of two points (3-4-5 among them), the
    cosine one 0, 1 or 2, the dot-product one 0, -1/4 or 1/4 -- exactly; the decode of a short recording is the brute-force optimum."""
    for kind, want in (("euclidean", {0.0, 5.0}), ("cosine", {0.0, 1.0}), ("dot_product", {-0.25, 0.0})):
        pts = RC.speaker_points(kind, 2, 2)
        truth = np.array([0, 0, 1, 1, 0, 1, 1])
        e = DZ.emissions_reference(pts[truth], truth, 2, kind)
        assert set(np.unique(e).tolist()) == want and e.dtype == np.float32
        for sc in (0.0, 0.25, 8.0):
            labels, cost = DZ.viterbi_reference(e, None, sc)
            assert cost == RC.brute_force(e, None, sc)


def test_tie_rules():
    # stay beats switch at equality: model 1 may stay at cost 1 + 0 or be left for model 0 at 0 + 1 -- the back pointer stays
    e = np.array([[0, 1], [5, 0], [5, 0]], np.float32)
    labels, cost = DZ.viterbi_reference(e, None, 1.0)
    assert labels.tolist() == [1, 1, 1] and cost == 1.0
    # ... and just below equality it switches
    labels, cost = DZ.viterbi_reference(e, None, 0.5)
    assert labels.tolist() == [0, 1, 1] and cost == 0.5
    # the lowest j* wins: models 0 and 2 tie at the first row, model 1 is entered from model 0
    e = np.array([[1, 9, 1], [9, 0, 9]], np.float32)
    assert DZ.viterbi_reference(e, None, 2.0)[0].tolist() == [0, 1]
    # the first minimum at the chain end
    e = np.array([[2, 2, 2], [1, 1, 1]], np.float32)
    assert DZ.viterbi_reference(e, None, 0.25)[0].tolist() == [0, 0]
    e = np.array([[3, 2, 2], [1, 1, 1]], np.float32)
    assert DZ.viterbi_reference(e, None, 0.25)[0].tolist() == [1, 1]


def test_a_chain_break_resets_the_penalty():
    e = np.array([[0, 4], [0, 4], [4, 0], [4, 0]], np.float32)
    glued, c1 = DZ.viterbi_reference(e, None, 100.0)
    assert len(set(glued.tolist())) == 1 and c1 == 8.0
    cut, c2 = DZ.viterbi_reference(e, [0, 0, 1, 0], 100.0)
    assert cut.tolist() == [0, 0, 1, 1] and c2 == 0.0
    assert DZ.viterbi_reference(e, [9, 0, 1, 0], 100.0)[0].tolist() == [0, 0, 1, 1]   # the first row starts a chain anyway


def test_switch_cost_zero_is_the_row_wise_first_minimum():
    """... on rows without a tie (every row a permutation of distinct values); where two models tie in a row, "a tie stays" may keep
    the later one, at the same cost."""
    rng = np.random.RandomState(3)
    e = np.array([rng.permutation(5) for _ in range(200)], np.float32) / 4.0
    labels, cost = DZ.viterbi_reference(e, None, 0.0)
    assert np.array_equal(labels, e.argmin(axis=1)) and cost == float(e.min(axis=1).astype(np.float64).sum())
    tied = dyadic_emissions(rng, 200, 5)
    labels, cost = DZ.viterbi_reference(tied, None, 0.0)
    assert cost == float(tied.min(axis=1).astype(np.float64).sum()) and np.array_equal(tied[np.arange(200), labels], tied.min(axis=1))


def test_a_dead_cluster_is_never_entered_and_keeps_its_number():
    case = RC.grid_case(1, [60], 5, 4, "euclidean", speakers=2)
    case["labels"][case["labels"] >= 2] = -1   # models 2, 3, 4 hold no row
    res = DZ.reseg_reference(case["emb"], case["row0"], case["n_models"], case["labels"], None, "euclidean", 0.5, 4)
    assert set(res.labels.tolist()) == {0, 1} and np.isinf(res.emis.reshape(60, 5)[:, 2:]).all() and np.isfinite(res.emis.reshape(60, 5)[:, :2]).all()
    # a cluster that dies on the way: model 1 holds one stray row of speaker 0's point, the decode takes it away, the numbering stays
    pts = RC.speaker_points("euclidean", 2, 2)
    truth = np.array([0] * 6 + [1] * 6)
    lab = np.array([0, 0, 1, 0, 0, 0] + [2] * 6, np.int32)
    res = DZ.reseg_reference(pts[truth], [0, 12], [3], lab, None, "euclidean", 1.0, 4)
    assert res.labels.tolist() == [0] * 6 + [2] * 6 and res.iters_run[0] == 2 and res.n_changed[0] == 0
    assert np.isinf(res.emis.reshape(12, 3)[:, 1]).all()


def test_all_models_absent():
    case = RC.grid_case(2, [9, 0, 4], 3, 2, "cosine")
    case["labels"][:9] = [-1, 3, 99, -7, -1, -1, 3, 3, -1]
    res = DZ.reseg_reference(case["emb"], case["row0"], case["n_models"], case["labels"], None, "cosine", 0.5, 3)
    assert (res.labels[:9] == -1).all() and np.isnan(res.path_cost[0]) and res.iters_run[0] == 0 and res.n_changed[0] == 0
    assert np.isinf(res.emis[:27]).all() and res.iters_run[1] == 0 and res.iters_run[2] >= 1


@pytest.mark.parametrize("kind", RC.KINDS)
def test_one_call_with_n_iterations_equals_n_calls_fed_back(kind):
    case = RC.general_case(5, [80, 33], 4, 6, chains="edges")
    args = (case["emb"], case["row0"], case["n_models"])
    whole = DZ.reseg_reference(*args, case["labels"], case["chain_start"], kind, 0.2, 6)
    assert whole.iters_run.max() >= 2
    lab, run, done = case["labels"], np.zeros(2, np.int32), np.zeros(2, bool)
    for _ in range(6):
        step = DZ.reseg_reference(*args, lab, case["chain_start"], kind, 0.2, 1)
        for r in range(2):   # a recording stops at its first unchanged decode
            if not done[r]:
                lo, hi = case["row0"][r], case["row0"][r + 1]
                lab = lab.copy()
                lab[lo:hi] = step.labels[lo:hi]
                run[r] += 1
                done[r] = step.n_changed[r] == 0
                if done[r] or run[r] == 6:
                    assert step.path_cost[r] == whole.path_cost[r] and step.n_changed[r] == whole.n_changed[r]
    assert np.array_equal(run, whole.iters_run) and np.array_equal(lab, whole.labels)


def test_the_reference_refuses_what_the_kernel_cannot_decode():
    case = RC.grid_case(0, [5], 2, 2, "cosine")
    for K in (0, 65):
        with pytest.raises(ValueError, match="models"):
            DZ.reseg_reference(case["emb"], case["row0"], [K], case["labels"], None, "cosine", 0.5, 1)
    for sc, it in ((-1.0, 1), (float("nan"), 1), (0.5, 0), (0.5, 17)):
        with pytest.raises(ValueError):
            DZ.reseg_reference(case["emb"], case["row0"], [2], case["labels"], None, "cosine", sc, it)
        with pytest.raises(ValueError):
            DZ.ResegPolicy(sc, it)


# ---- make_conversations -----------------------------------------------------------------------------------------------------------------
class TinyCorpus:
    """Six speakers x three files of 0.3 .. 0.5 s of seeded int16 noise, in memory: what make_conversations reads of a dataset."""

    def __init__(self):
        rng = np.random.RandomState(42)
        self._code = np.repeat(np.arange(6), 3)
        self.file_length = rng.randint(4800, 8000, size=18).astype(np.int64)
        self.pcm = [rng.randint(-3000, 3000, size=int(n)).astype(np.int16) | 1 for n in self.file_length]   # never zero
        self.device_audio = None

    def _pcm(self, f):
        return self.pcm[f]


def digest(conv):
    h = hashlib.sha256()
    h.update(conv.audio.cpu().numpy().tobytes())
    for x in (conv.offsets, conv.lens):
        h.update(np.asarray(x, dtype=np.int64).tobytes())
    for seg, turn in zip(conv.segments, conv.turns):
        h.update(np.asarray(seg, dtype=np.int64).tobytes())
        h.update(np.asarray(turn, dtype=np.int64).tobytes())
    return h.hexdigest()


# computed with make_conversations as it was before the pause option existed, on TinyCorpus, for seeds 0, 1, 2
PARENT_DIGESTS = {
    0: "18995dfb8362865011381a3c40dca5b0c3bb3e8010cd9512ad0e2166ee5ebd42",
    1: "88d1948d5570a581e24498365858d0b1dfce45bc7f85da2322d14d3dede93777",
    2: "b37c3d22d277806df86ac41fcbbb2cdd27d580f655a91e637e530290cae59404",
}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_conversations_at_the_defaults_are_byte_identical_to_before(seed):
    kw = dict(speakers=(2, 4), turns=(3, 6), turn_seconds=(0.1, 0.4), seed=seed)
    conv = DZ.make_conversations(TinyCorpus(), 4, **kw)
    assert digest(conv) == PARENT_DIGESTS[seed]
    assert digest(DZ.make_conversations(TinyCorpus(), 4, pause_seconds=(0.5, 1.0), pause_prob=0.0, **kw)) == PARENT_DIGESTS[seed]
    assert all(sum(g) == 0 for g in conv.pauses)


def test_conversations_with_pauses():
    ds = TinyCorpus()
    conv = DZ.make_conversations(ds, 6, speakers=(2, 3), turns=(4, 7), turn_seconds=(0.1, 0.3), seed=3, pause_seconds=(0.05, 0.2), pause_prob=0.5)
    audio = conv.audio.cpu().numpy()
    assert audio.size == int(conv.lens.sum()) and any(sum(g) > 0 for g in conv.pauses)
    for r in range(len(conv)):
        seg, gaps, a = conv.segments[r], conv.pauses[r], audio[conv.offsets[r]:conv.offsets[r] + conv.lens[r]]
        assert gaps[0] == 0 and all(800 <= g <= 3200 or g == 0 for g in gaps)
        assert seg[0, 0] == 0 and seg[-1, 1] == conv.lens[r] and (seg[:, 1] > seg[:, 0]).all()
        assert np.array_equal(seg[1:, 0] - seg[:-1, 1], gaps[1:])   # disjoint, ordered, the gaps where the pauses were drawn
        speech = np.zeros(len(a), bool)
        for (b, e, who), (f, s, k) in zip(seg, conv.turns[r]):
            speech[b:e] = True
            assert ds._code[f] == who and np.array_equal(a[b:e], ds.pcm[f][s:s + k])
        assert (a[~speech] == 0).all() and (a[speech] != 0).all()   # zero exactly in the gaps
    with pytest.raises(ValueError, match="pause"):
        DZ.make_conversations(ds, 1, pause_prob=1.5)
    with pytest.raises(ValueError, match="pause"):
        DZ.make_conversations(ds, 1, pause_seconds=(0.3, 0.1), pause_prob=0.5)


# ---- gating, chains, cutting, the lattice -----------------------------------------------------------------------------------------------
def test_voiced_share_and_chain_starts_on_hand_made_masks():
    mask = [1, 1, 1, 0, 0, 0, 0, 1, 1, 0]   # frames of 10 samples, a recording of 95 samples
    starts = np.array([0, 10, 20, 30, 40, 50, 60, 65])
    share = DZ.voiced_share(mask, 10, starts, 30)
    #  window            frames        voiced
    want = [3 / 3,     # 0 .. 29      0 1 2
            2 / 3,     # 10 .. 39     1 2 3
            1 / 3,     # 20 .. 49     2 3 4
            0 / 3,     # 30 .. 59     3 4 5
            0 / 3,     # 40 .. 69     4 5 6
            1 / 3,     # 50 .. 79     5 6 7
            2 / 3,     # 60 .. 89     6 7 8
            2 / 4]     # 65 .. 94     6 7 8 9
    assert np.array_equal(share, np.array(want))
    kept = share >= 0.5
    assert kept.tolist() == [True, True, False, False, False, False, True, True]
    assert DZ.chain_starts(kept).tolist() == [1, 0, 1, 0]
    assert DZ.chain_starts([False, True, True, False, True]).tolist() == [1, 0, 1] and DZ.chain_starts([False, False]).size == 0
    assert DZ.chain_starts([True, True, True]).tolist() == [1, 0, 0]
    assert DZ.voiced_share([1, 0], 10, [0], 20)[0] == 0.5 and DZ.voiced_share([1, 0], 10, [0], 15)[0] == 0.5   # a short last frame counts as one


def test_segments_are_cut_to_the_voiced_frames():
    mask = [1, 1, 0, 0, 1, 0, 1]   # frames of 10 samples, 65 samples: the last frame is short
    seg = [[0, 15, 4], [15, 45, 2], [45, 65, 4]]
    assert DZ.cut_to_voiced(seg, mask, 10, 65).tolist() == [[0, 15, 4], [15, 20, 2], [40, 45, 2], [45, 50, 4], [60, 65, 4]]
    assert DZ.cut_to_voiced(seg, [0] * 7, 10, 65).shape == (0, 3)
    assert DZ.cut_to_voiced(seg, [1] * 7, 10, 65).tolist() == seg
    assert DZ.cut_to_voiced(np.zeros((0, 3)), mask, 10, 65).shape == (0, 3)


def test_the_coarse_lattice_among_the_fine_windows():
    # 10000 samples: the coarse windows sit on the lattice; 8100: the flush-end window (4100) is on neither lattice
    fine, coarse = DZ.lattice_windows([10000, 8100, 4000], 4000, 2000, 500)
    assert fine[0].tolist() == list(range(0, 6001, 500)) and fine[0][coarse[0]].tolist() == [0, 2000, 4000, 6000]
    assert fine[1].tolist() == list(range(0, 4001, 500)) + [4100] and fine[1][coarse[1]].tolist() == [0, 2000, 4000, 4100]
    assert fine[2].tolist() == [0] and coarse[2].tolist() == [True]
    # 9500: the coarse flush-end window (5500) IS a fine lattice window
    fine, coarse = DZ.lattice_windows([9500], 4000, 2000, 500)
    assert fine[0][coarse[0]].tolist() == [0, 2000, 4000, 5500] and fine[0][-1] == 5500
    for f, c, n in zip(fine, coarse, [9500]):
        assert np.array_equal(f[c], DZ.sliding_windows([n], 4000, 2000)[0])
    same, every = DZ.lattice_windows([10000, 8100], 4000, 2000, 2000)
    assert all(c.all() for c in every) and all(np.array_equal(a, b) for a, b in zip(same, DZ.sliding_windows([10000, 8100], 4000, 2000)))
    with pytest.raises(ValueError, match="multiple"):
        DZ.lattice_windows([10000], 4000, 2000, 1500)
