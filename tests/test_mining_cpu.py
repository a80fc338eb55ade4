"""CPU (no GPU) checks of hard-pair mining: the contract of vm_mine_pairs as mine_pairs_numpy states it on hand-made score matrices, the
HardPairSampler over the synthetic dataset (labels, the mined share, shapes, the untouched np.random stream when mining is off, update)
and the argument errors of the entry point."""
import sys
import os

import numpy as np
import pytest

from voicemap_amd import _lib
from voicemap_amd import mining as MN
from voicemap_amd.librispeech import SyntheticSpeechDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.nan


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mine(s, label, k_neg, k_pos, **kw):
    ni, nv, pi, pv = MN.mine_pairs_numpy(np.asarray(s, np.float32), np.asarray(label), k_neg, k_pos, **kw)
    assert ni.dtype == pi.dtype == np.int32 and nv.dtype == pv.dtype == np.float32
    assert ni.shape == nv.shape == (len(s), k_neg) and pi.shape == pv.shape == (len(s), k_pos)
    assert np.array_equal(np.isnan(nv), ni < 0) and np.array_equal(np.isnan(pv), pi < 0)
    return ni, nv, pi, pv


def test_order_ties_and_padding_on_a_hand_made_matrix():
    #        j:   0    1    2    3    4    5
    s = [[0.0, 2.0, 1.0, 1.0, 3.0, 1.0],     # anchor 0 (speaker 0)
         [2.0, 0.0, 5.0, 5.0, 5.0, 5.0],     # anchor 1 (speaker 0): every other-speaker score ties
         [1.0, 5.0, 0.0, -0.0, 0.0, 7.0]]    # anchor 2 (speaker 1): -0.0 and +0.0 are one key, so j decides
    label = [0, 0, 1, 1, 2, 0]
    ni, nv, pi, pv = _mine(s, label, 3, 2)
    # negatives: (key, j) ascending among the other speakers; anchor 0: 1.0 at j = 2, 3 then 3.0 at j = 4 (j = 5 is its own speaker)
    assert ni.tolist() == [[2, 3, 4], [2, 3, 4], [4, 0, 1]]
    assert nv.tolist() == [[1.0, 1.0, 3.0], [5.0, 5.0, 5.0], [0.0, 1.0, 5.0]]
    # positives: key DESCENDING, ties to the lower j; the anchor itself never; anchor 2 has one same-speaker file: padded
    assert pi.tolist() == [[1, 5], [5, 0], [3, -1]]
    assert pv[0].tolist() == [2.0, 1.0] and pv[1].tolist() == [5.0, 2.0]
    assert _bits(pv[2, :1])[0] == 0x80000000 and np.isnan(pv[2, 1])   # the value keeps its own bits: -0.0 stays -0.0
    # K larger than the number of candidates: -1 / NaN padding
    ni, nv, pi, pv = _mine(s, label, 6, 6)
    assert ni[0].tolist() == [2, 3, 4, -1, -1, -1] and pi[0].tolist() == [1, 5, -1, -1, -1, -1]
    # one list alone
    ni, nv, pi, pv = _mine(s, label, 2, 0)
    assert ni.tolist() == [[2, 3], [2, 3], [4, 0]] and pi.shape == (3, 0)


def test_heavy_ties_are_cut_in_index_order():
    N = 40
    s = np.ones((N, N), np.float32)
    label = np.arange(N) % 2
    ni, nv, pi, pv = _mine(s, label, 5, 5)
    for i in range(N):
        other = [j for j in range(N) if j % 2 != i % 2]
        same = [j for j in range(N) if j % 2 == i % 2 and j != i]
        assert ni[i].tolist() == other[:5] and pi[i].tolist() == same[:5]
    assert (nv == 1).all() and (pv == 1).all()


def test_nan_scores_unlabelled_rows_and_single_file_speakers():
    r = np.random.default_rng(0)
    N = 12
    s = r.integers(0, 4, (N, N)).astype(np.float32)
    s[3, :] = NAN          # a NaN row: that anchor selects nothing
    s[:, 7] = NAN          # a NaN column: that candidate is never selected
    label = np.array([0, 0, 0, 1, 1, 1, 2, 2, -1, 0, 3, 1])   # row 8 unlabelled, speaker 3 has a single file (row 10)
    ni, nv, pi, pv = _mine(s, label, 4, 3)
    assert (ni[3] == -1).all() and (pi[3] == -1).all()
    assert not (ni == 7).any() and not (pi == 7).any()
    assert not (ni == 8).any() and not (pi == 8).any()          # an unlabelled candidate is never selected ...
    assert (ni[8] == -1).all() and (pi[8] == -1).all()          # ... and an unlabelled anchor gets empty lists
    assert (pi[10] == -1).all() and (ni[10] >= 0).all()         # the single-file speaker: no positive, negatives as usual
    for i in range(N):
        for j in ni[i][ni[i] >= 0]:
            assert label[j] != label[i] and label[j] >= 0 and j != i
        for j in pi[i][pi[i] >= 0]:
            assert label[j] == label[i] and j != i
    # brute force per row
    for i in (0, 5, 9):
        cand = [j for j in range(N) if j != i and label[j] >= 0 and not np.isnan(s[i, j])]
        neg = sorted((j for j in cand if label[j] != label[i]), key=lambda j: (s[i, j], j))[:4]
        pos = sorted((j for j in cand if label[j] == label[i]), key=lambda j: (-s[i, j], j))[:3]
        assert ni[i][:len(neg)].tolist() == neg and pi[i][:len(pos)].tolist() == pos


def test_floor_is_strict_nan_floor_is_none_and_row0_shifts_the_anchor():
    s = np.array([[9.0, 1.0, 2.0, 2.0, 3.0, -1.0],
                  [1.0, 9.0, 2.0, 2.0, 3.0, -0.0]], np.float32)
    label = [0, 0, 1, 2, 3, 4]
    ni, nv, _, _ = _mine(s, label, 3, 0, neg_floor=[2.0, NAN])
    assert ni[0].tolist() == [4, -1, -1]            # 2.0 itself is NOT beyond the floor 2.0
    assert ni[1].tolist() == [5, 2, 3]              # NaN: no floor
    ni, _, _, _ = _mine(s, label, 3, 0, neg_floor=[-1.0, 0.0])
    assert ni[0].tolist() == [2, 3, 4]              # -1.0 == floor: excluded
    assert ni[1].tolist() == [2, 3, 4]              # key(-0.0) == key(+0.0): not beyond a floor of 0.0
    # rows of a shard: row m is anchor row0 + m
    big = np.arange(36, dtype=np.float32).reshape(6, 6)
    lab = [0, 1, 0, 1, 0, 1]
    full = _mine(big, lab, 2, 2)
    part = _mine(big[2:5], lab, 2, 2, row0=2)
    for a, b in zip(full, part):
        assert np.array_equal(a[2:5], b, equal_nan=True)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------
def _dataset(**kw):
    return SyntheticSpeechDataset(num_speakers=12, files_per_speaker=6, seconds=0.5, pad=True, **kw)


def _pools(ds, k_neg=3, k_pos=2, seed=0, shift=0):
    """Hand-made mined lists over the files of ds: valid by construction (positives share the speaker, negatives do not)."""
    r = np.random.RandomState(seed)
    code = np.asarray(ds._code)
    N = len(ds)
    ni, pi = np.full((N, k_neg), -1, np.int32), np.full((N, k_pos), -1, np.int32)
    for i in range(N):
        same = np.flatnonzero((code == code[i]) & (np.arange(N) != i))
        other = np.flatnonzero(code != code[i])
        if i % 5 != shift:   # some anchors have empty lists, some short ones
            ni[i, :k_neg - (i % 2)] = r.choice(other, k_neg - (i % 2), replace=False)
            pi[i, :k_pos - (i % 2)] = r.choice(same, k_pos - (i % 2), replace=False)
    nv = np.where(ni >= 0, 1.0, NAN).astype(np.float32)
    pv = np.where(pi >= 0, 2.0, NAN).astype(np.float32)
    return MN.MinedPairs(ni, nv, pi, pv, "euclidean", (0, N))


def _member(mined_idx, pair):
    return pair[1] in mined_idx[pair[0]][mined_idx[pair[0]] >= 0]


@pytest.mark.parametrize("hard_fraction,batchsize", [(0.5, 16), (0.3, 20), (1.0, 8), (0.25, 6)])
def test_sampler_draws_the_mined_share_with_the_right_labels(hard_fraction, batchsize):
    ds = _dataset()
    mined = _pools(ds)
    sm = MN.HardPairSampler(ds, mined, hard_fraction=hard_fraction, seed=3)
    half = batchsize // 2
    n_hard = int(round(hard_fraction * half))
    asked = {"alike": [], "differing": []}
    ga, gd = ds.get_alike_pairs, ds.get_differing_pairs
    ds.get_alike_pairs = lambda n: (asked["alike"].append(n), ga(n))[1]
    ds.get_differing_pairs = lambda n: (asked["differing"].append(n), gd(n))[1]
    code = np.asarray(ds._code)
    np.random.seed(1)
    for _ in range(5):
        alike, differing = sm.verification_pairs(batchsize)
        assert len(alike) == len(differing) == half
        assert all(code[i] == code[j] for i, j in alike) and all(code[i] != code[j] for i, j in differing)
        # the first n_hard of each half come from the pools, and the dataset was asked for exactly the rest
        assert all(_member(mined.pos_idx, pr) for pr in alike[:n_hard])
        assert all(_member(mined.neg_idx, pr) for pr in differing[:n_hard])
    want = [half - n_hard] * 5 if half - n_hard else []
    assert asked == {"alike": want, "differing": want}
    assert mined.pos_fraction == pytest.approx(np.mean(np.arange(len(ds)) % 5 != 0))
    assert mined.neg_mean == 1.0 and mined.pos_mean == 2.0


def test_sampler_batches_have_the_datasets_shapes_and_outputs():
    ds = _dataset()
    sm = MN.HardPairSampler(ds, _pools(ds), hard_fraction=0.5, seed=0)
    np.random.seed(2)
    (a1, a2), ya = ds.build_verification_batch(10)
    (b1, b2), yb = sm.build_verification_batch(10)
    assert a1.shape == b1.shape == a2.shape == b2.shape and a1.dtype == b1.dtype
    assert np.array_equal(ya, yb) and yb.shape == (10, 1) and yb[:5].sum() == 0 and yb[5:].sum() == 5
    (c1, c2), yc = next(sm.yield_verification_batches(10))
    assert c1.shape == a1.shape and np.array_equal(yc, ya)


@pytest.mark.parametrize("how", ["zero_fraction", "no_pools"])
def test_sampler_without_mining_is_the_dataset_bit_for_bit(how):
    ds = _dataset()
    sm = MN.HardPairSampler(ds, _pools(ds), hard_fraction=0.0) if how == "zero_fraction" else MN.HardPairSampler(ds, None, hard_fraction=0.5)
    np.random.seed(11)
    ref = [ds.build_verification_batch(8) for _ in range(3)]
    state_ref = np.random.get_state()
    np.random.seed(11)
    got = [sm.build_verification_batch(8) for _ in range(3)]
    state_got = np.random.get_state()
    for ((r1, r2), ry), ((g1, g2), gy) in zip(ref, got):
        assert np.array_equal(r1, g1) and np.array_equal(r2, g2) and np.array_equal(ry, gy)
    assert state_ref[0] == state_got[0] and np.array_equal(state_ref[1], state_got[1]) and state_ref[2:] == state_got[2:]


def test_mined_draws_leave_np_random_to_the_dataset():
    """The mined pairs come from the sampler's own stream: the dataset's random pairs of a batch are those it would draw alone."""
    ds = _dataset()
    sm = MN.HardPairSampler(ds, _pools(ds), hard_fraction=0.5, seed=5)
    np.random.seed(4)
    alike, differing = sm.verification_pairs(8)
    np.random.seed(4)
    assert alike[2:] == list(ds.get_alike_pairs(2)) and differing[2:] == list(ds.get_differing_pairs(2))
    # and the same seed gives the same mined pairs
    sm2 = MN.HardPairSampler(ds, _pools(ds), hard_fraction=0.5, seed=5)
    np.random.seed(4)
    assert sm2.verification_pairs(8) == (alike, differing)


def test_update_takes_effect_on_the_next_batch():
    ds = _dataset()
    sm = MN.HardPairSampler(ds, None, hard_fraction=1.0, seed=1)
    np.random.seed(0)
    first = _pools(ds, seed=1)
    second = _pools(ds, seed=2, shift=1)
    sm.update(first)
    alike, differing = sm.verification_pairs(12)
    assert all(_member(first.pos_idx, pr) for pr in alike) and all(_member(first.neg_idx, pr) for pr in differing)
    sm.update(second)
    alike, differing = sm.verification_pairs(12)
    assert all(_member(second.pos_idx, pr) for pr in alike) and all(_member(second.neg_idx, pr) for pr in differing)
    assert not all(_member(first.neg_idx, pr) for pr in differing)
    sm.update(None)
    state = np.random.get_state()[1].copy()
    alike, _ = sm.verification_pairs(12)
    assert not np.array_equal(state, np.random.get_state()[1])   # back to the dataset's own draws
    with pytest.raises(ValueError):
        sm.update(MN.MinedPairs(first.neg_idx[:5], first.neg_val[:5], first.pos_idx[:5], first.pos_val[:5], "euclidean", (0, 5)))
    with pytest.raises(ValueError):
        MN.HardPairSampler(ds, None, hard_fraction=1.5)


# ---- the entry point -------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_report_argument_errors_without_a_gpu():
    names = ("vm_mine_pairs", "vm_mine_pairs_workspace_bytes")
    for n in names:
        assert n in _lib.header_functions() and n in _lib.SIGNATURES
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib.cdll, n)
    # one rank's share of train-clean-360: the workspace is the norms, the anchors and the partial lists -- far below an M x N tile
    nbytes = lib.query("vm_mine_pairs_workspace_bytes", 104014, 64, 0, 13002, 8, 4)
    assert 104014 * 4 + 13002 * 64 * 4 <= nbytes < 64 << 20
    assert nbytes < 13002 * 104014 * 4 // 50
    ok = dict(emb=16, label=16, N=100, E=64, kind=0, lo=0, hi=10, k_neg=8, k_pos=4, floor=None, ni=16, nv=16, pi=16, pv=16, ws=256)

    def call(**kw):
        a = dict(ok, **kw)
        lib.call("vm_mine_pairs", a["emb"], a["label"], a["N"], a["E"], a["kind"], a["lo"], a["hi"], a["k_neg"], a["k_pos"], a["floor"],
                 a["ni"], a["nv"], a["pi"], a["pv"], a["ws"], None)
    for kw in (dict(emb=None), dict(label=None), dict(ws=None)):
        with pytest.raises(_lib.VoicemapHipError, match="null pointer"):
            call(**kw)
    with pytest.raises(_lib.VoicemapHipError, match=r"\[0, 64\]"):
        call(k_neg=65)
    with pytest.raises(_lib.VoicemapHipError, match=r"\[0, 64\]"):
        call(k_pos=65)
    with pytest.raises(_lib.VoicemapHipError, match="both zero"):
        call(k_neg=0, k_pos=0, ni=None, nv=None, pi=None, pv=None)
    with pytest.raises(_lib.VoicemapHipError, match="E <= 256"):
        call(E=257)
    with pytest.raises(_lib.VoicemapHipError, match="neg_idx and neg_val"):
        call(ni=None)                      # an output pair is optional only as a pair, together with its k = 0
    with pytest.raises(_lib.VoicemapHipError, match="pos_idx and pos_val"):
        call(k_pos=0)
    with pytest.raises(_lib.VoicemapHipError, match="score_kind"):
        call(kind=3)
    with pytest.raises(_lib.VoicemapHipError, match="row range"):
        call(hi=101)
    with pytest.raises(_lib.VoicemapHipError, match="16-byte aligned"):
        call(emb=20)


def test_script_flags_default_to_off():
    sys.path.insert(0, ROOT)
    from experiments import _common as C
    a = C.base_parser("x").parse_args([])
    assert (a.hard_fraction, a.mine_k_neg, a.mine_k_pos, a.mine_every, a.semi_hard) == (0.0, 8, 4, 1, False)
    a = C.base_parser("x").parse_args(["--hard-fraction", "0.5", "--semi-hard", "--mine-every", "2", "--mine-k-neg", "16"])
    assert (a.hard_fraction, a.mine_k_neg, a.mine_every, a.semi_hard) == (0.5, 16, 2, True)
    ds = _dataset()
    batches, cbs = C.mined_batches(C.base_parser("x").parse_args([]), ds, None, device=False)
    assert batches is None and cbs == []   # off: the scripts keep the dataset's own generator
