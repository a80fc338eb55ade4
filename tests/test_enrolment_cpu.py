"""CPU checks of speaker models (voicemap_amd/enrolment.py): the float64 numpy twins against the oracle's n-shot prediction and against
literal re-summing, the trial order on hand-made scores, the exact sweep on model trials, and the argument checks of the new entry points
(no GPU: nothing is launched)."""
import numpy as np
import pytest

from oracle import voicemap_oracle as O
from voicemap_amd import _lib
from voicemap_amd import enrolment as EN
from voicemap_amd import verification as V

DISTANCES = ["euclidean", "cosine", "dot_product"]


def _corpus(seed, counts, E=24, noise=0.7):
    r = np.random.default_rng(seed)
    label = np.repeat(np.arange(len(counts)), counts)
    r.shuffle(label)
    cent = r.normal(0, 1, (len(counts), E))
    emb = (cent[label] + r.normal(0, noise, (len(label), E))).astype(np.float32)
    return emb, label.astype(np.int32)


@pytest.mark.parametrize("distance", DISTANCES)
def test_twin_scores_equal_the_oracle_n_shot_prediction(distance):
    r = np.random.default_rng(3)
    for k, n, E in ((2, 1, 8), (5, 1, 64), (5, 5, 64), (20, 3, 33), (7, 10, 100)):
        support = r.normal(0, 1, (k * n, E)).astype(np.float32)
        q = r.normal(0, 1, (3, E)).astype(np.float32)
        label = np.repeat(np.arange(k), n)
        got, trial = EN.trial_scores_numpy(support, label, q, np.full(3, -1), distance, False)
        assert trial.all()
        for m in range(3):
            ref = O.n_shot_prediction(q[m], support, n, k, distance)
            assert np.all(np.abs(got[m] - ref) <= 1e-12 * np.maximum(np.abs(ref), 1.0)), (k, n, E)


@pytest.mark.parametrize("distance", DISTANCES)
def test_leave_one_out_twin_is_the_speaker_re_summed_without_the_row(distance):
    emb, label = _corpus(5, [1, 2, 3, 9, 17, 4])
    got, trial = EN.trial_scores_numpy(emb, label, emb, label, distance, True)
    full, trial_full = EN.trial_scores_numpy(emb, label, emb, label, distance, False)
    assert trial_full.all()
    for m in range(len(label)):
        others = np.arange(len(label)) != m
        lab = label[others]
        ref, tr = EN.trial_scores_numpy(emb[others], lab, emb[m:m + 1], [-1], distance, False, S=6)
        if label[m] == 0:   # the one-file speaker: no model is left, no trial
            assert not trial[m, 0] and not tr[0, 0] and np.isnan(got[m, 0])
        else:
            assert trial[m].all() and tr.all()
        ok = trial[m]
        assert np.array_equal(ok, tr[0])
        assert np.all(np.abs(got[m, ok] - ref[0, ok]) <= 1e-12 * np.maximum(np.abs(ref[0, ok]), 1.0)), m
        # only the own speaker's model differs from the shared one
        rest = np.arange(6) != label[m]
        assert np.array_equal(got[m, rest], full[m, rest])


def test_speaker_sums_twin_counts_and_ignores_unenrolled_rows():
    emb, label = _corpus(6, [3, 1, 5])
    label[2] = -1
    for kind in (0, 1, 2):
        sums, msum, count = EN.speaker_sums_numpy(emb, label, 4, kind)
        assert list(count) == [int((label == s).sum()) for s in range(4)] and count[3] == 0
        mag = np.linalg.norm(emb.astype(np.float64), axis=1)
        c = emb.astype(np.float64) if kind == 0 else emb / mag[:, None]
        for s in range(3):
            np.testing.assert_allclose(sums[s], c[label == s].sum(0), rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(msum[s], mag[label == s].sum(), rtol=1e-13)
        assert not sums[3].any()


def test_ranks_follow_the_key_then_index_order_with_ties_signed_zero_and_nan():
    nan = np.nan
    row = np.array([1.0, 1.0, -0.0, 0.0, nan, nan, 0.5])
    # order: 2 (-0.0 == +0.0, lower index), 3, 6, 0, 1, then the NaN by index: 4, 5
    order = [2, 3, 6, 0, 1, 4, 5]
    scores = np.tile(row, (8, 1))
    q_label = np.array([0, 1, 2, 3, 4, 5, 6, -1])
    trial = np.ones_like(scores, dtype=bool)
    r = EN.ranks_numpy(scores, trial, q_label)
    assert list(r["rank"]) == [order.index(s) for s in range(7)] + [-1]
    assert list(r["best_idx"]) == [2] * 8
    assert np.signbit(r["best_val"][0]) and r["best_val"][0] == 0.0
    assert np.array_equal(np.isnan(r["true_score"]), np.array([0, 0, 0, 0, 1, 1, 0, 1], bool))
    # cells that are no trial are in no order: not counted before anyone, never the best, and an own cell without a model is unranked
    trial[:, 2] = False
    r = EN.ranks_numpy(scores, trial, q_label)
    order = [3, 6, 0, 1, 4, 5]
    assert list(r["rank"]) == [order.index(0), order.index(1), -1, 0, order.index(4), order.index(5), order.index(6), -1]
    assert list(r["best_idx"]) == [3] * 8 and not np.signbit(r["best_val"][0])
    assert np.isnan(r["true_score"][2])
    # a row without any trial; a row of NaN only
    r = EN.ranks_numpy(np.array([[1.0, 2.0], [nan, nan]]), np.array([[False, False], [True, True]]), np.array([0, 1]))
    assert list(r["best_idx"]) == [-1, 0] and list(r["rank"]) == [-1, 1] and np.isnan(r["best_val"]).all()
    # negative scores order below positive ones (dot_product)
    r = EN.ranks_numpy(np.array([[-1.0, -3.0, 2.0, -3.0]]), np.ones((1, 4), bool), np.array([0]))
    assert r["rank"][0] == 2 and r["best_idx"][0] == 1


@pytest.mark.parametrize("distance", DISTANCES)
def test_exact_sweep_on_model_trials_equals_the_sorted_definition(distance):
    """M x S trials with a 1 : (S - 1) class imbalance, leave-one-out (the one-file speaker's own cell is no trial)."""
    emb, label = _corpus(7, [1, 6, 9, 14, 20, 25, 30, 12, 8, 11, 16, 21], E=16, noise=1.2)
    sc, trial = EN.trial_scores_numpy(emb, label, emb, label, distance, True)
    target = label[:, None] == np.arange(sc.shape[1])[None, :]
    s32, tg = sc[trial].astype(np.float32), target[trial]
    assert tg.sum() == len(label) - 1 and (~tg).sum() == len(label) * 11
    ref = V.sorted_metrics(s32, tg)
    lo, hi = float(s32.min()), float(s32.max())
    got = V.exact_sweep(lambda wins, bins: V.bin_scores(s32, tg, wins, bins), V.pass1_window(lo, hi))
    for k in ("eer", "eer_threshold", "far_at_eer", "frr_at_eer", "best_balanced_accuracy", "best_threshold", "n_target", "n_nontarget",
              "n_nan"):
        assert got[k] == ref[k], k
    assert 0.0 < got["eer"] < 0.5


def test_argument_errors_of_the_new_entry_points_are_reported_without_a_gpu():
    lib = _lib.lib()
    one = 16   # any non-null, 16-byte aligned address: the checks return before anything is read or launched
    cases = [
        ("vm_speaker_sums", (None, one, 4, 8, 2, 0, one, one, one, one, None), "null pointer"),
        ("vm_speaker_sums", (one, one, 4, 257, 2, 0, one, one, one, one, None), "E must be"),
        ("vm_speaker_sums", (one, one, 4, 8, 2, 3, one, one, one, one, None), "unknown kind"),
        ("vm_speaker_identify", (one, None, 4, 8, one, one, one, 2, 0, 0, None, one, one, one, one, one, None), "null pointer"),
        ("vm_speaker_identify", (one, one, 4, 0, one, one, one, 2, 0, 0, None, one, one, one, one, one, None), "E must be"),
        ("vm_speaker_identify", (one, one, 4, 8, one, one, one, 2, -1, 0, None, one, one, one, one, one, None), "unknown kind"),
        ("vm_speaker_identify", (one, one, 4, 8, one, one, one, 2, 0, 0, None, None, one, one, one, one, None), "null pointer"),
        ("vm_speaker_trial_hist", (one, one, 4, 8, one, one, one, 2, 0, 0, None, 1, 16, one, one, None), "null pointer"),
        ("vm_speaker_trial_hist", (one, one, 4, 300, one, one, one, 2, 0, 0, one, 1, 16, one, one, None), "E must be"),
        ("vm_speaker_trial_hist", (one, one, 4, 8, one, one, one, 2, 7, 0, one, 1, 16, one, one, None), "unknown kind"),
    ]
    for name, args, text in cases:
        with pytest.raises(_lib.VoicemapHipError) as e:
            lib.call(name, *args)
        assert text in str(e.value), (name, str(e.value))
    win = np.array([[0, 0]] * 5, dtype=np.int64)
    with pytest.raises(_lib.VoicemapHipError) as e:   # the window / bin limits of vm_pair_score_hist
        lib.call("vm_speaker_trial_hist", one, one, 4, 8, one, one, one, 2, 0, 0, win.ctypes.data, 5, 16, one, one, None)
    assert "windows" in str(e.value)
    with pytest.raises(_lib.VoicemapHipError) as e:
        lib.call("vm_speaker_trial_hist", one, one, 4, 8, one, one, one, 2, 0, 0, win.ctypes.data, 1, 5000, one, one, None)
    assert "LDS words" in str(e.value)
    assert lib.query("vm_speaker_identify_workspace_bytes", 1000, 64, 40) >= 40 * 64 * 8 + 1000 * 12
    assert lib.query("vm_speaker_sums_workspace_bytes", 1000, 64, 40) >= 8000


def test_enrol_labels_and_per_speaker_choice_need_no_gpu_to_define(monkeypatch):
    """``enrol``'s host side: dense labels from np.unique, a seeded choice of n rows per speaker, all but one for a short speaker."""
    import torch
    from voicemap_amd.retrieval import EmbeddingCache
    emb, label = _corpus(9, [1, 2, 3, 6, 10], E=8)
    codes = np.array([40, 7, 19, 3, 88])[label]
    cache = EmbeddingCache(torch.as_tensor(emb), codes)
    seen = {}

    def fake_sums(e, lab, S, kind):
        seen["label"], seen["S"] = lab.numpy().copy(), S
        return [torch.as_tensor(a) for a in EN.speaker_sums_numpy(e.numpy(), lab.numpy(), S, kind)]
    monkeypatch.setattr(EN, "speaker_sums", fake_sums)
    m = EN.enrol(cache, "cosine")
    assert list(m.speakers) == [3, 7, 19, 40, 88] and seen["S"] == 5
    assert np.array_equal(m.speakers[seen["label"]], codes)
    assert list(m.labels_of([88, 5, 3])) == [4, -1, 0]
    m3 = EN.enrol(cache, "cosine", per_speaker=3, seed=1)
    lab = seen["label"]
    by_code = {c: int((lab[codes == c] >= 0).sum()) for c in (40, 7, 19, 3, 88)}   # sizes 1, 2, 3, 6, 10
    assert by_code == {40: 0, 7: 1, 19: 2, 3: 3, 88: 3}
    assert np.array_equal(lab[lab >= 0], m.label[lab >= 0])
    EN.enrol(cache, "cosine", per_speaker=3, seed=1)
    assert np.array_equal(seen["label"], lab) and np.array_equal(m3.label, lab)
    idx, q_label, loo = EN._queries(m3, cache, None)
    assert np.array_equal(idx, np.flatnonzero(lab < 0)) and loo is False and len(idx) == len(lab) - 9
    assert EN._queries(m, cache, None)[2] is True
