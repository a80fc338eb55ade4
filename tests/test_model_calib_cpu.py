"""CPU checks of the calibration of speaker-model trials (voicemap_amd/enrolment.py model_calib_sums_numpy, fit_model_calibration,
model_cllr, model_detection_costs; vm_[plda_]speaker_trial_calib_sums' argument checks; the options of
experiments/speaker_identification.py).  No GPU: the fit runs through the numpy twin."""
import math
import types

import numpy as np
import pytest

from tests import model_calib_cases as MC
from voicemap_amd import _lib
from voicemap_amd import calibration as C
from voicemap_amd import enrolment as EN
from voicemap_amd import verification as V


@pytest.mark.parametrize("loo", [False, True])
@pytest.mark.parametrize("kind", ["euclidean", "cosine", "dot_product"])
def test_the_twin_equals_a_literal_double_loop(kind, loo):
    emb, label, q, q_label, S = MC.small_corpus()
    scores, trial = EN.trial_scores_numpy(emb, label, q, q_label, kind, loo, S)
    assert not trial[:, 1].any()                                   # the speaker with no rows: never a trial
    assert trial[3, 2] != loo and trial[q_label == 5, 5].all() != loo   # the single-file speakers' own cells, gone under leave-one-out
    s32 = scores.astype(np.float32)
    s32[0, 3] = np.inf                                             # a skipped non-target and a skipped target
    s32[4, 3] = np.nan
    for abt in MC.ABT[:2] + [(0.0, 0.0, 0.0)]:
        got = EN.model_calib_sums_numpy(s32, trial, q_label, *abt)
        ref = MC.literal_sums(s32, trial, q_label, *abt)
        assert np.array_equal(got[:, :2], ref[:, :2]), (got, ref)
        assert got[:, 1].tolist() == [1.0, 1.0]
        assert got[0, 0] == (trial & MC.target_mask(q_label, S)).sum() - 1 and got[:, :2].sum() == trial.sum()
        # the same float64 terms, added in another order: either sum of n <= 55 terms is within (n - 1) u sum|term| of the exact one
        mag = MC.literal_sums(s32, trial, q_label, *abt, magnitude=True)
        assert np.all(np.abs(got[:, 2:] - ref[:, 2:]) <= 2 * 55 * 2.0 ** -53 * mag[:, 2:]), (got, ref)
    # the row labelled -1 has non-target trials only
    only = np.zeros_like(trial)
    only[1] = trial[1]
    assert EN.model_calib_sums_numpy(s32, only, q_label, 0.0, 0.0, 0.0)[0, 0] == 0


class _Models:
    """What the evaluators read of a ``SpeakerModels``, over a planted score matrix."""

    def __init__(self, distance):
        self.distance = distance


def _planted(seed=1, M=400, S=12, shift=2.0):
    """A score matrix whose targets (one per row) sit ``shift`` below the non-targets: both classes overlap, so the fit has a minimiser."""
    r = np.random.default_rng(seed)
    q_label = r.integers(0, S, M)
    tg = MC.target_mask(q_label, S)
    scores = (r.normal(5.0, 1.0, (M, S)) - shift * tg).astype(np.float32)
    trial = r.random((M, S)) > 0.05
    return scores, trial, q_label, tg


@pytest.mark.parametrize("prior", [0.5, 0.05])
def test_the_fit_through_the_twin_ends_where_the_gradient_vanishes(monkeypatch, prior):
    scores, trial, q_label, tg = _planted()
    calls = []

    def source(models, cache, leave_one_out, norm, rows=None):
        calls.append((leave_one_out, norm))
        return lambda a, b, tau: EN.model_calib_sums_numpy(scores, trial, q_label, a, b, tau)
    monkeypatch.setattr(EN, "_calib_source", source)
    models = _Models("cosine")
    cal = EN.fit_model_calibration(models, None, prior=prior)
    assert (cal.trials, cal.score, cal.normalised, cal.prior) == ("model", "cosine", False, prior)
    assert cal.converged and cal.a < 0 and 0 < cal.cllr_train < 1 and cal.passes >= cal.iterations + 2
    Cv, g, H = C.objective_terms(EN.model_calib_sums_numpy(scores, trial, q_label, cal.a, cal.b, C.logit(prior)), prior)
    lam = math.sqrt(C.newton_decrement2(g, H))   # the gradient in the norm of the stopping rule
    assert lam <= cal.stop * math.sqrt(Cv) * (1 + 1e-9) and Cv == cal.objective
    # the same trials as a flat array give the same fit: the model twin is calib_sums_numpy over the set cells
    ref = C.fit_calibration_numpy(scores[trial], tg[trial], prior=prior)
    assert (ref.a, ref.b, ref.iterations) == (cal.a, cal.b, cal.iterations) and ref.trials == "pair"
    assert EN.model_cllr(models, None, cal) == C.cllr_of(EN.model_calib_sums_numpy(scores, trial, q_label, cal.a, cal.b, 0.0)) == cal.cllr_train
    normed = EN.fit_model_calibration(models, None, prior=prior, norm=object(), leave_one_out=True)
    assert normed.normalised and normed.trials == "model" and calls[-1][0] is True and calls[-1][1] is not None


def test_calibrations_of_the_other_trial_kind_are_refused_in_both_directions(monkeypatch):
    pair = C.fit_calibration_numpy(np.array([0.0, 1.0, 2.0, 3.0], np.float32), np.array([1, 1, 0, 1], bool), score="euclidean")
    assert pair.trials == "pair" and C.Calibration(-1.0, 0.0, 0.5, "euclidean", False, 0, True, 0.0, 0.0).trials == "pair"
    model = C.Calibration(-1.0, 0.0, 0.5, "euclidean", False, 0, True, 0.0, 0.0, trials="model")
    with pytest.raises(ValueError, match="model trials, not pair trials"):
        C.cllr(None, model)
    with pytest.raises(ValueError, match="model trials, not pair trials"):
        V.detection_costs(None, model, [0.01])
    models = _Models("euclidean")
    for fn in (lambda c, **k: EN.model_cllr(models, None, c, **k), lambda c, **k: EN.model_detection_costs(models, None, c, [0.01], **k)):
        with pytest.raises(ValueError, match="pair trials, not model trials"):
            fn(pair)
        with pytest.raises(ValueError, match="fitted on 'euclidean' scores, the models score 'cosine'"):
            EN.model_cllr(_Models("cosine"), None, model)
        with pytest.raises(ValueError, match="fitted on raw scores"):
            fn(model, norm=object())
        with pytest.raises(ValueError, match="fitted on normalised scores"):
            fn(C.Calibration(-1.0, 0.0, 0.5, "euclidean", True, 0, True, 0.0, 0.0, trials="model"))
    # a pair calibration without the field (an object of an older shape) still counts as one of pair trials
    old = types.SimpleNamespace(a=0.0, b=0.0, score="euclidean", normalised=False)
    with pytest.raises(ValueError, match="not negative"):
        V.detection_costs(None, old, [0.01])
    flat = C.Calibration(0.0, 0.0, 0.5, "euclidean", False, 0, True, 0.0, 0.0, trials="model")
    with pytest.raises(ValueError, match="not negative"):   # before any pass over the trials
        EN.model_detection_costs(models, None, flat, [0.01])


def test_detection_costs_mirror_the_pair_evaluator(monkeypatch):
    """model_detection_costs on stand-ins for the two passes: the minimum from ``metrics``, the actual cost counted at the Bayes
    threshold in score units."""
    scores, trial, q_label, tg = _planted(seed=3)
    s, t = scores[trial], tg[trial]
    points = [(0.01, 1.0, 1.0), (0.05, 10.0, 1.0)]
    seen = []

    def at_threshold(models, cache, thr, leave_one_out=None, norm=None):
        seen.append(thr)
        return {"far": float((s[~t] < thr).sum()) / (~t).sum(), "frr": float((s[t] >= thr).sum()) / t.sum()}
    monkeypatch.setattr(EN, "model_trial_accuracy_at_threshold", at_threshold)
    monkeypatch.setattr(EN, "model_trial_metrics", lambda models, cache, leave_one_out=None, dcf_points=(), norm=None: {
        "dcf": V.sorted_dcf(s, t, dcf_points)})
    cal = C.fit_calibration_numpy(s, t, prior=0.05, score="euclidean")
    cal.trials = "model"
    costs = EN.model_detection_costs(_Models("euclidean"), None, cal, points)
    assert seen == [V.bayes_threshold(cal, pt) for pt in points]
    for pt, d, ref in zip(points, costs, V.sorted_dcf(s, t, points)):
        assert d["min_dcf"] == ref["min_dcf"] and d["act_threshold"] == V.bayes_threshold(cal, pt)
        assert d["act_dcf"] == V.dcf_value(pt, d["far_at_act"], d["frr_at_act"]) >= d["min_dcf"]
    with pytest.raises(ValueError, match="other detection-cost points"):
        EN.model_detection_costs(_Models("euclidean"), None, cal, points, metrics={"dcf": V.sorted_dcf(s, t, points[:1])})


def test_argument_errors_of_the_new_entry_points_are_reported_without_a_gpu():
    lib = _lib.lib()
    one = 16   # any non-null, 16-byte aligned address: the checks return before anything is read or launched
    nan, inf = float("nan"), float("inf")
    geo = lambda **k: _geo_args(one, **k)
    pl = lambda **k: _plda_args(one, **k)
    cases = [
        ("vm_speaker_trial_calib_sums", geo(q=None), "null pointer"),
        ("vm_speaker_trial_calib_sums", geo(calib=None), "null pointer"),
        ("vm_speaker_trial_calib_sums", geo(ws=None), "null pointer"),
        ("vm_speaker_trial_calib_sums", geo(calib=one + 4), "8-byte aligned"),
        ("vm_speaker_trial_calib_sums", geo(E=257), "E must be"),
        ("vm_speaker_trial_calib_sums", geo(kind=3), "unknown kind"),
        ("vm_speaker_trial_calib_sums", geo(a=nan), "must be finite"),
        ("vm_speaker_trial_calib_sums", geo(b=inf), "must be finite"),
        ("vm_speaker_trial_calib_sums", geo(tau=-inf), "must be finite"),
        ("vm_speaker_trial_calib_sums", geo(stats=(one, None, one, one, None, None)), "null pointer"),       # not NULL all together
        ("vm_speaker_trial_calib_sums", geo(stats=(None, None, None, None, one, one), loo=1), "null pointer"),
        ("vm_speaker_trial_calib_sums", geo(stats=(one, one, one, one, one, None), loo=1), "go together"),
        ("vm_speaker_trial_calib_sums", geo(stats=(one, one, one, one, one, one), loo=0), "must be NULL without leave_one_out"),
        ("vm_speaker_trial_calib_sums", geo(stats=(one, one, one, one, None, None), loo=1), "leave_one_out needs"),
        ("vm_plda_speaker_trial_calib_sums", pl(q=None), "null pointer"),
        ("vm_plda_speaker_trial_calib_sums", pl(calib=None), "null pointer"),
        ("vm_plda_speaker_trial_calib_sums", pl(D=8), "1 <= D < P"),
        ("vm_plda_speaker_trial_calib_sums", pl(n_max=0), "n_max must be"),
        ("vm_plda_speaker_trial_calib_sums", pl(a=nan), "must be finite"),
        ("vm_plda_speaker_trial_calib_sums", pl(stats=(one, one, one, None, None, None)), "null pointer"),
        ("vm_plda_speaker_trial_calib_sums", pl(stats=(one, one, one, one, None, None), loo=1), "leave_one_out needs"),
        ("vm_plda_speaker_trial_calib_sums", pl(stats=(one, one, one, one, one, one), loo=0), "must be NULL without leave_one_out"),
    ]
    for name, args, text in cases:
        with pytest.raises(_lib.VoicemapHipError) as e:
            lib.call(name, *args)
        assert text in str(e.value) and name in str(e.value), (name, text, str(e.value))
    q = lib.query
    assert q("vm_speaker_trial_calib_sums_splits", 0, 5) == 0 == q("vm_speaker_trial_calib_sums_splits", 5, 0)
    assert q("vm_speaker_trial_calib_sums_splits", 2048, 8192) == 64 and q("vm_speaker_trial_calib_sums_splits", 1024, 8192) == 128
    assert q("vm_speaker_trial_calib_sums_splits", 100, 65) == 2 and q("vm_speaker_trial_calib_sums_splits", 1 << 20, 64) == 1
    # the workspace: the histogram's scratch and one column of 16 doubles per workgroup
    for M, E, S in ((2048, 4, 8192), (300, 64, 37), (1, 1, 1)):
        parts = -(-M // 64) * q("vm_speaker_trial_calib_sums_splits", M, S)
        assert q("vm_speaker_trial_calib_sums_workspace_bytes", M, E, S) >= q("vm_speaker_trial_hist_workspace_bytes", M, E, S) + parts * 128
        assert q("vm_plda_speaker_trial_calib_sums_workspace_bytes", M, E, S) >= q("vm_plda_speaker_trial_hist_workspace_bytes", M, E, S) + parts * 128
    assert q("vm_speaker_trial_calib_sums_workspace_bytes", 0, 4, 4) > 0 and q("vm_speaker_trial_calib_sums_workspace_bytes", 4, 0, 4) == 0


def _geo_args(one, q=16, calib=16, ws=16, E=8, kind=0, loo=0, a=-1.0, b=0.0, tau=0.0, stats=(None,) * 6):
    return (q, one, 4, E, one, one, one, 2, kind, loo) + tuple(stats) + (a, b, tau, calib, ws, None)


def _plda_args(one, q=16, calib=16, ws=16, D=7, n_max=3, loo=0, a=-1.0, b=0.0, tau=0.0, stats=(None,) * 6):
    return (q, one, 4, 8, D, one, one, 2, one, one, one, one, n_max, loo) + tuple(stats) + (a, b, tau, calib, ws, None)


def test_the_script_refuses_to_calibrate_on_the_set_it_judges(capsys):
    from experiments import speaker_identification as SI
    for argv in (["--synthetic", "--calibrate"], ["--synthetic", "--calibrate", "--enrol-set", "x", "--test-set", "x"]):
        with pytest.raises(SystemExit) as e:
            SI.main(argv)
        assert e.value.code == 2
        assert "--calibrate needs a --test-set other than the enrolled set" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        SI._parser().parse_args(["--dcf", "1.5"])                 # parse_dcf of verification_accuracy.py: a prior outside (0, 1)
    a = SI._parser().parse_args(["--dcf", "0.01", "--dcf", "0.05,10,1", "--calibrate", "--calib-prior", "0.1", "--test-set", "t"])
    assert a.dcf == [(0.01, 1.0, 1.0), (0.05, 10.0, 1.0)] and a.calibrate and a.calib_prior == 0.1
    with pytest.raises(ValueError, match="calibrate needs a test set"):
        SI.evaluate(None, None, None, None, calibrate=True)


def test_the_script_defaults_leave_evaluate_as_it_was(monkeypatch):
    from experiments import _common
    from experiments import speaker_identification as SI
    import inspect
    a = SI._parser().parse_args([])
    assert (a.dcf, a.calibrate, a.calib_prior) == ([], False, 0.5)
    par = inspect.signature(SI.evaluate).parameters
    assert [(k, par[k].default) for k in list(par)[-3:]] == [("dcf", ()), ("calibrate", False), ("calib_prior", 0.5)]
    seen = {}

    def evaluate(*args, **kwargs):
        seen["args"], seen["kwargs"] = args, kwargs
        return {"row": 1}
    monkeypatch.setattr(SI, "evaluate", evaluate)
    monkeypatch.setattr(_common, "setup", lambda: (1, 1))          # not rank 0: nothing is printed
    monkeypatch.setattr("voicemap_amd.models.get_baseline_convolutional_encoder", lambda *a, **k: None)
    monkeypatch.setattr("voicemap_amd.models.build_siamese_net", lambda *a, **k: "net")
    row = SI.main(["--synthetic", "--n-seconds", "1"])
    assert row == {"row": 1, "enrol_set": "synthetic", "test_set": "synthetic"}
    assert seen["args"][0] == "net" and seen["args"][2] is None and seen["args"][4:] == ("euclidean", None, False, 0)
    k = seen["kwargs"]
    assert (k.pop("dcf"), k.pop("calibrate"), k.pop("calib_prior")) == ([], False, 0.5)   # the new arguments, all off
    assert k == {"vad": None, "backend": "none", "plda_train": None, "lda_dim": None, "length_norm": True, "score_norm": "none",
                 "cohort": None, "top_k": 300}                                            # ... and the ones it had
