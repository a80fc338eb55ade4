"""Closed-set speaker identification and model-trial verification of a trained siamese network: enrol every speaker of a set as a
speaker model (voicemap_amd/enrolment.py: the reference's n-shot prototypes with k = every speaker), name the speaker of every utterance
and verify every utterance against every model.  Prints one JSON line: rank-1 / rank-5 accuracy, mean reciprocal rank, the model-trial
EER and thresholds.
    python -m experiments.speaker_identification --siamese models/x.hdf5 [--enrol-set dev-clean] [--test-set test-clean]
        [--per-speaker N] [--distance euclidean|cosine|dot_product] [--whole-utterance] [--synthetic]
        [--vad --vad-threshold-db 25 --vad-hang 10 --vad-min-run 3 --vad-frame-ms 10]
        [--backend plda --plda-train train|validation --plda-train-set train-clean-100 --lda-dim D --no-length-norm]
        [--score-norm none|s-norm|as-norm --cohort-set train-clean-100 --cohort-size 5000 --top-k 300]
        [--dcf P[,CMISS,CFA] ...] [--calibrate --calib-prior 0.5]
Without --test-set (or with the same set) the enrolled set is also the test set: leave-one-out (every utterance is scored against its own
speaker's model built from the speaker's OTHER utterances), or with --per-speaker N a seeded choice of N utterances per speaker is
enrolled and the others are the queries.  With another --test-set its utterances are scored against the enrolled set's models (its
speakers that were not enrolled give non-target trials only), and the best threshold of the enrolled set is applied to it.  Under
torchrun the query rows are sharded like the other evaluation scripts.  With --vad the pauses are trimmed out of every file first
(voicemap_amd/vad.py); the trimming summary is printed and joins the row.
--backend plda (off by default) puts a PLDA back end (voicemap_amd/plda.py) in front, as experiments/verification_accuracy.py does: it is
fitted on the training set (--plda-train train: --plda-train-set, a further generated set with --synthetic) or on the enrolled set itself
(--plda-train validation), both sets are projected by it, and every speaker model is scored by the book from ALL its enrolment rows
(multi-session PLDA, enrolment.enrol(plda=...)); --distance is then not used and the row says distance "plda".
--score-norm s-norm / as-norm (off by default; the options of experiments/verification_accuracy.py) normalises the model-trial scores
against a cohort (enrolment.model_score_norm): a seeded random subset of --cohort-set's files (a third generated set with --synthetic),
as-norm over the --top-k most alike per side; with --backend plda the cohort is projected by the same model.  The trial figures and
thresholds of the row are then those of the normalised scores and the row gains score_norm / top_k / cohort_size; the identification
figures rank by the raw score.  Without it the printed row is what it was.
--dcf P[,CMISS,CFA] (repeatable, off by default; the option of experiments/verification_accuracy.py) adds the exact minimum detection
cost of the row's model trials at each operating point (trial_min_dcf_<point>, with its threshold).  --calibrate [--calib-prior P]
(off by default) needs a --test-set other than the enrolled set -- a calibration is fitted on other data than it is judged on -- and
fits llr = a s + b (enrolment.fit_model_calibration) on the enrolled set's own leave-one-out (or --per-speaker) trials, the trials
enrol_best_threshold comes from; the row gains calib_a / calib_b / calib_prior / calib_converged / calib_iterations / calib_passes, Cllr
of both sets (enrol_cllr, test_cllr) and per --dcf point (without one: (P, 1, 1) at the calibration prior) the test set's actDCF at the
Bayes threshold, that threshold and FAR / FRR there, beside the minimum.  With --backend plda the scores calibrated are the PLDA
scores; with --score-norm the normalised ones (the fit uses the enrolled set's statistics, the test figures the test set's).  Under
leave-one-out the fit's models hold n - 1 rows of a speaker and the test's hold all n: the calibration moves between models of
slightly different sizes, exactly as the threshold transfer above already does.  A fitted slope a >= 0 has no Bayes threshold in
score units: the script says "no actDCF" and the minimum costs stand alone.  Without these options the printed row is what it was."""
import argparse
import json

from experiments.verification_accuracy import parse_dcf, point_name
from voicemap_amd import enrolment, retrieval, verification
from voicemap_amd.librispeech import LibriSpeechDataset, SyntheticSpeechDataset
from voicemap_amd.utils import BatchPreProcessor, preprocess_instances
from voicemap_amd.vad import add_vad_args, policy_from_args


def evaluate(net, enrol_set, test_set, pre, distance="euclidean", per_speaker=None, whole_utterance=False, seed=0, vad=None,
             backend="none", plda_train=None, lda_dim=None, length_norm=True, score_norm="none", cohort=None, top_k=300, dcf=(),
             calibrate=False, calib_prior=0.5):
    """The result row: identification and model-trial figures of ``test_set`` (None: the enrolled set itself) against the models of
    ``enrol_set``.  ``vad`` (a ``vad.VadPolicy``): both sets are embedded with their pauses trimmed out.  ``backend`` "plda": a
    ``plda.PldaModel`` is fitted on the embeddings of ``plda_train`` (a dataset; None: the enrolled set) with ``lda_dim`` /
    ``length_norm``, both sets are projected by it and the models are multi-session PLDA models (``distance`` is not used).
    ``score_norm`` "s-norm" / "as-norm": the model trials are normalised against the embeddings of ``cohort`` (a dataset; projected by
    the back end where there is one), as-norm over the ``top_k`` most alike per side.  ``dcf``: detection-cost points for the row's
    trials; ``calibrate`` (needs a ``test_set``): fit llr = a s + b on the enrolled set's own trials at ``calib_prior`` and report Cllr
    and, per point, actDCF on the test set (module docstring)."""
    dcf = verification.as_dcf_points(dcf)
    if calibrate and test_set is None:
        raise ValueError("calibrate needs a test set other than the enrolled set")
    if calibrate and not dcf:
        dcf = [(float(calib_prior), 1.0, 1.0)]
    wu = {"whole_utterance": True} if whole_utterance else {}
    if vad is not None:
        wu["vad"] = vad
    ce = retrieval.embed_corpus(net, enrol_set, pre, "siamese", **wu)
    back = None
    if backend == "plda":
        from voicemap_amd import plda
        back = plda.fit_plda(ce if plda_train is None else retrieval.embed_corpus(net, plda_train, pre, "siamese", **wu), lda_dim=lda_dim,
                             length_norm=length_norm)
        ce, distance = back.project(ce), "plda"
        models = enrolment.enrol(ce, per_speaker=per_speaker, seed=seed, plda=back)
    elif backend != "none":
        raise ValueError("backend must be none or plda")
    else:
        models = enrolment.enrol(ce, distance, per_speaker=per_speaker, seed=seed)
    ct = ce if test_set is None else retrieval.embed_corpus(net, test_set, pre, "siamese", **wu)
    if back is not None and test_set is not None:
        ct = back.project(ct)
    ident = enrolment.identify(models, ct)
    cc, k, nt = None, None, None
    if score_norm != "none":
        cc = retrieval.embed_corpus(net, cohort, pre, "siamese", **wu)
        if back is not None:
            cc = back.project(cc)
        k = None if score_norm == "s-norm" else top_k
        nt = enrolment.model_score_norm(models, ct, cc, top_k=k)
    mt = enrolment.model_trial_metrics(models, ct, dcf_points=dcf, norm=nt)
    cmc = ident["cmc"]
    row = {"distance": distance, "speakers": models.S, "per_speaker": per_speaker, "leave_one_out": ident["leave_one_out"],
           "queries": ident["n_queries"], "unranked": ident["n_unranked"], "rank1_accuracy": ident["rank1_accuracy"],
           "rank5_accuracy": float(cmc[min(5, len(cmc)) - 1]), "mean_reciprocal_rank": ident["mean_reciprocal_rank"],
           "trial_eer": mt["eer"], "trial_eer_threshold": mt["eer_threshold"], "trial_best_balanced_accuracy": mt["best_balanced_accuracy"],
           "trial_best_threshold": mt["best_threshold"], "target_trials": mt["n_target"], "nontarget_trials": mt["n_nontarget"],
           "whole_utterance": bool(whole_utterance)}
    if test_set is not None:   # the enrolled set's own threshold applied to the test set, as verification_accuracy.py does for pairs
        ne = enrolment.model_score_norm(models, ce, cc, top_k=k) if cc is not None else None
        me = enrolment.model_trial_metrics(models, ce, norm=ne)
        at = enrolment.model_trial_accuracy_at_threshold(models, ct, me["best_threshold"], norm=nt)
        row.update(enrol_best_threshold=me["best_threshold"], test_balanced_accuracy_at_enrol_threshold=at["balanced_accuracy"],
                   test_far=at["far"], test_frr=at["frr"])
    costs = mt.get("dcf", [])
    if calibrate:   # fitted on the enrolled set's own trials (ne), judged on the test set's (nt)
        cal = enrolment.fit_model_calibration(models, ce, prior=calib_prior, norm=ne)
        row.update(calib_a=cal.a, calib_b=cal.b, calib_prior=cal.prior, calib_converged=cal.converged, calib_iterations=cal.iterations,
                   calib_passes=cal.passes, enrol_cllr=cal.cllr_train, test_cllr=enrolment.model_cllr(models, ct, cal, norm=nt))
        try:
            costs = enrolment.model_detection_costs(models, ct, cal, dcf, norm=nt, metrics=mt)
        except ValueError as e:   # a >= 0: there is no Bayes threshold in score units; the minimum costs stand alone
            print("--calibrate: no actDCF:", e)
    for d in costs:
        name = point_name((d["p_target"], d["c_miss"], d["c_fa"]))
        row["trial_min_dcf_" + name], row["trial_min_dcf_threshold_" + name] = d["min_dcf"], d["min_dcf_threshold"]
        if calibrate:
            nan = float("nan")
            row.update({"test_act_dcf_" + name: d.get("act_dcf", nan), "test_act_threshold_" + name: d.get("act_threshold", nan),
                        "test_far_at_act_" + name: d.get("far_at_act", nan), "test_frr_at_act_" + name: d.get("frr_at_act", nan)})
    if back is not None:
        row.update(backend="plda", plda_dim=back.D, lda_dim=back.A1.shape[0], length_norm=back.length_norm,
                   plda_train="validation" if plda_train is None else "train", model_rows_max=models.n_max)
    if score_norm != "none":
        row.update(score_norm=score_norm, top_k=top_k if score_norm == "as-norm" else None, cohort_size=len(cohort))
    if vad is not None:
        from voicemap_amd.vad import summarise
        summary = summarise([c.vad_counts for c in ((ce,) if test_set is None else (ce, ct)) + ((cc,) if cc is not None else ())])
        print("--vad:", summary)
        row.update({"vad_" + k: v for k, v in summary.items()})
    return row


def _parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--siamese", default=None, help="a saved siamese network (not needed with --synthetic)")
    p.add_argument("--enrol-set", default="dev-clean")
    p.add_argument("--test-set", default=None, help="default: the enrolled set itself (leave-one-out, or the rows --per-speaker left out)")
    p.add_argument("--per-speaker", type=int, default=None, help="enrol a seeded choice of N utterances per speaker")
    p.add_argument("--distance", default="euclidean", choices=["euclidean", "cosine", "dot_product"])
    p.add_argument("--n-seconds", type=float, default=3)
    p.add_argument("--downsampling", type=int, default=4)
    p.add_argument("--whole-utterance", action="store_true", help="embed every file whole, at its own length")
    p.add_argument("--synthetic", action="store_true", help="generated speaker sets and a freshly built model")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--backend", default="none", choices=["none", "plda"], help="a trained back end in front of the models (off by default)")
    p.add_argument("--plda-train", default="train", choices=["train", "validation"], help="the set the PLDA back end is fitted on")
    p.add_argument("--plda-train-set", default="train-clean-100", help="the training subset of --plda-train train")
    p.add_argument("--lda-dim", type=int, default=None, help="LDA directions kept in front of PLDA (default: all)")
    p.add_argument("--no-length-norm", action="store_true", help="no length normalisation between LDA and PLDA")
    p.add_argument("--score-norm", default="none", choices=["none", "s-norm", "as-norm"], help="cohort score normalisation of the model trials")
    p.add_argument("--cohort-set", default="train-clean-100", help="the cohort's subset (a third generated set with --synthetic)")
    p.add_argument("--cohort-size", type=int, default=5000, help="files of the cohort set taken (seeded random subset)")
    p.add_argument("--top-k", type=int, default=300, help="as-norm: cohort models / rows per side")
    p.add_argument("--dcf", action="append", default=[], type=parse_dcf, metavar="P[,CMISS,CFA]",
                   help="a detection-cost operating point for the model trials (repeatable)")
    p.add_argument("--calibrate", action="store_true", help="fit llr = a s + b on the enrolled set's trials; Cllr and actDCF on --test-set")
    p.add_argument("--calib-prior", type=float, default=0.5, help="the target prior of the calibration fit")
    add_vad_args(p)   # --vad ...: off by default; every set embedded, the cohort included, is trimmed first
    return p


def main(argv=None):
    p = _parser()
    a = p.parse_args(argv)
    vad = policy_from_args(a)
    same = a.test_set is None or a.test_set == a.enrol_set
    if a.calibrate and same:
        p.error("--calibrate needs a --test-set other than the enrolled set: a calibration is judged on other data than it is fitted on")
    from experiments._common import setup
    rank, _ = setup()
    if a.synthetic:
        from voicemap_amd import models
        enrol_set = SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=a.n_seconds, stochastic=False, seed=1,
                                           subset="synthetic-enrol")
        test_set = None if same else SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=a.n_seconds, stochastic=False,
                                                            seed=1, subset="synthetic-test")
        if a.siamese:
            net = models.load_model(a.siamese)
        else:
            enc = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
            net = models.build_siamese_net(enc, (int(a.n_seconds * 16000) // a.downsampling, 1), distance_metric="uniform_euclidean")
    else:
        from voicemap_amd.models import load_model
        if not a.siamese:
            p.error("--siamese is required without --synthetic")
        net = load_model(a.siamese)
        enrol_set = LibriSpeechDataset(a.enrol_set, a.n_seconds, stochastic=False)
        test_set = None if same else LibriSpeechDataset(a.test_set, a.n_seconds, stochastic=False)
    plda_train = None
    if a.backend == "plda" and a.plda_train == "train":
        plda_train = (SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=a.n_seconds, stochastic=False, seed=4,
                                             subset="synthetic-train")
                      if a.synthetic else LibriSpeechDataset(a.plda_train_set, a.n_seconds, stochastic=False))
    cohort = None
    if a.score_norm != "none":
        from experiments.verification_accuracy import cohort_subset
        cohort = cohort_subset(SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=a.n_seconds, stochastic=False, seed=3,
                                                      subset="synthetic-cohort")
                               if a.synthetic else LibriSpeechDataset(a.cohort_set, a.n_seconds, stochastic=False), a.cohort_size)
    pre = BatchPreProcessor("siamese", preprocess_instances(a.downsampling))
    row = evaluate(net, enrol_set, test_set, pre, a.distance, a.per_speaker, a.whole_utterance, a.seed, vad=vad, backend=a.backend,
                   plda_train=plda_train, lda_dim=a.lda_dim, length_norm=not a.no_length_norm, score_norm=a.score_norm, cohort=cohort,
                   top_k=a.top_k, dcf=a.dcf, calibrate=a.calibrate, calib_prior=a.calib_prior)
    row.update(enrol_set="synthetic" if a.synthetic else a.enrol_set,
               test_set=("synthetic" if a.synthetic else a.enrol_set) if same else a.test_set)
    if rank == 0:
        print(json.dumps(row))
    return row


if __name__ == "__main__":
    main()
