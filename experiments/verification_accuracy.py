"""All-pairs speaker verification of a trained siamese network -- the reference's experiments/verification_accuracy.py, a stub whose
docstring "determines the best verification distance threshold on the validation set and then ... uses this to estimate the true
verification accuracy on the test set".  Each set is embedded once (retrieval.embed_corpus: one first-fragment window per file, each
window whitened alone -- the deviation documented there); the best-balanced-accuracy threshold of the validation set's all-pairs trials
is applied to the test set's (voicemap_amd/verification.py).  Results go to logs/verification_accuracy_<valid>_<test>_<score>.csv.
With --score-norm s-norm / as-norm both sets are normalised against the same cohort (a seeded random subset of --cohort-set's files;
as-norm over the --top-k cohort rows most like each row) and the file name gains _<score-norm>[_k<top-k>]_c<cohort-size>.
    python -m experiments.verification_accuracy --siamese models/x.hdf5 [--score euclidean|cosine|dot_product|head] [--synthetic]
        [--score-norm none|s-norm|as-norm --cohort-set train-clean-100 --cohort-size 5000 --top-k 300] [--whole-utterance]
With --whole-utterance every file is embedded whole, at its own length (retrieval.embed_corpus(whole_utterance=True)), and the file
name gains _whole.  With --vad [--vad-threshold-db --vad-hang --vad-min-run --vad-frame-ms] the pauses are trimmed out of every file of
every set first (voicemap_amd/vad.py), the trimming summary is printed and joins the row, and the file name gains _vad.
--dcf P[,CMISS,CFA] (repeatable) adds the test set's exact minimum detection cost at each operating point (columns
test_min_dcf_<point>, with its threshold), and the file name gains _dcf.  --calibrate [--calib-prior P] fits llr = a s + b on the
validation trials (voicemap_amd/calibration.py) and adds Cllr of both sets and, per --dcf point (without one: (P, 1, 1) at the
calibration prior), the test set's actDCF at the Bayes threshold beside its minDCF; the file name gains _calib.
--backend plda [--plda-train train|validation --plda-train-set train-clean-100 --lda-dim D --no-length-norm] puts a PLDA back end
(voicemap_amd/plda.py: LDA, length normalisation, two-covariance PLDA) in front of everything: it is fitted on the training set
(--plda-train train: --plda-train-set, a further generated set with --synthetic) or on the validation set itself, every set and the
cohort are projected by it and scored by minus its log-likelihood ratio (--score is then not used); the file name gains _plda."""
import argparse

import numpy as np
import pandas as pd

from config import PATH
from voicemap_amd import retrieval, verification
from voicemap_amd.librispeech import LibriSpeechDataset, SyntheticSpeechDataset
from voicemap_amd.utils import BatchPreProcessor, preprocess_instances
from voicemap_amd.vad import add_vad_args, policy_from_args


class CohortSubset:
    """The files ``index`` of a dataset, in that order, as far as ``retrieval.embed_corpus`` reads a dataset."""

    def __init__(self, dataset, index):
        self.base, self.index = dataset, np.asarray(index, dtype=np.int64)
        self.fragment_length, self.pad = dataset.fragment_length, dataset.pad
        self._code = np.asarray(dataset._code)[self.index]

    def __len__(self):
        return len(self.index)

    def _load(self, i):
        return self.base._load(int(self.index[i]))


def cohort_subset(dataset, size, seed=0):
    """A seeded random subset of ``size`` files of ``dataset`` (all of them if it has fewer), in file order."""
    n = len(dataset)
    if size >= n:
        return CohortSubset(dataset, np.arange(n))
    return CohortSubset(dataset, np.sort(np.random.default_rng(seed).choice(n, size, replace=False)))


def point_name(pt):
    """Column suffix of a detection-cost point: p0.01, or p0.05_cm10_cf1 with costs other than 1."""
    return "p%g" % pt[0] + ("" if (pt[1], pt[2]) == (1.0, 1.0) else "_cm%g_cf%g" % (pt[1], pt[2]))


def parse_dcf(text):
    """P or P,CMISS,CFA -> (P, C_miss, C_fa)."""
    try:
        v = [float(x) for x in text.split(",")]
        return verification.as_dcf_points([v[0] if len(v) == 1 else tuple(v)])[0]
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def evaluate(net, valid, test, pre, score="euclidean", score_norm="none", cohort=None, top_k=300, whole_utterance=False, vad=None,
             dcf=(), calibrate=False, calib_prior=0.5, backend="none", plda_train=None, lda_dim=None, length_norm=True):
    """Embed both sets once, take the best-balanced-accuracy threshold of the validation trials and apply it to the test trials.
    ``score_norm`` "s-norm" / "as-norm": both sets' scores are normalised against the embeddings of ``cohort`` (a dataset).
    ``vad`` (a ``vad.VadPolicy``): every set, the cohort included, is embedded with its pauses trimmed out.
    ``dcf``: detection-cost points for the test set; ``calibrate``: fit llr = a s + b on the validation trials at ``calib_prior`` and
    report Cllr and, per point, actDCF on the test set (module docstring).
    ``backend`` "plda": a ``plda.PldaModel`` is fitted on the embeddings of ``plda_train`` (a dataset; None: the validation set) with
    ``lda_dim`` / ``length_norm``, every set and the cohort are projected by it and the score is "plda"."""
    dcf = verification.as_dcf_points(dcf)
    if calibrate and not dcf:
        dcf = [(float(calib_prior), 1.0, 1.0)]
    model = net if score == "head" else None
    wu = {"whole_utterance": True} if whole_utterance else {}
    if vad is not None:
        wu["vad"] = vad
    cv = retrieval.embed_corpus(net, valid, pre, "siamese", **wu)
    ct = retrieval.embed_corpus(net, test, pre, "siamese", **wu)
    back = None
    if backend == "plda":
        from voicemap_amd import plda
        back = plda.fit_plda(cv if plda_train is None else retrieval.embed_corpus(net, plda_train, pre, "siamese", **wu), lda_dim=lda_dim,
                             length_norm=length_norm)
        cv, ct, score, model = back.project(cv), back.project(ct), "plda", None
    elif backend != "none":
        raise ValueError("backend must be none or plda")
    nv = nt = None
    if score_norm != "none":
        cc = retrieval.embed_corpus(net, cohort, pre, "siamese", **wu)
        if back is not None:
            cc = back.project(cc)
        k = None if score_norm == "s-norm" else top_k
        nv = verification.score_norm(cv, cc, score, top_k=k, model=model)
        nt = verification.score_norm(ct, cc, score, top_k=k, model=model)
    mv = verification.verification_metrics(cv, score, model=model, norm=nv)
    mt = verification.verification_metrics(ct, score, model=model, norm=nt, dcf_points=dcf)
    at = verification.accuracy_at_threshold(ct, mv["best_threshold"], score, model=model, norm=nt)
    row = {"score": score, "threshold": mv["best_threshold"], "valid_balanced_accuracy": mv["best_balanced_accuracy"],
           "valid_eer": mv["eer"], "valid_eer_threshold": mv["eer_threshold"], "test_balanced_accuracy": at["balanced_accuracy"],
           "test_far": at["far"], "test_frr": at["frr"], "test_eer": mt["eer"], "test_eer_threshold": mt["eer_threshold"],
           "valid_pairs": mv["n_target"] + mv["n_nontarget"], "test_pairs": mt["n_target"] + mt["n_nontarget"]}
    if "best_threshold_p" in mv:
        row["threshold_p"] = mv["best_threshold_p"]
    costs = mt.get("dcf", [])
    if calibrate:
        from voicemap_amd import calibration
        cal = calibration.fit_calibration(cv, prior=calib_prior, score=score, model=model, norm=nv)
        row.update(calib_a=cal.a, calib_b=cal.b, calib_prior=cal.prior, calib_converged=cal.converged, calib_iterations=cal.iterations,
                   calib_passes=cal.passes, valid_cllr=cal.cllr_train, test_cllr=calibration.cllr(ct, cal, model=model, norm=nt))
        try:
            costs = verification.detection_costs(ct, cal, dcf, model=model, norm=nt, metrics=mt)
        except ValueError as e:   # a >= 0: there is no Bayes threshold in score units; the minimum costs stand alone
            print("--calibrate: no actDCF:", e)
    for d in costs:
        name = point_name((d["p_target"], d["c_miss"], d["c_fa"]))
        row["test_min_dcf_" + name], row["test_min_dcf_threshold_" + name] = d["min_dcf"], d["min_dcf_threshold"]
        if calibrate:
            row["test_act_dcf_" + name] = d.get("act_dcf", float("nan"))
            row["test_act_threshold_" + name] = d.get("act_threshold", float("nan"))
    if back is not None:
        row.update(backend="plda", plda_dim=back.D, lda_dim=back.A1.shape[0], length_norm=back.length_norm,
                   plda_train="validation" if plda_train is None else "train")
    if whole_utterance:
        row["whole_utterance"] = True
    if score_norm != "none":
        row.update(score_norm=score_norm, top_k=top_k if score_norm == "as-norm" else None, cohort_size=len(cohort))
    if vad is not None:
        from voicemap_amd.vad import summarise
        summary = summarise([c.vad_counts for c in (cv, ct) + ((cc,) if score_norm != "none" else ())])
        print("--vad:", summary)
        row.update({"vad_" + k: v for k, v in summary.items()})
    return row


def result_name(a):
    """logs/ file name of a run (``a``: the parsed arguments)."""
    name = "verification_accuracy_{}_{}_{}".format("synthetic" if a.synthetic else a.validation_set,
                                                   "synthetic" if a.synthetic else a.test_set,
                                                   "plda" if getattr(a, "backend", "none") == "plda" else a.score)
    if a.score_norm != "none":
        name += "_" + a.score_norm.replace("-", "") + ("_k%d" % a.top_k if a.score_norm == "as-norm" else "") + "_c%d" % a.cohort_size
    if getattr(a, "whole_utterance", False):
        name += "_whole"
    if getattr(a, "vad", False):
        name += "_vad"
    if getattr(a, "dcf", None):
        name += "_dcf"
    if getattr(a, "calibrate", False):
        name += "_calib"
    return name + ".csv"


def parse_args(argv=None):
    return _parser().parse_args(argv)


def _parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--siamese", default=None, help="a saved siamese network (not needed with --synthetic)")
    p.add_argument("--validation-set", default="dev-clean")
    p.add_argument("--test-set", default="test-clean")
    p.add_argument("--n-seconds", type=float, default=3)
    p.add_argument("--downsampling", type=int, default=4)
    p.add_argument("--score", default="euclidean", choices=["euclidean", "cosine", "dot_product", "head"])
    p.add_argument("--synthetic", action="store_true", help="two generated speaker sets and a freshly built model")
    p.add_argument("--score-norm", default="none", choices=["none", "s-norm", "as-norm"], help="cohort score normalisation")
    p.add_argument("--cohort-set", default="train-clean-100", help="the cohort's subset (a third generated set with --synthetic)")
    p.add_argument("--cohort-size", type=int, default=5000, help="files of the cohort set taken (seeded random subset)")
    p.add_argument("--top-k", type=int, default=300, help="as-norm: cohort rows per side")
    p.add_argument("--whole-utterance", action="store_true", help="embed every file whole, at its own length (not its first --n-seconds)")
    p.add_argument("--dcf", action="append", default=[], type=parse_dcf, metavar="P[,CMISS,CFA]",
                   help="a detection-cost operating point for the test set's minDCF (repeatable)")
    p.add_argument("--calibrate", action="store_true", help="fit llr = a s + b on the validation set; Cllr and actDCF on the test set")
    p.add_argument("--calib-prior", type=float, default=0.5, help="the target prior of the calibration fit")
    p.add_argument("--backend", default="none", choices=["none", "plda"], help="a trained back end in front of the scorers (off by default)")
    p.add_argument("--plda-train", default="train", choices=["train", "validation"], help="the set the PLDA back end is fitted on")
    p.add_argument("--plda-train-set", default="train-clean-100", help="the training subset of --plda-train train")
    p.add_argument("--lda-dim", type=int, default=None, help="LDA directions kept in front of PLDA (default: all)")
    p.add_argument("--no-length-norm", action="store_true", help="no length normalisation between LDA and PLDA")
    add_vad_args(p)   # --vad ...: off by default; every set embedded, the cohort included, is trimmed first
    return p


def main(argv=None):
    p = _parser()
    a = p.parse_args(argv)
    vad = policy_from_args(a)
    from experiments._common import setup
    rank, _ = setup()
    if a.synthetic:
        from voicemap_amd import models
        valid = SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=a.n_seconds, stochastic=False, seed=1,
                                       subset="synthetic-valid")
        test = SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=a.n_seconds, stochastic=False, seed=2,
                                      subset="synthetic-test")
        cohort = None
        if a.score_norm != "none":
            cohort = SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=a.n_seconds, stochastic=False, seed=3,
                                            subset="synthetic-cohort")
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
        valid = LibriSpeechDataset(a.validation_set, a.n_seconds, stochastic=False)
        test = LibriSpeechDataset(a.test_set, a.n_seconds, stochastic=False)
        cohort = None
        if a.score_norm != "none":
            cohort = LibriSpeechDataset(a.cohort_set, a.n_seconds, stochastic=False)
    if cohort is not None:
        cohort = cohort_subset(cohort, a.cohort_size)
    plda_train = None
    if a.backend == "plda" and a.plda_train == "train":
        plda_train = (SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=a.n_seconds, stochastic=False, seed=4,
                                             subset="synthetic-train")
                      if a.synthetic else LibriSpeechDataset(a.plda_train_set, a.n_seconds, stochastic=False))
    pre = BatchPreProcessor("siamese", preprocess_instances(a.downsampling))
    row = evaluate(net, valid, test, pre, a.score, a.score_norm, cohort, a.top_k, a.whole_utterance, vad=vad, dcf=a.dcf,
                   calibrate=a.calibrate, calib_prior=a.calib_prior, backend=a.backend, plda_train=plda_train, lda_dim=a.lda_dim,
                   length_norm=not a.no_length_norm)
    results = pd.DataFrame([row])
    if rank == 0:
        results.to_csv(PATH + "/logs/" + result_name(a), index=False)
        print(results.to_string(index=False))
    return results


if __name__ == "__main__":
    main()
