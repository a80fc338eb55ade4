"""All-pairs speaker verification of a trained siamese network -- the reference's experiments/verification_accuracy.py, a stub whose
docstring "determines the best verification distance threshold on the validation set and then ... uses this to estimate the true
verification accuracy on the test set".  Each set is embedded once (retrieval.embed_corpus: one first-fragment window per file, each
window whitened alone -- the deviation documented there); the best-balanced-accuracy threshold of the validation set's all-pairs trials
is applied to the test set's (voicemap_amd/verification.py).  Results go to logs/verification_accuracy_<valid>_<test>_<score>.csv.
    python -m experiments.verification_accuracy --siamese models/x.hdf5 [--score euclidean|cosine|dot_product|head] [--synthetic]"""
import argparse

import pandas as pd

from config import PATH
from voicemap_amd import retrieval, verification
from voicemap_amd.librispeech import LibriSpeechDataset, SyntheticSpeechDataset
from voicemap_amd.utils import BatchPreProcessor, preprocess_instances


def evaluate(net, valid, test, pre, score="euclidean"):
    """Embed both sets once, take the best-balanced-accuracy threshold of the validation trials and apply it to the test trials."""
    model = net if score == "head" else None
    cv = retrieval.embed_corpus(net, valid, pre, "siamese")
    ct = retrieval.embed_corpus(net, test, pre, "siamese")
    mv = verification.verification_metrics(cv, score, model=model)
    mt = verification.verification_metrics(ct, score, model=model)
    at = verification.accuracy_at_threshold(ct, mv["best_threshold"], score, model=model)
    row = {"score": score, "threshold": mv["best_threshold"], "valid_balanced_accuracy": mv["best_balanced_accuracy"],
           "valid_eer": mv["eer"], "valid_eer_threshold": mv["eer_threshold"], "test_balanced_accuracy": at["balanced_accuracy"],
           "test_far": at["far"], "test_frr": at["frr"], "test_eer": mt["eer"], "test_eer_threshold": mt["eer_threshold"],
           "valid_pairs": mv["n_target"] + mv["n_nontarget"], "test_pairs": mt["n_target"] + mt["n_nontarget"]}
    if "best_threshold_p" in mv:
        row["threshold_p"] = mv["best_threshold_p"]
    return row


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--siamese", default=None, help="a saved siamese network (not needed with --synthetic)")
    p.add_argument("--validation-set", default="dev-clean")
    p.add_argument("--test-set", default="test-clean")
    p.add_argument("--n-seconds", type=float, default=3)
    p.add_argument("--downsampling", type=int, default=4)
    p.add_argument("--score", default="euclidean", choices=["euclidean", "cosine", "dot_product", "head"])
    p.add_argument("--synthetic", action="store_true", help="two generated speaker sets and a freshly built model")
    a = p.parse_args(argv)
    from experiments._common import setup
    rank, _ = setup()
    if a.synthetic:
        from voicemap_amd import models
        valid = SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=a.n_seconds, stochastic=False, seed=1,
                                       subset="synthetic-valid")
        test = SyntheticSpeechDataset(num_speakers=20, files_per_speaker=8, seconds=a.n_seconds, stochastic=False, seed=2,
                                      subset="synthetic-test")
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
    pre = BatchPreProcessor("siamese", preprocess_instances(a.downsampling))
    row = evaluate(net, valid, test, pre, a.score)
    results = pd.DataFrame([row])
    if rank == 0:
        results.to_csv(PATH + "/logs/verification_accuracy_{}_{}_{}.csv".format(
            "synthetic" if a.synthetic else a.validation_set, "synthetic" if a.synthetic else a.test_set, a.score), index=False)
        print(results.to_string(index=False))
    return results


if __name__ == "__main__":
    main()
