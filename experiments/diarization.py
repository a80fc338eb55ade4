"""Speaker diarization of synthetic conversations (new; the reference has no such experiment): conversations are cut together from the
single-speaker files of a dataset (voicemap_amd/diarization.py make_conversations), every conversation is cut into sliding windows,
the windows are embedded and clustered on the chip (diarize: vm_ahc, one workgroup per conversation) and the hypothesis is scored by
the sample-exact diarization error rate against the turns that were planted.  One of three stop rules:
    --threshold T              merging stops at the first height above T
    --oracle-speakers          every conversation is merged down to its true number of speakers
    --tune-conversations K     T is the recorded height that minimises the mean DER of the first K conversations (one full dendrogram
                               each, then diarization.cut over the recorded heights) and is applied to the rest
    python -m experiments.diarization --synthetic [--device-data DIR] [--siamese models/x.hdf5] --conversations 64 --speakers 2-4
        --window-seconds 1.5 --hop-seconds 0.75 --linkage average --distance cosine --tune-conversations 16
Prints one JSON line: the mean DER and its three parts (shares of the reference speech), and how many clusters were found against how
many speakers were present.  With --synthetic and no --siamese the encoder is untrained: the line then says how the pipeline runs, not
how well a model diarizes.
--distance plda: a PLDA back end (voicemap_amd/plda.py) is fitted on the embeddings of the single-speaker files the conversations are
built from (one first-fragment window per file, --lda-dim / --no-length-norm as in experiments/verification_accuracy.py) and the
windows are clustered on minus its log-likelihood ratio.
Pauses, speech gating and resegmentation, all off by default:
    --pause-seconds LO-HI --pause-prob P   digital silence of a drawn length in front of a turn, with probability P
    --vad [--vad-...] --min-voiced S       one voice activity detection over the conversations; a window with less than the share S of
                                           voiced frames is neither embedded nor clustered, no unvoiced frame carries a speaker
    --reseg --switch-cost C --reseg-iters N [--reseg-hop-seconds H]
                                           Viterbi resegmentation of the cluster labels (vm_reseg), at a finer hop H if given; the
                                           line then carries the error before ("ahc_*") and after it
    --vbx [--vbx-loop-prob P --vbx-fa A --vbx-fb B --vbx-iters N --vbx-hop-seconds H --vbx-init-threshold T]
                                           VBx behind the clustering (vm_vbx; --distance plda only, not with --reseg): a Bayesian HMM
                                           over the PLDA-space rows, started from the cluster labels.  With T the start is the
                                           clustering stopped at height T (meant to leave too many clusters: VBx drops speakers, it
                                           adds none) and the "before" figures are those of the stop rule chosen; the line carries the
                                           error and the speakers found before ("ahc_*") and after
With --tune-conversations the threshold is tuned on the clustering alone and the resegmentation runs on the labels it cuts (no
--reseg-hop-seconds there: the tuned cut has no finer rows)."""
import argparse
import json
import os

import numpy as np

from voicemap_amd import diarization as DZ
from voicemap_amd import vad as VAD
from voicemap_amd.librispeech import LibriSpeechDataset, SyntheticSpeechDataset
from voicemap_amd.utils import BatchPreProcessor, preprocess_instances


def parse_range(text):
    """LO-HI or N -> (lo, hi)."""
    try:
        lo, _, hi = text.partition("-")
        lo, hi = int(lo), int(hi or lo)
        if lo < 2 or hi < lo:
            raise ValueError
        return lo, hi
    except ValueError:
        raise argparse.ArgumentTypeError("a range LO-HI with 2 <= LO <= HI, not %r" % text)


def parse_seconds(text):
    """LO-HI or X -> (lo, hi) in seconds."""
    try:
        lo, _, hi = text.partition("-")
        lo, hi = float(lo), float(hi or lo)
        if lo < 0 or hi < lo:
            raise ValueError
        return lo, hi
    except ValueError:
        raise argparse.ArgumentTypeError("a range LO-HI in seconds with 0 <= LO <= HI, not %r" % text)


def _parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--siamese", default=None, help="a saved siamese network (optional with --synthetic: a fresh, untrained one is built)")
    p.add_argument("--synthetic", action="store_true", help="generated speakers instead of LibriSpeech on disk")
    p.add_argument("--device-data", metavar="DIR", default="",
                   help="decode the files once into int16 shards under DIR (reused if present) and keep them resident: the conversations "
                        "are then assembled on the device")
    p.add_argument("--dataset", default="dev-clean", help="the LibriSpeech subset the conversations are cut from")
    p.add_argument("--conversations", type=int, default=64)
    p.add_argument("--speakers", type=parse_range, default=(2, 4), metavar="LO-HI")
    p.add_argument("--turns", type=parse_range, default=(6, 12), metavar="LO-HI")
    p.add_argument("--window-seconds", type=float, default=1.5)
    p.add_argument("--hop-seconds", type=float, default=0.75)
    p.add_argument("--downsampling", type=int, default=4)
    p.add_argument("--linkage", default="average", choices=list(DZ.LINKAGES))
    p.add_argument("--distance", default="cosine", choices=["euclidean", "cosine", "dot_product", "plda"])
    p.add_argument("--lda-dim", type=int, default=None, help="--distance plda: LDA directions kept (default: all)")
    p.add_argument("--no-length-norm", action="store_true", help="--distance plda: no length normalisation between LDA and PLDA")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--pause-seconds", type=parse_seconds, default=(0.0, 0.0), metavar="LO-HI")
    p.add_argument("--pause-prob", type=float, default=0.0)
    VAD.add_vad_args(p)
    p.add_argument("--min-voiced", type=float, default=0.5, help="--vad: the share of voiced frames a window needs to be kept")
    p.add_argument("--reseg", action="store_true", help="resegment the cluster labels with a sticky HMM (vm_reseg)")
    p.add_argument("--switch-cost", type=float, default=0.5, help="--reseg: the cost of a speaker change, in units of the distance")
    p.add_argument("--reseg-iters", type=int, default=3)
    p.add_argument("--reseg-hop-seconds", type=float, default=None, help="--reseg: cut, embed and decode at this finer hop")
    p.add_argument("--vbx", action="store_true", help="VBx behind the clustering (vm_vbx); needs --distance plda")
    p.add_argument("--vbx-loop-prob", type=float, default=0.99)
    p.add_argument("--vbx-fa", type=float, default=0.3)
    p.add_argument("--vbx-fb", type=float, default=17.0)
    p.add_argument("--vbx-iters", type=int, default=20)
    p.add_argument("--vbx-hop-seconds", type=float, default=None, help="--vbx: cut, embed and model at this finer hop")
    p.add_argument("--vbx-init-threshold", type=float, default=None, metavar="T",
                   help="--vbx: the clustering that starts VBx stops at height T instead of at the stop rule chosen")
    stop = p.add_mutually_exclusive_group(required=True)
    stop.add_argument("--threshold", type=float, default=None)
    stop.add_argument("--oracle-speakers", action="store_true")
    stop.add_argument("--tune-conversations", type=int, default=0, metavar="K")
    return p


def score(conv, rows, segments):
    """The error of conversations ``rows`` under ``segments`` (one table per row): the mean DER and its parts as shares of the reference."""
    ds = [DZ.der(conv.segments[r], seg) for r, seg in zip(rows, segments)]
    part = lambda k: float(np.mean([d[k] / d["total"] for d in ds])) if ds else float("nan")
    return {"mean_der": part("missed") + part("false_alarm") + part("confusion") if ds else float("nan"),
            "missed": part("missed"), "false_alarm": part("false_alarm"), "confusion": part("confusion")}


def hyp_segments(conv, res, r, labels, starts=None):
    """The hypothesis of conversation r from one label per window (``starts``: default all embedded windows), cut to the voiced frames
    when the windows were gated."""
    if len(labels) == 0:
        return np.zeros((0, 3), np.int64)
    seg = DZ.window_segments(res.starts[r] if starts is None else starts, res.window, int(conv.lens[r]), labels)
    return seg if res.voiced is None else DZ.cut_to_voiced(seg, res.voiced[r], res.vad.policy.frame, int(conv.lens[r]))


def ahc_segments(conv, res, rows):
    """The hypothesis the clustering alone gives (its labels on the clustered windows): the "before" of a resegmentation."""
    return [hyp_segments(conv, res, r, res.recording(r).labels, res.starts[r][res.clustered[r]]) for r in rows]


def segments_at(conv, res, rows, threshold, reseg=None):
    """(hypothesis segments, clusters found) of conversations ``rows`` from their FULL dendrograms cut at ``threshold``; with ``reseg``
    (a ResegPolicy) the cut labels are resegmented first."""
    cuts = []
    for r in rows:
        rec = res.recording(r)
        cuts.append(DZ.cut(rec.merge_a, rec.merge_b, rec.merge_h, len(rec.labels), threshold=threshold))
    if reseg is not None:
        row0 = res.window_row0
        lab, k = np.full(int(row0[-1]), -1, np.int32), np.ones(len(row0) - 1, np.int64)
        for r, (labels, c) in zip(rows, cuts):
            lab[row0[r]:row0[r + 1]], k[r] = labels, max(c, 1)
        out = DZ.resegment(res.emb, row0, lab, k, res.chain_start, res.distance, reseg.switch_cost, reseg.iters, return_emis=False).host()
        cuts = [(out.labels[row0[r]:row0[r + 1]], c) for r, (_, c) in zip(rows, cuts)]
    return [hyp_segments(conv, res, r, labels) for r, (labels, _) in zip(rows, cuts)], [c for _, c in cuts]


def tune_threshold(conv, res, rows, candidates=64):
    """The threshold with the lowest mean DER over conversations ``rows``, among up to ``candidates`` quantiles of their recorded
    heights (a cut can only change at a recorded height); ties go to the lower threshold."""
    heights = np.concatenate([res.recording(r).merge_h for r in rows])
    heights = np.unique(heights[~np.isnan(heights)])
    if heights.size == 0:
        raise SystemExit("--tune-conversations: the development conversations recorded no merge")
    if heights.size > candidates:
        heights = np.unique(np.quantile(heights, np.linspace(0, 1, candidates), method="nearest"))
    errs = [score(conv, rows, segments_at(conv, res, rows, float(h))[0])["mean_der"] for h in heights]
    return float(heights[int(np.argmin(errs))])


def main(argv=None):
    p = _parser()
    a = p.parse_args(argv)
    from experiments._common import setup
    setup(a.seed)
    from voicemap_amd import models
    window = int(round(a.window_seconds * DZ.SAMPLING_RATE))
    if a.synthetic:
        data = SyntheticSpeechDataset(num_speakers=24, files_per_speaker=6, seconds=a.window_seconds, stochastic=False, seed=1,
                                      subset="synthetic-diarization")
    else:
        data = LibriSpeechDataset(a.dataset, a.window_seconds, stochastic=False)
    if a.siamese:
        net = models.load_model(a.siamese)
    elif a.synthetic:
        enc = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype="f32")
        net = models.build_siamese_net(enc, (window // a.downsampling, 1), distance_metric="uniform_euclidean")
    else:
        p.error("--siamese is required without --synthetic")
    if a.device_data:
        from voicemap_amd import shards
        if not os.path.exists(os.path.join(a.device_data, "index.csv")):
            shards.write_shards(data, a.device_data)
        data = shards.ShardedSpeechDataset(a.device_data, a.window_seconds, stochastic=False, pad=False)
        data.to_device("cuda")
    pre = BatchPreProcessor("siamese", preprocess_instances(a.downsampling))
    conv = DZ.make_conversations(data, a.conversations, speakers=a.speakers, turns=a.turns, seed=a.seed, pause_seconds=a.pause_seconds,
                                 pause_prob=a.pause_prob)
    policy = VAD.policy_from_args(a)
    try:
        reseg = DZ.ResegPolicy(a.switch_cost, a.reseg_iters, a.reseg_hop_seconds) if a.reseg else None
    except ValueError as e:
        p.error("--reseg: %s" % e)
    vbx = None
    if a.vbx:
        if a.distance != "plda" or a.reseg or a.tune_conversations:
            p.error("--vbx needs --distance plda and goes with neither --reseg nor --tune-conversations")
        try:
            vbx = DZ.VbxPolicy(a.vbx_loop_prob, a.vbx_fa, a.vbx_fb, iters=a.vbx_iters, hop_seconds=a.vbx_hop_seconds)
        except ValueError as e:
            p.error("--vbx: %s" % e)
    kw = dict(distance=a.distance, linkage=a.linkage, vad=policy, min_voiced=a.min_voiced)
    if a.distance == "plda":
        from voicemap_amd import plda, retrieval
        kw["plda"] = plda.fit_plda(retrieval.embed_corpus(net, data, pre, "siamese"), lda_dim=a.lda_dim, length_norm=not a.no_length_norm)
    rows = list(range(len(conv)))
    out = {"conversations": len(conv), "linkage": a.linkage, "distance": a.distance, "window_seconds": a.window_seconds,
           "hop_seconds": a.hop_seconds}
    if a.tune_conversations:
        if not 0 < a.tune_conversations < len(conv):
            p.error("--tune-conversations K needs 0 < K < --conversations")
        if reseg is not None and reseg.hop_seconds is not None:
            p.error("--reseg-hop-seconds does not go with --tune-conversations")
        _, res = DZ.diarize(net, conv.audio, conv.offsets, conv.lens, pre, a.window_seconds, a.hop_seconds, **kw)   # full dendrograms
        dev, rows = rows[:a.tune_conversations], rows[a.tune_conversations:]
        threshold = tune_threshold(conv, res, dev)
        segments, found = segments_at(conv, res, rows, threshold, reseg)
        before = segments_at(conv, res, rows, threshold)[0] if reseg is not None else None
        out.update(threshold=threshold, tuned_on=len(dev), dev_mean_der=score(conv, dev, segments_at(conv, res, dev, threshold)[0])["mean_der"])
    else:
        n_speakers = conv.speakers if a.oracle_speakers else None
        stop = dict(threshold=a.threshold, n_speakers=n_speakers)
        if vbx is not None and a.vbx_init_threshold is not None:
            stop = dict(threshold=a.vbx_init_threshold, n_speakers=None)
        segments, res = DZ.diarize(net, conv.audio, conv.offsets, conv.lens, pre, a.window_seconds, a.hop_seconds, reseg=reseg, vbx=vbx,
                                   **stop, **kw)
        found = res.host().n_clusters.tolist()
        before = ahc_segments(conv, res, rows) if reseg is not None or vbx is not None else None
        if vbx is not None:
            found_before, lab, row0 = found, res.vbx.host().labels, res.window_row0
            found = [len(np.unique(lab[row0[r]:row0[r + 1]])) for r in rows]
            if a.vbx_init_threshold is not None:   # "before" = the stop rule chosen, without VBx
                _, plain = DZ.diarize(net, conv.audio, conv.offsets, conv.lens, pre, a.window_seconds, a.hop_seconds, threshold=a.threshold,
                                      n_speakers=n_speakers, **kw)
                before, found_before = ahc_segments(conv, plain, rows), plain.host().n_clusters.tolist()
        out.update(threshold=a.threshold, oracle_speakers=bool(a.oracle_speakers))
    out.update(score(conv, rows, segments), scored=len(rows), windows=int(res.row0[-1]))
    if policy is not None:
        out.update(vad=True, min_voiced=a.min_voiced, windows_kept=int(res.window_row0[-1]), windows_cut=int(sum(len(k) for k in res.kept)))
    if reseg is not None:
        out.update({"ahc_" + k: v for k, v in score(conv, rows, before).items()}, reseg=True, switch_cost=reseg.switch_cost,
                   reseg_iters=reseg.iters, reseg_hop_seconds=reseg.hop_seconds, windows_decoded=int(res.window_row0[-1]))
    if vbx is not None:
        out.update({"ahc_" + k: v for k, v in score(conv, rows, before).items()}, vbx=True, vbx_loop_prob=vbx.loop_prob, vbx_fa=vbx.fa,
                   vbx_fb=vbx.fb, vbx_iters=vbx.iters, vbx_hop_seconds=vbx.hop_seconds, vbx_init_threshold=a.vbx_init_threshold,
                   windows_decoded=int(res.window_row0[-1]), ahc_speakers_found=[int(c) for c in found_before],
                   speakers_found=[int(c) for c in found],
                   vbx_iters_run=[int(i) for i in res.vbx.host().iters_run])
    table = {}
    for r, c in zip(rows, found):
        table.setdefault(int(conv.speakers[r]), {}).setdefault(int(c), 0)
        table[int(conv.speakers[r])][int(c)] += 1
    out["clusters_found_by_speakers_present"] = {str(s): {str(c): k for c, k in sorted(row.items())} for s, row in sorted(table.items())}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
