"""The bare encoder trained with a triplet loss mined inside the batch (Hermans et al. 2017; FaceNet) -- not in the reference, whose
objectives are the pair losses and the softmax classifier.  Every step is one batch of --batch-p speakers with --batch-k utterances
each, through ONE encoder call (one whitening batch, one set of BatchNorm statistics); vm_triplet_loss mines the triplets under the
current weights: --mining hard takes every anchor's farthest positive and nearest negative, --mining all every triplet of the batch;
the loss is max(0, margin + d_ap - d_an) or, with --soft-margin, softplus(d_ap - d_an).  Under torchrun every rank mines inside its
own batch and the gradients are summed by the usual hook.  The model has no head: it saves and loads as the encoder.
    python -m experiments.train_triplet [--synthetic] [--device-data DIR] ..."""
from experiments import _common as C
from voicemap_amd.keras_like import Adam
from voicemap_amd.models import get_baseline_convolutional_encoder
from voicemap_amd.utils import BatchPreProcessor, TripletLoss, preprocess_instances


def main(argv=None):
    ap = C.base_parser(__doc__)
    ap.add_argument("--batch-p", type=int, default=32, help="speakers per training batch")
    ap.add_argument("--batch-k", type=int, default=4, help="utterances per speaker")
    ap.add_argument("--margin", type=float, default=0.2, help="the hinge's margin on the euclidean distances")
    ap.add_argument("--soft-margin", action="store_true", help="softplus(d_ap - d_an) instead of the hinge (--margin is then unused)")
    ap.add_argument("--mining", choices=TripletLoss.MININGS, default="hard", help="batch hard or batch all")
    C.add_speed_args(ap)
    a = ap.parse_args(argv)
    C.speed_policy(a)   # --speed-perturb (off by default; needs --device-data): C.device_resident adds the copies; validation stays clean
    if a.hard_fraction > 0:
        raise SystemExit("--hard-fraction mines PAIRS over a cached corpus (voicemap_amd/mining.py); triplets are mined inside every batch")
    C.setup()
    train, valid = C.datasets(a, pad=a.pad)
    p, k = a.batch_p, a.batch_k
    pre = BatchPreProcessor("classifier", preprocess_instances(a.downsampling))   # a batch is (windows, speaker labels)
    batches = lambda ds: (pre(b) for b in ds.yield_speaker_batches(p, k))
    train_batches = batches(train)
    workers = a.workers
    if a.device_data:  # same batches, but the windows never exist on the host: offsets into an HBM-resident int16 buffer
        resident = C.device_resident(a, train)
        train_batches = (pre(b) for b in resident.yield_speaker_batches_device(p, k))
        workers = 0
    encoder = get_baseline_convolutional_encoder(a.filters, a.embedding_dimension, input_shape=(C.input_length(a), 1), dropout=a.dropout,
                                                 dtype=a.dtype)
    encoder.compile(loss=TripletLoss("soft" if a.soft_margin else a.margin, a.mining), optimizer=Adam(clipnorm=1.), metrics=["accuracy"])
    encoder.summary()
    C.apply_sync_bn(a, encoder)
    name = "triplet__p_{}__k_{}__{}__margin_{}__filters_{}__embed_{}__drop_{}__pad={}".format(
        p, k, a.mining, "soft" if a.soft_margin else a.margin, a.filters, a.embedding_dimension, a.dropout, a.pad)
    return encoder.fit_generator(generator=train_batches, steps_per_epoch=a.steps_per_epoch, validation_data=batches(valid),
                                 validation_steps=a.validation_steps, epochs=a.epochs, workers=workers, use_multiprocessing=True,
                                 callbacks=C.standard_callbacks(a, valid, pre, "encoder", name))


if __name__ == "__main__":
    main()
