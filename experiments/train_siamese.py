"""Siamese verification network trained with binary cross-entropy -- the MI355X counterpart of the reference's
experiments/train_siamese.py (filters 128, embedding 64, dropout 0, batch 64, Adam(clipnorm=1), 500-step epochs with
100 validation batches and 5-way 1-shot evaluation).     python -m experiments.train_siamese [--synthetic] ..."""
from experiments import _common as C
from voicemap_amd.augment import add_augment_args, policy_from_args
from voicemap_amd.keras_like import Adam
from voicemap_amd.models import build_siamese_net, get_baseline_convolutional_encoder, get_spectrogram_convolutional_encoder
from voicemap_amd.utils import BatchPreProcessor, preprocess_instances


def main(argv=None):
    ap = C.base_parser(__doc__)
    ap.add_argument("--frontend", default="waveform", choices=["waveform", "logmel"],
                    help="waveform: the reference's 1-D encoder on the decimated, whitened window; logmel: the log-mel + 2-D CNN variant "
                         "on the raw 16 kHz window (BASELINE.json config 4, not in the reference)")
    add_augment_args(ap)
    C.add_vad_args(ap)
    C.add_speed_args(ap)
    a = ap.parse_args(argv)
    C.speed_policy(a)   # --speed-perturb (off by default; needs --device-data): C.device_resident adds the copies; validation stays clean
    C.vad_policy(a)   # --vad (off by default; needs --device-data): C.device_resident trims the resident training set; validation stays as it is
    if a.frontend == "logmel":
        a.downsampling = 1   # the front-end works on the raw window: no decimation, no whitening
    augment = policy_from_args(a, a.downsampling)   # --augment (off by default; needs --device-data): training batches only
    if augment is not None and a.frontend == "logmel":
        raise SystemExit("--augment is for the waveform front-end (the augmentation runs inside its preprocessing launch)")
    C.setup()
    train, valid = C.datasets(a, pad=a.pad)
    pre = BatchPreProcessor("siamese", preprocess_instances(a.downsampling, whitening=a.frontend != "logmel"))
    batches = lambda ds: (pre(b) for b in ds.yield_verification_batches(a.batchsize))
    train_batches = batches(train)
    workers = a.workers
    if a.device_data:  # same pairs, but the windows never exist on the host: offsets into an HBM-resident int16 buffer
        resident = C.device_resident(a, train)
        train_batches = (pre(b) for b in resident.yield_verification_batches_device(a.batchsize, augment))
        workers = 0
    # --hard-fraction: part of every batch from mined pairs (off by default: the generators above, unchanged)
    mined, mining_cbs = C.mined_batches(a, resident if a.device_data else train, pre, device=bool(a.device_data), augment=augment)
    if mined is not None:
        train_batches = mined
    build = get_spectrogram_convolutional_encoder if a.frontend == "logmel" else get_baseline_convolutional_encoder
    encoder = build(a.filters, a.embedding_dimension, dropout=a.dropout, dtype=a.dtype)
    siamese = build_siamese_net(encoder, (C.input_length(a), 1), distance_metric="uniform_euclidean")
    siamese.compile(loss="binary_crossentropy", optimizer=Adam(clipnorm=1.), metrics=["accuracy"])
    siamese.summary()
    C.apply_sync_bn(a, siamese)
    name = "siamese__filters_{}__embed_{}__drop_{}__pad={}".format(a.filters, a.embedding_dimension, a.dropout, a.pad)
    if a.frontend == "logmel":
        name = "logmel_" + name
    return siamese.fit_generator(generator=train_batches, steps_per_epoch=a.steps_per_epoch, validation_data=batches(valid),
                                 validation_steps=a.validation_steps, epochs=a.epochs, workers=workers,
                                 use_multiprocessing=True, callbacks=mining_cbs + C.standard_callbacks(a, valid, pre, "siamese", name))


if __name__ == "__main__":
    main()
