"""Siamese network trained with the contrastive loss of Hadsell et al. -- counterpart of the reference's
experiments/siamese_contrastive_loss.py (filters 32, embedding 128, default dropout 0.05, batch 32, no ReduceLROnPlateau).
    python -m experiments.siamese_contrastive_loss [--synthetic] ..."""
from config import PATH
from experiments import _common as C
from voicemap_amd.augment import add_augment_args, policy_from_args
from voicemap_amd.keras_like import Adam, CSVLogger, ModelCheckpoint
from voicemap_amd.models import build_siamese_net, get_baseline_convolutional_encoder
from voicemap_amd.utils import BatchPreProcessor, NShotEvaluationCallback, contrastive_loss, preprocess_instances


def main(argv=None):
    p = C.base_parser(__doc__, batchsize=32, filters=32, embedding_dimension=128, dropout=0.05, epochs=25, pad=False)
    add_augment_args(p)
    C.add_vad_args(p)
    C.add_speed_args(p)
    a = p.parse_args(argv)
    C.speed_policy(a)   # --speed-perturb (off by default; needs --device-data): C.device_resident adds the copies; validation stays clean
    C.vad_policy(a)   # --vad (off by default; needs --device-data): C.device_resident trims the resident training set; validation stays as it is
    augment = policy_from_args(a, a.downsampling)   # --augment (off by default; needs --device-data): training batches only
    C.setup()
    train, valid = C.datasets(a, pad=False)
    whiten_downsample = BatchPreProcessor("siamese", preprocess_instances(a.downsampling, whitening=True))
    stream = lambda ds: (whiten_downsample(b) for b in ds.yield_verification_batches(a.batchsize))
    train_batches = stream(train)
    workers = a.workers
    if a.device_data:  # the windows never exist on the host: offsets into an HBM-resident int16 buffer (as in train_siamese.py)
        resident = C.device_resident(a, train)
        train_batches = (whiten_downsample(b) for b in resident.yield_verification_batches_device(a.batchsize, augment))
        workers = 0
    # --hard-fraction: part of every batch from mined pairs (off by default: the generators above, unchanged)
    mined, mining_cbs = C.mined_batches(a, resident if a.device_data else train, whiten_downsample, device=bool(a.device_data),
                                        augment=augment)
    if mined is not None:
        train_batches = mined
    encoder = get_baseline_convolutional_encoder(a.filters, a.embedding_dimension, dropout=a.dropout, dtype=a.dtype)
    siamese = build_siamese_net(encoder, (C.input_length(a), 1))
    siamese.compile(loss=contrastive_loss, optimizer=Adam(clipnorm=1.), metrics=["accuracy"])
    key = "val_{}-shot_acc".format(a.n_shot)
    cbs = mining_cbs + [NShotEvaluationCallback(a.num_evaluation_tasks, a.n_shot, a.k_way, valid, preprocessor=whiten_downsample),
                        CSVLogger(PATH + "/logs/convnet_contrastive_loss.csv"),
                        ModelCheckpoint(PATH + "/models/convnet_contrastive_loss.hdf5", monitor=key, mode="max", save_best_only=True,
                                        verbose=True)]
    return siamese.fit_generator(generator=train_batches, steps_per_epoch=a.steps_per_epoch, validation_data=stream(valid),
                                 validation_steps=a.validation_steps, epochs=a.epochs, workers=workers,
                                 use_multiprocessing=True, callbacks=cbs)


if __name__ == "__main__":
    main()
