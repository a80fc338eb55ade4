"""The bare encoder trained on k-way n-shot episodes with a prototypical loss (Snell et al. 2017) -- not in the reference, whose
objectives are the pair losses and the softmax classifier; this one optimises what its n-shot evaluation measures: the distance of a
query to the mean of n support embeddings.  Every step is one episode of --episode-k speakers with --episode-n support and --episode-q
query windows each, through ONE encoder call (one whitening batch, one set of BatchNorm statistics); the loss is
-log softmax(-alpha |q - prototype|^2) of the query's own class (vm_proto_loss).  The model has no head: it saves and loads as the
encoder.     python -m experiments.train_prototypical [--synthetic] [--device-data DIR] ..."""
from experiments import _common as C
from voicemap_amd.keras_like import Adam
from voicemap_amd.models import get_baseline_convolutional_encoder
from voicemap_amd.utils import BatchPreProcessor, PrototypicalLoss, preprocess_instances


def main(argv=None):
    ap = C.base_parser(__doc__)
    ap.add_argument("--episode-k", type=int, default=32, help="speakers (classes) per training episode")
    ap.add_argument("--episode-n", type=int, default=2, help="support windows per speaker")
    ap.add_argument("--episode-q", type=int, default=4, help="query windows per speaker")
    ap.add_argument("--proto-alpha", type=float, default=1.0, help="scale of the squared distance in the logits")
    C.add_speed_args(ap)
    a = ap.parse_args(argv)
    C.speed_policy(a)   # --speed-perturb (off by default; needs --device-data): C.device_resident adds the copies; validation stays clean
    if a.hard_fraction > 0:
        raise SystemExit("--hard-fraction mines PAIRS (voicemap_amd/mining.py); episodes are drawn uniformly")
    C.setup()
    train, valid = C.datasets(a, pad=a.pad)
    k, n, q = a.episode_k, a.episode_n, a.episode_q
    pre = BatchPreProcessor("classifier", preprocess_instances(a.downsampling))   # an episode is (windows, query labels)
    batches = lambda ds: (pre(b) for b in ds.yield_episodes(k, n, q))
    train_batches = batches(train)
    workers = a.workers
    if a.device_data:  # same episodes, but the windows never exist on the host: offsets into an HBM-resident int16 buffer
        resident = C.device_resident(a, train)
        train_batches = (pre(b) for b in resident.yield_episodes_device(k, n, q))
        workers = 0
    encoder = get_baseline_convolutional_encoder(a.filters, a.embedding_dimension, input_shape=(C.input_length(a), 1), dropout=a.dropout,
                                                 dtype=a.dtype)
    encoder.compile(loss=PrototypicalLoss(k, n, alpha=a.proto_alpha), optimizer=Adam(clipnorm=1.), metrics=["accuracy"])
    encoder.summary()
    C.apply_sync_bn(a, encoder)
    name = "prototypical__k_{}__n_{}__q_{}__filters_{}__embed_{}__drop_{}__pad={}".format(k, n, q, a.filters, a.embedding_dimension,
                                                                                           a.dropout, a.pad)
    return encoder.fit_generator(generator=train_batches, steps_per_epoch=a.steps_per_epoch, validation_data=batches(valid),
                                 validation_steps=a.validation_steps, epochs=a.epochs, workers=workers, use_multiprocessing=True,
                                 callbacks=C.standard_callbacks(a, valid, pre, "encoder", name))


if __name__ == "__main__":
    main()
