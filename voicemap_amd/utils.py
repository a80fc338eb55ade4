"""Drop-in mirror of ``voicemap/utils.py``: same names, arguments and error behaviour.

    get_bottleneck(classifier, samples)                                                        utils.py:9
    preprocess_instances(downsampling, whitening=True)                                         utils.py:22
    BatchPreProcessor(mode, instance_preprocessor, target_preprocessor=identity)               utils.py:37
    contrastive_loss(y_true, y_pred)                                                           utils.py:77
    whiten(batch, rms=0.038021)                                                                utils.py:88
    n_shot_task_evaluation(model, dataset, preprocessor, num_tasks, n, k, network_type, distance)   utils.py:104
    NShotEvaluationCallback(num_tasks, n_shot, k_way, dataset, preprocessor, mode)             utils.py:219
    PrototypicalLoss(k_way, n_shot, alpha=1.0)                                                 (not in the reference)
    TripletLoss(margin=0.2, mining="hard")                                                     (not in the reference)
    MarginSoftmaxLoss(kind="angular", margin=0.2, scale=30.0)                                  (not in the reference)

What is different underneath: ``preprocess_instances`` returns a *lazy* batch (``LazyWindows``) that remembers the raw
16 kHz windows; the HIP models decimate + whiten it on the GPU (vm_decimate_whiten) instead of in three numpy passes on
the host, and the n-shot evaluation runs all tasks of a run through batched launches instead of ``num_tasks``
sequential ``predict`` calls.  A ``LazyWindows`` converts to the reference's float64 array on demand (``np.asarray``).
"""
from __future__ import annotations

import numpy as np

from .keras_like import Callback


# ---------------------------------------------------------------------------------------------------------
class LazyWindows:
    """Result of ``preprocess_instances(d)(instances)``: (n, T, 1) raw windows + the preprocessing still to apply.
    ``np.asarray(lazy)`` gives exactly what the reference's preprocessor returns (float64, decimated, whitened)."""

    def __init__(self, raw, downsampling: int, whitening: bool):
        if type(raw).__name__ != "DeviceWindows":  # shards.DeviceWindows: offsets into a device-resident buffer, kept as is
            raw = np.asarray(raw)
        if raw.ndim != 3:
            raise ValueError("Input must be a 3D array of shape (n_segments, n_timesteps, 1).")
        self.raw, self.downsampling, self.whitening = raw, int(downsampling), bool(whitening)

    @property
    def shape(self):
        n, t, c = self.raw.shape
        return (n, (t + self.downsampling - 1) // self.downsampling, c)

    def __len__(self):
        return self.raw.shape[0]

    def __array__(self, dtype=None, copy=None):
        x = np.asarray(self.raw)[:, ::self.downsampling, :]
        if self.whitening:
            x = whiten(x)
        return np.asarray(x, dtype=dtype) if dtype is not None else np.asarray(x)


def whiten(batch, rms=0.038021):
    """voicemap/utils.py:88-101: subtract each window's mean, then multiply the WHOLE batch by one scalar
    rms / sqrt(mean(batch**2)) (mean of squares of the un-centred batch, utils.py:98).  Host numpy, float64 in / out like
    the reference; the GPU path for training is vm_decimate_whiten."""
    batch = np.asarray(batch)
    if len(batch.shape) != 3:
        raise ValueError("Input must be a 3D array of shape (n_segments, n_timesteps, 1).")
    centred = batch - batch.mean(axis=1, keepdims=True)
    return centred * (rms / np.sqrt(np.power(batch, 2).mean()))


def preprocess_instances(downsampling, whitening=True):
    """voicemap/utils.py:22-34: the canonical preprocessing -- take every ``downsampling``-th sample, then whiten."""
    def preprocess_instances_(instances):
        return LazyWindows(instances, downsampling, whitening)

    return preprocess_instances_


class BatchPreProcessor(object):
    """voicemap/utils.py:37-74: applies the instance preprocessor to classifier batches ``(inputs, outputs)`` and to
    siamese batches ``([input_1, input_2], outputs)`` -- each tower separately (utils.py:59-60) -- and the target
    preprocessor to the labels."""

    def __init__(self, mode, instance_preprocessor, target_preprocessor=lambda x: x):
        assert mode in ("siamese", "classifier")
        self.mode = mode
        self.instance_preprocessor = instance_preprocessor
        self.target_preprocessor = target_preprocessor

    def __call__(self, batch):
        if self.mode == "siamese":
            ([input_1, input_2], labels) = batch
            return [self.instance_preprocessor(input_1), self.instance_preprocessor(input_2)], self.target_preprocessor(labels)
        elif self.mode == "classifier":
            instances, labels = batch
            return self.instance_preprocessor(instances), self.target_preprocessor(labels)
        raise ValueError


def contrastive_loss(y_true, y_pred):
    """voicemap/utils.py:77-85 (Hadsell et al. '06, margin 1): mean((1-y) p^2 + y max(1-p, 0)^2).  Pass it to
    ``model.compile(loss=contrastive_loss)``: the siamese model recognises it and evaluates loss + gradient inside the
    fused head kernel (vm_siamese_head_loss).  Called directly it evaluates the same expression with numpy."""
    y_true = np.asarray(y_true, dtype=np.float64)
    y_pred = np.asarray(y_pred, dtype=np.float64)
    margin = 1
    return np.mean((1 - y_true) * np.square(y_pred) + y_true * np.square(np.maximum(margin - y_pred, 0)))


class PrototypicalLoss:
    """Prototypical loss (Snell et al. 2017) on k-way n-shot episodes, for ``encoder.compile(loss=PrototypicalLoss(k, n))`` on the
    bare encoder (not in the reference).  A batch is ``(x, y)``: x the episode's ``k_way * n_shot + m`` windows -- the support set
    first, class-major, as ``LibriSpeechDataset.build_episode`` lays them out -- and y the m queries' classes in [0, k_way).
    loss = mean_j (logsumexp_c l[j] - l[j, y_j]) with l[j, c] = -alpha |q_j - mean(support of c)|^2, evaluated with its gradient by
    vm_proto_loss; the metric beside it is the share of queries whose nearest prototype is their own."""

    __name__ = "prototypical_loss"

    def __init__(self, k_way, n_shot, alpha=1.0):
        if int(k_way) < 2 or int(n_shot) < 1 or not float(alpha) > 0:
            raise ValueError("PrototypicalLoss needs k_way >= 2, n_shot >= 1, alpha > 0")
        self.k_way, self.n_shot, self.alpha = int(k_way), int(n_shot), float(alpha)

    def get_config(self):
        return {"k_way": self.k_way, "n_shot": self.n_shot, "alpha": self.alpha}

    def __call__(self, emb, labels):
        """The same expression with numpy (float64) on (k n + m, E) embeddings and (m,) labels."""
        e = np.asarray(emb, dtype=np.float64)
        k, n = self.k_way, self.n_shot
        y = np.asarray(labels).reshape(-1).astype(np.int64)
        p = e[:k * n].reshape(k, n, -1).mean(axis=1)
        lg = -self.alpha * np.square(e[k * n:, None, :] - p[None]).sum(-1)
        mx = lg.max(axis=1, keepdims=True)
        lse = np.log(np.exp(lg - mx).sum(axis=1)) + mx[:, 0]
        return float(np.mean(lse - lg[np.arange(len(y)), y]))


class TripletLoss:
    """Triplet loss with mining inside the batch (Hermans et al. 2017: "batch hard" / "batch all"; FaceNet's margin), for
    ``encoder.compile(loss=TripletLoss(margin, mining))`` on the bare encoder (not in the reference).  A batch is ``(x, y)``: x the
    windows of P speakers x K utterances (``LibriSpeechDataset.build_speaker_batch``), y the speaker of every window (a negative label
    takes its window out).  ``mining="hard"``: per anchor its farthest positive and nearest negative; ``"all"``: every triplet, the
    hinge averaged over the active ones.  ``margin="soft"``: softplus(d_ap - d_an) instead of max(0, margin + d_ap - d_an).  Evaluated
    with its gradient by vm_triplet_loss; the metric beside it is the share of active (x > 0) anchors / triplets."""

    __name__ = "triplet_loss"
    MININGS = ("hard", "all")

    def __init__(self, margin=0.2, mining="hard"):
        if mining not in self.MININGS:
            raise ValueError("TripletLoss mining must be one of (hard, all)")
        self.soft = isinstance(margin, str)
        if self.soft and margin != "soft":
            raise ValueError('TripletLoss margin must be a number >= 0 or "soft"')
        if not self.soft and not (0 <= float(margin) < float("inf")):
            raise ValueError('TripletLoss margin must be a finite number >= 0 or "soft"')
        self.margin = "soft" if self.soft else float(margin)
        self.mining = mining

    @property
    def mining_code(self):
        """VM_TRIPLET_HARD / VM_TRIPLET_ALL"""
        return self.MININGS.index(self.mining)

    @property
    def margin_value(self):
        return 0.0 if self.soft else self.margin

    def get_config(self):
        return {"margin": self.margin, "mining": self.mining}

    def __call__(self, emb, labels):
        """The same expression with numpy (float64) on (N, E) embeddings and (N,) labels."""
        e = np.asarray(emb, dtype=np.float64)
        y = np.asarray(labels).reshape(-1).astype(np.int64)
        d = np.sqrt(np.square(e[:, None, :] - e[None, :, :]).sum(-1))
        part = y >= 0
        both = part[:, None] & part[None, :]
        pos = both & (y[:, None] == y[None, :]) & ~np.eye(len(y), dtype=bool)
        neg = both & (y[:, None] != y[None, :])
        valid = pos.any(1) & neg.any(1)
        term = (lambda x: np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))) if self.soft else (lambda x: np.maximum(x, 0))
        if not valid.any():
            return 0.0
        if self.mining == "hard":
            x = self.margin_value + np.where(pos, d, -np.inf).max(1)[valid] - np.where(neg, d, np.inf).min(1)[valid]
            return float(term(x).mean())
        x = np.concatenate([(self.margin_value + d[a, pos[a]][:, None] - d[a, neg[a]][None, :]).ravel() for a in np.flatnonzero(valid)])
        return float(term(x).sum() / (len(x) if self.soft else max(1, (x > 0).sum())))


class MarginSoftmaxLoss:
    """Softmax over scaled cosines with a margin at the label, for ``classifier.compile(loss=MarginSoftmaxLoss(kind, margin, scale))``
    on the encoder WITH its ``Dense(num_classes, activation="softmax")`` head (not in the reference).  ``kind="none"``: the normalised
    softmax (NormFace); ``"cosine"``: cos(theta) - margin at the label (AM-softmax / CosFace); ``"angular"``: cos(theta + margin)
    (AAM-softmax / ArcFace, with the usual fallback past pi - margin).  The logits are ``scale`` times the cosines between the
    embedding and the columns of the head's kernel; the head's bias takes no part and never moves.  A batch is the classifier's
    ``(windows, labels)`` (one-hot or ids).  Evaluated with its gradients by vm_margin_softmax; the metric beside it is the accuracy
    of the un-margined cosines, and ``predict()`` returns their softmax."""

    __name__ = "margin_softmax_loss"
    KINDS = ("none", "cosine", "angular")

    def __init__(self, kind="angular", margin=0.2, scale=30.0):
        if kind not in self.KINDS:
            raise ValueError("MarginSoftmaxLoss kind must be one of (none, cosine, angular)")
        if not (0 <= float(margin) < np.pi / 2):
            raise ValueError("MarginSoftmaxLoss margin must be a number with 0 <= margin < pi / 2")
        if not (0 < float(scale) < float("inf")):
            raise ValueError("MarginSoftmaxLoss scale must be a finite number > 0")
        self.kind, self.margin, self.scale = kind, float(margin), float(scale)

    @property
    def kind_code(self):
        """VM_MARGIN_NONE / VM_MARGIN_COSINE / VM_MARGIN_ANGULAR"""
        return self.KINDS.index(self.kind)

    def get_config(self):
        return {"kind": self.kind, "margin": self.margin, "scale": self.scale}

    def __call__(self, cosine, labels):
        """The same expression with numpy (float64) on the (N, S) cosines and (N,) class ids."""
        c = np.asarray(cosine, dtype=np.float64)
        y = np.asarray(labels).reshape(-1).astype(np.int64)
        rows = np.flatnonzero((y >= 0) & (y < c.shape[1]))
        cy = c[rows, y[rows]]
        m = float(np.float32(self.margin))
        if self.kind == "cosine":
            cp = cy - m
        elif self.kind == "angular":
            cos_m, sin_m = float(np.float32(np.cos(m))), float(np.float32(np.sin(m)))
            cp = np.where(cy > float(np.float32(-np.cos(m))), cy * cos_m - np.sqrt(np.maximum(0.0, 1.0 - cy * cy)) * sin_m,
                          cy - float(np.float32(m * np.sin(m))))
        else:
            cp = cy
        z = self.scale * c[rows]
        z[np.arange(len(rows)), y[rows]] = self.scale * cp
        zmax = z.max(1)
        return float((np.log(np.exp(z - zmax[:, None]).sum(1)) - (self.scale * cp - zmax)).sum() / len(c))


def get_bottleneck(classifier, samples):
    """voicemap/utils.py:9-19: activations of the layer before the classification layer (= the embedding) in
    inference mode."""
    enc = classifier.clone()
    enc.set_weights(classifier.get_weights())
    enc.pop()
    return enc.predict(samples)


# ---------------------------------------------------------------------------------------------------------
_DIST = {"euclidean": 0, "cosine": 1, "dot_product": 2}


def _as_raw(pre, windows):
    """windows: (m, T, 1) raw -> what to hand to the engine."""
    out = pre(windows)
    return out


def n_shot_task_evaluation(model, dataset, preprocessor, num_tasks, n, k, network_type="siamese", distance="euclidean"):
    """voicemap/utils.py:104-216 with the same task semantics and return value (``n_correct``):

    * n == 1 and a siamese network (:121-137): the query repeated k times against the k support windows through the
      verification head; each side is preprocessed (whitened) as its own batch of k (:131); correct iff
      ``argmin(pred[:, 0]) == 0`` (:135).
    * n > 1 or a classifier (:138-212): embed query and support with the encoder (``model.layers[2]`` for the siamese
      net :141, the classifier minus its last layer :143-145; ``network_type="encoder"``, not in the reference: the model is
      the encoder itself, e.g. one trained with PrototypicalLoss), whitening the query alone and the support set as one
      batch (:153-154), class prototypes + distance (:159-206) on the GPU (vm_nshot_distances), correct iff argmin == 0.

    Tasks are sampled one by one with ``dataset.build_n_shot_task(k, n)`` exactly like the reference, but embedded in
    batched launches (the per-task whitening batches are kept as towers of the preprocessing kernel).

    Under torchrun (BASELINE.json config 5) the ``num_tasks`` tasks are sharded over the ranks: every rank samples and
    evaluates its own ``parallel.shard_range`` share (tasks are independent draws) and the counts are summed with one
    all-reduce, so every rank returns the global ``n_correct``."""
    import torch
    from . import parallel
    rank, world = parallel.rank_world()
    if world > 1:
        lo, hi = parallel.shard_range(num_tasks, rank, world)
        local = _n_shot_local(model, dataset, preprocessor, hi - lo, n, k, network_type, distance)
        return int(round(parallel.sum_over_ranks(float(local))))
    return _n_shot_local(model, dataset, preprocessor, num_tasks, n, k, network_type, distance)


def _n_shot_local(model, dataset, preprocessor, num_tasks, n, k, network_type="siamese", distance="euclidean"):
    """This rank's share of ``n_shot_task_evaluation``."""
    import torch
    if n < 1:
        raise ValueError("n must be >= 1")
    if network_type not in ("siamese", "classifier", "encoder"):
        raise ValueError("mode must be one of (siamese, classifier, encoder)")
    if not (n == 1 and network_type == "siamese") and distance not in _DIST:
        raise ValueError("Distance must be in (euclidean, cosine, dot_product)")
    inst = preprocessor.instance_preprocessor if hasattr(preprocessor, "instance_preprocessor") else None

    if num_tasks == 0:
        return 0
    if getattr(dataset, "device_audio", None) is not None and hasattr(dataset, "build_n_shot_tasks_device"):
        # device-resident corpus (shards.py): tasks are start offsets, windows are cropped by the preprocessing kernel
        return _n_shot_device(model, dataset, preprocessor, num_tasks, n, k, network_type, distance)
    queries, supports = [], []
    for _ in range(num_tasks):
        query_sample, support_set_samples = dataset.build_n_shot_task(k, n)
        queries.append(np.asarray(query_sample[0]))
        supports.append(np.asarray(support_set_samples[0]))

    n_correct = 0
    chunk = max(1, 256 // max(k * n, 1))  # tasks per launch
    if n == 1 and network_type == "siamese":
        eng = model._ensure_engine()
        for t0 in range(0, num_tasks, chunk):
            qs, ss = queries[t0:t0 + chunk], supports[t0:t0 + chunk]
            nt = len(qs)
            in1 = np.concatenate([np.stack([q] * k) for q in qs])[:, :, np.newaxis]   # (nt*k, T, 1)
            in2 = np.concatenate(ss)[:, :, np.newaxis]
            lazy1, lazy2 = _lazy_pair(preprocessor, in1, in2)
            pred = _siamese_predict_towers(eng, lazy1, lazy2, tower=k).reshape(nt, k)
            n_correct += int((pred.argmin(axis=1) == 0).sum())
        return n_correct

    # embedding route
    if network_type == "siamese":
        encoder = model.layers[2]
        encoder.engine = model._ensure_engine()
    elif network_type == "encoder":   # the model IS the encoder (trained on episodes: PrototypicalLoss)
        encoder = model
    else:
        encoder = model.clone()
        encoder.set_weights(model.get_weights())
        encoder.pop()
    eng = encoder._ensure_engine()
    for t0 in range(0, num_tasks, chunk):
        qs, ss = queries[t0:t0 + chunk], supports[t0:t0 + chunk]
        nt = len(qs)
        qraw = np.stack(qs)[:, :, np.newaxis]            # (nt, T, 1): each query is whitened alone (tower = 1)
        sraw = np.concatenate(ss)[:, :, np.newaxis]      # (nt*k*n, T, 1): each task's support set is one whitening batch
        ql, sl = inst(qraw), inst(sraw)
        qe = _embed_towers(eng, ql, tower=1)
        se = _embed_towers(eng, sl, tower=k * n)
        pred = torch.empty(nt, k, dtype=torch.float32, device=eng.device)
        am = torch.empty(nt, dtype=torch.int32, device=eng.device)
        eng._call("vm_nshot_distances", qe.data_ptr(), se.data_ptr(), nt, k, n, eng.E, _DIST[distance], pred.data_ptr(),
                  am.data_ptr(), eng.stream())
        n_correct += int((am == 0).sum().item())
    return n_correct


def _n_shot_device(model, dataset, preprocessor, num_tasks, n, k, network_type, distance):
    """n_shot_task_evaluation over ``ShardedSpeechDataset.build_n_shot_tasks_device``: identical task semantics and
    whitening batches (query alone / repeated k times, support set of a task as one batch), windows addressed by offset."""
    import torch
    model._require_resident_input()   # every window below is an offset into the resident corpus
    q, s, _, _ = dataset.build_n_shot_tasks_device(num_tasks, k, n)
    lazy = preprocessor.instance_preprocessor(q) if hasattr(preprocessor, "instance_preprocessor") else None
    if not isinstance(lazy, LazyWindows):
        raise ValueError("the device n-shot path needs a BatchPreProcessor over preprocess_instances")
    ds, wh, T = lazy.downsampling, lazy.whitening, q.length
    n_correct = 0
    chunk = max(1, 256 // max(k * n, 1))  # tasks per launch
    siamese_1shot = n == 1 and network_type == "siamese"
    if siamese_1shot:
        eng = model._ensure_engine()
    elif network_type == "siamese":
        encoder = model.layers[2]
        encoder.engine = model._ensure_engine()
        eng = encoder._ensure_engine()
    elif network_type == "encoder":
        eng = model._ensure_engine()
    else:
        encoder = model.clone()
        encoder.set_weights(model.get_weights())
        encoder.pop()
        eng = encoder._ensure_engine()
    for t0 in range(0, num_tasks, chunk):
        nt = min(chunk, num_tasks - t0)
        qo = q.offsets[t0:t0 + nt]
        so = s.offsets[t0 * k * n:(t0 + nt) * k * n]
        if siamese_1shot:
            off = torch.cat([qo.repeat_interleave(k), so])  # input_1 = the query k times, input_2 = the k support windows
            eng.embed_from_offsets(q.audio, off, T, ds, wh, windows_per_tower=k)
            pl = eng.plan(2 * nt * k, eng.last_infer_l0, False)
            pred = eng.siamese_head(pl, None).reshape(nt, k)
            n_correct += int((pred.argmin(dim=1) == 0).sum().item())
            continue
        qe = eng.embed_from_offsets(q.audio, qo, T, ds, wh, windows_per_tower=1).clone()
        se = eng.embed_from_offsets(q.audio, so, T, ds, wh, windows_per_tower=k * n).clone()
        pred = torch.empty(nt, k, dtype=torch.float32, device=eng.device)
        am = torch.empty(nt, dtype=torch.int32, device=eng.device)
        eng._call("vm_nshot_distances", qe.data_ptr(), se.data_ptr(), nt, k, n, eng.E, _DIST[distance], pred.data_ptr(),
                  am.data_ptr(), eng.stream())
        n_correct += int((am == 0).sum().item())
    return n_correct


def _lazy_pair(preprocessor, in1, in2):
    ([a, b], _) = preprocessor(([in1, in2], []))
    return a, b


def _embed_towers(eng, lazy, tower: int):
    """Embed a LazyWindows batch in inference mode with whitening statistics taken per group of ``tower`` windows."""
    import torch
    if isinstance(lazy, LazyWindows):
        return eng.embed(torch.as_tensor(np.ascontiguousarray(lazy.raw, dtype=np.float32)), preprocessed=False,
                         downsampling=lazy.downsampling, whitening=lazy.whitening, windows_per_tower=tower).clone()
    return eng.embed(np.asarray(lazy, dtype=np.float32)).clone()


def _siamese_predict_towers(eng, lazy1, lazy2, tower: int):
    import torch
    if isinstance(lazy1, LazyWindows) and isinstance(lazy2, LazyWindows):
        x = np.concatenate([lazy1.raw, lazy2.raw]).astype(np.float32)
        pairs = lazy1.raw.shape[0]
        eng.embed(torch.as_tensor(x), preprocessed=False, downsampling=lazy1.downsampling, whitening=lazy1.whitening,
                  windows_per_tower=tower)
        pl = eng.plan(2 * pairs, eng.last_infer_l0, False)
        return eng.siamese_head(pl, None).cpu().numpy().copy()
    return eng.siamese_predict(np.asarray(lazy1, dtype=np.float32), np.asarray(lazy2, dtype=np.float32)).cpu().numpy()[:, 0]


class NShotEvaluationCallback(Callback):
    """voicemap/utils.py:219-252: after every epoch evaluate ``num_tasks`` k-way n-shot tasks and store the accuracy in
    ``logs['val_{n}-shot_acc']`` (later callbacks in the list monitor that key)."""

    def __init__(self, num_tasks, n_shot, k_way, dataset, preprocessor=lambda x: x, mode="siamese"):
        super(NShotEvaluationCallback, self).__init__()
        self.num_tasks = num_tasks
        self.n_shot = n_shot
        self.k_way = k_way
        self.dataset = dataset
        self.preprocessor = preprocessor
        assert mode in ("siamese", "classifier", "encoder")
        self.mode = mode

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        n_correct = n_shot_task_evaluation(self.model, self.dataset, self.preprocessor, self.num_tasks, self.n_shot,
                                           self.k_way, network_type=self.mode)
        n_shot_acc = n_correct * 1. / self.num_tasks
        logs["val_{}-shot_acc".format(self.n_shot)] = n_shot_acc
        from . import parallel
        if parallel.rank_world()[0] == 0:   # every rank holds the same (summed) figure; one line like the reference's
            print("val_{}-shot_acc: {:.4f}".format(self.n_shot, n_shot_acc))
