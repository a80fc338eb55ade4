"""Hard-pair mining for siamese training (new; the reference samples every pair uniformly: voicemap/librispeech.py:139-177).

After a few epochs nearly every uniformly drawn different-speaker pair lies beyond the contrastive margin (or is classified with
p ~ 1 by the sigmoid head) and its gradient is ~0.  Mining picks, from the embeddings of the model being trained, per file its
``k_neg`` NEAREST files of other speakers and its ``k_pos`` FARTHEST files of its own speaker (``vm_mine_pairs``, csrc/mine.hip: score
and small-K selection in one pass, only the (N, K) lists leave the chip), and ``HardPairSampler`` draws a fraction of every batch from
those lists.  ``HardPairMiner`` is the callback that re-embeds and re-mines between epochs.

The contract of the selection is restated on a given score matrix by ``mine_pairs_numpy``: the reference of the tests.  Nothing here
claims better convergence: whether mined pairs lower the EER on LibriSpeech has not been measured.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, parallel
from .keras_like import Callback
from .verification import score_keys

_DIST = _lib.DIST
MAX_K = 64   # csrc/mine.hip MN_MAX_K: a list is one entry per lane of a wave
_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the contract on a score matrix ------------------------------------------------------------------------------------------------
def _take(entry, eligible, k, scores_row, idx_out, val_out):
    e = np.where(eligible, entry, _NONE)
    if k < len(e):
        part = np.argpartition(e, k - 1)[:k]
    else:
        part = np.arange(len(e))
    part = part[np.argsort(e[part], kind="stable")]
    part = part[e[part] != _NONE]
    idx_out[:len(part)] = part
    val_out[:len(part)] = scores_row[part]


def mine_pairs_numpy(scores, label, k_neg: int, k_pos: int, row0: int = 0, neg_floor=None):
    """numpy twin of ``vm_mine_pairs`` on a given (M, N) fp32 score matrix (row m = anchor ``row0 + m``, lower = more alike):
    (neg_idx (M, k_neg) int32, neg_val fp32, pos_idx (M, k_pos), pos_val).  A candidate j != anchor with ``label[j] >= 0`` and a
    non-NaN score takes part; an anchor with a negative label gets empty lists.  Negatives: another label and, with ``neg_floor`` (M),
    key(score) > key(floor) (a NaN floor: none); the k_neg smallest by (key, j).  Positives: the same label; the k_pos largest by key,
    ties to the lower j.  The key is ``verification.score_keys`` (-0.0 as +0.0).  Unused slots: -1 / NaN.  It scores nothing itself."""
    s = np.ascontiguousarray(np.asarray(scores, dtype=np.float32))
    M, N = s.shape
    label = np.asarray(label).astype(np.int64).reshape(-1)
    assert len(label) == N and 0 <= row0 and row0 + M <= N
    floor = None if neg_floor is None else np.asarray(neg_floor, dtype=np.float32).reshape(-1)
    neg_idx, pos_idx = np.full((M, k_neg), -1, np.int32), np.full((M, k_pos), -1, np.int32)
    neg_val, pos_val = np.full((M, k_neg), np.nan, np.float32), np.full((M, k_pos), np.nan, np.float32)
    cols = np.arange(N, dtype=np.uint64)
    labelled = label >= 0
    for m in range(M):
        i = row0 + m
        if label[i] < 0:
            continue
        key = score_keys(s[m]).astype(np.uint64)
        ok = labelled & ~np.isnan(s[m])
        ok[i] = False
        same = label == label[i]
        if k_neg:
            neg = ok & ~same
            if floor is not None and not np.isnan(floor[m]):
                neg &= key > np.uint64(score_keys(floor[m:m + 1])[0])
            _take((key << np.uint64(32)) | cols, neg, k_neg, s[m], neg_idx[m], neg_val[m])
        if k_pos:
            _take(((key ^ np.uint64(0xFFFFFFFF)) << np.uint64(32)) | cols, ok & same, k_pos, s[m], pos_idx[m], pos_val[m])
    return neg_idx, neg_val, pos_idx, pos_val


# ---- the device call ----------------------------------------------------------------------------------------------------------------
def mine_rows(emb: torch.Tensor, label: torch.Tensor, kind: int, rows: Tuple[int, int], k_neg: int, k_pos: int,
              neg_floor: Optional[torch.Tensor] = None):
    """``vm_mine_pairs`` on device tensors: emb (N, E) fp32, label (N) int32, anchors ``rows = (lo, hi)``, neg_floor (hi - lo) fp32 or
    None -> (neg_idx, neg_val, pos_idx, pos_val) on the device ((hi - lo, 0) tensors for a list that was not asked for)."""
    lib = _lib.lib()
    dev = emb.device
    emb = emb.contiguous()
    label = label.to(device=dev, dtype=torch.int32).contiguous()
    N, E = emb.shape
    lo, hi = int(rows[0]), int(rows[1])
    M = hi - lo
    neg_idx = torch.empty(M, k_neg, dtype=torch.int32, device=dev)
    pos_idx = torch.empty(M, k_pos, dtype=torch.int32, device=dev)
    neg_val = torch.empty(M, k_neg, dtype=torch.float32, device=dev)
    pos_val = torch.empty(M, k_pos, dtype=torch.float32, device=dev)
    if neg_floor is not None:
        neg_floor = neg_floor.to(device=dev, dtype=torch.float32).contiguous()
        if neg_floor.numel() != M:
            raise ValueError("neg_floor must hold one value per anchor row")
    ws = lib.workspace("vm_mine_pairs_workspace_bytes", N, E, lo, hi, k_neg, k_pos, device=dev)
    ptr = lambda t, k: t.data_ptr() if k > 0 else None
    lib.call("vm_mine_pairs", emb.data_ptr(), label.data_ptr(), N, E, kind, lo, hi, k_neg, k_pos,
             None if neg_floor is None else neg_floor.data_ptr(), ptr(neg_idx, k_neg), ptr(neg_val, k_neg), ptr(pos_idx, k_pos),
             ptr(pos_val, k_pos), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return neg_idx, neg_val, pos_idx, pos_val


class MinedPairs:
    """The mined lists of a corpus: ``neg_idx`` (M, k_neg) int32 / ``neg_val`` fp32 and ``pos_idx`` / ``pos_val`` (M, k_pos) as numpy
    arrays (row m = file ``rows[0] + m``; -1 / NaN where a list ends), the ``distance`` they were mined under, and a summary:
    ``neg_mean`` / ``pos_mean`` = the mean hardest-negative / hardest-positive score over the anchors that have one, ``pos_fraction`` =
    the share of anchors with at least one positive."""

    def __init__(self, neg_idx, neg_val, pos_idx, pos_val, distance: str, rows: Tuple[int, int], semi_hard: bool = False):
        self.neg_idx, self.neg_val = np.asarray(neg_idx, np.int32), np.asarray(neg_val, np.float32)
        self.pos_idx, self.pos_val = np.asarray(pos_idx, np.int32), np.asarray(pos_val, np.float32)
        self.distance, self.rows, self.semi_hard = distance, (int(rows[0]), int(rows[1])), bool(semi_hard)

        def first_mean(idx, val):
            if idx.shape[1] == 0:
                return float("nan")
            have = idx[:, 0] >= 0
            return float(val[have, 0].astype(np.float64).mean()) if have.any() else float("nan")
        self.neg_mean = first_mean(self.neg_idx, self.neg_val)
        self.pos_mean = first_mean(self.pos_idx, self.pos_val)
        self.pos_fraction = float((self.pos_idx[:, 0] >= 0).mean()) if self.pos_idx.size else 0.0

    @property
    def k_neg(self) -> int:
        return int(self.neg_idx.shape[1])

    @property
    def k_pos(self) -> int:
        return int(self.pos_idx.shape[1])


def dense_labels(speaker) -> np.ndarray:
    """The dense speaker index of every row (``np.unique`` order, as ``enrolment.enrol`` builds it)."""
    return np.unique(np.asarray(speaker), return_inverse=True)[1].astype(np.int32).reshape(-1)


def mine_pairs(cache, distance: str = "euclidean", k_neg: int = 8, k_pos: int = 4, semi_hard: bool = False,
               rows: Optional[Tuple[int, int]] = None) -> MinedPairs:
    """Mine every row of an ``EmbeddingCache`` against all the others under ``distance``.  ``semi_hard``: the positives are mined first
    and a row's negatives must lie beyond its hardest positive (``neg_floor = pos_val[:, 0]``; a row without a positive has no floor).
    ``rows = (lo, hi)``: only those anchors, no communication.  Otherwise, under torchrun, every rank mines ``parallel.shard_range`` of
    the rows and the lists are all-gathered like ``embed_corpus``'s rows."""
    if distance not in _DIST:
        raise ValueError("Distance must be in (euclidean, cosine, dot_product)")
    if not (0 <= k_neg <= MAX_K and 0 <= k_pos <= MAX_K and k_neg + k_pos > 0):
        raise ValueError("k_neg and k_pos must be in [0, %d] and not both zero" % MAX_K)
    if semi_hard and (k_pos < 1 or k_neg < 1):
        raise ValueError("semi_hard needs k_pos >= 1 (the floor is the hardest positive) and k_neg >= 1")
    kind = _DIST[distance]
    label = torch.as_tensor(dense_labels(cache.speaker)).to(cache.emb.device)
    rank, world = parallel.rank_world()
    lo, hi = rows if rows is not None else parallel.shard_range(cache.n, rank, world)
    if semi_hard:
        _, _, pi, pv = mine_rows(cache.emb, label, kind, (lo, hi), 0, k_pos)
        ni, nv, _, _ = mine_rows(cache.emb, label, kind, (lo, hi), k_neg, 0, neg_floor=pv[:, 0])
    else:
        ni, nv, pi, pv = mine_rows(cache.emb, label, kind, (lo, hi), k_neg, k_pos)
    if rows is None and world > 1:
        ni, nv, pi, pv = (parallel.all_gather_rows(t, cache.n) if t.shape[1] else torch.empty(cache.n, 0, dtype=t.dtype, device=t.device)
                          for t in (ni, nv, pi, pv))
        lo, hi = 0, cache.n
    return MinedPairs(ni.cpu().numpy(), nv.cpu().numpy(), pi.cpu().numpy(), pv.cpu().numpy(), distance, (lo, hi), semi_hard)


# ---- sampling ------------------------------------------------------------------------------------------------------------------------
class HardPairSampler:
    """Verification batches in which a fraction of the pairs is drawn from mined lists.  The methods and the shapes are the dataset's
    (``build_verification_batch``, ``yield_verification_batches`` and, over a ``ShardedSpeechDataset``, the ``_device`` forms):
    ``batchsize // 2`` same-speaker pairs, then as many different-speaker pairs; outputs zeros then ones.

    In each half the first ``round(hard_fraction * half)`` pairs are mined: the anchor is drawn uniformly among the rows whose list is
    not empty, the partner uniformly among that row's valid slots (a half whose pool is empty draws no mined pair); the rest come from
    the dataset's own ``get_alike_pairs`` / ``get_differing_pairs``.  Fragments are chosen as the dataset chooses them.  The mined draws
    use the sampler's own ``RandomState(seed)``; the dataset keeps drawing from ``np.random`` -- so with ``hard_fraction = 0`` or
    ``mined = None`` the batches AND the consumption of ``np.random`` are exactly the dataset's."""

    def __init__(self, dataset, mined: Optional[MinedPairs] = None, hard_fraction: float = 0.5, seed: int = 0):
        if not 0.0 <= hard_fraction <= 1.0:
            raise ValueError("hard_fraction must be in [0, 1]")
        self.dataset, self.hard_fraction = dataset, float(hard_fraction)
        self.rng = np.random.RandomState(seed)
        self._pools = None
        self.mined = None
        self.update(mined)

    def update(self, mined: Optional[MinedPairs]):
        """Swap the pools: the next batch that is built draws from ``mined`` (None: no mined pairs)."""
        pools = None
        if mined is not None:
            if mined.rows != (0, len(self.dataset)):
                raise ValueError("the mined lists must cover every file of the dataset (rows %r, %d files)" % (mined.rows, len(self.dataset)))
            pools = tuple((np.flatnonzero((idx >= 0).any(axis=1)) if idx.shape[1] else np.zeros(0, np.int64), idx)
                          for idx in (mined.pos_idx, mined.neg_idx))
        self.mined, self._pools = mined, pools   # one assignment each: a producer thread sees the old or the new pools

    def _mined_pairs(self, which: int, n: int):
        anchors_ok, idx = self._pools[which]
        a = anchors_ok[self.rng.randint(0, len(anchors_ok), size=n)]
        valid = (idx[a] >= 0)
        cnt = valid.sum(axis=1)
        pick = (self.rng.random_sample(n) * cnt).astype(np.int64)   # uniform over each row's valid slots
        pick = np.minimum(pick, cnt - 1)
        # the valid slots of a row are its first cnt ones (the lists are padded at the end)
        return list(zip(a.tolist(), idx[a, pick].tolist()))

    def _pairs(self, which: int, half: int):
        pools = self._pools
        n_hard = 0
        if pools is not None and self.hard_fraction > 0 and len(pools[which][0]):
            n_hard = int(round(self.hard_fraction * half))
        pairs = self._mined_pairs(which, n_hard) if n_hard else []
        if half - n_hard > 0:
            draw = self.dataset.get_differing_pairs if which else self.dataset.get_alike_pairs
            pairs = pairs + list(draw(half - n_hard))
        return pairs

    def verification_pairs(self, batchsize: int):
        """(alike, differing): the two lists of (file id, file id) of one batch, WITHOUT their fragments (host tests, diagnostics)."""
        half = batchsize // 2
        return self._pairs(0, half), self._pairs(1, half)

    def build_verification_batch(self, batchsize: int):
        ds = self.dataset
        half = batchsize // 2
        # the dataset's order of np.random draws (librispeech.build_verification_batch): alike pairs, their fragments, differing pairs, theirs
        alike = self._pairs(0, half)
        left = [ds[i][0] for i, _ in alike]
        right = [ds[j][0] for _, j in alike]
        differing = self._pairs(1, half)
        left += [ds[i][0] for i, _ in differing]
        right += [ds[j][0] for _, j in differing]
        input_1 = np.stack(left)[:, :, np.newaxis]
        input_2 = np.stack(right)[:, :, np.newaxis]
        outputs = np.append(np.zeros(half), np.ones(half))[:, np.newaxis]
        return [input_1, input_2], outputs

    def yield_verification_batches(self, batchsize: int):
        while True:
            yield self.build_verification_batch(batchsize)

    def build_verification_batch_offsets(self, batchsize: int, files: bool = False):
        ds = self.dataset
        half = batchsize // 2
        alike = self._pairs(0, half)
        l_a = ds.window_starts([i for i, _ in alike])
        r_a = ds.window_starts([j for _, j in alike])
        differing = self._pairs(1, half)
        l_d = ds.window_starts([i for i, _ in differing])
        r_d = ds.window_starts([j for _, j in differing])
        outputs = np.append(np.zeros(half), np.ones(half))[:, np.newaxis]
        out = (np.concatenate([l_a, l_d]), np.concatenate([r_a, r_d]), outputs)
        if files:   # the file id every window was cut from (augment.AugmentPolicy keeps a window's own speaker out of its babble)
            pairs = list(alike) + list(differing)
            out += (np.array([i for i, _ in pairs], dtype=np.int64), np.array([j for _, j in pairs], dtype=np.int64))
        return out

    def build_verification_batch_device(self, batchsize: int, augment=None):
        """``augment``: an ``augment.AugmentPolicy`` (its own random stream: the pairs and crops stay the ones drawn without it)."""
        from .shards import DeviceWindows, augmented_pair
        ds = self.dataset
        assert getattr(ds, "device_audio", None) is not None, 'call to_device() first'
        T = ds.fragment_length
        if augment is None:
            o1, o2, outputs = self.build_verification_batch_offsets(batchsize)
            return [DeviceWindows(ds.device_audio, o1, T), DeviceWindows(ds.device_audio, o2, T)], outputs
        o1, o2, outputs, f1, f2 = self.build_verification_batch_offsets(batchsize, files=True)
        return augmented_pair(ds, augment, o1, o2, f1, f2), outputs

    def yield_verification_batches_device(self, batchsize: int, augment=None):
        while True:
            yield self.build_verification_batch_device(batchsize, augment)


class HardPairMiner(Callback):
    """Keeps a ``HardPairSampler``'s pools current: at the start of training and after every ``every``-th epoch the training files are
    embedded with the model being trained (``embed_corpus``: inference mode, first fragment per file), mined (``mine_pairs`` with
    ``mine_kwargs``: distance, k_neg, k_pos, semi_hard) and handed to ``sampler.update``.  ``mined_neg_mean`` / ``mined_pos_mean`` (the
    mean hardest-negative / hardest-positive score of the pools now in use) go into the epoch logs: list it BEFORE ``CSVLogger``.
    Batches that producer threads built ahead (``fit_generator(workers > 0)``) still come from the previous pools."""

    def __init__(self, sampler: HardPairSampler, dataset, preprocessor, every: int = 1, network_type: str = "siamese", **mine_kwargs):
        super().__init__()
        if every < 1:
            raise ValueError("every must be >= 1")
        self.sampler, self.dataset, self.preprocessor = sampler, dataset, preprocessor
        self.every, self.network_type, self.mine_kwargs = int(every), network_type, mine_kwargs
        self.refreshes = 0

    def refresh(self) -> MinedPairs:
        from .retrieval import embed_corpus
        cache = embed_corpus(self.model, self.dataset, self.preprocessor, network_type=self.network_type)
        mined = mine_pairs(cache, **self.mine_kwargs)
        self.sampler.update(mined)
        self.refreshes += 1
        return mined

    def on_train_begin(self, logs=None):
        self.refresh()

    def on_epoch_end(self, epoch, logs=None):
        if (epoch + 1) % self.every == 0:
            self.refresh()
        if logs is not None and self.sampler.mined is not None:
            logs["mined_neg_mean"] = self.sampler.mined.neg_mean
            logs["mined_pos_mean"] = self.sampler.mined.pos_mean
