"""One asynchronous host-to-device copy per training step: a byte layout over named host arrays and a ring of pinned staging slots.

torch's ``.to(device)`` of a pageable array is a blocking copy ordered behind everything already enqueued on the stream: three of them
per step made the host wait for the GPU to drain, then left the GPU idle while the host prepared the next step (fit_generator at 64
pairs: 1.67 ms per step against 1.45 ms of GPU work).  A step's offsets, labels and per-window parameters therefore travel as ONE
buffer: ``layout`` places the arrays, ``Ring`` owns 32 pinned and 32 device copies of that buffer.  The device side is a ring as well:
a step reads ITS slot, so the next step's copy needs no ordering against this step's kernels.
"""
from __future__ import annotations

import numpy as np
import torch

SLOTS = 32


def layout(segments):
    """[(name, array)] -> ({name: byte offset}, total bytes): the arrays one after the other in list order, each padded to a multiple
    of 8 bytes, so every segment -- the int64 ones above all -- starts 8-byte aligned."""
    offsets, off = {}, 0
    for name, a in segments:
        offsets[name] = off
        off += (a.nbytes + 7) // 8 * 8
    return offsets, off


def pack(buf: "np.ndarray", segments):
    """Fill the uint8 buffer ``buf`` (at least ``layout(segments)[1]`` bytes; the padding is left as it is) and return the offsets."""
    offsets, total = layout(segments)
    assert buf.dtype == np.uint8 and buf.size >= total
    for name, a in segments:
        o = offsets[name]
        buf[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return offsets


def step_segments(offsets, labels, n_labels: int, label_dtype, aug=None):
    """The segments of one training step: the towers' window offsets (int64, tower after tower), its ``n_labels`` labels (fp32 for the
    siamese losses, int32 class ids otherwise) and, with ``aug`` (the two towers' augment.AugmentRecord), the per-window parameters
    snr_lin, gain (fp32), rir_id (int32) and -- when K > 0 -- the (2 pairs, K) int64 noise offsets."""
    seg = [("offsets", np.concatenate([np.asarray(o, dtype=np.int64).reshape(-1) for o in offsets])),
           ("labels", np.asarray(labels).reshape(n_labels).astype(label_dtype, copy=False))]
    if aug is not None:
        seg += [(f, np.concatenate([getattr(aug[0], f), getattr(aug[1], f)])) for f in ("snr_lin", "gain", "rir_id")]
        if aug[0].K:
            seg.append(("noise_offsets", np.concatenate([aug[0].noise_offsets, aug[1].noise_offsets])))
    return seg


class Ring:
    """32 pinned + 32 device slots of ``nbytes`` each.  A slot is reused after 32 uploads; the step that last read it has its
    end-of-enqueue event (``enqueued``) waited for first (long done)."""

    def __init__(self, nbytes: int, device):
        self.dev = [torch.empty(nbytes, dtype=torch.uint8, device=device) for _ in range(SLOTS)]
        self.pin = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(SLOTS)]
        self.ev = [None] * SLOTS
        self.k = 0

    def upload(self, segments, stream=None):
        """Pack ``segments`` into the next slot and enqueue its copy on ``stream`` (None: the current one).  Returns ({name: device
        view of the array's dtype, flat}, slot); call ``enqueued(slot)`` once the step that reads the views is enqueued."""
        s = self.k % SLOTS
        self.k += 1
        if self.ev[s] is not None:
            self.ev[s].synchronize()
        offsets = pack(self.pin[s].numpy(), segments)
        dev = self.dev[s]
        if stream is not None:
            with torch.cuda.stream(stream):
                dev.copy_(self.pin[s], non_blocking=True)
        else:
            dev.copy_(self.pin[s], non_blocking=True)
        return {name: dev[offsets[name]:offsets[name] + a.nbytes].view(getattr(torch, a.dtype.name)) for name, a in segments}, s

    def enqueued(self, slot: int):
        """The step that reads ``slot`` is enqueued: the slot may be refilled once everything enqueued so far has run."""
        ev = self.ev[slot] = self.ev[slot] or torch.cuda.Event()
        ev.record()
