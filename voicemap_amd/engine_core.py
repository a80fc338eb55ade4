"""What the two engines share (engine.py: the waveform encoder; spectro_engine.py: the log-mel + 2-D CNN variant) and nothing else:
the flat fp32 parameter / gradient / Adam store and its initial draw, the funnel every C-ABI call and stream hand-over goes through,
loss scaling, the Adam step and the siamese head with its evaluation and prediction calls.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import VM_BF16, VM_F16, VM_F32, VM_F32S
from .program import DynF, DynI

# "f32s": fp32 storage, split-bf16 products in the k=3 convolution GEMMs (VM_F32S in include/voicemap_hip.h)
# "f16": IEEE half storage -- the bf16 kernels with 11 instead of 8 significand bits per stored value, loss-scaled gradients
_DT = {"f32": VM_F32, "fp32": VM_F32, "float32": VM_F32, "bf16": VM_BF16, "bfloat16": VM_BF16, "f32s": VM_F32S,
       "f16": VM_F16, "fp16": VM_F16, "float16": VM_F16}
_TORCH_DT = {VM_F32: torch.float32, VM_BF16: torch.bfloat16, VM_F32S: torch.float32, VM_F16: torch.float16}
DEFAULT_F16_LOSS_SCALE = 4096.0
# the drop-in surface's default storage mode: the 16-bit one whose embeddings stay within 1e-3 of the reference arithmetic (DESIGN.md
# 4.6b); "bf16" -- BASELINE.json's word for config 2 -- is the same kernels with 8 significand bits (2 % faster, 6e-3)
DEFAULT_DTYPE = "f16"
HEADS = {"uniform_euclidean": _lib.VM_HEAD_UNIFORM_EUCLIDEAN, "weighted_l1": _lib.VM_HEAD_WEIGHTED_L1}
LOSSES = {"contrastive": _lib.VM_LOSS_CONTRASTIVE, "contrastive_loss": _lib.VM_LOSS_CONTRASTIVE,
          "bce": _lib.VM_LOSS_BCE, "binary_crossentropy": _lib.VM_LOSS_BCE}


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _align(n: int, a: int = 64) -> int:
    return (n + a - 1) // a * a


def head_spec(head: Optional[str], embedding_dimension: int, num_classes: int = 0) -> List[Tuple[str, Tuple[int, ...]]]:
    """The parameter tensors behind the embedding: the siamese Dense(1) over a distance, or the classifier's Dense(num_classes)."""
    E = int(embedding_dimension)
    if head is None:
        return []
    if head == "uniform_euclidean":
        return [("head.kernel", (1, 1)), ("head.bias", (1,))]
    if head == "weighted_l1":
        return [("head.kernel", (E, 1)), ("head.bias", (1,))]
    if head == "classifier":
        return [("head.kernel", (E, num_classes)), ("head.bias", (num_classes,))]
    raise NotImplementedError(head)


def spec_layout(spec: Sequence[Tuple[str, Tuple[int, ...]]], bn_channels: Sequence[int]):
    """A parameter spec [(name, stored shape)] and the channel count of every BatchNorm layer -> (offsets {name: (offset, size,
    shape)}, n_flat, nt_off {name: (offset, size)}, n_nt): every tensor starts on a 64-element boundary."""
    offsets: Dict[str, Tuple[int, int, Tuple[int, ...]]] = OrderedDict()
    off = 0
    for name, shape in spec:
        n = int(np.prod(shape))
        offsets[name] = (off, n, shape)
        off += _align(n)
    n_flat = off
    nt_off: Dict[str, Tuple[int, int]] = OrderedDict()
    off = 0
    for i, c in enumerate(bn_channels):
        nt_off[f"bn{i+1}.moving_mean"] = (off, c)
        off += _align(c)
        nt_off[f"bn{i+1}.moving_variance"] = (off, c)
        off += _align(c)
    return offsets, n_flat, nt_off, off


def flat_layout(blocks: Sequence[Tuple[int, int, int]], embedding_dimension: int, head: Optional[str], num_classes: int = 0):
    """Layout of the flat fp32 buffers (parameters / gradients / Adam slots share it): tensors in Keras ``trainable_weights``
    order, each starting on a 64-element boundary, and the non-trainable BatchNorm moving statistics in a second buffer.
    Returns (spec, offsets {name: (offset, size, shape)}, n_flat, nt_off {name: (offset, size)}, n_nt).  Pure host code:
    parallel.py's collectives and the CPU tests use the same layout the engine does."""
    spec: List[Tuple[str, Tuple[int, ...]]] = []
    for i, (k, c, _) in enumerate(blocks):
        cin = 1 if i == 0 else blocks[i - 1][1]
        spec += [(f"conv{i+1}.kernel", (k, cin, c)), (f"conv{i+1}.bias", (c,)),
                 (f"bn{i+1}.gamma", (c,)), (f"bn{i+1}.beta", (c,))]
    E = int(embedding_dimension)
    spec += [("dense.kernel", (blocks[-1][1], E)), ("dense.bias", (E,))] + head_spec(head, E, num_classes)
    return (spec,) + spec_layout(spec, [c for _, c, _ in blocks])


class FlatState:
    """The flat buffers themselves (P parameters, G gradients, M / V Adam slots, NT moving statistics) on ``device``."""

    def __init__(self, blocks, embedding_dimension, head, num_classes, device):
        self._build(flat_layout(blocks, embedding_dimension, head, num_classes)[0], [c for _, c, _ in blocks], device)

    @classmethod
    def from_spec(cls, spec, bn_channels, device) -> "FlatState":
        """``spec`` [(name, stored shape)] in ``trainable_weights`` order, ``bn_channels`` the channels of every BatchNorm layer."""
        st = cls.__new__(cls)
        st._build(spec, bn_channels, device)
        return st

    def _build(self, spec, bn_channels, device):
        self.spec = spec
        self.offsets, self.n_flat, self.nt_off, n_nt = spec_layout(spec, bn_channels)
        self.n_params = sum(n for _, n, _ in self.offsets.values())
        self.P = torch.zeros(self.n_flat, dtype=torch.float32, device=device)
        self.G = torch.zeros_like(self.P)
        self.M = torch.zeros_like(self.P)
        self.V = torch.zeros_like(self.P)
        self.NT = torch.zeros(n_nt, dtype=torch.float32, device=device)
        self.iterations = 0

    def view(self, name: str, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        if name in self.nt_off:
            o, n = self.nt_off[name]
            return self.NT[o:o + n]
        o, n, shape = self.offsets[name]
        return (self.P if buf is None else buf)[o:o + n].view(shape)

    def refresh_weights(self):  # the engine re-derives its GEMM-layout weight copies here
        pass


def initial_params(offsets, seed: int, public_shape=None) -> "OrderedDict[str, np.ndarray]":
    """Keras default initialisers over a layout, as float64 arrays in the tensors' public shapes (``public_shape(name)``; None: the
    stored ones): glorot_uniform kernels -- one draw per kernel, in layout order, from a CPU generator seeded with ``seed``; every
    axis but the last two is the receptive field -- zero biases and beta, gamma 1.  Pure host code: set_params rounds it once to fp32."""
    g = torch.Generator().manual_seed(int(seed))
    params = OrderedDict()
    for name, (_, _, shape) in offsets.items():
        if name.endswith(".kernel"):
            ps = tuple(shape if public_shape is None else public_shape(name))
            field = int(np.prod(ps[:-2]))
            lim = math.sqrt(6.0 / (field * ps[-2] + field * ps[-1]))
            params[name] = ((torch.rand(ps, generator=g, dtype=torch.float64) * 2 - 1) * lim).numpy()
        elif name.endswith(".gamma"):
            params[name] = np.ones(shape)
        else:
            params[name] = np.zeros(shape)
    return params


def require_resident_input(engine_cls):
    """Before offsets into a device-resident buffer or preprocessed windows go to an engine (models.py, utils.py, retrieval.py)."""
    if not engine_cls.resident_input:
        raise NotImplementedError("the spectrogram engine takes raw windows; its front-end is vm_stft_logmel")


# entry points timed under the name (and argument positions) of the plain form: name -> (plain name, argument indices to drop)
_TIMED_AS = {"vm_conv_dgrad_bnred": ("vm_conv_dgrad", ()), "vm_conv_fwd_e": ("vm_conv_fwd", (3,)),
             "vm_conv_fwd_fold": ("vm_conv_fwd", (3, 4, 6, 15)), "vm_conv_wgrad_fold": ("vm_conv_wgrad", (3,)),
             "vm_bn_pool_bwd_apply_pairs": ("vm_bn_pool_bwd_apply", (1,))}


try:
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:   # older torch: the documented way
    def _raw_stream(index):
        return torch.cuda.current_stream(index).cuda_stream


_SHARED_STREAMS: Dict[tuple, "torch.cuda.Stream"] = {}


def _shared_stream(device: torch.device, role: str) -> "torch.cuda.Stream":
    """The process's ONE stream per (device, role) -- every engine's tower / side / misc stream.  The runtime multiplexes streams onto a
    few hardware queues (four by default): with three private streams per engine, the streams of the fourth and sixth engine of a
    process landed on shared queues and their three-stream step ran 7.5 % slower than the first engine's (2.80 against 2.60 ms, every
    launch as fast as before when run serially: tools/probe/placement_spread.py).  Engines of one process enqueue one after the other,
    so sharing the streams costs them nothing."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _SHARED_STREAMS.get((idx, role))
    if st is None:
        st = _SHARED_STREAMS[(idx, role)] = torch.cuda.Stream(device=device)
    return st


class EngineCore:
    """One encoder + optional head on one MI355X: the state and the methods that do not depend on the encoder's architecture.

    A subclass builds its FlatState and hands it to ``__init__`` with the architecture as ``blocks`` [(kernel, channels, pool)], then
    sets its own switches and GEMM-layout weight copies and calls ``init_params(seed)`` last.  It provides
      refresh_weights()                       fp32 master kernels -> the copies its GEMMs read
      plan(n, length, training)               the activation workspaces of one batch shape, cached in ``_plans``
      forward(pl, per_tower, drop_masks), backward(pl, sync_tail)
      _infer(x, preprocessed, downsampling, whitening, windows_per_tower) -> the inference plan of host windows x
      _pair_windows(x1, x2)                   the two towers' windows as one batch, tower 1 first
      make_drop_masks(n, generator)
    and says what it serves in two class attributes: ``losses`` (the names models.py may compile it with) and ``resident_input``
    (it takes offsets into a device-resident buffer and preprocessed windows).  Where its stored kernels differ from the public
    (Keras) ones it overrides ``public_shape`` / ``_to_stored`` / ``_to_public``."""

    losses: frozenset = frozenset()
    resident_input = False
    # the funnel outside a recording: no program, torch's current stream (test doubles of the funnel do not run __init__)
    _rec = None
    _stream_stack = ()

    @classmethod
    def _require_gpu(cls):
        """First line of a subclass's __init__: its FlatState is built on the device before this class's __init__ runs."""
        if not torch.cuda.is_available():
            raise RuntimeError("%s needs a GPU (torch.cuda.is_available() is False); there is no CPU path" % cls.__name__)

    def __init__(self, blocks, embedding_dimension: int, dropout: float, head: Optional[str], num_classes: int, dtype: str, device,
                 bn_eps: float, bn_momentum: float, unbiased_moving_variance: bool, state: FlatState):
        self.lib = _lib.lib()
        self.timed = {}
        self._call("vm_check_device")
        self.blocks = blocks
        self.nb = len(blocks)
        self.E = int(embedding_dimension)
        self.dropout = float(dropout)
        self.head = head
        self.num_classes = int(num_classes)
        self.dtype = _DT[dtype]
        self.tdt = _TORCH_DT[self.dtype]
        self.device = torch.device(device)
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._views = {}
        self.bn_eps, self.bn_momentum = float(bn_eps), float(bn_momentum)
        self.unbiased = bool(unbiased_moving_variance)
        self.is16 = self.dtype in (VM_BF16, VM_F16)
        self._init_loss_scale()
        # the flat parameter store, Keras trainable_weights order
        self.spec, self.offsets, self.n_flat = state.spec, state.offsets, state.n_flat
        self.n_params = sum(int(np.prod(self.public_shape(name))) for name in self.offsets)
        self.P, self.G, self.M, self.V = state.P, state.G, state.M, state.V
        self.nt_off, self.NT = state.nt_off, state.NT
        self._init_zero_debias()
        self._sq_ws = torch.empty(self.lib.query("vm_sqnorm_workspace_bytes", self.n_flat) // 8, dtype=torch.float64, device=self.device)
        self._sqnorm = torch.zeros(1, dtype=torch.float32, device=self.device)
        # Adam(clipnorm=1.) defaults of the reference scripts
        self.lr, self.beta_1, self.beta_2, self.adam_eps, self.decay, self.clipnorm = 1e-3, 0.9, 0.999, 1e-7, 0.0, 1.0
        self.iterations = 0
        self.last_infer_l0 = 0
        # weight-gradient GEMMs only feed the optimizer: they run on a side stream, concurrently with the dgrad -> BN-backward
        # chain of the earlier blocks (the critical path of backward).  Measured +4.5 % step throughput at cfg-A (4.29 -> 4.11
        # ms); the results are bit-identical either way (tests/test_gpu_e2e.py).  Per-kernel timings of the backward pass are
        # only attributable with it off (bench.py --breakdown / --no-overlap-wgrad).
        self.overlap_wgrad = True
        self.defer_head_reduce = False   # backward() enqueues the siamese head's sums itself (the 1-D engine: on its side stream)
        self.grad_sync = None       # callable(flat_grad_tensor) for data parallelism (parallel.py)
        self.grad_prescale = 1.0
        self._plans: Dict[Tuple, dict] = {}
        self._rec = None            # the step being recorded (program.Program)
        self._stream_stack: List[int] = []

    def _init_loss_scale(self):
        """f16 storage: activation gradients of this net are 1e-5 .. 1e-8 per element -- under half's normal range (6e-5) -- so the
        loss gradient is multiplied by loss_scale in the head kernel (every kernel between the head and the optimizer is linear in
        it), the flat gradient buffer G then holds loss_scale x the gradients and the optimizer kernel divides it out again
        (grad_prescale) before the clip; a step whose scaled gradients overflowed (non-finite norm) is skipped on the device and
        counted in ``skipped_steps()``.  1.0 for the other storage types: their arithmetic is untouched."""
        self.loss_scaled = (self.dtype == VM_F16)   # the switch for scaling / skipping -- NOT the scale's value
        self.loss_scale = DEFAULT_F16_LOSS_SCALE if self.loss_scaled else 1.0
        self._skipped = torch.zeros(1, dtype=torch.int32, device=self.device)   # running count, incremented by the optimizer kernel
        self._skip_seen, self._clean_checks = 0, 0
        # dynamic scale driven from optimizer_step (every train_on_batch loop gets it, not only fit_generator): every
        # ``scale_poll_every`` steps the count is copied to pinned memory behind the step; ``scale_poll_lag`` steps later -- a fixed
        # lag, so data-parallel replicas change their scale at the same step -- it is read (the copy is long done: no drain)
        self.scale_poll_every, self.scale_poll_lag = 16, 8
        self.scale_grow_after, self.scale_max, self.scale_min = 2000, 2.0 ** 24, 1.0
        # ... and the scale follows the gradient's SIZE, not only its overflows: the same poll reads the squared norm of the scaled
        # gradient buffer the optimizer kernel leaves behind; under ``scale_norm_low`` (a gradient of norm 1e-6 -- a net whose pairs
        # sit past the contrastive margin -- leaves activation gradients of 1e-10 that 4096 does not lift into half's range: measured
        # 58 % error on the first layer's gradient, 5 % with a scale of 2^20) the scale is multiplied by 8 per poll.  A scaled norm of
        # 2^6 keeps every element 2^10 under half's maximum, so the growth itself cannot overflow the parameter gradients.
        self.scale_norm_low = 64.0
        self.scale_norm_hold_polls, self._norm_growth_hold = 8, 0   # polls without a norm-driven lift after a skipped step
        self._opt_calls, self._clean_steps, self._poll = 0, 0, None
        self._skip_host = torch.zeros(1, dtype=torch.int32).pin_memory() if self.loss_scaled else None
        self._norm_host = torch.zeros(1, dtype=torch.float32).pin_memory() if self.loss_scaled else None

    def _init_zero_debias(self):
        """Keras 2.2.2 BatchNormalization updates its moving statistics with TF 1.10's assign_moving_average(zero_debias=True)
        (keras/backend/tensorflow_backend.py moving_average_update [3P]): per encoder call (tower) and statistic a zero-initialised
        "biased" accumulator and a step counter, moving = biased / (1 - momentum^step).  ZD holds the accumulators of every
        BatchNorm layer as (2 towers, 2 statistics, C) blocks; they are NOT Keras weights (a Keras checkpoint does not carry them:
        after load_model the first update overwrites the moving statistics with the de-biased batch statistics, here as there).
        ``bn_zero_debias = False`` gives the plain exponential average."""
        self.bn_zero_debias = True
        self.zd_off = OrderedDict()
        off = 0
        for i, (_, c, _) in enumerate(self.blocks):
            self.zd_off[i] = (off, c)
            off += 4 * _align(c)
        self.ZD = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.bn_steps = 0

    def _zd(self, i: int):
        """(pointer to the block's accumulators, 1 / (1 - momentum^t)) for the training forward in progress, or (None, 0)."""
        if not self.bn_zero_debias:
            return None, 0.0
        o, c = self.zd_off[i]
        return self.ZD[o:o + 4 * c].data_ptr(), 1.0 / (1.0 - self.bn_momentum ** self._bn_t)

    # ------------------------------------------------------------------------------------------------
    def stream(self):
        # the raw HIP stream of torch's current stream (asked ~25 times per step; torch.cuda.current_stream() costs 8 us a call)
        return self._stream_stack[-1] if self._stream_stack else _raw_stream(self._dev_index)

    def _call(self, name, *args):
        """Enqueue one C-ABI entry point; entry points listed in ``self.timed`` are bracketed by HIP events on the
        launch stream (bench.py uses this for the per-kernel roofline figure)."""
        as_name, drop = _TIMED_AS.get(name, (name, ()))
        rec = self.timed.get(as_name) if self.timed else None
        if rec is None:
            self.lib.call(name, *args)
            if self._rec is not None:
                self._rec.call(getattr(self.lib.cdll, name), name, args)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.lib.call(name, *args)
        e1.record()
        rec.append((e0, e1, tuple(a for k, a in enumerate(args) if k not in drop) + ((name,) if as_name != name else ())))

    # ---- stream hand-overs: through these, so that a recorded step (program.py) carries them ----------------------------------
    def _dyn(self, key, value):
        """Mark a C-ABI argument whose value changes from step to step (None stays None: its presence is part of the configuration)."""
        if self._rec is None or value is None:
            return value
        return DynF(value, key) if isinstance(value, float) else DynI(value, key)

    class _On:
        def __init__(self, eng, stream):
            self.eng, self.stream, self.ctx = eng, stream, torch.cuda.stream(stream)

        def __enter__(self):
            self.ctx.__enter__()
            self.eng._stream_stack.append(self.stream.cuda_stream)

        def __exit__(self, *exc):
            self.eng._stream_stack.pop()
            return self.ctx.__exit__(*exc)

    def _on(self, stream):
        """``with torch.cuda.stream(stream)`` + the raw handle for stream() (no torch lookups inside)."""
        return EngineCore._On(self, stream)

    def _record(self, ev):
        """ev.record() on the current stream."""
        ev.record()
        if self._rec is not None:
            self._rec.record(id(ev), self.stream())

    def _wait(self, stream, ev):
        """stream.wait_event(ev)"""
        stream.wait_event(ev)
        if self._rec is not None:
            self._rec.wait(stream.cuda_stream, id(ev))

    def _join(self, waiter, waited):
        """waiter.wait_stream(waited): everything enqueued on ``waited`` so far precedes what ``waiter`` gets from here on."""
        waiter.wait_stream(waited)
        if self._rec is not None:
            self._rec.join(waiter.cuda_stream, waited.cuda_stream)

    def _host_call(self, fn):
        """A step's host-side call that is not a C-ABI entry point (torch.distributed collectives): run now and, in a step being
        recorded, kept in the program at this position -- a replay calls it again between the same launches."""
        fn()
        if self._rec is not None:
            self._rec.host_call(fn)

    def view(self, name: str, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        # (memoised per (name, buffer): a training step asks ~70 times, and at small batches the step is bound by the host)
        nt = name in self.nt_off
        base = self.NT if nt else (self.P if buf is None else buf)
        key = (name, None if (nt or buf is None) else id(buf))
        v = self._views.get(key)
        if v is not None and v[0] is base:
            return v[1]
        if nt:
            o, n = self.nt_off[name]
            out = self.NT[o:o + n]
        else:
            o, n, shape = self.offsets[name]
            out = base[o:o + n].view(shape)
        self._views[key] = (base, out)
        return out

    # ---- parameters: public (Keras) form <-> the flat store ---------------------------------------------------------------------
    def public_shape(self, name: str) -> Tuple[int, ...]:
        """The shape get_params / set_params speak for a trainable tensor (the stored one unless the engine says otherwise)."""
        return self.offsets[name][2]

    def _to_stored(self, name: str, a: np.ndarray) -> np.ndarray:
        return a

    def _to_public(self, name: str, a: np.ndarray) -> np.ndarray:
        return a

    def init_params(self, seed: Optional[int] = None):
        """Keras default initialisers (glorot_uniform kernels, zero biases, gamma 1, beta 0, moving 0 / 1)."""
        if seed is None:
            # like Keras' unseeded initialisers: a fresh draw per model, reproducible through torch.manual_seed
            # (experiments/_common.seed_everything sets it)
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        self.seed = int(seed)
        # dropout masks come from an engine-owned generator: reproducible under the same seed, decorrelated across
        # data-parallel ranks (every rank holds the same weights but must drop different channels)
        self._drop_gen = torch.Generator(device=self.device)
        self._drop_gen.manual_seed(self.seed * 1000003 + 7919 * (int(os.environ.get("RANK", "0")) + 1))
        self.P.zero_()
        for name, (o, n) in self.nt_off.items():
            self.NT[o:o + n] = 1.0 if name.endswith("moving_variance") else 0.0
        self.M.zero_()
        self.V.zero_()
        self.iterations = 0
        self.ZD.zero_()
        self.bn_steps = 0
        self.set_params(initial_params(self.offsets, self.seed, self.public_shape))

    def set_params(self, params: Dict[str, "np.ndarray"]):
        for name, val in params.items():
            a = self._to_stored(name, np.asarray(val, dtype=np.float32))
            v = self.view(name)
            v.copy_(torch.as_tensor(a).to(self.device).reshape(v.shape))
        self.refresh_weights()

    def get_params(self) -> "OrderedDict[str, np.ndarray]":
        return OrderedDict((name, self._to_public(name, self.view(name).detach().cpu().numpy().copy()))
                           for name in list(self.offsets) + list(self.nt_off))

    def get_grads(self) -> "OrderedDict[str, np.ndarray]":
        """The gradients of the last backward pass (G holds loss_scale x them with f16 storage: divided out here)."""
        inv = np.float32(1.0 / float(self.loss_scale))
        return OrderedDict((name, self._to_public(name, self.view(name, self.G).detach().cpu().numpy().copy()) * inv)
                           for name in self.offsets)

    # ---- loss scale -----------------------------------------------------------------------------------------------------------
    def skipped_steps(self) -> int:
        """Optimizer steps skipped because the loss-scaled gradients were not finite (f16 storage only; synchronises)."""
        return int(self._skipped.item())

    def _account_skips(self, total: int) -> int:
        """``total`` skipped steps so far: the new ones are taken off ``iterations`` again (a skipped step is not an Adam step: its
        bias correction and lr decay must not advance) and reported once."""
        # two readers feed this (the lagged pinned copy of _poll_loss_scale and the live counter of adjust_loss_scale /
        # skipped_steps): a stale total must neither move the watermark backwards nor count a step twice
        new = max(0, total - self._skip_seen)
        self._skip_seen = max(self._skip_seen, total)
        if new > 0:
            self.iterations = max(0, self.iterations - new)
            import warnings
            warnings.warn("f16 storage: %d optimizer step(s) skipped (non-finite loss-scaled gradients, scale %g); %d in total"
                          % (new, self.loss_scale, total), RuntimeWarning, stacklevel=3)
        return new

    def adjust_loss_scale(self, grow_after: int = 4, max_scale: float = 65536.0) -> float:
        """Dynamic loss scaling at the caller's cadence (one device read per call; ``optimizer_step`` does the same on its own
        without a read on the critical path, see ``_poll_loss_scale``): steps were skipped since the last look -> halve the scale
        once per skipped step (at most 2^-4); none for ``grow_after`` calls in a row -> double it.  No-op for the storage types
        that do not scale.  The scale may reach ``scale_min`` (1.0) and grows back from there."""
        if not self.loss_scaled:
            return 1.0
        new = self._account_skips(self.skipped_steps())
        self._poll = None   # a copy in flight predates this read: consumed here, not a second time 8 steps later
        if new > 0:
            self.loss_scale = max(self.loss_scale / float(2 ** min(new, 4)), self.scale_min)
            self._clean_checks = self._clean_steps = 0
            self._norm_growth_hold = self.scale_norm_hold_polls
        else:
            self._clean_checks += 1
            if self._clean_checks >= grow_after:
                self.loss_scale = min(self.loss_scale * 2.0, max_scale)
                self._clean_checks = 0
        return self.loss_scale

    def calibrate_loss_scale(self, run_backward, max_rounds: int = 8) -> float:
        """The norm-driven part of the loss-scale search, synchronously: ``run_backward()`` runs one forward + backward (no update)
        and leaves the scaled gradient in G; while its norm (as Adam will see it after grad_prescale) is under ``scale_norm_low`` the
        scale is multiplied by 8 -- what ``_poll_loss_scale`` does every ``scale_poll_every`` steps of a training loop -- and halved
        on an overflow.  For callers that take ONE step from a cold start (tests, a first evaluation of gradients)."""
        if not self.loss_scaled:
            return 1.0
        for _ in range(max_rounds):
            run_backward()
            g = float(self.G.double().norm().item()) * float(self.grad_prescale)
            if not math.isfinite(g):
                self.loss_scale = max(self.loss_scale / 2.0, self.scale_min)
            elif 0.0 < g < self.scale_norm_low and self.loss_scale < self.scale_max:
                self.loss_scale = min(self.loss_scale * 8.0, self.scale_max)
            else:
                break
        return self.loss_scale

    def _poll_loss_scale(self):
        """Called once per optimizer step (f16 storage).  Step k with k % scale_poll_every == 0 enqueues a copy of the device's skip
        count to pinned memory; step k + scale_poll_lag consumes it."""
        k = self._opt_calls
        self._opt_calls += 1
        if self._poll is not None and k >= self._poll[0] + self.scale_poll_lag:
            k0, ev = self._poll
            self._poll = None
            ev.synchronize()   # enqueued scale_poll_lag steps ago
            new = self._account_skips(int(self._skip_host[0]))
            sq = float(self._norm_host[0])   # sum of squares of the scaled gradient buffer at the polled step (inf / nan: a skipped one)
            # G holds the SUM over data-parallel ranks; grad_prescale (1 / world) is applied in the clip: compare what Adam sees
            sq *= float(self.grad_prescale) ** 2
            if new > 0:
                self.loss_scale = max(self.loss_scale / float(2 ** min(new, 4)), self.scale_min)
                self._clean_steps = 0
                self._norm_growth_hold = self.scale_norm_hold_polls   # no x8 lifts right after an overflow (limit cycle)
            elif (math.isfinite(sq) and 0.0 < sq < self.scale_norm_low ** 2 and self.loss_scale < self.scale_max
                  and self._norm_growth_hold == 0):
                self.loss_scale = min(self.loss_scale * 8.0, self.scale_max)   # a tiny gradient: lift it (see _init_loss_scale)
                self._clean_steps = 0
            else:
                self._norm_growth_hold = max(0, self._norm_growth_hold - 1)
                self._clean_steps += self.scale_poll_every
                if self._clean_steps >= self.scale_grow_after:
                    self.loss_scale = min(self.loss_scale * 2.0, self.scale_max)
                    self._clean_steps = 0
        if self._poll is None and k % self.scale_poll_every == 0:
            with torch.cuda.stream(torch.cuda.current_stream(self.device)):
                self._skip_host.copy_(self._skipped, non_blocking=True)
                self._norm_host.copy_(self._sqnorm, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
            self._poll = (k, ev)

    # ---- the optimizer --------------------------------------------------------------------------------------------------------
    def _adam_scalars(self):
        """(t, lr_t) of the Adam step about to run (Keras: lr decays with the iteration count BEFORE this step)."""
        lr = self.lr
        if self.decay > 0:
            lr = lr * (1.0 / (1.0 + self.decay * self.iterations))
        t = self.iterations + 1
        return t, lr * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def optimizer_step(self):
        """Keras Adam(clipnorm) on the flat buffers (after the optional data-parallel gradient sum)."""
        if self.grad_sync is not None:
            gs, G = self.grad_sync, self.G
            self._host_call(lambda: gs(G))
        lib, st = self.lib, self.stream()
        skip = self.loss_scaled   # loss-scaled storage: a non-finite gradient norm skips the update on the device
        if (self.clipnorm and self.clipnorm > 0) or skip:
            self._call("vm_grad_sqnorm", _p(self.G), self.n_flat, _p(self._sq_ws), None, st)   # partials; the optimizer kernel adds them
        t, lr_t = self._adam_scalars()
        self._call("vm_adam_clip_step", _p(self.P), _p(self.G), _p(self.M), _p(self.V), self.n_flat, self._dyn("lr_t", float(lr_t)), self.beta_1,
                 self.beta_2, self.adam_eps, float(self.clipnorm or 0.0),
                 self._dyn("gpre", float(self.grad_prescale) / float(self.loss_scale)),
                 _p(self._sqnorm), _p(self._sq_ws), int(skip), _p(self._skipped) if skip else None, st)
        self.iterations = t
        if skip and self._rec is None:
            self._poll_loss_scale()   # after the launch: the copy it may enqueue sees this step's count
        self.refresh_weights()
        if skip and self._rec is not None:
            self._poll_loss_scale()   # a step being recorded: torch's copies stay out of the recorded list and go behind it, as in a replay

    # ---- the siamese head, its evaluation and prediction ------------------------------------------------------------------------
    def siamese_head(self, pl: dict, y: Optional[torch.Tensor], loss: str = "contrastive"):
        """Twin distance -> Dense(1, sigmoid) -> loss (+ backward into pl['demb'] and the head gradients)."""
        assert self.head in HEADS, "engine was built without a siamese head"
        pairs = pl["n"] // 2
        G = self.G
        train = y is not None
        # training with the side stream on: only the per-pair pass here; the fixed-order sums (loss, accuracy, head gradients --
        # nobody's input before the optimizer) are enqueued on the side stream by backward()
        if pl.get("tail_pending"):
            assert train, "forward(defer_tail=True) must be followed by siamese_head with labels"
            cl, parts, seg = self.blocks[-1][1], pl["gmax_ws"], self._seg_rows
            pv = parts.data_ptr() if pl["tail_parts"] else None
            pi = parts.data_ptr() + pl["n"] * seg * cl * 4 if pl["tail_parts"] else None
            self._call("vm_tail_fwd_bwd", pv, pi, seg, _p(pl["gmax"]), _p(pl["gidx"]), _p(self.view("dense.kernel")), _p(self.view("dense.bias")),
                       _p(self.view("head.kernel")), _p(self.view("head.bias")), self._dyn("y", _p(y)), pairs, cl, self.E, HEADS[self.head],
                       LOSSES[loss], self._dyn("loss_scale", float(self.loss_scale)), _p(pl["emb"]), _p(pl["pred"]), _p(pl["demb"]), _p(pl["dgmax"]), _p(pl["head_ws"]), self.stream())
            pl["tail_pending"], pl["tail_grads_pending"], pl["head_pending"] = False, True, False
            return pl["pred"][:pairs]
        defer = train and self.overlap_wgrad and pl["training"] and self.defer_head_reduce
        self._call("vm_siamese_head_loss", _p(pl["emb"]), _p(self.view("head.kernel")), _p(self.view("head.bias")),
                      self._dyn("y", _p(y)), pairs, self.E, HEADS[self.head], LOSSES[loss], self._dyn("loss_scale", float(self.loss_scale)),
                      _p(pl["pred"]),
                      _p(pl["loss_acc"]) if (train and not defer) else None, _p(pl["demb"]) if train else None,
                      _p(self.view("head.kernel", G)) if train else None, _p(self.view("head.bias", G)) if train else None,
                      _p(pl["head_ws"]), self.stream())
        pl["head_pending"] = defer
        return pl["pred"][:pairs]

    def _target(self, y, n: int, dt) -> torch.Tensor:
        """Labels -> (n,) device tensor: fp32 for the siamese losses (converted on the host), int32 class ids (on the device)."""
        if dt == torch.float32:
            return torch.as_tensor(y, dtype=dt).reshape(n).to(self.device).contiguous()
        return torch.as_tensor(y).reshape(n).to(self.device, dt).contiguous()

    def siamese_eval(self, x1, x2, y, loss: str = "contrastive", preprocessed: bool = True, downsampling: int = 4,
                     whitening: bool = True):
        """test_on_batch of the siamese model: inference-mode forward + loss / accuracy (no gradients are used; the
        head kernel writes its backward outputs into scratch)."""
        x = self._pair_windows(x1, x2)
        pairs = x.shape[0] // 2
        pl = self._infer(x, preprocessed, downsampling, whitening, pairs)
        yd = self._target(y, pairs, torch.float32)
        if "scratch" not in pl:
            pl["scratch"] = torch.empty(2 * pairs * self.E + self.E + 8, dtype=torch.float32, device=self.device)
        sc = pl["scratch"]
        off = 2 * pairs * self.E
        self._call("vm_siamese_head_loss", _p(pl["emb"]), _p(self.view("head.kernel")), _p(self.view("head.bias")), _p(yd),
                   pairs, self.E, HEADS[self.head], LOSSES[loss], 1.0, _p(pl["pred"]), _p(pl["loss_acc"]), _p(sc),
                   sc.data_ptr() + 4 * off, sc.data_ptr() + 4 * (off + self.E), _p(pl["head_ws"]), self.stream())
        return pl

    def siamese_predict(self, x1, x2, preprocessed: bool = True, downsampling: int = 4, whitening: bool = True):
        """siamese.predict([x1, x2]) -> (pairs, 1) probabilities (inference-mode BN)."""
        x = self._pair_windows(x1, x2)
        pairs = x.shape[0] // 2
        return self.siamese_head(self._infer(x, preprocessed, downsampling, whitening, pairs), None).reshape(pairs, 1)
