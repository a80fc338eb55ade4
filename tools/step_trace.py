"""The launch sequence of one step, as text: what HipEncoderEngine enqueues for a configuration -- every C-ABI call with its arguments,
every event record / wait and stream join, every host call -- in a canonical form that two checkouts over the same library can be
diffed on.  Pointers are printed as p<k>, streams as s<k> and events as e<k>, k the order of first appearance within the step; integers,
floats and None exactly.  Behind each replayable training configuration: the per-step slots (``patches``) of the program the store
records on the configuration's second sighting.

    python tools/step_trace.py [name-substring ...] > trace.txt

A change of the engine that claims to leave the step as it is shows an empty diff of this output before and after."""
import ctypes
import sys

import numpy as np
import torch

from voicemap_amd import _lib
from voicemap_amd.engine import HipEncoderEngine

E = 64
_POINTERS = (ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p))


def baseline(f):
    return [(32, f, 4), (3, 2 * f, 2), (3, 3 * f, 2), (3, 4 * f, 2)]


class Trace:
    """Wraps the five funnels of one engine; ``lines`` is the step so far."""

    def __init__(self, eng):
        self.eng, self.lines, self.ids = eng, [], {"p": {}, "s": {}, "e": {}}
        self.streams = {eng.stream()} | {s.cuda_stream for s in (eng.side_stream, eng.tower_stream, eng.misc_stream)}
        for name in ("_call", "_record", "_wait", "_join", "_host_call"):
            setattr(eng, name, self._wrap(getattr(eng, name), getattr(self, name)))

    @staticmethod
    def _wrap(orig, note):
        def both(*a):
            note(*a)
            return orig(*a)
        return both

    def _id(self, kind, key):
        tab = self.ids[kind]
        return "%s%d" % (kind, tab.setdefault(key, len(tab)))

    def _arg(self, v, ctype):
        if v is None:
            return "None"
        if isinstance(v, ctypes.Array):   # a host-side block of pointers / sizes (the batched entry points)
            return "[%s]" % ", ".join(self._arg(x, v._type_) for x in v)
        if ctype in _POINTERS:
            if not isinstance(v, int):
                return "<%s>" % type(v).__name__
            return self._id("s" if v in self.streams else "p", int(v))
        return repr(float(v)) if ctype in (ctypes.c_float, ctypes.c_double) else repr(int(v))

    def _call(self, name, *args):
        types = _lib.SIGNATURES[name][1]
        assert len(types) == len(args), (name, len(types), len(args))
        self.lines.append("%s(%s)" % (name, ", ".join(self._arg(v, t) for v, t in zip(args, types))))

    def _record(self, ev):
        self.lines.append("record %s on %s" % (self._id("e", id(ev)), self._id("s", self.eng.stream())))

    def _wait(self, stream, ev):
        self.lines.append("wait %s for %s" % (self._id("s", stream.cuda_stream), self._id("e", id(ev))))

    def _join(self, waiter, waited):
        self.lines.append("join %s behind %s" % (self._id("s", waiter.cuda_stream), self._id("s", waited.cuda_stream)))

    def _host_call(self, fn):
        self.lines.append("host call")


class StubHook:
    """A gradient hook that does nothing: its presence places the engine's early hand-over of the gradient tail."""

    def begin_tail(self, engine, event):
        pass

    def __call__(self, flat_grads):
        pass


def windows(n, l0, seed=0):
    return np.random.default_rng(seed).normal(0, 1, (n, l0)).astype(np.float32)


def siamese(eng, pairs=4, l0=4064, masks=False):
    x, y = windows(2 * pairs, l0), np.concatenate([np.zeros(pairs // 2), np.ones(pairs - pairs // 2)]).astype(np.float32)
    dm = [torch.ones(2 * pairs, c, device="cuda") for (_, c, _) in eng.blocks] if masks else None
    return lambda: eng.siamese_train_step(x[:pairs], x[pairs:], y, drop_masks=dm)


def classifier(eng):
    x, y = windows(6, 4064), np.arange(6) % 24
    return lambda: eng.classifier_train_step(x, y, drop_masks=None)


def triplet(eng):
    x, y = windows(8, 4064), np.arange(8) // 2
    return lambda: eng.triplet_train_step(x, y, drop_masks=None)


def episode(eng):
    x, y = windows(8, 4064), np.arange(4) % 2
    return lambda: eng.prototypical_train_step(x, y, 2, 2, drop_masks=None)


def resident(eng, pairs=4, raw_len=16256):
    audio = torch.from_numpy(windows(1, 8 * raw_len)[0]).cuda()
    o1, o2 = np.arange(pairs, dtype=np.int64) * 1000, np.arange(pairs, dtype=np.int64) * 1000 + 40000
    y = np.concatenate([np.zeros(pairs // 2), np.ones(pairs - pairs // 2)]).astype(np.float32)
    return lambda: eng.siamese_train_step_from_offsets(audio, o1, o2, y, raw_len, drop_masks=None)


def embed(eng, l0):
    x = windows(8, l0)
    return lambda: eng.embed(x)


def configurations():
    """(name, engine keyword arguments, switches set on the engine, step maker, replayed too?)"""
    sia = dict(f=128, dtype="f16", head="uniform_euclidean")
    out = [("siamese f16", sia, {}, siamese, True),
           ("siamese bf16", dict(sia, dtype="bf16"), {}, siamese, True),
           ("siamese f16, all-ones masks", sia, {}, lambda e: siamese(e, masks=True), True),
           ("fold_pairs=False", sia, {"fold_pairs": False}, siamese, True),
           ("center_blocks=()", sia, {"center_blocks": ()}, siamese, True)]
    for fpe in (False, True):
        out.append(("fold_affine=False fused_pool_extreme=%s" % fpe, sia, {"fold_affine": False, "fused_pool_extreme": fpe}, siamese, True))
    out += [("fused_bn_reduce=False", sia, {"fused_bn_reduce": False}, siamese, True),
            ("pooled_reduce=False fold_affine=False", sia, {"pooled_reduce": False, "fold_affine": False}, siamese, True),
            ("fused_sums_finalize=False", sia, {"fused_sums_finalize": False}, siamese, True),
            ("split_towers=False", sia, {"split_towers": False}, siamese, True),
            ("overlap_wgrad=False", sia, {"overlap_wgrad": False}, siamese, True),
            ("wgrad_after_dgrad=True", sia, {"wgrad_after_dgrad": True}, siamese, True),
            ("tower_stagger=1", sia, {"tower_stagger": 1}, siamese, True),
            ("tower_stagger=2", sia, {"tower_stagger": 2}, siamese, True),
            ("sync_bn=True sync_bn_world=1", sia, {"sync_bn": True, "sync_bn_world": 1}, siamese, False),
            ("stub gradient hook", sia, {"grad_sync": StubHook()}, siamese, False),
            ("classifier, one tower", dict(sia, head="classifier", num_classes=24), {}, classifier, True),
            ("head=None, triplet", dict(sia, head=None), {}, triplet, True),
            ("head=None, prototypical episode", dict(sia, head=None), {}, episode, True)]
    for fpe in (False, True):
        out.append(("baseline(64) 12000 samples fused_pool_extreme=%s" % fpe, dict(sia, f=64), {"fused_pool_extreme": fpe},
                    lambda e: siamese(e, l0=12000), True))
    out += [("baseline(16, 32) f16", dict(sia, f=16, e=32), {}, siamese, True),
            ("baseline(16, 32) f32", dict(sia, f=16, e=32, dtype="f32"), {}, siamese, True),
            ("resident corpus, host offsets", sia, {}, resident, True),
            ("inference embed 4064", sia, {}, lambda e: embed(e, 4064), False),
            ("inference embed 4072", sia, {}, lambda e: embed(e, 4072), False)]
    return out


def engine(kw, switches, replay):
    kw = dict(kw)
    eng = HipEncoderEngine(baseline(kw.pop("f")), kw.pop("e", E), dropout=0.0, seed=1, **kw)
    for k, v in switches.items():
        setattr(eng, k, v)
    eng.replay = replay
    return eng


def main(only):
    for name, kw, switches, make, replayed in configurations():
        if only and not any(o in name for o in only):
            continue
        print("== %s: one eager step" % name)
        eng = engine(kw, switches, False)
        step = make(eng)
        tr = Trace(eng)
        step()
        torch.cuda.synchronize()
        print("\n".join(tr.lines))
        if replayed:
            eng = engine(kw, switches, True)
            step = make(eng)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            progs = eng._programs.recorded()
            assert len(progs) == 1 and progs[0].finished, (name, len(progs))
            print("== %s: patches of the recorded step (command, argument, key)" % name)
            print("\n".join("%d %d %r" % p for p in progs[0].patches))
        sys.stdout.flush()


if __name__ == "__main__":
    main(sys.argv[1:])
