"""A recorded training step: the C-ABI calls, event records / waits and host calls one step enqueued, kept as a list that is replayed
while the step's configuration stays the same, and the store of such lists per configuration.  The reference runs the same
train_on_batch 500 times per epoch (experiments/train_siamese.py:65-94); at its batch sizes (32 / 64 pairs) the step here is bound by
the HOST deriving ~55 argument lists and stream hand-overs through Python, not by the GPU -- replaying the recorded list costs a third
of it.  Needs a library handle (voicemap_amd/_lib.py, or a stub with the same ``call`` / ``cdll`` / ``program_table``) and nothing of
the network: voicemap_amd/engine.py feeds it through its _call / _record / _wait / _join / _host_call funnels."""
import ctypes
import struct

import numpy as np


class DynI(int):
    """An integer C-ABI argument (a pointer, normally) that changes from step to step: recorded as a patch slot of the Program."""
    def __new__(cls, value, key):
        o = int.__new__(cls, value)
        o.key = key
        return o


class DynF(float):
    def __new__(cls, value, key):
        o = float.__new__(cls, value)
        o.key = key
        return o


def _word(v, t):
    """One argument as the int64 word vm_program_run expects: pointers / integers as they are, floats / doubles as their bits."""
    if t == "F":
        return struct.unpack("<I", struct.pack("<f", float(v)))[0]
    if t == "D":
        return struct.unpack("<q", struct.pack("<d", float(v)))[0]
    if v is None:
        return 0
    if isinstance(v, (ctypes.Array, ctypes.Structure)):   # a host-side argument block (pointer / size tables of the batched entry
        v = ctypes.addressof(v)                           # points): its address -- the object stays alive in the program's list
    elif isinstance(v, ctypes._SimpleCData):
        v = v.value or 0
    v = int(v)
    return v - (1 << 64) if v >= (1 << 63) else v


class Program:
    """One training step as a flat list of what the host enqueued -- [0, cfunc, args, name] C-ABI calls, [1, event, stream] records,
    [2, stream, event] waits, [3, fn, None, "host call"] host calls -- plus the (command, argument, key) slots whose value changes per
    step (input / label / mask pointers, the BatchNorm zero-debias factor, the loss scale, Adam's lr_t)."""

    def __init__(self):
        self.cmds, self.patches, self.events = [], [], {}
        self.finished = False
        # the same list for the library's own runner (vm_program_run): segments -- int64 word arrays, or host calls between them -- and
        # the (segment, word index, type, key) of every per-step slot; None: this program replays through the Python loop
        self.native = None

    # ---- recording ---------------------------------------------------------------------------------------------------------------
    def call(self, cfunc, name, args):
        """The C-ABI call ``name(*args)``; DynI / DynF arguments become patch slots and are stored as plain numbers."""
        a = list(args)
        for j, v in enumerate(a):
            if isinstance(v, (DynI, DynF)):
                self.patches.append((len(self.cmds), j, v.key))
                a[j] = int(v) if isinstance(v, DynI) else float(v)
        self.cmds.append([0, cfunc, a, name])

    def record(self, event_key, stream):
        self.cmds.append([1, event_key, stream])

    def wait(self, stream, event_key):
        self.cmds.append([2, stream, event_key])

    def join(self, waiter, waited):
        """``waiter`` waits for everything ``waited`` holds so far: an event of its own, recorded and waited for on the spot."""
        key = ("join", len(self.cmds))
        self.record(key, waited)
        self.wait(waiter, key)

    def host_call(self, fn):
        self.cmds.append([3, fn, None, "host call"])

    # ---- replay ------------------------------------------------------------------------------------------------------------------
    def finish(self, lib):
        """Event keys -> events of the program's own (created once; a replay never touches torch's events), and the native form."""
        for c in self.cmds:
            if c[0] == 0 or c[0] == 3:
                continue
            slot = 1 if c[0] == 1 else 2
            h = self.events.get(c[slot])
            if h is None:
                out = ctypes.c_void_p()
                lib.call("vm_event_create", ctypes.byref(out))
                h = self.events[c[slot]] = out.value
            c[slot] = h
        self._ev_record, self._ev_wait = lib.cdll.vm_event_record, lib.cdll.vm_stream_wait_event
        self._fail_at = ctypes.c_int64(0)
        self._fail_ref = ctypes.byref(self._fail_at)
        self.native = self._native(lib.program_table())
        self.finished = True
        return self

    def _native(self, tab):
        """The recorded step as word arrays for vm_program_run (include/voicemap_hip.h): one array per run of C-ABI calls and event
        records / waits, host calls (the gradient collectives of data parallelism) between them.  None where the library's table is
        not the binding's (``tab`` is None) or an argument is not a pointer / number."""
        if tab is None:
            return None
        ids, sigs = tab
        segs, cur, where = [], [], {}
        try:
            for ci, c in enumerate(self.cmds):
                if c[0] == 3:
                    segs.append(cur)
                    segs.append(c[1])
                    cur = []
                    continue
                if c[0] == 0:
                    name, args = c[3], c[2]
                elif c[0] == 1:
                    name, args = "vm_event_record", (c[1], c[2])
                else:
                    name, args = "vm_stream_wait_event", (c[1], c[2])
                sig = sigs[name]
                if len(sig) != len(args):
                    return None
                where[ci] = (len(segs), len(cur) + 2)
                cur += [ids[name], len(args)] + [_word(v, t) for v, t in zip(args, sig)]
            segs.append(cur)
            patches = []
            for ci, ai, key in self.patches:
                si, w0 = where[ci]
                patches.append((si, w0 + ai, sigs[self.cmds[ci][3]][ai], key))
        except (KeyError, TypeError, ValueError, struct.error):
            return None
        segs = [np.array(sg, dtype=np.int64) if isinstance(sg, list) else sg for sg in segs]
        return segs, patches

    def run(self, lib, dyn, native=True):
        """Enqueue the step again with the per-step values ``dyn`` {key: value}: through vm_program_run (``native``, where the program
        has that form) or one ctypes call per command."""
        if native and self.native is not None:
            segs, patches = self.native
            for si, wi, t, key in patches:
                segs[si][wi] = _word(dyn[key], t)
            run, fail = lib.cdll.vm_program_run, self._fail_ref
            for sg in segs:
                if isinstance(sg, np.ndarray):
                    if sg.size:
                        rc = run(sg.ctypes.data, sg.size, fail)
                        if rc != 0:
                            self._raise(lib, "a replayed step failed (%d) at word %d of its program" % (rc, self._fail_at.value))
                else:
                    sg()          # a host call of the step (the gradient collectives of data parallelism)
            return
        cmds = self.cmds
        for ci, ai, key in self.patches:
            cmds[ci][2][ai] = dyn[key]
        rec, wait = self._ev_record, self._ev_wait
        for c in cmds:
            k = c[0]
            if k == 0:
                rc = c[1](*c[2])
            elif k == 1:
                rc = rec(c[1], c[2])
            elif k == 2:
                rc = wait(c[1], c[2])
            else:
                c[1]()          # a host call of the step (the gradient collectives of data parallelism)
                rc = 0
            if rc != 0:
                self._raise(lib, "%s failed (%d) in a replayed step" % (c[3] if k == 0 else "stream ordering", rc))

    @staticmethod
    def _raise(lib, what):
        from ._lib import VoicemapHipError   # (here: _lib imports torch, this module does not)
        msg = lib.cdll.vm_last_error()
        raise VoicemapHipError("%s: %s" % (what, msg.decode() if msg else ""))

    def destroy(self, lib):
        for h in self.events.values():
            lib.cdll.vm_event_destroy(h)
        self.events = {}


class ProgramStore:
    """The programs of one engine by step configuration.  A configuration is run eagerly on its first sighting (lazy buffers get
    allocated), recorded on its second and replayed from the third on; the 64 most recently used are kept.  Programs hold raw device
    pointers and events a replayed step may still be waiting on: ``sync`` (a callable that drains the device) runs before the events of
    a finished program are destroyed."""
    BOUND = 64
    _SEEN = object()

    def __init__(self, lib, sync):
        self.lib, self.sync, self._by_key = lib, sync, {}

    def __len__(self):
        return len(self._by_key)

    def recorded(self):
        """The finished programs, least recently used first."""
        return [p for p in self._by_key.values() if p is not self._SEEN]

    def sight(self, key):
        """What the step of configuration ``key`` is to do: its finished Program -- replay it; a new Program -- record the step into
        it and hand it to finish(); None -- just run."""
        prog = self._by_key.get(key)
        if prog is None:
            self._by_key[key] = self._SEEN
            while len(self._by_key) > self.BOUND:    # the least recently used configuration goes (with its events)
                self._drop(self._by_key.pop(next(iter(self._by_key))))
            return None
        if prog is self._SEEN:
            return Program()
        self._by_key[key] = self._by_key.pop(key)   # most recently used last
        return prog

    def finish(self, key, prog):
        self._by_key[key] = prog.finish(self.lib)

    def _drop(self, prog):
        if prog is not self._SEEN:
            self.sync()
            prog.destroy(self.lib)

    def drop_all(self):
        """Forget every configuration.  Whoever frees or reallocates a buffer a program may reference (the fold buffers, a plan's
        lazily sized buffers, a stream) calls this."""
        if self._by_key:
            self.sync()
            for prog in self.recorded():
                prog.destroy(self.lib)
            self._by_key.clear()

    def __del__(self):
        # the programs' events are the only library-side objects a store owns
        try:
            for prog in self.recorded():
                prog.destroy(self.lib)
        except Exception:   # interpreter shutdown: the library may be gone already
            pass
