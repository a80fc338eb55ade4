"""CPU check of the recorded-step machinery of voicemap_amd/program.py (no GPU: the C ABI is a stub that logs what it is called with):
a recorded list of C-ABI calls, event records and waits is replayed in order, with only the marked per-step arguments patched, and
every event key mapped onto one event of the program's own.  The GPU side -- a replayed training step is bit-identical to the eager
one -- is tests/test_gpu_replay.py."""
import subprocess
import sys

from voicemap_amd.program import DynF, DynI, Program, ProgramStore


class _StubLib:
    def __init__(self):
        self.log, self.cdll, self.tuning_epoch, self._next_event = [], self, 0, 1000

    def call(self, name, *args):
        rc = getattr(self, name)(*args)
        assert rc == 0
        return rc

    def program_table(self):
        return None                                            # no vm_program_run in the stub: the Python replay loop

    def __getattr__(self, name):
        if not name.startswith("vm_"):
            raise AttributeError(name)

        def fn(*args):
            if name == "vm_event_create":
                self._next_event += 1
                args[0]._obj.value = self._next_event
            self.log.append((name,) + tuple(a for a in args if not hasattr(a, "_obj")))
            return 0
        return fn


def _call(lib, prog, name, *args):
    """What the engine's _call does: make the call, note it in the program being recorded."""
    lib.call(name, *args)
    prog.call(getattr(lib.cdll, name), name, args)


def test_the_program_module_needs_no_torch():
    code = "import sys, voicemap_amd.program; assert 'torch' not in sys.modules and 'voicemap_amd.engine' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0


def test_recorded_calls_are_replayed_in_order_with_only_the_dynamic_slots_patched():
    lib, rec = _StubLib(), Program()
    _call(lib, rec, "vm_first", 11, DynI(123, "y"), 5, DynF(0.5, "lr_t"))
    rec.record("ev-a", 7)                                       # record(ev-a) on stream 7 ...
    rec.wait(9, "ev-a")                                         # ... stream 9 waits for it
    _call(lib, rec, "vm_second", DynI(4096, ("drop", 2, 64)), None)
    rec.join(7, 9)                                              # stream 7 waits for what stream 9 holds
    assert [(c, a, k) for c, a, k in rec.patches] == [(0, 1, "y"), (0, 3, "lr_t"), (3, 0, ("drop", 2, 64))]
    assert type(rec.cmds[0][2][1]) is int and type(rec.cmds[0][2][3]) is float      # plain numbers are stored, not the markers
    eager = list(lib.log)
    assert eager == [("vm_first", 11, 123, 5, 0.5), ("vm_second", 4096, None)]
    prog = rec.finish(lib)
    assert len(prog.events) == 2 and len(set(prog.events.values())) == 2
    lib.log.clear()
    prog.run(lib, {"y": 999, "lr_t": 0.25, ("drop", 2, 64): 8192, "unused": 1})
    ea, ej = prog.events["ev-a"], prog.events[("join", 4)]
    assert lib.log == [("vm_first", 11, 999, 5, 0.25), ("vm_event_record", ea, 7), ("vm_stream_wait_event", 9, ea),
                           ("vm_second", 8192, None), ("vm_event_record", ej, 9), ("vm_stream_wait_event", 7, ej)]
    prog.run(lib, {"y": 1, "lr_t": 2.0, ("drop", 2, 64): 3})                        # a second replay patches the same slots again
    assert lib.log[-6] == ("vm_first", 11, 1, 5, 2.0) and lib.log[-3] == ("vm_second", 3, None)


def _funnel_engine(lib):
    from voicemap_amd.engine import HipEncoderEngine

    class FunnelOnly(HipEncoderEngine):                        # no GPU, no network: an engine that is only the funnel under test
        def __init__(self):
            self.lib, self.timed = lib, {}
    return FunnelOnly()


def test_outside_a_recording_the_markers_are_plain_values_and_nothing_is_logged():
    eng = _funnel_engine(_StubLib())
    assert eng._rec is None and eng._dyn("y", 5) == 5 and type(eng._dyn("y", 5)) is int
    eng._call("vm_only", 1, 2)
    assert eng.lib.log == [("vm_only", 1, 2)]
    seen = []
    eng._host_call(lambda: seen.append(-1))                    # outside a recording the call simply runs
    assert seen == [-1] and eng._rec is None


def test_the_engine_funnels_note_what_they_enqueue_in_the_program_being_recorded():
    eng = _funnel_engine(_StubLib())
    rec = eng._rec = Program()
    assert eng._dyn("y", None) is None                         # a NULL argument is part of the configuration, not a slot
    seen = []
    eng._call("vm_first", 11, eng._dyn("y", 123), 5, eng._dyn("lr_t", 0.5))
    eng._host_call(lambda: seen.append(len(eng.lib.log)))
    eng._call("vm_second", eng._dyn(("drop", 2, 64), 4096), None)
    eng._rec = None
    assert eng.lib.log == [("vm_first", 11, 123, 5, 0.5), ("vm_second", 4096, None)] and seen == [1]
    assert rec.patches == [(0, 1, "y"), (0, 3, "lr_t"), (2, 0, ("drop", 2, 64))] and [c[0] for c in rec.cmds] == [0, 3, 0]
    assert type(rec.cmds[0][2][1]) is int and type(rec.cmds[0][2][3]) is float
    eng.lib.log.clear()
    rec.finish(eng.lib).run(eng.lib, {"y": 999, "lr_t": 0.25, ("drop", 2, 64): 8192})
    assert eng.lib.log == [("vm_first", 11, 999, 5, 0.25), ("vm_second", 8192, None)] and seen == [1, 1]


def _recorded(lib, store, key):
    """Take configuration ``key`` through the store as a training step does; returns what the store said."""
    prog = store.sight(key)
    if prog is not None and not prog.finished:
        _call(lib, prog, "vm_step", key)
        prog.record("ev", 7)
        store.finish(key, prog)
    return prog


def test_the_store_runs_records_then_replays_and_keeps_the_64_most_recently_used():
    lib, syncs = _StubLib(), []
    store = ProgramStore(lib, lambda: syncs.append(len(lib.log)))
    assert _recorded(lib, store, "a") is None and store.recorded() == [] and len(store) == 1      # first sighting: just run
    rec = _recorded(lib, store, "a")                                                                # second: recorded
    assert isinstance(rec, Program) and rec.finished and store.recorded() == [rec]
    assert _recorded(lib, store, "a") is rec and _recorded(lib, store, "a") is rec                  # from the third on: replayed
    for k in range(ProgramStore.BOUND - 1):                                                         # 63 more configurations, seen once
        assert _recorded(lib, store, k) is None
    assert len(store) == 64 and not syncs
    assert _recorded(lib, store, "a") is rec                                                        # "a" is the most recently used again
    assert _recorded(lib, store, "b") is None and len(store) == 64 and store.recorded() == [rec]   # ... so a sighting went, no sync
    assert not syncs and _recorded(lib, store, 0) is None                                           # (0 was that sighting: seen anew)
    for k in range(100, 100 + ProgramStore.BOUND):                                                  # "a" becomes the least recently used
        _recorded(lib, store, k)
    destroyed = [e for e in lib.log if e[0] == "vm_event_destroy"]
    assert store.recorded() == [] and len(store) == 64 and destroyed == [("vm_event_destroy", 1001)] and rec.events == {}
    assert len(syncs) == 1 and syncs[0] == lib.log.index(destroyed[0])                              # the device drained before its event went
    _recorded(lib, store, 100), _recorded(lib, store, 100)
    assert len(store.recorded()) == 1
    store.drop_all()
    assert len(store) == 0 and store.recorded() == [] and len(syncs) == 2
    assert [e for e in lib.log if e[0] == "vm_event_destroy"][1:] == [("vm_event_destroy", 1002)]
    store.drop_all()                                                                                # nothing held: nothing to wait for
    assert len(syncs) == 2


def test_a_failing_call_in_a_replay_raises_with_its_name():
    import pytest
    from voicemap_amd import _lib
    lib, rec = _StubLib(), Program()
    _call(lib, rec, "vm_ok", 1)
    prog = rec.finish(lib)
    prog.cmds[0][1] = lambda *a: -1
    lib.vm_last_error = lambda: b"boom"
    with pytest.raises(_lib.VoicemapHipError, match="vm_ok.*boom"):
        prog.run(lib, {})


def test_host_calls_keep_their_place_in_a_recorded_step():
    """Round 6: a step's host-side calls that are not C-ABI entry points (the two gradient collectives of data parallelism,
    voicemap_amd/parallel.py) are slots of the program: run when recorded and again, at the same position, in every replay."""
    lib, rec = _StubLib(), Program()
    seen = []

    def fn():
        seen.append(len(lib.log))
    _call(lib, rec, "vm_before", 1)
    fn()
    rec.host_call(fn)
    _call(lib, rec, "vm_after", 2)
    assert seen == [1] and [c[0] for c in rec.cmds] == [0, 3, 0]
    prog = rec.finish(lib)
    assert prog.events == {}                                   # a host call is not an event key
    lib.log.clear()
    prog.run(lib, {})
    assert seen == [1, 1] and lib.log == [("vm_before", 1), ("vm_after", 2)]


def test_a_step_inputs_signature_is_what_a_recorded_step_depends_on():
    """The replay key's part for the preprocessing: kind, dtype, and the windows' shape (raw) or length (offsets) -- the resident
    buffer's own length is never read by the offsets path, so two corpora share one program."""
    import torch
    from voicemap_amd.engine import HipEncoderEngine, StepInput
    raw = lambda dt, n=4, L=64: StepInput("raw", torch.zeros(n, L, dtype=dt), None, None, 4, True)
    offs = lambda dt, size, raw_len: StepInput("offsets", torch.zeros(size, dtype=dt), torch.zeros(4, dtype=torch.int64), raw_len, 4, True)
    sigs = [raw(torch.float32).signature(), raw(torch.int16).signature(), raw(torch.float32, L=128).signature(),
            offs(torch.float32, 1000, 64).signature(), offs(torch.int16, 1000, 64).signature(), offs(torch.float32, 1000, 128).signature(),
            raw(torch.float32)._replace(downsampling=2).signature(), raw(torch.float32)._replace(whitening=False).signature()]
    assert len(set(sigs)) == len(sigs) and all(hash(s) is not None for s in sigs)
    assert offs(torch.int16, 1000, 64).signature() == offs(torch.int16, 77777, 64).signature()
    assert raw(torch.float32).signature() == ("raw", torch.float32, (4, 64), 4, True)
    assert offs(torch.int16, 9, 64).signature() == ("offsets", torch.int16, 64, 4, True)
    # ... and the loss's part: one uniform key, the triplet key normalised so that the same step is one program
    assert [HipEncoderEngine._loss_key(l) for l in (None, "bce", ("prototypical", 3, 2, 1.0))] == \
        [("classifier",), ("siamese", "bce"), ("prototypical", 3, 2, 1.0)]
    assert HipEncoderEngine._triplet_loss_key(0, True, 0.7) == HipEncoderEngine._triplet_loss_key(0, 1, 0.2) == ("triplet", 0, 1, 0.0)
