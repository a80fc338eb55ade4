"""CPU checks of the voice activity detector's numpy statement (voicemap_amd/vad.py ``vad_reference``), of ``voiced()`` on the host
path and of the scripts' --vad flags.  Every comparison is equality."""
import os

import numpy as np
import pytest

from tests import vad_cases as VC
from voicemap_amd import vad as V
from voicemap_amd.vad import VadPolicy, vad_reference


# ---- the rule, with its quantifiers evaluated literally -----------------------------------------------------------------------------
def brute_force(pcm, policy, min_keep):
    """The module docstring of vad.py in Python loops: the two double multiplies of the comparison are numpy float64 scalars (one IEEE
    multiply each), everything else is Python integers and ``any`` / ``all`` over the quantifiers' ranges."""
    s = [int(x) for x in pcm]
    n, Fr, m, h = len(s), policy.frame, policy.min_run, policy.hang
    F = -(-n // Fr)
    n_f = [min(Fr, n - f * Fr) for f in range(F)]
    E = [sum(x * x for x in s[f * Fr:f * Fr + n_f[f]]) for f in range(F)]
    T = sum(E)
    D = np.float64
    a = [E[f] > 0 and bool(D(E[f]) * D(n) >= D(policy.rel) * (D(T) * D(n_f[f]))) and bool(D(E[f]) >= D(policy.floor_energy) * D(n_f[f]))
         for f in range(F)]
    p = [any(g >= 0 and g + m - 1 <= F - 1 and all(a[g:g + m]) for g in range(f - m + 1, f + 1)) for f in range(F)]
    v = [any(p[g] for g in range(max(0, f - h), min(F - 1, f + h) + 1)) for f in range(F)]
    Vk = sum(n_f[f] for f in range(F) if v[f])
    fallback = int(Vk < min_keep)
    if fallback:
        v, Vk = [True] * F, n
    dst, out = [], []
    for f in range(F):
        dst.append(len(out))   # the kept samples before frame f
        if v[f]:
            out += s[f * Fr:f * Fr + n_f[f]]
    assert len(out) == Vk
    return {"energy": E, "active": a, "mask": v, "new_len": Vk, "fallback": fallback, "pcm": out, "dst": dst}


@pytest.mark.parametrize("case", VC.cases(), ids=[c["name"] for c in VC.cases()])
def test_reference_against_brute_force(case):
    ref = VC.reference(case)
    pol = case["policy"]
    fb = ref["frame_base"]
    outs = np.concatenate([[0], np.cumsum(ref["new_lens"])])
    for u, (o, n) in enumerate(zip(case["offsets"], case["lens"])):
        b = brute_force(case["buf"][o:o + n], pol, pol.keep())
        sl = slice(fb[u], fb[u + 1])
        assert ref["energy"][sl].tolist() == b["energy"], (case["name"], u)
        assert ref["active"][sl].tolist() == b["active"], (case["name"], u)
        assert ref["mask"][sl].astype(bool).tolist() == b["mask"], (case["name"], u)
        assert int(ref["new_lens"][u]) == b["new_len"] and int(ref["info"][u, 3]) == b["fallback"]
        assert tuple(ref["info"][u, :3]) == (len(b["energy"]), sum(b["active"]), sum(b["mask"]))
        assert ref["dst"][sl].tolist() == b["dst"]
        assert ref["out"][outs[u]:outs[u + 1]].tolist() == b["pcm"]


def test_the_case_grid_plants_what_it_says():
    """The chunk cases: the run of min_run frames at a chunk edge is kept and the run of min_run - 1 is dropped, on both sides of the
    edge; the all-zero utterance is kept whole by the fallback."""
    C = V.DECIDE_CHUNK
    for case in VC.cases():
        if not case["name"].startswith("chunk-m"):
            continue
        pol, ref, fb = case["policy"], VC.reference(case), VC.reference(case)["frame_base"]
        m, h = pol.min_run, pol.hang
        u = 6   # runs ENDING at the edges
        a, v = ref["active"][fb[u]:fb[u + 1]], ref["mask"][fb[u]:fb[u + 1]]
        assert a[C - m:C].all() and not a[C] and v[C - 1] and (h == 0 or v[C]) and v[min(C - 1 + h, len(v) - 1)]
        if m > 1:
            assert a[2 * C - (m - 1):2 * C].all() and not v[2 * C - 1] and not v[2 * C]
        u = 7   # runs STARTING at the edges
        a, v = ref["active"][fb[u]:fb[u + 1]], ref["mask"][fb[u]:fb[u + 1]]
        assert a[2 * C:2 * C + m].all() and v[2 * C] and (h == 0 or v[2 * C - 1]) and v[2 * C - h]
        if m > 1:
            assert a[C:C + m - 1].all() and not v[C] and not v[C - 1]
    zero = next(c for c in VC.cases() if c["name"] == "all-zero")
    info = VC.reference(zero)["info"]
    assert tuple(info[1]) == (7, 0, 7, 1) and VC.reference(zero)["new_lens"][1] == 1000


def test_the_flat_reference_of_the_many_utterance_case():
    """tests/test_gpu_vad.py compares 70 000 utterances against ``reference_many``: on 3000 of them it is ``vad_reference`` exactly."""
    case = VC.many_utterances(3000)
    flat, ref = VC.reference_many(case), VC.reference(case)
    assert set(flat) == set(ref)
    for k in ref:
        assert np.array_equal(flat[k], ref[k]), k
    assert flat["info"][:, 3].sum() > 0 and (flat["mask"] == 0).any()


# ---- real speech --------------------------------------------------------------------------------------------------------------------
def test_known_answer_on_the_golden_clips(golden_dir):
    """The default policy (10 ms frames, 25 dB below the mean, bursts of 3, hangover 10) on the eight LibriSpeech clips of 3 s."""
    a = np.load(os.path.join(golden_dir, "clips_human_eval.npz"))
    b = np.load(os.path.join(golden_dir, "clips_embedding_vis.npz"))
    clips = [a["query"]] + [a["support"][i] for i in range(5)] + [b["clips"][i] for i in range(2)]
    kept = []
    for c in clips:
        assert c.dtype == np.int16 and c.shape == (48000,)
        r = vad_reference(c, VadPolicy())
        assert r["info"][0] == 300 and r["new_len"] == 160 * r["info"][2] == len(r["pcm"])
        kept.append(r["info"][2])
    assert kept == [277, 250, 274, 300, 300, 266, 265, 293]


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def test_planted_ties():
    """rel = 1/4 exactly, 4 frames of 4 samples.  E = (16, 64, 16, 160): T = 256, len = 16, n_f = 4, so E_f len == rel T n_f holds for
    E_f = 16 exactly (16 * 16 = 0.25 * 256 * 4): active.  One unit of energy lower (E = 15, the other frames raised so that T stays
    256): inactive.  All zeros: T = 0 makes both sides of the comparison 0 and only E_f > 0 keeps the frames inactive; the fallback
    keeps the file whole."""
    pol = VadPolicy(frame_ms=4.0, sampling_rate=1000, rel=0.25, min_run=1, hang=0)
    assert pol.rel == 0.25 and pol.frame == 4

    def frames(*rows):
        return np.array(rows, dtype=np.int16).reshape(-1)
    r = vad_reference(frames([2, 2, 2, 2], [4, 4, 4, 4], [4, 0, 0, 0], [12, 4, 0, 0]), pol)
    assert r["energy"].tolist() == [16, 64, 16, 160]
    assert r["active"].tolist() == [True, True, True, True] and r["fallback"] == 0
    r = vad_reference(frames([2, 2, 2, 1 + 2], [4, 4, 4, 4], [3, 2, 1, 1], [12, 4, 0, 0]), pol)
    assert r["energy"].tolist() == [21, 64, 15, 160] and int(r["energy"].sum()) == 260
    assert r["active"].tolist() == [True, True, False, True]       # 15 * 16 = 240 < 0.25 * 260 * 4 = 260
    r = vad_reference(frames([2, 2, 2, 2], [4, 4, 4, 4], [3, 2, 1, 1], [12, 4, 1, 0]), pol)
    assert r["energy"].tolist() == [16, 64, 15, 161] and int(r["energy"].sum()) == 256
    assert r["active"].tolist() == [True, True, False, True]       # the tie's neighbour: 15 * 16 = 240 < 256
    assert r["mask"].tolist() == [1, 1, 0, 1] and r["dst"].tolist() == [0, 4, 8, 8] and r["new_len"] == 12
    # a short last frame ties too, at rel = 1: len = 14, n_f = (4, 4, 4, 2), E = (16, 16, 16, 8), T = 56: 16 * 14 = 56 * 4, 8 * 14 = 56 * 2
    r = vad_reference(np.array([2] * 14, dtype=np.int16), VadPolicy(frame_ms=4.0, sampling_rate=1000, rel=1.0, min_run=1, hang=0))
    assert r["energy"].tolist() == [16, 16, 16, 8] and r["active"].tolist() == [True] * 4   # E_f len == 1.0 T n_f in every frame
    r = vad_reference(np.zeros(16, dtype=np.int16), pol)
    assert r["active"].tolist() == [False] * 4 and r["fallback"] == 1 and r["new_len"] == 16 and r["mask"].tolist() == [1] * 4
    assert r["info"] == (4, 0, 4, 1)


def test_fallback_edge():
    """V = 72 kept samples: min_keep = 73 (V == min_keep - 1) keeps the file whole, min_keep = 72 trims it."""
    trims, whole = VC.reference(VC.fallback_edge(0)), VC.reference(VC.fallback_edge(1))
    assert tuple(trims["info"][0]) == (40, 9, 9, 0) and trims["new_lens"][0] == 72
    assert tuple(whole["info"][0]) == (40, 9, 40, 1) and whole["new_lens"][0] == 320
    assert np.array_equal(whole["dst"], 8 * np.arange(40))
    case = VC.fallback_edge(1)
    assert np.array_equal(whole["out"], case["buf"][2:2 + 320])


# ---- limits -------------------------------------------------------------------------------------------------------------------------
def test_argument_limits():
    for kw in (dict(frame_ms=0.0), dict(frame_ms=4097.0, sampling_rate=1000), dict(min_run=0), dict(min_run=65), dict(hang=-1), dict(hang=257),
               dict(rel=-1.0), dict(floor_energy=-1.0), dict(min_keep=0), dict(threshold_db=float("nan"))):
        with pytest.raises(ValueError):
            VadPolicy(**kw)
    for kw in (dict(frame_ms=1.0, sampling_rate=1000), dict(frame_ms=4096.0, sampling_rate=1000), dict(min_run=1), dict(min_run=64),
               dict(hang=0), dict(hang=256)):
        VadPolicy(**kw)
    assert VadPolicy().frame == 160 and VadPolicy().rel == 10.0 ** -2.5 and VadPolicy(frame_ms=25.0, sampling_rate=8000).frame == 200
    with pytest.raises(ValueError):
        vad_reference(np.zeros(0, dtype=np.int16), VadPolicy())
    with pytest.raises(TypeError, match="int16 PCM"):
        vad_reference(np.zeros(100, dtype=np.float32), VadPolicy())
    with pytest.raises(TypeError, match="int16 PCM"):
        V.detect(np.zeros(100, dtype=np.float32), [0], [100], VadPolicy())
    import torch
    with pytest.raises(TypeError, match="int16 PCM"):
        V.detect(torch.zeros(100, dtype=torch.float32), [0], [100], VadPolicy())


def test_the_library_refuses_bad_arguments_without_a_launch():
    from voicemap_amd import _lib
    lib = _lib.lib()
    good = dict(frame=160, min_run=3, hang=10)
    for bad, word in ((dict(frame=0), "frame"), (dict(frame=4097), "frame"), (dict(min_run=0), "min_run"), (dict(min_run=65), "min_run"),
                      (dict(hang=-1), "hang"), (dict(hang=257), "hang")):
        k = dict(good, **bad)
        with pytest.raises(_lib.VoicemapHipError, match=word):
            lib.call("vm_vad_frames", None, None, None, None, 0, k["frame"], 0.1, 0.0, k["min_run"], k["hang"], 1, None, None, None, None, None, None)
    with pytest.raises(_lib.VoicemapHipError, match="frame"):
        lib.call("vm_vad_compact", None, None, None, None, None, None, None, 0, 5000, None, None)
    with pytest.raises(_lib.VoicemapHipError, match="null pointer"):
        lib.call("vm_vad_frames", None, None, None, None, 1, 160, 0.1, 0.0, 3, 10, 1, None, None, None, None, None, None)
    # no utterances: nothing to do, whatever the pointers
    lib.call("vm_vad_frames", None, None, None, None, 0, 160, 0.1, 0.0, 3, 10, 1, None, None, None, None, None, None)
    lib.call("vm_vad_compact", None, None, None, None, None, None, None, 0, 160, None, None)


# ---- voiced() on the host path ------------------------------------------------------------------------------------------------------
def test_voiced_on_the_host_path(tmp_path):
    """No ``to_device()``: the lengths and the files come from the numpy statement alone."""
    ds = VC.pause_corpus(tmp_path)
    before = (ds.file_length.copy(), ds.global_offset.copy(), ds.df.copy())
    pol = VadPolicy(frame_ms=2.0, min_run=2, hang=3)
    vo = ds.voiced(pol)
    assert type(vo) is type(ds) and vo._vad.min_keep == ds.fragment_length == 800
    refs = [vad_reference(np.asarray(ds._pcm(i)), vo._vad) for i in range(len(ds))]
    lens = np.array([r["new_len"] for r in refs])
    assert np.array_equal(vo.file_length, lens) and np.array_equal(vo.df["length"].values, lens)
    assert np.array_equal(vo.df["seconds"].values, lens / 16000.0)
    assert np.array_equal(vo.global_offset, np.concatenate([[0], np.cumsum(lens)[:-1]]))
    assert (lens < before[0]).any() and (lens >= ds.fragment_length).all()
    for i in range(len(ds)):
        assert np.array_equal(vo._pcm(i), refs[i]["pcm"]) and np.array_equal(vo._load(i), refs[i]["pcm"] / 32768.0)
    # a fragment can still be cut from every file, and batches of offsets draw
    np.random.seed(0)
    starts = vo.window_starts(np.arange(len(vo)))
    assert np.all(starts >= vo.global_offset) and np.all(starts + vo.fragment_length <= vo.global_offset + vo.file_length)
    o1, o2, y = vo.build_verification_batch_offsets(4)
    assert len(o1) == len(o2) == 4
    x, label = vo[0]
    assert len(x) == vo.fragment_length
    s = V.summarise([vo.vad_counts])
    assert s["files"] == len(ds) and 0 < s["kept_share"] < 1 and s["kept_whole"] == int(sum(r["fallback"] for r in refs))
    # the original is untouched
    assert np.array_equal(ds.file_length, before[0]) and np.array_equal(ds.global_offset, before[1]) and ds.df.equals(before[2])
    assert ds._vad is None and np.array_equal(np.asarray(ds._pcm(0)), np.asarray(ds._maps[0][:before[0][0]]))
    with pytest.raises(ValueError):
        vo.voiced(pol)
    # with speaker_shard
    from voicemap_amd import shards
    sh = shards.ShardedSpeechDataset(str(tmp_path), 0.05, pad=False, speaker_shard=(1, 2))
    vs = sh.voiced(pol)
    assert len(vs) == len(sh) and np.array_equal(vs.global_offset, np.concatenate([[0], np.cumsum(vs.file_length)[:-1]]))
    assert np.array_equal(vs._pcm(1), vad_reference(np.asarray(sh._pcm(1)), vs._vad)["pcm"])


# ---- script flags -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", ["train_siamese", "siamese_contrastive_loss"])
def test_training_script_flags(module, monkeypatch):
    import argparse
    import importlib
    mod = importlib.import_module("experiments." + module)
    from experiments import _common as C
    seen = {}

    class Stop(Exception):
        pass

    def setup(*a, **k):
        raise Stop()
    monkeypatch.setattr(C, "setup", setup)
    orig = argparse.ArgumentParser.parse_args

    def spy(self, argv=None, ns=None):
        seen["a"] = orig(self, argv, ns)
        return seen["a"]
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", spy)
    with pytest.raises(Stop):
        mod.main(["--synthetic"])
    a = seen["a"]
    assert a.vad is False and a.vad_threshold_db is None and a.vad_hang is None and a.vad_min_run is None and a.vad_frame_ms is None
    assert C.vad_policy(a) is None
    with pytest.raises(Stop):
        mod.main(["--synthetic", "--device-data", "/nonexistent", "--vad", "--vad-threshold-db", "30", "--vad-hang", "5", "--vad-min-run", "2",
                  "--vad-frame-ms", "20"])
    p = C.vad_policy(seen["a"])
    assert (p.threshold_db, p.hang, p.min_run, p.frame, p.min_keep) == (30.0, 5, 2, 320, None)
    with pytest.raises(SystemExit, match="--device-data"):
        mod.main(["--synthetic", "--vad"])
    with pytest.raises(SystemExit, match="needs --vad"):
        mod.main(["--synthetic", "--vad-hang", "5"])


@pytest.mark.parametrize("module", ["verification_accuracy", "speaker_identification"])
def test_evaluation_script_flags(module):
    import importlib
    mod = importlib.import_module("experiments." + module)
    a = mod._parser().parse_args(["--synthetic"])
    assert a.vad is False and a.vad_threshold_db is None and a.vad_hang is None and a.vad_min_run is None and a.vad_frame_ms is None
    assert V.policy_from_args(a) is None
    a = mod._parser().parse_args(["--synthetic", "--vad", "--vad-threshold-db", "20", "--vad-hang", "0", "--vad-min-run", "1", "--vad-frame-ms", "5"])
    p = V.policy_from_args(a)
    assert (p.threshold_db, p.hang, p.min_run, p.frame) == (20.0, 0, 1, 80)
    with pytest.raises(SystemExit):
        V.policy_from_args(mod._parser().parse_args(["--vad", "--vad-hang", "300"]))
