"""-m gpu tests of vm_vad_frames / vm_vad_compact (voicemap_amd/csrc/vad.hip) against ``vad_reference`` (tests/vad_cases.py holds the
cases and their references), and of trimming through the public surface.  Every comparison is equality; guard words lie around every
output of the entry points."""
import numpy as np
import pytest
import torch

from tests import vad_cases as VC
from voicemap_amd import vad as V

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = {torch.int64: -7, torch.int32: -7, torch.uint8: 0xAB, torch.int16: 12345}


class Guarded:
    """n elements between two runs of GUARD sentinel words (``shift`` more in front: the payload's alignment)."""

    def __init__(self, n, dtype, shift=0):
        self.n, self.lo, self.sent = int(n), GUARD + shift, SENT[dtype]
        self.buf = torch.full((self.lo + self.n + GUARD,), self.sent, dtype=dtype, device="cuda")

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.buf.element_size()

    def host(self):
        h = self.buf.cpu().numpy()
        assert (h[:self.lo] == self.sent).all() and (h[self.lo + self.n:] == self.sent).all(), "a guard word was overwritten"
        return h[self.lo:self.lo + self.n]


def _upload(case):
    n = len(case["lens"])
    fb = np.concatenate([[0], np.cumsum((case["lens"] + case["policy"].frame - 1) // case["policy"].frame)]).astype(np.int64)
    tab = torch.from_numpy(np.concatenate([case["offsets"], case["lens"], fb]).astype(np.int64)).cuda()
    return torch.from_numpy(case["buf"]).cuda(), tab, n, fb


def run_frames(case):
    """One vm_vad_frames call on a case -> its outputs on the host (guards checked) and what vm_vad_compact needs."""
    from voicemap_amd import _lib
    pol = case["policy"]
    audio, tab, n, fb = _upload(case)
    total = int(fb[-1])
    g = {"energy": Guarded(total, torch.int64), "mask": Guarded(total, torch.uint8), "dst": Guarded(total, torch.int64),
         "new_lens": Guarded(n, torch.int64), "info": Guarded(4 * n, torch.int32)}
    e = tab.element_size()
    _lib.lib().call("vm_vad_frames", audio.data_ptr(), tab.data_ptr(), tab.data_ptr() + n * e, tab.data_ptr() + 2 * n * e, n, pol.frame, pol.rel,
                    pol.floor_energy, pol.min_run, pol.hang, pol.keep(), g["energy"].ptr, g["mask"].ptr, g["dst"].ptr, g["new_lens"].ptr,
                    g["info"].ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {k: v.host().copy() for k, v in g.items()}
    out["info"] = out["info"].reshape(n, 4)
    return out, (audio, tab, n, g)


def run_compact(case, state, new_lens, shift=0):
    from voicemap_amd import _lib
    audio, tab, n, g = state
    no = torch.from_numpy(np.concatenate([[0], np.cumsum(new_lens)[:-1]]).astype(np.int64)).cuda()
    out = Guarded(int(new_lens.sum()), torch.int16, shift)
    e = tab.element_size()
    _lib.lib().call("vm_vad_compact", audio.data_ptr(), tab.data_ptr(), tab.data_ptr() + n * e, tab.data_ptr() + 2 * n * e, g["mask"].ptr,
                    g["dst"].ptr, no.data_ptr(), n, case["policy"].frame, out.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.host().copy()


def _check(case, got, ref):
    for k in ("energy", "mask", "dst", "new_lens", "info"):
        assert np.array_equal(got[k], ref[k]), (case["name"], k, np.flatnonzero(np.asarray(got[k]).reshape(-1) != np.asarray(ref[k]).reshape(-1))[:8])


@pytest.mark.parametrize("case", VC.cases(), ids=[c["name"] for c in VC.cases()])
def test_case_grid(case):
    """energy, mask, dst, new_lens, info and the compacted buffer equal the reference.  The compaction runs with its output at every
    2-byte offset from a 16-byte boundary (the alignment cases; two offsets elsewhere): source and destination alignments differ in
    every way."""
    ref = VC.reference(case)
    got, state = run_frames(case)
    _check(case, got, ref)
    for shift in (range(8) if case["name"].startswith("align") else (0, 3)):
        out = run_compact(case, state, ref["new_lens"], shift)
        assert np.array_equal(out, ref["out"]), (case["name"], shift, np.flatnonzero(out != ref["out"])[:8])


def test_no_utterances():
    from voicemap_amd import _lib
    lib = _lib.lib()
    lib.call("vm_vad_frames", None, None, None, None, 0, 160, 0.1, 0.0, 3, 10, 1, None, None, None, None, None, None)
    lib.call("vm_vad_compact", None, None, None, None, None, None, None, 0, 160, None, None)
    audio = torch.zeros(100, dtype=torch.int16, device="cuda")
    res = V.detect(audio, [], [], V.VadPolicy())
    assert res.mask.numel() == 0 and res.new_lens.numel() == 0 and res.summary()["files"] == 0
    out, offs, lens, _ = V.trim(audio, [], [], V.VadPolicy())
    assert out.numel() == 0 and out.dtype == torch.int16 and len(offs) == 0 and len(lens) == 0


def test_many_utterances():
    """70 000 utterances of 3 to 9 samples: more than a grid's second dimension holds."""
    case = VC.many_utterances()
    ref = VC.reference_many(case)
    got, state = run_frames(case)
    _check(case, got, ref)
    assert np.array_equal(run_compact(case, state, ref["new_lens"], 1), ref["out"])


def test_two_launches_give_identical_bytes():
    for case in (VC.cases()[10], VC.many_utterances(5000)):
        a, sa = run_frames(case)
        b, sb = run_frames(case)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (case["name"], k)
        assert run_compact(case, sa, a["new_lens"]).tobytes() == run_compact(case, sb, b["new_lens"]).tobytes()


# ---- through the public surface -----------------------------------------------------------------------------------------------------
def test_trim_against_the_numpy_concatenation():
    case = VC.cases()[9]
    ref = VC.reference(case)
    audio = torch.from_numpy(case["buf"]).cuda()
    out, offs, lens, res = V.trim(audio, case["offsets"], torch.from_numpy(case["lens"]), case["policy"])
    assert out.dtype == torch.int16 and np.array_equal(out.cpu().numpy(), ref["out"])
    assert np.array_equal(lens, ref["new_lens"]) and np.array_equal(offs, np.concatenate([[0], np.cumsum(ref["new_lens"])[:-1]]))
    assert np.array_equal(res.mask.cpu().numpy(), ref["mask"]) and np.array_equal(res.energy.cpu().numpy(), ref["energy"])
    assert np.array_equal(res.dst.cpu().numpy(), ref["dst"]) and np.array_equal(res.info.cpu().numpy(), ref["info"])
    assert np.array_equal(res.frame_base.cpu().numpy(), ref["frame_base"])
    s = res.summary()
    assert s == {"files": len(lens), "frames": int(ref["frame_base"][-1]), "active_share": ref["active"].sum() / ref["frame_base"][-1],
                 "kept_share": ref["new_lens"].sum() / case["lens"].sum(), "kept_whole": int(ref["info"][:, 3].sum())}
    with pytest.raises(TypeError, match="int16 PCM"):
        V.detect(audio.float(), case["offsets"], case["lens"], case["policy"])
    with pytest.raises(ValueError, match="outside"):
        V.detect(audio, [audio.numel() - 5], [6], case["policy"])
    with pytest.raises(ValueError):
        V.detect(audio, [0], [0], case["policy"])


POLICY = dict(frame_ms=2.0, min_run=2, hang=3)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """(the resident dataset with planted pauses, its voiced() form, the host-trimmed files)"""
    ds = VC.pause_corpus(tmp_path_factory.mktemp("vad_shards"), seconds=0.15)
    ds.to_device("cuda")
    vo = ds.voiced(V.VadPolicy(**POLICY))
    host = [V.vad_reference(np.asarray(ds._pcm(i)), vo._vad)["pcm"] for i in range(len(ds))]
    return ds, vo, host


def test_voiced_resident_corpus(corpus):
    ds, vo, host = corpus
    assert type(vo) is type(ds) and vo._vad.min_keep == ds.fragment_length == 2400
    lens = np.array([len(h) for h in host])
    assert np.array_equal(vo.file_length, lens) and (lens < ds.file_length).any() and (lens >= 2400).all()
    assert np.array_equal(vo.df["length"].values, lens) and np.array_equal(vo.df["seconds"].values, lens / 16000.0)
    assert np.array_equal(vo.device_audio.cpu().numpy(), np.concatenate(host))
    for i in (0, len(ds) - 1):
        assert np.array_equal(vo._pcm(i), host[i])
    # the original is untouched
    assert ds._vad is None and ds.device_audio.numel() == int(ds.file_length.sum()) > vo.device_audio.numel()
    # device crops are the host's: offsets into the trimmed buffer against slices of the host-trimmed files
    np.random.seed(3)
    o1, o2, y, f1, f2 = vo.build_verification_batch_offsets(8, files=True)
    np.random.seed(3)
    (w1, w2), y2 = vo.build_verification_batch_device(8)
    assert np.array_equal(w1.offsets_host, o1) and np.array_equal(w2.offsets_host, o2)
    for w, o, f in ((w1, o1, f1), (w2, o2, f2)):
        crops = np.stack([host[k][s:s + 2400] for k, s in zip(f, o - vo.global_offset[f])]).astype(np.float64) / 32768.0
        assert np.array_equal(np.asarray(w)[:, :, 0], crops)
    # a speaker shard trims its own layout
    from voicemap_amd import shards
    sh = shards.ShardedSpeechDataset(ds.shard_dir, 0.15, pad=False, speaker_shard=(0, 2))
    sh.to_device("cuda")
    vs = sh.voiced(V.VadPolicy(**POLICY))
    assert np.array_equal(vs.device_audio.cpu().numpy(), np.concatenate([vs._pcm(i) for i in range(len(vs))]))


def test_one_training_step_on_a_voiced_batch(corpus):
    from voicemap_amd import keras_like as K
    from voicemap_amd import models, utils
    _, vo, _ = corpus
    enc = models.get_baseline_convolutional_encoder(16, 24, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (600, 1), distance_metric="uniform_euclidean")
    net.compile(loss="binary_crossentropy", optimizer=K.Adam(clipnorm=1.), metrics=["accuracy"])
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    np.random.seed(1)
    loss = np.asarray(net.train_on_batch(*bp(vo.build_verification_batch_device(8))), dtype=np.float64).reshape(-1)[0]
    assert np.isfinite(loss)


def test_embed_corpus_with_vad(corpus):
    """Whole utterances: the resident path (trimmed on the device) and the host path (trimmed file by file in numpy) both equal
    ``embed_varlen`` of the host-trimmed int16 files; first fragments agree too; ``vad=None`` is the call without the argument."""
    from voicemap_amd import models, retrieval, shards, utils
    ds, vo, host = corpus
    enc = models.get_baseline_convolutional_encoder(16, 24, dropout=0.0, dtype="f32")
    net = models.build_siamese_net(enc, (600, 1), distance_metric="uniform_euclidean")
    bp = utils.BatchPreProcessor("siamese", utils.preprocess_instances(4))
    pol = V.VadPolicy(**POLICY)
    eng = retrieval._encoder_engine(net, "siamese")
    q = 4 * int(np.prod([p for (_, _, p) in eng.blocks]))
    want_files = [V.vad_reference(np.asarray(ds._pcm(i)), pol.with_min_keep(q))["pcm"] for i in range(len(ds))]
    want = eng.embed_varlen(want_files, None, None, 4, True).clone()
    res = retrieval.embed_corpus(net, ds, bp, whole_utterance=True, vad=pol)
    assert torch.equal(res.emb, want)
    assert res.vad_counts["files"] == len(ds) and res.vad_counts["kept"] == sum(len(w) for w in want_files)
    plain = shards.ShardedSpeechDataset(ds.shard_dir, 0.15, stochastic=False, pad=False)   # no to_device(): the host dataset path
    hres = retrieval.embed_corpus(net, plain, bp, whole_utterance=True, vad=pol)
    assert torch.equal(hres.emb, want) and hres.vad_counts == res.vad_counts
    assert not torch.equal(retrieval.embed_corpus(net, ds, bp, whole_utterance=True).emb, want)
    # first fragments: device crops of the trimmed corpus against host windows of the trimmed files
    a = retrieval.embed_corpus(net, ds, bp, vad=pol)
    b = retrieval.embed_corpus(net, vo, bp)
    assert torch.equal(a.emb, b.emb)
    # vad=None is today's call
    assert torch.equal(retrieval.embed_corpus(net, ds, bp, vad=None).emb, retrieval.embed_corpus(net, ds, bp).emb)
