"""-m gpu: whole-utterance embedding in length-masked buckets (HipEncoderEngine.embed_varlen, the *_varlen entry points).

Every kernel test goes through the C ABI.  The end-to-end tests hold each recording's embedding to the float64 oracle run on that
recording ALONE (oracle.encoder_forward(training=False) at its own length), with the fragment-length test's bounds: per row < 1e-4 for
f32 / f32s and < 1e-3 for f16, Frobenius < 1.5e-2 for bf16.  One exception, measured: an f16 recording shorter than 1 s (4 000 decimated
samples) is held to 2e-3 per row.  Its global max sees a handful of rows, so no rounding averages out; the oracle's own f16 storage
emulation is 6.1e-4 off float64 at the 32-sample minimum against 1.2e-4 .. 2.0e-4 from 1 s up, and the kernels measured 1.15e-3 there."""
import os

import numpy as np
import pytest
import torch

from oracle import voicemap_oracle as O
from tests.gpu_util import DTYPES, L, dev, p, rel_err, report, row_rel_err, stream

pytestmark = pytest.mark.gpu

DS = 4
MODES = ["f32", "f32s", "f16", "bf16"]
ROW_TOL = {"f32": 1e-4, "f32s": 1e-4, "f16": 1e-3, "bf16": None}
EMB_TOL = {"f32": 1e-4, "f32s": 1e-4, "f16": 1e-3, "bf16": 1.5e-2}
VARLEN = ("vm_crop_decimate_whiten_varlen", "vm_conv1_fused_fwd_varlen", "vm_conv_fwd_pool_varlen", "vm_bn_drop_pool_fwd_varlen",
          "vm_bn_drop_pool_gmax_fwd_varlen", "vm_global_maxpool_fwd_varlen")


def _np_whiten_alone(x, ds, rms=0.038021):
    d = np.asarray(x, np.float64)[::ds]
    return (d - d.mean()) * (rms / np.sqrt((d * d).mean()))


# ---- preprocessing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i16", [False, True])
def test_crop_decimate_whiten_varlen_against_numpy(i16):
    r = np.random.default_rng(1)
    raw_lens = np.array([129, 4000, 997, 128, 6001, 3333, 2048], dtype=np.int64)
    gap = 513   # loud samples after every file (the next file of a resident corpus); the last file ends at the buffer's end
    offs = np.concatenate([[0], np.cumsum(raw_lens + gap)[:-1]]).astype(np.int64)
    total = int(offs[-1] + raw_lens[-1])
    buf = r.normal(0, 0.05, total)
    for o, n in zip(offs[:-1], raw_lens[:-1]):
        buf[o + n:o + n + gap] = 0.9 * np.sign(r.normal(size=gap))          # loud, never part of any window
    if i16:
        buf = np.round(buf * 32767).astype(np.int16)
        host = buf.astype(np.float64) / 32768.0
        audio = torch.as_tensor(buf).cuda()
    else:
        buf = buf.astype(np.float32)
        host = buf.astype(np.float64)
        audio = dev(buf)
    l0s = (raw_lens + DS - 1) // DS
    L0 = int(-(-l0s.max() // 32) * 32)
    n = len(raw_lens)
    out = dev(np.full((n, L0 + 31), 7.0, np.float32))
    ws = dev(np.zeros(L().query("vm_decimate_whiten_workspace_bytes", n) // 4, np.float32))
    od, rd = dev(offs, torch.int64), dev(raw_lens, torch.int64)
    L().call("vm_crop_decimate_whiten_varlen", p(audio), int(i16), p(od), p(rd), n, L0, DS, 1, 0.038021, p(out), p(ws), stream())
    got = out.cpu().numpy().astype(np.float64)
    for k in range(n):
        want = _np_whiten_alone(host[offs[k]:offs[k] + raw_lens[k]], DS)
        row = got[k]
        assert (row[:15] == 0).all() and (row[15 + l0s[k]:] == 0).all(), k        # halo and padded tail are zero
        assert np.abs(row[15:15 + l0s[k]] - want).max() < 1e-6 * max(np.abs(want).max(), 1e-30) + 1e-7, k


def test_crop_decimate_whiten_varlen_equal_lengths_is_bit_identical():
    r = np.random.default_rng(2)
    n, raw_len = 9, 4803
    buf = r.normal(0, 0.05, n * raw_len + 1000).astype(np.float32)
    audio = dev(buf)
    offs = np.sort(r.choice(1000, n, replace=False)).astype(np.int64) + np.arange(n) * raw_len
    L0 = (raw_len + DS - 1) // DS
    a, b = (dev(np.zeros((n, L0 + 31), np.float32)) for _ in range(2))
    ws = dev(np.zeros(L().query("vm_decimate_whiten_workspace_bytes", n) // 4, np.float32))
    od, rd = dev(offs, torch.int64), dev(np.full(n, raw_len), torch.int64)
    L().call("vm_crop_decimate_whiten", p(audio), 0, p(od), n, raw_len, DS, 1, 0.038021, 1, p(a), p(ws), stream())
    L().call("vm_crop_decimate_whiten_varlen", p(audio), 0, p(od), p(rd), n, L0, DS, 1, 0.038021, p(b), p(ws), stream())
    assert torch.equal(a, b)


# ---- masked pool / global max ---------------------------------------------------------------------------------------------------
def _rnd(x, mode):
    t = torch.as_tensor(x, dtype=torch.float64)
    return t.to(DTYPES[mode][1]).to(torch.float64).numpy()


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("pool", [2, 4])
def test_bn_pool_varlen_against_numpy(mode, pool):
    vm, tdt = DTYPES[mode]
    r = np.random.default_rng(3 + pool)
    n, Lz, C = 6, 67, 24
    lens = np.array([67, 4, 5, 33, 61, pool], dtype=np.int32)             # odd ones included
    z = _rnd(r.normal(0, 1, (n, Lz, C)), mode)
    sc, sh = r.normal(0, 1, C), r.normal(0, 0.3, C)
    sc[::3] *= -1
    zd = dev(z, tdt)
    scd, shd, ld = dev(sc), dev(sh), dev(lens, torch.int32)
    Lq = Lz // pool
    act = dev(np.full((n, Lq + 2, C), 5.0), tdt)
    L().call("vm_bn_drop_pool_fwd_varlen", p(zd), p(scd), p(shd), p(ld), n, Lz, C, pool, vm, p(act), stream())
    y = np.fmax.reduce(np.stack([z[:, j:Lq * pool:pool] * sc + sh for j in range(pool)]), axis=0)   # fp64 of the affine, then pool
    got = act.cpu().to(torch.float64).numpy()
    for k in range(n):
        v = lens[k] // pool
        np.testing.assert_allclose(got[k, 1:1 + v], _rnd(y[k, :v], mode), rtol=1e-2 if mode != "f32" else 1e-5, atol=1e-5)
        assert (got[k, 1 + v:1 + Lq] == 0).all(), k                          # the next conv's SAME padding
        assert (got[k, 0] == 5).all() and (got[k, -1] == 5).all()           # halo rows untouched
    # global max over the valid pooled rows only (the pooled rows are zero / padding past them)
    gmax, gidx = dev(np.zeros((n, C))), dev(np.zeros((n, C)), torch.int32)
    ws = dev(np.zeros(L().query("vm_bn_drop_pool_gmax_workspace_bytes", n, C) // 4, np.float32))
    L().call("vm_bn_drop_pool_gmax_fwd_varlen", p(zd), p(scd), p(shd), p(ld), n, Lz, C, pool, vm, p(gmax), p(gidx), p(ws), stream())
    g, gi = gmax.cpu().numpy(), gidx.cpu().numpy()
    for k in range(n):
        v = lens[k] // pool
        want = got[k, 1:1 + v].max(axis=0)
        np.testing.assert_array_equal(g[k], want.astype(np.float32))
        assert ((gi[k] >= 0) & (gi[k] < v)).all()
        np.testing.assert_array_equal(got[k, 1 + gi[k], np.arange(C)], want)
    # vm_global_maxpool_fwd_varlen on the padded pooled tensor: valid rows only, first maximum
    lq = dev(lens // pool, torch.int32)
    g2, gi2 = dev(np.zeros((n, C))), dev(np.zeros((n, C)), torch.int32)
    L().call("vm_global_maxpool_fwd_varlen", p(act), p(lq), n, Lq, C, vm, p(g2), p(gi2), p(ws), stream())
    assert torch.equal(g2, gmax) and torch.equal(gi2, gidx)
    act_neg = dev(-np.abs(got) - 1.0, tdt)        # every valid row negative: the zero padding would win a max that saw it
    L().call("vm_global_maxpool_fwd_varlen", p(act_neg), p(lq), n, Lq, C, vm, p(g2), p(gi2), p(ws), stream())
    an = act_neg.cpu().to(torch.float64).numpy()
    for k in range(n):
        v = lens[k] // pool
        np.testing.assert_array_equal(g2.cpu().numpy()[k], an[k, 1:1 + v].max(axis=0).astype(np.float32))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _trained_cfgA():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_cfgA_state.npz"))
    return O.EncoderArch.baseline(128, 64, dropout=0.0), {k: torch.tensor(z[k].astype(np.float64)) for k in z.files if not k.startswith("__")}


def _small():
    arch = O.EncoderArch.baseline(16, 32, dropout=0.0)
    prm = O.init_params(arch, head="uniform_euclidean", seed=11)
    r = np.random.default_rng(11)
    for k in list(prm):   # non-trivial inference statistics, negative gammas
        if k.endswith("moving_variance"):
            prm[k] = torch.tensor(r.uniform(0.3, 2.0, prm[k].shape))
        elif k.endswith("moving_mean"):
            prm[k] = torch.tensor(r.normal(0, 0.2, prm[k].shape))
        elif k.endswith("gamma"):
            prm[k] = torch.tensor(r.normal(0.8, 0.6, prm[k].shape))
        elif k.endswith("beta"):
            prm[k] = torch.tensor(r.normal(0, 0.2, prm[k].shape))
    return arch, prm


def _engine(arch, prm, mode):
    from voicemap_amd.engine import HipEncoderEngine
    eng = HipEncoderEngine(arch.blocks, arch.embedding_dimension, dropout=0.0, head="uniform_euclidean", dtype=mode)
    eng.set_params({k: v.numpy() for k, v in prm.items()})
    return eng


def _recordings(seed, max_raw):
    """Raw lengths from the minimum (32 decimated samples) up to max_raw, odd and prime ones included."""
    r = np.random.default_rng(seed)
    lens = [128, 129, 131, 4 * 97 + 1, 1009, 4096, 7919, 16000 + 3, 4 * 8191, max_raw // 2 + 1, max_raw]
    lens += list(r.integers(128, max_raw, 5))
    return [r.normal(0, 0.05, int(n)).astype(np.float32) for n in lens]


def _oracle(arch, prm, waves):
    pre = O.preprocess_instances(DS)
    out = []
    with torch.no_grad():
        for w in waves:
            x = torch.tensor(pre(w.astype(np.float64)[None, :, None]))
            out.append(O.encoder_forward(arch, prm, x, training=False).numpy()[0])
    return np.stack(out)


_ORACLE = {}


def _oracle_cached(name, arch, prm, waves):
    if name not in _ORACLE:
        _ORACLE[name] = _oracle(arch, prm, waves)
    return _ORACLE[name]


def _calls(eng):
    calls = []
    orig = eng._call
    eng._call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    return calls


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", ["small", "cfgA"])
def test_embed_varlen_against_oracle_per_recording(cfg, mode):
    arch, prm = _small() if cfg == "small" else _trained_cfgA()
    waves = _recordings(21, 20 * 16000)
    ref = _oracle_cached(cfg, arch, prm, waves)
    eng = _engine(arch, prm, mode)
    calls = _calls(eng)
    got = eng.embed_varlen(waves, downsampling=DS, row_budget=400000).cpu().numpy()
    tag = "utterance_embed[%s %s]" % (cfg, mode)
    d = rel_err(got, ref)
    rows = np.array([row_rel_err(got[k:k + 1], ref[k:k + 1]) for k in range(len(waves))])
    short = np.array([(len(w) + DS - 1) // DS < 4000 for w in waves])
    rr = float(rows[~short].max())
    report(tag, "emb_rel_err_vs_fp64_oracle", d)
    report(tag, "emb_row_rel_err_vs_fp64_oracle", rr)
    report(tag, "emb_row_rel_err_vs_fp64_oracle_under_1s", float(rows[short].max()))
    report(tag, "buckets", float(len(eng.last_bucket_plan.buckets)))
    assert "vm_crop_decimate_whiten_varlen" in calls
    if cfg == "cfgA" and mode in ("f16", "bf16"):
        assert "vm_conv1_fused_fwd_varlen" in calls and "vm_conv_fwd_pool_varlen" in calls and "vm_global_maxpool_fwd_varlen" in calls
    if mode in ("f32", "f32s"):
        assert "vm_bn_drop_pool_fwd_varlen" in calls and "vm_bn_drop_pool_gmax_fwd_varlen" in calls
    assert np.isfinite(got).all()
    assert d < EMB_TOL[mode], (cfg, mode, d)
    if ROW_TOL[mode] is not None:
        assert rr < ROW_TOL[mode], (cfg, mode, rr)
        assert rows[short].max() < (2e-3 if mode == "f16" else ROW_TOL[mode]), (cfg, mode, rows)


@pytest.mark.parametrize("mode", MODES)
def test_embed_varlen_is_invariant_to_order_and_buckets(mode):
    arch, prm = _trained_cfgA()
    r = np.random.default_rng(24)
    waves = _recordings(22, 2 * 16000) + [r.normal(0, 0.05, 3000 + k).astype(np.float32) for k in range(40)]   # 40 on one rung
    eng = _engine(arch, prm, mode)
    calls = _calls(eng)
    a = eng.embed_varlen(waves, downsampling=DS, row_budget=400000)
    names_a, nb_a = sorted({c for c in calls if "pack" not in c}), len(eng.last_bucket_plan.buckets)   # (weight packing: once)
    calls.clear()
    perm = np.random.default_rng(0).permutation(len(waves))
    b = eng.embed_varlen([waves[i] for i in perm], downsampling=DS, row_budget=10000)
    names_b, nb_b = sorted({c for c in calls if "pack" not in c}), len(eng.last_bucket_plan.buckets)
    assert nb_a != nb_b                       # different buckets ...
    assert names_a == names_b, (names_a, names_b)   # ... served by the same entry points: the bits must agree
    assert torch.equal(a[torch.as_tensor(perm, device=a.device)], b)


def _masked_lengths_with_fused_dispatch(lib, vm, blocks, count):
    """Decimated lengths l0 (multiples of 32) that are padded inside their bucket (l0 < its ladder rung L0) and whose every k=3 block is
    served by vm_conv_fwd_pool both at l0 (embed, one window) and at L0 (embed_varlen): the same launches on both paths."""
    from voicemap_amd._lib import VM_BF16, VM_F16
    from voicemap_amd.utterances import DEFAULT_MAX_PAD_FRAC, ladder
    rungs = ladder(32, DEFAULT_MAX_PAD_FRAC, 40000)
    out = []
    for l0 in range(32 * 60, 32 * 1000, 32):
        L0 = min(r for r in rungs if r >= l0)
        if L0 == l0:
            continue
        ok = True
        for l in (l0, L0) if vm in (VM_BF16, VM_F16) else ():   # fp32 storage runs the unfused launches at every length
            L = l // blocks[0][2]
            for i in range(1, len(blocks)):
                ok = ok and bool(lib.query("vm_conv_fwd_pool_supported", 1, L, blocks[i - 1][1], blocks[i][1], vm))
                L //= blocks[i][2]
        if ok and (not out or l0 > 1.3 * out[-1]):
            out.append(l0)
        if len(out) == count:
            return out
    return out


@pytest.mark.parametrize("mode", MODES)
def test_embed_varlen_matches_embed_bit_for_bit(mode):
    """Recordings padded inside their buckets, through the masked kernels, against embed() of each recording alone at its own length:
    where the same kernels serve both (asserted), the rows are bit-identical.  In the 16-bit modes those kernels are the fused masked
    ones (vm_conv1_fused_fwd_varlen, vm_conv_fwd_pool_varlen, vm_global_maxpool_fwd_varlen)."""
    arch, prm = _trained_cfgA()
    eng = _engine(arch, prm, mode)
    l0s = _masked_lengths_with_fused_dispatch(eng.lib, DTYPES[mode][0], arch.blocks, 4)
    assert len(l0s) == 4, l0s
    r = np.random.default_rng(5)
    waves = [r.normal(0, 0.05, 4 * l0).astype(np.float32) for l0 in l0s]
    eng._ensure_wfp()         # the one-time weight packing goes before the hook: it is in neither launch sequence
    calls = _calls(eng)
    v = eng.embed_varlen(waves, downsampling=DS, row_budget=400000).cpu().numpy()
    bp = eng.last_bucket_plan
    assert all(len(idx) == 1 and L0 > l0s[idx[0]] for L0, idx in bp.buckets)   # one recording per bucket, each padded
    # the launches of each bucket: the calls between two preprocessing launches (the BatchNorm affines come once, in front)
    starts = [j for j, c in enumerate(calls) if c == "vm_crop_decimate_whiten_varlen"] + [len(calls)]
    front = {c for c in calls[:starts[0]] if "pack" not in c}
    per_bucket = [front | set(calls[starts[j] + 1:starts[j + 1]]) for j in range(len(bp.buckets))]
    bucket_of = {int(idx[0]): j for j, (_, idx) in enumerate(bp.buckets)}
    for k, w in enumerate(waves):
        names = {c.replace("_varlen", "") for c in per_bucket[bucket_of[k]]}
        if mode in ("f16", "bf16"):
            assert {"vm_conv1_fused_fwd_varlen", "vm_conv_fwd_pool_varlen", "vm_global_maxpool_fwd_varlen"} <= per_bucket[bucket_of[k]]
        calls.clear()
        e = eng.embed(w[None, :], preprocessed=False, downsampling=DS, windows_per_tower=1).cpu().numpy()[0]
        fixed = {c for c in calls if c != "vm_decimate_whiten" and "pack" not in c}
        assert fixed == names, (k, fixed ^ names)   # the same launches serve both ...
        np.testing.assert_array_equal(v[k], e)       # ... so the bits agree


def test_plan_count_is_bounded():
    from voicemap_amd.utterances import MAX_PLANS
    arch, prm = _small()
    eng = _engine(arch, prm, "f16")
    r = np.random.default_rng(9)
    lens = 128 + 7 * np.arange(2000) + r.integers(0, 7, 2000)     # 2 000 distinct lengths, 8 ms .. 0.9 s
    waves = [r.normal(0, 0.05, int(n)).astype(np.float32) for n in lens]
    e = eng.embed_varlen(waves, downsampling=DS)
    assert e.shape == (2000, arch.embedding_dimension) and torch.isfinite(e).all()
    report("utterance_embed_plans", "shapes", float(len(eng.last_bucket_plan.shapes)))
    assert eng.plan_count() <= MAX_PLANS and len(eng._plans) == 0


def test_too_short_recording_raises():
    arch, prm = _small()
    eng = _engine(arch, prm, "f32")
    with pytest.raises(ValueError, match="recording 1 is too short"):
        eng.embed_varlen([np.zeros(400, np.float32), np.zeros(124, np.float32)], downsampling=DS)


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_embed_corpus_whole_utterance_sharded(tmp_path, mode):
    from voicemap_amd import models, retrieval, shards, verification as V
    from voicemap_amd.librispeech import SyntheticSpeechDataset
    from voicemap_amd.utils import BatchPreProcessor, preprocess_instances
    src = SyntheticSpeechDataset(num_speakers=8, files_per_speaker=4, seconds=2, stochastic=False, seed=4)
    shards.write_shards(src, str(tmp_path), shard_samples=300000)
    sd = shards.ShardedSpeechDataset(str(tmp_path), 1, stochastic=False)
    enc = models.get_baseline_convolutional_encoder(16, 32, dropout=0.0, dtype=mode)
    net = models.build_siamese_net(enc, (4000, 1), distance_metric="uniform_euclidean")
    pre = BatchPreProcessor("siamese", preprocess_instances(DS))
    host = retrieval.embed_corpus(net, sd, pre, whole_utterance=True)
    sd.to_device()
    devc = retrieval.embed_corpus(net, sd, pre, whole_utterance=True)
    assert devc.n == len(sd) and np.array_equal(devc.speaker, host.speaker)
    d = row_rel_err(devc.emb.cpu().numpy(), host.emb.cpu().numpy())
    report("utterance_embed_corpus[%s]" % mode, "device_vs_host_row_rel_err", d)
    assert d < ROW_TOL[mode]
    m = V.verification_metrics(devc, "euclidean")
    assert 0.0 <= m["eer"] <= 1.0 and m["n_target"] + m["n_nontarget"] == len(sd) * (len(sd) - 1) // 2
    frag = retrieval.embed_corpus(net, sd, pre)   # the first-fragment cache is another thing (1 s of a 2 s file)
    assert not torch.equal(frag.emb, devc.emb)


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_global_maxpool_varlen_keeps_negative_zero(mode):
    """Valid rows whose maximum is -0: the same bits as vm_global_maxpool_fwd on the same rows (no fma in front of the max)."""
    vm, tdt = DTYPES[mode]
    n, Lq, C = 3, 9, 16
    x = -np.abs(np.random.default_rng(8).normal(0, 1, (n, Lq + 2, C))) - 0.5
    x[:, 3] = -0.0
    act = dev(x, tdt)
    lens = dev(np.full(n, Lq, np.int32), torch.int32)
    ws = dev(np.zeros(L().query("vm_bn_drop_pool_gmax_workspace_bytes", n, C) // 4, np.float32))
    g1, i1 = dev(np.zeros((n, C))), dev(np.zeros((n, C)), torch.int32)
    g2, i2 = dev(np.zeros((n, C))), dev(np.zeros((n, C)), torch.int32)
    L().call("vm_global_maxpool_fwd", p(act), n, Lq, C, vm, p(g1), p(i1), stream())
    L().call("vm_global_maxpool_fwd_varlen", p(act), p(lens), n, Lq, C, vm, p(g2), p(i2), p(ws), stream())
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and torch.equal(i1, i2)
    assert (g2.view(torch.int32).cpu().numpy() == np.int32(-2 ** 31)).all()      # -0.0f


def test_embed_varlen_mixed_int16_and_float_waves():
    """A list that mixes int16 PCM and float waveforms: int16 is read as x / 32768, as the device buffer path reads it."""
    arch, prm = _small()
    eng = _engine(arch, prm, "f32")
    r = np.random.default_rng(12)
    pcm = [np.round(r.normal(0, 2000, n)).astype(np.int16) for n in (3001, 1777)]
    flt = [w.astype(np.float32) / np.float32(32768.0) for w in pcm]
    extra = r.normal(0, 0.05, 2222).astype(np.float32)
    for wh in (False, True):
        mixed = eng.embed_varlen([pcm[0], extra, pcm[1]], downsampling=DS, whitening=wh)
        ref = eng.embed_varlen([flt[0], extra, flt[1]], downsampling=DS, whitening=wh)
        assert torch.equal(mixed, ref), wh
