"""-m gpu: the training step and inference of cfg-A against the CPU oracle at every fragment length of the reference's own sweep.

experiments/n_seconds_accuracy.py of the reference trains cfg-A (filters 128, embedding 64, dropout 0, batch 32 pairs, downsampling 4)
at n_seconds = 1.0, 1.5, ..., 6.0.  The kernels' dispatch follows the window length: blocks 2-4 run folded (vm_conv_fwd_fold, pair-form
backward) only where vm_conv_fwd_fold_supported and vm_conv_dgrad_bnred_supported serve every block, and inference falls back from
vm_conv_fwd_pool wherever a block's length is odd.  Here each length, in every storage mode, runs on a fresh engine from the trained
state tests/golden/trained_cfgA_state.npz (real pedestals and negative gammas), with the whitening kernel, and is held to:
  * the oracle's float64 autograd step: embeddings (Frobenius and worst row), loss, the BatchNorm batch statistics per tower, every
    gradient tensor and the gradient cosine.  (Not its fp32 step: at 4.5 s and 6.0 s that step's own conv1.bias gradient is 4.9e-3 and
    7.9e-3 from the float64 one -- a sum of small terms that cancel -- which is the f32 bound below.  At 64 windows the float64
    backward fits in a few GB of host memory.)
  * the oracle's float64 inference forward: embeddings (Frobenius and worst row);
  * the path the C ABI predicates say it must take (folded or not, fused conv + pool or not).
One f16 engine also steps through all lengths in turn and must give the fresh engines' bits (stale plans or workspaces would not).

The f16 storage emulation of the oracle (training mode, forward only) calibrates the f16 bounds: it is reported next to the kernel's
figure at every length.  Bounds (fixed before the first measurement):
  f32, f32s  embeddings < 1e-4 (training and inference, Frobenius and per row); gradients < 5e-3 (f32), < 3e-2 (f32s) per tensor
  f16        embeddings < 1e-3 (training and inference, Frobenius and per row); gradients < 0.25 per tensor, cosine > 0.99
  bf16       embeddings (Frobenius) < 1.5e-2, cosine > 0.95; per-row and per-tensor figures reported only
dense.bias and bn4.beta have analytically zero gradients (the two towers' contributions cancel): they are held to an absolute 1e-6.
"""
import os
import time

import numpy as np
import pytest
import torch

from oracle import voicemap_oracle as O
from tests.gpu_util import DTYPES, cosine, grad_close, rel_err, report, row_rel_err

pytestmark = pytest.mark.gpu

PAIRS, F, E, DS = 32, 128, 64, 4
SECONDS = [1.0 + 0.5 * i for i in range(11)]
MODES = ["f32", "f32s", "f16", "bf16"]
ORACLE_THREADS = 16
EMB_TOL = {"f32": 1e-4, "f32s": 1e-4, "f16": 1e-3, "bf16": 1.5e-2}
ROW_TOL = {"f32": 1e-4, "f32s": 1e-4, "f16": 1e-3, "bf16": None}
GRAD_TOL = {"f32": 5e-3, "f32s": 3e-2, "f16": 0.25, "bf16": None}
GRAD_COS = {"f32": 0.9999, "f32s": 0.9999, "f16": 0.99, "bf16": 0.95}
ZERO_GRADS, ZERO_ATOL = ("dense.bias", "bn4.beta"), 1e-6


def _seed(s):
    return 4000 + int(round(10 * s))


def _trained_params():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_cfgA_state.npz"))
    return {k: torch.tensor(z[k].astype(np.float64)) for k in z.files if not k.startswith("__")}


@pytest.fixture(scope="module")
def fragment_oracle():
    """Per length, on the host: the oracle's float64 autograd step, its f16 storage emulation (training-mode forward) and its float64
    inference forward, on the same windows."""
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, ORACLE_THREADS)))
    try:
        arch = O.EncoderArch.baseline(F, E, dropout=0.0)
        p = _trained_params()
        pre = O.preprocess_instances(DS)
        t0 = time.time()
        out = {}
        for s in SECONDS:
            x1, x2, y = O.synthetic_pairs(PAIRS, _seed(s), samples=int(16000 * s))
            a, b = torch.tensor(pre(x1.astype(np.float64))), torch.tensor(pre(x2.astype(np.float64)))
            st = O.siamese_train_step(arch, p, None, a, b, torch.tensor(y, dtype=torch.float64), loss="contrastive")
            stats = [(torch.stack([st["collect1"]["bn_mean"][i], st["collect2"]["bn_mean"][i]]).numpy(),
                      torch.stack([st["collect1"]["bn_var"][i], st["collect2"]["bn_var"][i]]).numpy())
                     for i in range(len(arch.blocks))]
            with torch.no_grad():
                _, f1, f2 = O.siamese_forward(arch, p, a, b, True, "uniform_euclidean", None, None, None, None, storage="f16")
                inf = O.encoder_forward(arch, p, torch.cat([a, b]), training=False)
            out[s] = {"x1": x1, "x2": x2, "y": y, "emb": np.concatenate([st["e1"].numpy(), st["e2"].numpy()]),
                      "loss": float(st["loss"]), "stats": stats, "grads": {k: g.numpy() for k, g in st["grads"].items()},
                      "emb_f16_emulation": torch.cat([f1, f2]).numpy(), "infer": inf.numpy()}
            del st
        report("fragment_lengths_oracle", "cpu_seconds", time.time() - t0)
        return {"arch": arch, "p": p, "len": out}
    finally:
        torch.set_num_threads(threads)


def _lengths(s):
    ls = [(int(16000 * s) + DS - 1) // DS]
    for (_, _, pool) in O.EncoderArch.baseline(F, E, dropout=0.0).blocks:
        ls.append(ls[-1] // pool)
    return ls


def _expected_paths(mode, s):
    """(folded training step, number of blocks whose inference runs vm_conv_fwd_pool), from the C ABI predicates on each block's shape."""
    from voicemap_amd import _lib
    lib, vm = _lib.lib(), DTYPES[mode][0]
    blocks, ls, n = O.EncoderArch.baseline(F, E, dropout=0.0).blocks, _lengths(s), 2 * PAIRS
    is16 = mode in ("f16", "bf16")
    fold, pool = is16, 0
    for i in range(1, len(blocks)):
        cin, c, L = blocks[i - 1][1], blocks[i][1], ls[i]
        fold = fold and bool(lib.query("vm_conv_fwd_fold_supported", n, L, cin, c, vm, int(i < len(blocks) - 1)))
        fold = fold and bool(lib.query("vm_conv_dgrad_bnred_supported", n, L, cin, c, vm))
        pool += int(is16 and blocks[i][2] == 2 and bool(lib.query("vm_conv_fwd_pool_supported", n, L, cin, c, vm)))
    return fold, pool


def _engine(mode, p):
    from voicemap_amd.engine import HipEncoderEngine
    eng = HipEncoderEngine(O.EncoderArch.baseline(F, E, dropout=0.0).blocks, E, dropout=0.0, head="uniform_euclidean", dtype=mode)
    eng.set_params({k: v.numpy() for k, v in p.items()})
    return eng


def _train(eng, o):
    pl = eng.siamese_train_step(o["x1"], o["x2"], o["y"], loss="contrastive", preprocessed=False, downsampling=DS, drop_masks=None,
                                apply_update=False)
    torch.cuda.synchronize()
    return pl


_fresh_f16 = {}   # s -> (loss scale of the step, embeddings, loss, gradient buffer) of a fresh f16 engine


@pytest.mark.parametrize("s", SECONDS)
@pytest.mark.parametrize("mode", MODES)
def test_fragment_length_against_the_cpu_oracle(mode, s, fragment_oracle):
    o, arch = fragment_oracle["len"][s], fragment_oracle["arch"]
    eng = _engine(mode, fragment_oracle["p"])
    tag = "fragment_lengths[%s %.1fs]" % (mode, s)
    calls = []
    orig = eng._call
    eng._call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    fold_want, pool_want = _expected_paths(mode, s)

    # inference first (the training step updates the moving statistics)
    x = np.concatenate([o["x1"], o["x2"]]).reshape(2 * PAIRS, -1)
    inf = eng.embed(x, preprocessed=False, downsampling=DS, windows_per_tower=PAIRS).cpu().numpy()
    assert calls.count("vm_conv_fwd_pool") == pool_want and calls.count("vm_conv_fwd") == len(arch.blocks) - 1 - pool_want, calls
    d_inf, r_inf = rel_err(inf, o["infer"]), row_rel_err(inf, o["infer"])
    report(tag, "infer_emb_rel_err_vs_fp64_oracle", d_inf)
    report(tag, "infer_emb_row_rel_err_vs_fp64_oracle", r_inf)
    report(tag, "infer_conv_fwd_pool_blocks", float(pool_want))

    calls.clear()
    scale = float(eng.loss_scale)
    pl = _train(eng, o)
    assert bool(pl["fold_now"]) == fold_want, (mode, s, pl["fold_now"])
    if fold_want:
        # blocks 2-4 folded; the pair-form backward of blocks 2-3 (the last block's sparse apply pass has the z form either way)
        assert "vm_conv_fwd_fold" in calls and "vm_conv_fwd" not in calls
        assert "vm_bn_pool_bwd_apply_pairs" in calls and "vm_bn_pool_bwd_apply" not in calls
    else:
        assert "vm_conv_fwd_fold" not in calls
        assert "vm_bn_pool_bwd_apply_pairs" not in calls and "vm_bn_pool_bwd_apply_pairs_gmax" not in calls
        assert "vm_bn_pool_bwd_apply" in calls
    report(tag, "train_folded", float(fold_want))

    emb = pl["emb"].cpu().numpy()
    d_emb, r_emb = rel_err(emb, o["emb"]), row_rel_err(emb, o["emb"])
    report(tag, "emb_rel_err_vs_fp64_oracle", d_emb)
    report(tag, "emb_row_rel_err_vs_fp64_oracle", r_emb)
    if mode == "f16":
        report(tag, "f16_emulation_emb_rel_err_vs_fp64_oracle", rel_err(o["emb_f16_emulation"], o["emb"]))
        report(tag, "f16_emulation_emb_row_rel_err_vs_fp64_oracle", row_rel_err(o["emb_f16_emulation"], o["emb"]))
    loss = float(pl["loss_acc"][0].item())
    report(tag, "loss_abs_err_vs_fp64_oracle", abs(loss - o["loss"]))
    stat_err = []
    for i, (mean_ref, var_ref) in enumerate(o["stats"]):
        mean = pl[i]["mean"].cpu().numpy().astype(np.float64)
        var = 1.0 / pl[i]["invstd"].cpu().numpy().astype(np.float64) ** 2 - arch.bn_eps
        d_m = float(np.abs(mean - mean_ref).max() / max(np.sqrt(var_ref).max(), 1e-30))
        d_v = rel_err(var, var_ref)
        report(tag, "bn%d_mean_abs_err_over_max_std" % (i + 1), d_m)
        report(tag, "bn%d_var_rel_err" % (i + 1), d_v)
        stat_err.append((i, d_m, d_v))
    grads = eng.get_grads()
    assert all(np.isfinite(g).all() for g in grads.values())
    flat_h = np.concatenate([grads[k].ravel() for k in o["grads"]])
    flat_o = np.concatenate([o["grads"][k].ravel() for k in o["grads"]])
    cos = cosine(flat_h, flat_o)
    report(tag, "grad_cosine_vs_fp64_oracle", cos)
    far = []
    for k, g in o["grads"].items():
        report(tag, "grad_rel_err[%s]" % k, rel_err(grads[k], g))
        if GRAD_TOL[mode] is not None and not grad_close(grads[k], g, GRAD_TOL[mode], atol=ZERO_ATOL if k in ZERO_GRADS else 0.0):
            far.append((k, rel_err(grads[k], g)))
    if mode == "f16":
        _fresh_f16[s] = (scale, pl["emb"].clone(), pl["loss_acc"][0].clone(), eng.G.clone())

    assert d_emb < EMB_TOL[mode], (mode, s, d_emb)
    assert d_inf < EMB_TOL[mode], (mode, s, d_inf)
    if ROW_TOL[mode] is not None:
        assert r_emb < ROW_TOL[mode], (mode, s, r_emb)
        assert r_inf < ROW_TOL[mode], (mode, s, r_inf)
    assert abs(loss - o["loss"]) < max(EMB_TOL[mode], 1e-5) * max(1.0, abs(o["loss"]))
    for i, d_m, d_v in stat_err:
        assert d_m < 10 * EMB_TOL[mode] and d_v < 10 * EMB_TOL[mode], (mode, s, i, d_m, d_v)
    assert not far, (mode, s, far)
    assert cos > GRAD_COS[mode], (mode, s, cos)
    del eng, pl
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_fragment_length_sweep_covers_both_training_paths(mode):
    """The sweep must keep exercising what it was written for: in each 16-bit mode at least one folded and one unfolded training length,
    and at least one length whose inference falls back from vm_conv_fwd_pool at an odd block length (the cases above assert that the
    engine takes exactly these paths)."""
    paths = {s: _expected_paths(mode, s) for s in SECONDS}
    n_pool = len(O.EncoderArch.baseline(F, E, dropout=0.0).blocks) - 1
    for s, (fold, pool) in paths.items():
        report("fragment_lengths_paths[%s %.1fs]" % (mode, s), "folded", float(fold))
        report("fragment_lengths_paths[%s %.1fs]" % (mode, s), "conv_fwd_pool_blocks", float(pool))
    assert any(f for f, _ in paths.values()) and not all(f for f, _ in paths.values())
    assert any(pool < n_pool and any(L % 2 for L in _lengths(s)[2:n_pool + 2]) for s, (_, pool) in paths.items())


def test_one_f16_engine_through_every_length_matches_fresh_engines(fragment_oracle):
    """One f16 engine stepped through all lengths in turn gives the bits of a fresh engine per length: embeddings and loss always, the
    gradients while the loss scale is the one the fresh engine stepped with."""
    lens = fragment_oracle["len"]
    eng = _engine("f16", fragment_oracle["p"])
    compared = 0
    for s in SECONDS:
        if s not in _fresh_f16:
            fresh = _engine("f16", fragment_oracle["p"])
            scale = float(fresh.loss_scale)
            pl = _train(fresh, lens[s])
            _fresh_f16[s] = (scale, pl["emb"].clone(), pl["loss_acc"][0].clone(), fresh.G.clone())
            del fresh, pl
        scale, emb, loss, g = _fresh_f16[s]
        before = float(eng.loss_scale)
        pl = _train(eng, lens[s])
        assert torch.equal(pl["emb"], emb), s
        assert torch.equal(pl["loss_acc"][0], loss), s
        if before == scale:
            assert torch.equal(eng.G, g), s
            compared += 1
    report("fragment_lengths_reuse[f16]", "lengths_with_gradients_compared", float(compared))
    assert compared > 0
    del eng
    torch.cuda.empty_cache()
