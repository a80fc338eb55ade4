"""The reference helpers of tests/test_gpu_step_tail.py, checked on the host: the constants they quote are the kernels', the derived
bounds hold for float32 reference arithmetic and break for a wrong result, the constructions give what they promise."""
import os
import re

import numpy as np
import torch

from oracle import voicemap_oracle as O
from tests import tail_refs as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voicemap_amd", "csrc")


def _const(fname, name):
    src = open(os.path.join(CSRC, fname)).read()
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert m, (fname, name)
    return int(m.group(1))


def test_constants_are_the_kernels():
    assert _const("optim.hip", "SQ_BLOCKS") == R.SQ_BLOCKS and R.S == 65536
    assert _const("tail.hip", "DENSE_KS") == R.DENSE_KS
    assert _const("common.hpp", "SLAB_RCH") == R.SLAB_RCH
    assert _const("conv1.hip", "C1_K") == R.C1_K
    src = open(os.path.join(CSRC, "optim.hip")).read()
    assert "i + 7 * STRIDE < n; i += 8 * STRIDE" in src       # the loop edges sqnorm_sizes() and hot_indices() are built around


def test_sqnorm_sizes_and_hot_indices():
    n = R.n_cfg_a()
    assert n == R.n_cfg_a_from_architecture()
    assert 7 * R.S < n and n in R.sqnorm_sizes() and max(R.sqnorm_sizes()) < 2 ** 24
    assert R.hot_indices(1) == [0] and R.hot_indices(R.S) == [0, R.S - 1]
    assert R.hot_indices(R.S + 1) == [0, R.S - 1, R.S]
    h = R.hot_indices(8 * R.S + 1)
    assert {7 * R.S - 1, 7 * R.S, 7 * R.S + 1, 8 * R.S - 1, 8 * R.S}.issubset(h) and 8 * R.S + 1 not in h
    g = R.graded_gradient(np.random.default_rng(0), 5000)
    assert g.dtype == np.float32 and 50 < np.abs(g[:1000]).mean() / np.abs(g[3000:4000]).mean() < 20000


def test_float32_and_float64_saturation_figures():
    """What the loss costs at the clip: float32 gives logit 15.9424 at the high clip (1 - 1e-7 rounds to 1 - 2^-23) and -16.1181 at the
    low one; float64 gives +-16.1181.  A high-saturated pair with y = 0 costs 15.9424 in the reference's arithmetic."""
    y0, y1 = np.zeros(1), np.ones(1)
    hi32, lo32 = R.bce_pair_f32([1.0], y0)[0], R.bce_pair_f32([1e-9], y1)[0]
    assert abs(hi32 - 15.9424) < 1e-4 and abs(lo32 - 16.1181) < 1e-4
    f64 = lambda pv, yv: float(O.binary_crossentropy(torch.tensor([yv], dtype=torch.float64), torch.tensor([pv], dtype=torch.float64)))
    assert abs(f64(1.0, 0.0) - 16.1181) < 1e-4 and abs(f64(1e-9, 1.0) - 16.1181) < 1e-4
    assert abs(f64(1.0, 0.0) - hi32) > 0.17
    assert np.float32(1.0 - 1e-7) == np.float32(1.0 - 2.0 ** -23)
    # the cheap side of the clip: ~1.2e-7 in float32
    assert abs(R.bce_pair_f32([1.0], y1)[0] - 1.1920930e-07) < 1e-12
    # in float32 the sigmoid IS 1 from a = 20 on, and p(1 - p) is 0
    assert np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-20.0))) == np.float32(1.0)


def test_dot_product_bound_holds_for_float32_and_breaks_for_a_dropped_term():
    r = np.random.default_rng(1)
    for rows, ni, no in R.DENSE_TRIPLES:
        x, w, b = (r.standard_normal(s).astype(np.float32) for s in [(rows, ni), (ni, no), (no,)])
        x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
        ref = x64 @ w64 + b64
        bound = R.dot_bound(ni, np.abs(x64) @ np.abs(w64) + np.abs(b64))
        got = (x @ w + b).astype(np.float64)                       # float32 matmul, whatever order BLAS takes
        assert (np.abs(got - ref) <= bound).all(), (rows, ni, no)
        # the kernel's own order in float32: 16 slices, 4 accumulators, fixed-order tree
        seq = np.zeros((rows, no), np.float32)
        for lo, hi in R.dense_slices(ni):
            part = np.zeros((rows, no), np.float32)
            for i in range(lo, hi):
                part += x[:, i:i + 1] * w[i:i + 1, :]
            seq += part
        assert (np.abs((seq + b).astype(np.float64) - ref) <= bound).all(), (rows, ni, no)
        # one term of one output dropped, or counted twice
        i, rr, oo = ni // 2, rows // 2, no // 2
        term = x64[rr, i] * w64[i, oo]
        for wrong in (ref[rr, oo] - term, ref[rr, oo] + term):
            assert (abs(wrong - ref[rr, oo]) > bound[rr, oo]) == (abs(term) > bound[rr, oo])
    # and a typical term is far outside even at the longest reduction: the median |x w| against the largest bound at K = 512
    # (at K <= 128 the margin is two orders of magnitude)
    x, w = r.standard_normal((64, 512)), r.standard_normal((512, 64))
    assert np.median(np.abs(x[:, :1] * w[:1, :])) > 10 * R.dot_bound(512, np.abs(x) @ np.abs(w)).max()
    assert np.median(np.abs(x[:, :1] * w[:1, :])) > 100 * R.dot_bound(128, np.abs(x[:, :128]) @ np.abs(w[:128])).max()
    assert [hi - lo for lo, hi in R.dense_slices(72)] == [5] * 14 + [2, 0] and [hi - lo for lo, hi in R.dense_slices(113)][:2] == [8, 8]


def test_chosen_preactivation_construction():
    """O.siamese_head returns sigmoid(a) for the constructed pairs, to 1e-12 in float64."""
    r = np.random.default_rng(2)
    a = np.concatenate([r.uniform(-6, 6, 20), r.uniform(20, 30, 20), r.uniform(-21, -20, 20)])
    for head, e in (("uniform_euclidean", 1), ("uniform_euclidean", 64), ("uniform_euclidean", 65), ("weighted_l1", 1), ("weighted_l1", 256)):
        hw = np.array([[1.5]]) if head == "uniform_euclidean" else r.uniform(0.2, 1.0, (e, 1))
        hb = np.array([-21.0])
        emb = R.pairs_with_chosen_a(r, a, e, head, hw, hb)
        prm = {"head.kernel": torch.tensor(hw), "head.bias": torch.tensor(hb)}
        pr = O.siamese_head(prm, torch.tensor(emb[:60]), torch.tensor(emb[60:]), head).numpy()[:, 0]
        assert np.abs(pr - 1.0 / (1.0 + np.exp(-a))).max() < 1e-12, head
        ref = R.head_oracle(emb, hw, hb, (np.arange(60) % 2).astype(np.float64), head, "bce")
        assert np.abs(ref["pred"] - pr).max() == 0.0 and abs(ref["loss_pair"].mean() - ref["loss"]) < 1e-12
        assert abs(ref["dlda"].sum() - ref["ghb"][0]) < 1e-12 * max(1.0, abs(ref["ghb"][0]))      # d a / d bias = 1
        assert (ref["dlda"][20:] == 0.0).all()                                                 # clip_by_value: no gradient outside
    try:
        R.pairs_with_chosen_a(r, [-22.0], 8, "uniform_euclidean", [[1.5]], [-21.0])
        raise RuntimeError("a below the bias was accepted")
    except AssertionError:
        pass


def test_slab_sum_regime_table():
    """slab_sum's rule (csrc/reduce.hip) restated, and the table the device test's comment gives."""
    src = open(os.path.join(CSRC, "reduce.hip")).read()
    for line in ("int64_t rch = cdiv(2048, blocks);", "if (rch > slabs / 4) rch = slabs / 4;", "if (rch > SLAB_RCH) rch = SLAB_RCH;",
                 "if (slabs <= 64 && blocks >= 256) rch = 1;", "if (rch <= 1) {"):
        assert line in src, line
    nel = R.C1_K * 8
    want = {1: ("single", 1), 3: ("single", 1), 4: ("single", 1), 7: ("single", 1), 8: ("two-stage", 2, 4, 0), 9: ("two-stage", 2, 5, 0),
            31: ("two-stage", 7, 5, 0), 32: ("two-stage", 8, 4, 0), 33: ("two-stage", 8, 5, 1), 64: ("two-stage", 16, 4, 0),
            65: ("two-stage", 16, 5, 3), 67: ("two-stage", 16, 5, 2), 130: ("two-stage", 16, 9, 1), 1000: ("two-stage", 16, 63, 0)}
    assert sorted(want) == R.CONV1_WGRAD_SLABS_F8
    for slabs, regime in want.items():
        assert R.slab_regime(slabs, nel) == regime, slabs
    nel = R.C1_K * 2048
    assert nel >= 65281 and -(-nel // 256) >= 256
    want = {1: ("single", 1), 4: ("single", 1), 5: ("single", 1), 7: ("single", 1), 64: ("single", 1), 65: ("two-stage", 8, 9, 0)}
    assert sorted(want) == R.CONV1_WGRAD_SLABS_F2048
    for slabs, regime in want.items():
        assert R.slab_regime(slabs, nel) == regime, slabs


def test_colsum_bound_tells_float64_from_float32_accumulation():
    r = np.random.default_rng(3)
    x = R.cancelling_columns(r, 4096, 8)
    assert (x == 1e4).sum(0).tolist() == [1] * 8 and (x == -1e4).sum(0).tolist() == [1] * 8
    x64 = x.astype(np.float64)
    ref = x64.sum(0)
    bound = R.colsum_bound(np.abs(x64).sum(0), ref, 4096)
    assert (np.abs(ref.astype(np.float32).astype(np.float64) - ref) <= bound).all()           # float64 sum, one rounding: inside
    assert (np.abs(np.cumsum(x, axis=0, dtype=np.float32)[-1].astype(np.float64) - ref) > bound).any()   # fp32 accumulation: outside
    assert (np.abs((ref - x64[7]) - ref) > bound).sum() >= 7                                   # a dropped row: outside
    assert R.cancelling_columns(r, 1, 8).shape == (1, 8)


def test_adam_reference_arithmetic():
    """The float32 numpy step stays within the kernel test's bounds of the float64 oracle, so those bounds are satisfiable."""
    r = np.random.default_rng(4)
    n = 20000
    pv, m0 = r.standard_normal(n).astype(np.float32), (r.standard_normal(n) * 0.01).astype(np.float32)
    v0 = (r.random(n) * 1e-3).astype(np.float32)
    for norm, roundings in ((0.5, 4), (30.0, 8)):
        g = r.standard_normal(n)
        g = (g * (norm / np.linalg.norm(g))).astype(np.float32)
        gn = float(np.linalg.norm(g.astype(np.float64)))
        p64, m64, v64 = R.adam_oracle(R.adam_state(6, m0, v0), pv, g)
        p32, m32, v32 = R.adam_step_f32(pv, g, m0, v0, 7)
        assert np.abs(p32 - p64).max() < 2e-6
        gs = g.astype(np.float64) / (gn if gn >= 1.0 else 1.0)
        assert (np.abs(m32.astype(np.float64) - m64) <= R.adam_m_bound(m0, gs, roundings)).all()
        # one element that missed the update is far outside
        assert abs(np.float64(m0[5]) - m64[5]) > R.adam_m_bound(m0, gs, roundings)[5]
    assert abs(R.lr_t(7) / (1e-3 * np.sqrt(1 - 0.999 ** 7) / (1 - 0.9 ** 7)) - 1.0) < 1e-4    # the betas as fp32 scalars: what the kernel is handed
