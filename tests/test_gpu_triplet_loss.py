"""-m gpu: vm_triplet_loss through the C ABI, {batch hard, batch all} x {hinge, soft margin}, against the float64 statement of the
loss in two stages (tests/triplet_refs.py): the kernel's selections are admissible, and the float64 loss and gradient evaluated WITH
those selections agree inside the error bounds derived there by counting roundings (tests/test_triplet_refs_cpu.py shows on the
host that fp32 arithmetic in two summation orders stays inside them, that five wrong variants do not, and that every input used here
is inside its ambiguity caps)."""
import numpy as np
import pytest
import torch

from tests import triplet_refs as R
from tests.gpu_util import L, dev, p, report, stream

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
INPUTS = R.gpu_inputs()
_REF = {}      # (input name, variant) -> the analysis with the reference's own selections, computed once


def _run(emb, labels, mining, soft, margin=R.MARGIN, grad_scale=1.0, train=True, indices=True):
    """One call.  Outputs are sentinel-filled beforehand and come back as numpy arrays (hp, hn, la, demb) + loss / share."""
    N, E = emb.shape
    e, lab = dev(emb), dev(labels, torch.int32)
    assert L().query("vm_triplet_loss_supported", N, E) == 1
    ws_n = L().query("vm_triplet_loss_workspace_bytes", N, E, mining) // 4
    la, demb, ws = (dev(np.full(s, SENTINEL, np.float32)) for s in ((2,), (N, E), (ws_n,)))
    hp, hn = dev(np.full(N, -7, np.int32), torch.int32), dev(np.full(N, -7, np.int32), torch.int32)
    L().call("vm_triplet_loss", p(e), p(lab), N, E, mining, soft, float(margin), float(grad_scale), p(hp) if indices else None,
             p(hn) if indices else None, p(la), p(demb) if train else None, p(ws), stream())
    torch.cuda.synchronize()
    o = {"hp": hp.cpu().numpy(), "hn": hn.cpu().numpy(), "la": la.cpu().numpy(), "demb": demb.cpu().numpy()}
    o["loss"], o["share"] = float(o["la"][0]), float(o["la"][1])
    return o


def _check(tag, emb, labels, variant, margin=R.MARGIN, grad_scale=1.0, key=None):
    mining, soft = variant
    o = _run(emb, labels, mining, soft, margin, grad_scale)
    assert np.isfinite(o["la"]).all() and np.isfinite(o["demb"]).all()
    an = _REF.get(key) if key else None
    if an is None:
        an = R.analyse(emb, labels, mining, soft, margin)
        if key:
            _REF[key] = an
    if not (np.array_equal(o["hp"], an["hp_ref"]) and np.array_equal(o["hn"], an["hn_ref"])):
        an = R.analyse(emb, labels, mining, soft, margin, o["hp"], o["hn"])    # stage 2 is evaluated with the kernel's selections
    bad = R.admissible(o["hp"], o["hn"], an)
    assert not bad, bad[:3]
    w = R.ratios(o, an, grad_scale)
    for k, v in w.items():
        report(tag, "err_over_bound[%s]" % k, v)
    print(tag, "loss %.6f share %.4f V %d T %d A %d ambiguous %d" % (an["loss"], an["share"], an["V"], an["T"], an["A"], an["n_amb"]),
          {a: "%.4f" % b for a, b in w.items()})
    assert all(v <= 1.0 for v in w.values()), w
    return o, an


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
@pytest.mark.parametrize("inp", INPUTS, ids=[i[0] for i in INPUTS])
def test_outputs_are_inside_the_derived_bounds(inp, variant):
    name, kind, emb, lab = inp
    o, an = _check("triplet_loss[%s-%s]" % (name, R.variant_id(variant)), emb, lab, variant, key=(name, variant))
    if kind == "small":     # no ambiguity there: the selections are the reference's and the counts exact
        assert np.array_equal(o["hp"], an["hp_ref"]) and np.array_equal(o["hn"], an["hn_ref"])
        assert o["share"] == np.float32(an["A"]) / np.float32(an["T"])


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_ragged_batch_rows_that_take_no_part_or_have_no_positive(variant):
    emb, lab = R.ragged_batch()
    o, an = _check("triplet_loss[ragged-%s]" % R.variant_id(variant), emb, lab, variant)
    out = int(np.flatnonzero(lab == -1)[0])
    assert (o["demb"][out] == 0).all() and o["hp"][out] == -1 and o["hn"][out] == -1
    assert out not in o["hp"] and out not in o["hn"]
    single = [int(np.flatnonzero(lab == c)[0]) for c in (10, 14)]
    assert (o["hp"][single] == -1).all() and (o["hn"][single] == -1).all() and not an["valid"][single].any()
    for a in single:      # no anchor, yet a negative of others: wherever the reference gives it gradient the kernel does too
        if np.abs(an["demb"][a]).max() > 0:
            assert np.abs(o["demb"][a]).max() > 0
    if variant[0] == R.ALL:
        assert all(np.abs(an["demb"][a]).max() > 0 for a in single)
    # a row that takes no part may hold anything
    emb2 = emb.copy()
    emb2[out] = np.nan
    o2 = _run(emb2, lab, *variant)
    assert np.array_equal(o2["la"], o["la"]) and np.array_equal(o2["demb"], o["demb"])


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_one_label_means_no_valid_anchor(variant):
    emb, _ = R.pk_batch(3, 3, 16)
    o = _run(emb, np.full(9, 5, np.int32), *variant)
    assert (o["la"] == 0).all() and (o["hp"] == -1).all() and (o["hn"] == -1).all()
    assert (o["demb"].view(np.uint32) == 0).all()


@pytest.mark.parametrize("mining", [R.HARD, R.ALL], ids=["hard", "all"])
def test_well_separated_classes_at_margin_zero(mining):
    rng = np.random.default_rng(7)
    lab = np.repeat(np.arange(4), 3).astype(np.int32)
    emb = (100.0 * np.eye(4, 8)[lab] + rng.normal(0, 0.1, (12, 8))).astype(np.float32)
    o = _run(emb, lab, mining, 0, margin=0.0)
    assert o["la"][0] == 0.0 and o["la"][1] == 0.0 and (o["demb"].view(np.uint32) == 0).all()
    assert (o["hp"] >= 0).all() and (o["hn"] >= 0).all()


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_duplicate_rows_within_a_class(variant):
    emb, lab = R.pk_batch(3, 2, 8, seed=4)
    emb[1] = emb[0]                                  # class 0 is one point twice: s_01 = 0, its pair has no direction
    o, an = _check("triplet_loss[duplicates-%s]" % R.variant_id(variant), emb, lab, variant)
    assert o["hp"][0] == 1 and o["hp"][1] == 0
    # rows 0 and 1 are then moved by their negatives alone, and alike
    assert np.array_equal(o["demb"][0], o["demb"][1])
    # all rows one point: every s is 0, nothing is divided by it
    z = _run(np.ones((4, 8), np.float32), np.array([0, 0, 1, 1], np.int32), *variant)
    assert np.isfinite(z["la"]).all() and (z["demb"] == 0).all()


def _grid(N, E, classes, seed):
    """Integer embeddings (in -4..4; in -1..1 for a long row, so that equal distances still occur) and random labels."""
    rng = np.random.default_rng(seed)
    lo, hi = (-4, 5) if E <= 64 else (-1, 2)
    return rng.integers(lo, hi, (N, E)).astype(np.float32), rng.integers(0, classes, N).astype(np.int32)


def test_ties_go_to_the_lower_row():
    #               anchor   near+   far+ a  far+ b  far-    near- a near- b
    emb = np.array([[0, 0], [1, 0], [3, 4], [5, 0], [7, 7], [0, 2], [2, 0]], np.float32)
    lab = np.array([0, 0, 0, 0, 1, 1, 1], np.int32)
    for variant in R.VARIANTS:
        o = _run(emb, lab, *variant)
        assert o["hp"][0] == 2 and o["hn"][0] == 5, variant          # s = 25 twice, s = 4 twice
    o = _run(emb[[0, 1, 3, 2, 4, 6, 5]], lab, R.HARD, 0)             # the equidistant rows swapped: still the lower index
    assert o["hp"][0] == 2 and o["hn"][0] == 5


@pytest.mark.parametrize("shape", [(40, 16, 5), (300, 7, 9), (129, 130, 4)], ids=str)
def test_integer_grid_selections_are_exactly_the_references(shape):
    """Every s is a small integer, exact in fp32 in any order: the selections (ties included) are the float64 reference's."""
    emb, lab = _grid(*shape, seed=shape[0])
    lab[3] = -1
    s = R.sq_dists(emb.astype(np.float64))
    hp, hn, valid = R.select(s, *R.masks(lab))
    ties = sum(int((np.where(m[a], s[a], -1) == s[a, i[a]]).sum() > 1) for m, i in zip(R.masks(lab), (hp, hn)) for a in np.flatnonzero(valid))
    assert ties > 0
    for variant in ((R.HARD, 0), (R.ALL, 1)):
        o = _run(emb, lab, *variant)
        assert np.array_equal(o["hp"], hp) and np.array_equal(o["hn"], hn)


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_grad_scale_is_an_exact_factor(variant):
    emb, lab = R.pk_batch(12, 4, 64)
    a, b = _run(emb, lab, *variant), _run(emb, lab, *variant, grad_scale=1024.0)
    assert np.array_equal(b["demb"], np.float32(1024.0) * a["demb"]) and np.abs(a["demb"]).max() > 0
    assert np.array_equal(a["la"], b["la"]) and np.array_equal(a["hp"], b["hp"]) and np.array_equal(a["hn"], b["hn"])


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_evaluation_leaves_demb_alone_and_the_indices_are_optional(variant):
    emb, lab = R.ragged_batch()
    full = _run(emb, lab, *variant)
    ev = _run(emb, lab, *variant, train=False)
    assert (ev["demb"] == SENTINEL).all() and not (full["demb"] == SENTINEL).any()     # training writes every row
    assert np.array_equal(ev["la"], full["la"]) and np.array_equal(ev["hp"], full["hp"]) and np.array_equal(ev["hn"], full["hn"])
    noidx = _run(emb, lab, *variant, indices=False)
    assert np.array_equal(noidx["la"], full["la"]) and np.array_equal(noidx["demb"], full["demb"])
    assert (noidx["hp"] == -7).all() and (noidx["hn"] == -7).all()


@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_two_calls_are_bit_identical(variant):
    emb, lab = R.pk_batch(64, 4, 64, seed=3)
    a, b = _run(emb, lab, *variant), _run(emb, lab, *variant)
    for key in ("la", "demb", "hp", "hn"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("variant", R.VARIANTS, ids=R.variant_id)
def test_a_non_finite_row_makes_loss_and_gradient_non_finite(variant, value):
    """What the f16 loss-scale skip relies on."""
    emb, lab = R.pk_batch(12, 4, 64)
    emb[17, 5] = value
    o = _run(emb, lab, *variant)
    assert not np.isfinite(o["la"][0]) and not np.isfinite(o["demb"]).all()
