"""-m gpu: vm_proto_loss through the C ABI against the float64 statement of the loss, inside the error bounds tests/proto_refs.py
derives by counting roundings (tests/test_proto_refs_cpu.py shows on the host that fp32 arithmetic in two summation orders stays
inside them and that three wrong variants do not)."""
import numpy as np
import pytest
import torch

from tests import proto_refs as R
from tests.gpu_util import L, dev, p, report, stream

pytestmark = pytest.mark.gpu

SENTINEL = -777.0


def _run(emb, labels, k, n, alpha=1.0, grad_scale=1.0, mode="train"):
    """One call; ``mode``: "train", "eval" (demb NULL) or "predict" (labels NULL).  Outputs are sentinel-filled beforehand and come
    back as numpy arrays (logits, loss_acc, demb, ws)."""
    N, E = emb.shape
    m = N - k * n
    e = dev(emb)
    lab = dev(labels, torch.int32) if mode != "predict" else None
    ws_n = L().query("vm_proto_loss_workspace_bytes", k, n, m, E) // 4
    logits, la, demb, ws = (dev(np.full(s, SENTINEL, np.float32)) for s in ((m, k), (2,), (N, E), (ws_n,)))
    assert L().query("vm_proto_loss_supported", k, n, m, E) == 1
    L().call("vm_proto_loss", p(e), p(lab), k, n, m, E, float(alpha), float(grad_scale), p(logits),
             p(la) if mode != "predict" else None, p(demb) if mode == "train" else None, p(ws) if mode != "predict" else None, stream())
    torch.cuda.synchronize()
    return {"logits": logits.cpu().numpy(), "la": la.cpu().numpy(), "demb": demb.cpu().numpy(), "ws": ws.cpu().numpy()}


def _out(o):
    return {"logits": o["logits"].astype(np.float64), "loss": float(o["la"][0]), "acc": float(o["la"][1]), "demb": o["demb"]}


def _check(tag, emb, labels, k, n, alpha, grad_scale=1.0):
    ref = R.proto_ref(emb, labels, k, n, alpha)
    bnd = R.proto_bounds(emb, labels, k, n, alpha, ref)
    o = _run(emb, labels, k, n, alpha, grad_scale)
    assert np.isfinite(o["logits"]).all() and np.isfinite(o["la"]).all() and np.isfinite(o["demb"]).all()
    w = R.ratios(_out(o), ref, bnd, grad_scale)
    for key, v in w.items():
        report(tag, "err_over_bound[%s]" % key, v)
    print(tag, "loss %.6f acc %.4f" % (ref["loss"], ref["acc"]), {a: "%.4f" % b for a, b in w.items()})
    assert all(v <= 1.0 for v in w.values()), w
    # queries whose argmax the bounds pin down are classified as the reference classifies them
    sure = ~bnd["ambiguous"]
    assert (o["logits"].argmax(1)[sure] == ref["pred"][sure]).all()
    return o, ref, bnd


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_outputs_are_inside_the_derived_bounds(case):
    k, n, m, E, alpha = case
    emb, lab = R.episode(k, n, m, E)
    _check("proto_loss[%s]" % R.case_id(case), emb, lab, k, n, alpha)


def test_a_class_without_a_query():
    k, n, m, E = 5, 2, 9, 64
    lab = np.array([0, 1, 1, 3, 4, 4, 4, 0, 3])            # nobody asks for class 2
    emb, lab = R.episode(k, n, m, E, labels=lab)
    o, ref, _ = _check("proto_loss[no-query-class]", emb, lab, k, n, 1.0)
    assert np.abs(ref["demb"][2 * n:3 * n]).max() > 0        # it still repels the other classes' queries


def test_identical_supports_tie_to_the_lower_class():
    k, n, m, E = 4, 2, 6, 32
    emb, lab = R.episode(k, n, m, E, labels=np.array([1, 3, 1, 3, 0, 2]))
    emb[3 * n:4 * n] = emb[1 * n:2 * n]                      # class 3 = class 1
    emb[k * n + 1], emb[k * n + 3] = emb[k * n + 0], emb[k * n + 2]   # the queries labelled 3 are copies of those labelled 1
    o = _run(emb, lab, k, n)
    assert np.array_equal(o["logits"][:, 1], o["logits"][:, 3])
    assert np.isfinite(o["demb"]).all() and np.isfinite(o["la"]).all()
    ref = R.proto_ref(emb, lab, k, n, 1.0)
    assert (ref["pred"][:4] == 1).all() and (o["logits"].argmax(1)[:4] == 1).all()   # nearest to both 1 and 3: the lower one wins
    # accuracy counts the class-1 queries as hits and the class-3 queries as misses, exactly
    hits = (ref["pred"] == lab).sum()
    assert o["la"][1] == np.float32(hits) / np.float32(m)
    w = R.ratios({"logits": o["logits"].astype(np.float64), "loss": float(o["la"][0]), "acc": float(ref["acc"]), "demb": o["demb"]},
                 ref, R.proto_bounds(emb, lab, k, n, 1.0, ref))
    assert all(v <= 1.0 for v in w.values()), w


def test_a_query_equal_to_its_prototype():
    k, n, m, E = 3, 1, 4, 48
    emb, lab = R.episode(k, n, m, E, labels=np.array([2, 0, 1, 2]))
    emb[k * n + 0] = emb[2]                                  # n = 1: the prototype is the support row, bit for bit
    o, ref, _ = _check("proto_loss[zero-distance]", emb, lab, k, n, 1.0)
    assert o["logits"][0, 2] == 0.0 and ref["logits"][0, 2] == 0.0


@pytest.mark.parametrize("case", [(5, 2, 9, 64, 1.0), (64, 2, 128, 64, 1.0)], ids=R.case_id)
def test_embeddings_times_twelve(case):
    """Logit gaps in the thousands: exp underflows; everything stays finite and inside the bounds."""
    k, n, m, E, alpha = case
    emb, lab = R.episode(k, n, m, E, scale=12.0)
    o, ref, _ = _check("proto_loss_x12[%s]" % R.case_id(case), emb, lab, k, n, alpha)
    assert np.ptp(ref["logits"], axis=1).max() > 1000


def test_grad_scale_is_an_exact_factor():
    k, n, m, E = 20, 5, 40, 64
    emb, lab = R.episode(k, n, m, E)
    a, b = _run(emb, lab, k, n, 1.0, 1.0), _run(emb, lab, k, n, 1.0, 1024.0)
    assert np.array_equal(b["demb"], np.float32(1024.0) * a["demb"])
    assert np.array_equal(a["la"], b["la"]) and np.array_equal(a["logits"], b["logits"])


def test_predict_only_and_evaluation_leave_the_other_outputs_alone():
    k, n, m, E = 5, 5, 25, 128
    emb, lab = R.episode(k, n, m, E)
    full = _run(emb, lab, k, n, 2.0)
    pred = _run(emb, lab, k, n, 2.0, mode="predict")
    assert np.array_equal(pred["logits"], full["logits"])
    assert (pred["la"] == SENTINEL).all() and (pred["demb"] == SENTINEL).all() and (pred["ws"] == SENTINEL).all()
    ev = _run(emb, lab, k, n, 2.0, mode="eval")
    assert np.array_equal(ev["logits"], full["logits"]) and np.array_equal(ev["la"], full["la"])
    assert (ev["demb"] == SENTINEL).all()
    assert not (full["demb"] == SENTINEL).any()              # training writes every row of demb


def test_two_calls_are_bit_identical():
    k, n, m, E = 64, 2, 128, 64
    emb, lab = R.episode(k, n, m, E)
    a, b = _run(emb, lab, k, n), _run(emb, lab, k, n)
    for key in ("logits", "la", "demb"):
        assert np.array_equal(a[key], b[key]), key


def test_a_label_outside_the_classes_takes_its_query_out():
    """include/voicemap_hip.h: such a query has no loss term, no hit and no gradient, its logits are written, the means still divide
    by m -- so loss and accuracy are (m - 1) / m of those of the episode without it, and the other rows' gradients scale alike."""
    k, n, m, E = 5, 2, 9, 64
    emb, lab = R.episode(k, n, m, E)
    for bad in (-1, k, 1 << 20):
        lab2 = lab.copy()
        lab2[4] = bad
        o = _run(emb, lab2, k, n)
        keep = np.r_[0:k * n + 4, k * n + 5:k * n + m]
        ref = R.proto_ref(emb[keep], np.delete(lab, 4), k, n, 1.0)
        bnd = R.proto_bounds(emb[keep], np.delete(lab, 4), k, n, 1.0, ref)
        f = (m - 1) / m
        assert np.isfinite(o["demb"]).all() and (o["demb"][k * n + 4] == 0).all()
        assert np.abs(o["logits"][np.arange(m) != 4] - ref["logits"]).max() <= bnd["logits"].max()
        assert abs(o["la"][0] - f * ref["loss"]) <= bnd["loss"] + 4 * R.U32 * ref["loss"]
        assert abs(o["la"][1] - f * ref["acc"]) <= bnd["acc"]
        assert (np.abs(o["demb"][keep] - f * ref["demb"]) <= bnd["demb"] + 4 * R.U32 * np.abs(ref["demb"])).all()
