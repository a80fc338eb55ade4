"""-m gpu: vm_margin_softmax through the C ABI, {none, additive cosine, additive angular} x two scales, against the float64 statement
of the loss in two stages (tests/margin_refs.py): the kernel's argmax is admissible, and the cosines, the probabilities, the loss, the
hits counted WITH that argmax and both gradients agree inside the error bounds derived there by counting roundings
(tests/test_margin_refs_cpu.py shows on the host that fp32 arithmetic in two summation orders stays inside them, that five planted
defects do not, and that every input used here is inside its ambiguity caps)."""
import numpy as np
import pytest
import torch

from tests import margin_refs as R
from tests.gpu_util import L, dev, p, report, stream

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
GUARD = 64           # guard words on either side of every output and of ws
INPUTS = R.gpu_inputs()
CASES = [(k, m, s) for (k, m) in R.KINDS for s in R.SCALES]
_COS = {}            # input name -> cosines64, computed once
WORST = {}           # quantity -> the worst error / bound ratio seen (printed by the last test)


def _case_id(c):
    return "%s-s%g" % (R.kind_id(c[:2]), c[2])


def _guarded(n, dtype=torch.float32, fill=SENTINEL):
    t = dev(np.full(n + 2 * GUARD, fill, np.float32 if dtype == torch.float32 else np.int32), dtype)
    return t, t[GUARD:GUARD + n]


def _intact(t, n):
    h = t.cpu().numpy()
    return (h[:GUARD] == h[0]).all() and (h[GUARD + n:] == h[0]).all() and h[0] in (SENTINEL, -7)


def _run(emb, w, labels, kind, margin, scale, grad_scale=1.0, train=True, want=("cosine", "prob", "pred", "grad_b"), expect_rc=0):
    """One call.  Outputs are sentinel-filled beforehand, sit between guard words and come back as numpy arrays; the guards of every
    buffer (ws included) are checked after the call.  ``labels`` None: predict only; ``train`` False: evaluation."""
    N, E = emb.shape
    S = w.shape[1]
    e, wd = dev(emb), dev(w)
    lab = None if labels is None else dev(labels, torch.int32)
    assert L().query("vm_margin_softmax_supported", N, S, E) == 1
    ws_n = L().query("vm_margin_softmax_workspace_bytes", N, S, E) // 4
    sizes = {"cosine": N * S, "prob": N * S, "la": 2, "demb": N * E, "grad_w": E * S, "grad_b": S, "ws": ws_n}
    buf = {k: _guarded(n) for k, n in sizes.items()}
    buf["pred"] = _guarded(N, torch.int32, -7)
    sizes["pred"] = N
    arg = lambda k, on=True: p(buf[k][1]) if on else None
    L().call("vm_margin_softmax", p(e), p(wd), p(lab), N, S, E, kind, float(margin), float(scale), float(grad_scale),
             arg("cosine", "cosine" in want), arg("prob", "prob" in want), arg("pred", "pred" in want), arg("la", labels is not None),
             arg("demb", train and labels is not None), arg("grad_w", train and labels is not None),
             arg("grad_b", train and labels is not None and "grad_b" in want), arg("ws"), stream())
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert _intact(buf[k][0], n), "guard words of %s" % k
    shape = {"cosine": (N, S), "prob": (N, S), "demb": (N, E), "grad_w": (E, S)}
    o = {k: buf[k][1].cpu().numpy().reshape(shape.get(k, (-1,))) for k in sizes if k != "ws"}
    o["loss"], o["acc"] = float(o["la"][0]), float(o["la"][1])
    return o


def _check(tag, name, emb, w, lab, case, grad_scale=1.0):
    kind, margin, scale = case
    o = _run(emb, w, lab, kind, margin, scale, grad_scale)
    if name not in _COS:
        _COS.clear()          # one input's float64 cosines at a time (the parametrisation keeps an input's cases together)
        _COS[name] = R.cosines64(emb, w)
    bad, r, an = R.check(o, emb, w, lab, kind, margin, scale, grad_scale, cos=_COS[name])
    assert not bad, bad[:3]
    for k, v in r.items():
        report(tag, "err_over_bound[%s]" % k, v)
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(tag, "loss %.6f acc %.4f ambiguous pred rows %d" % (an["loss"], an["acc"], an["pred_amb"].sum()), {a: "%.4f" % b for a, b in r.items()})
    assert all(v <= 1.0 for v in r.values()), r
    return o, an


@pytest.mark.parametrize("case", CASES, ids=_case_id)
@pytest.mark.parametrize("inp", INPUTS, ids=[i[0] for i in INPUTS])
def test_outputs_are_inside_the_derived_bounds(inp, case):
    name, cap, emb, w, lab = inp
    o, an = _check("margin_softmax[%s-%s]" % (name, _case_id(case)), name, emb, w, lab, case)
    assert np.isfinite(o["la"]).all() and np.isfinite(o["demb"]).all() and np.isfinite(o["grad_w"]).all()
    assert (o["grad_b"].view(np.uint32) == 0).all()
    assert np.abs(o["prob"].astype(np.float64).sum(1) - 1.0).max() < (w.shape[1] + 8) * R.U32
    if cap == "small":       # no ambiguity there: the argmax is the reference's
        assert np.array_equal(o["pred"], an["pred_ref"])
    # grad_scale = 1024, a power of two: the gradients scale exactly, nothing else moves
    kind, margin, scale = case
    b = _run(emb, w, lab, kind, margin, scale, grad_scale=1024.0)
    assert np.array_equal(b["demb"], np.float32(1024.0) * o["demb"]) and np.array_equal(b["grad_w"], np.float32(1024.0) * o["grad_w"])
    assert np.abs(o["demb"]).max() > 0 and np.abs(o["grad_w"]).max() > 0
    for k in ("la", "cosine", "prob", "pred", "grad_b"):
        assert np.array_equal(b[k], o[k]), k


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_plants(case):
    emb, w, lab, what = R.planted_batch()
    S = w.shape[1]
    o, an = _check("margin_softmax[planted-%s]" % _case_id(case), "planted", emb, w, lab, case)
    for i in what["out"]:                      # a label of -1 and a label of S: out of every sum, the predictions still written
        assert (o["demb"][i].view(np.uint32) == 0).all()
        assert not (o["cosine"][i] == SENTINEL).any() and not (o["prob"][i] == SENTINEL).any() and 0 <= o["pred"][i] < S
    assert (o["cosine"][what["zero_row"]] == 0).all() and (o["demb"][what["zero_row"]] == 0).all()
    assert (o["cosine"][:, what["zero_col"]] == 0).all() and (o["grad_w"][:, what["zero_col"]] == 0).all()
    a, b = what["twins"]
    assert np.array_equal(o["cosine"][:, a].view(np.uint32), o["cosine"][:, b].view(np.uint32))
    assert o["pred"][what["twin_row"]] == a and lab[what["twin_row"]] == b        # the first maximum wins: no hit
    assert o["acc"] == np.float32(np.float32((o["pred"][an["rows"]] == lab[an["rows"]]).sum()) / np.float32(len(emb)))
    fr = what["floor_row"]
    assert o["cosine"][fr, lab[fr]] > 1.0 - an["bounds"]["c"] and np.isfinite(o["demb"][fr]).all()   # (sin_t is under the floor there)
    # rows that take no part may hold anything
    emb2 = emb.copy()
    emb2[list(what["out"])] = np.nan
    o2 = _run(emb2, w, lab, *case)
    for k in ("la", "demb", "grad_w"):
        assert np.array_equal(o2[k], o[k]), k


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_one_component(case):
    """E = 1: every cosine is +-1 exactly, every row ties and the first maximum wins."""
    emb, w, lab = R.e1_batch()
    o, an = _check("margin_softmax[E1-%s]" % _case_id(case), "E1", emb, w, lab, case)
    assert np.array_equal(o["cosine"], np.sign(emb) * np.sign(w))
    assert np.array_equal(o["pred"], an["pred_ref"]) and np.isfinite(o["demb"]).all() and np.isfinite(o["grad_w"]).all()


@pytest.mark.parametrize("case", CASES[2:4] + CASES[6:], ids=_case_id)
def test_modes(case):
    emb, w, lab = R.batch(65, 257, 65)
    full = _run(emb, w, lab, *case)
    ev = _run(emb, w, lab, *case, train=False)
    for k in ("demb", "grad_w", "grad_b"):     # evaluation leaves the gradients alone; training writes every element
        assert (ev[k] == SENTINEL).all() and not (full[k] == SENTINEL).any(), k
    for k in ("la", "cosine", "prob", "pred"):
        assert np.array_equal(ev[k], full[k]), k
    pr = _run(emb, w, None, *case)
    assert (pr["la"] == SENTINEL).all() and (pr["demb"] == SENTINEL).all() and (pr["grad_w"] == SENTINEL).all()
    for k in ("cosine", "prob", "pred"):
        assert np.array_equal(pr[k], full[k]), k
    none = _run(emb, w, lab, *case, want=())  # outputs passed as NULL are not touched, the rest does not change
    assert (none["cosine"] == SENTINEL).all() and (none["prob"] == SENTINEL).all() and (none["pred"] == -7).all()
    assert (none["grad_b"] == SENTINEL).all()
    for k in ("la", "demb", "grad_w"):
        assert np.array_equal(none[k], full[k]), k


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_two_calls_are_bit_identical(case):
    emb, w, lab = R.batch(64, 1000, 64, seed=3)
    a, b = _run(emb, w, lab, *case), _run(emb, w, lab, *case)
    for k in ("la", "cosine", "prob", "pred", "demb", "grad_w"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("where", ["row", "column"])
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("case", CASES[:1] + CASES[2:3] + CASES[7:], ids=_case_id)
def test_a_non_finite_input_makes_loss_and_gradient_nan(case, value, where):
    """What the f16 loss-scale skip relies on: an input value, not a fault."""
    emb, w, lab = R.batch(7, 65, 63)
    if where == "row":
        emb[4, 5] = value
    else:
        w[5, 11] = value
    o = _run(emb, w, lab, *case)
    assert np.isnan(o["la"][0])
    rows = [4] if where == "row" else range(7)
    assert all(np.isnan(o["demb"][i]).all() for i in rows)


def test_refusals_come_before_any_launch():
    from voicemap_amd._lib import VoicemapHipError
    assert L().query("vm_margin_softmax_supported", 4096, 16384, 256) == 1 and L().query("vm_margin_softmax_supported", 1, 2, 1) == 1
    assert L().query("vm_margin_softmax_supported", 8, 1, 8) == 0 and L().query("vm_margin_softmax_supported", 8, 8, 257) == 0
    assert L().query("vm_margin_softmax_supported", 4097, 8, 8) == 0 and L().query("vm_margin_softmax_supported", 8, 16385, 8) == 0
    emb, w, lab = R.batch(7, 65, 63)
    e257, w257, _ = R.batch(7, 65, 257)
    for what, (ee, ww, kind, margin, scale) in {"S = 1": (emb, w[:, :1], R.ANGULAR, 0.2, 30.0), "E = 257": (e257, w257, R.ANGULAR, 0.2, 30.0),
                                                 "margin < 0": (emb, w, R.COSINE, -0.1, 30.0), "margin >= pi / 2": (emb, w, R.ANGULAR, 1.6, 30.0),
                                                 "kind = 3": (emb, w, 3, 0.2, 30.0), "scale = 0": (emb, w, R.ANGULAR, 0.2, 0.0),
                                                 "margin nan": (emb, w, R.ANGULAR, float("nan"), 30.0)}.items():
        N, E = ee.shape
        S = ww.shape[1]
        la, (dt, demb), (ct, cosine) = dev(np.full(2, SENTINEL, np.float32)), _guarded(N * E), _guarded(N * S)
        ws = dev(np.full(S + N * E + 2 * N + 2 * N * S, SENTINEL, np.float32))
        gw = dev(np.full(E * S, SENTINEL, np.float32))
        with pytest.raises(VoicemapHipError):
            L().call("vm_margin_softmax", p(dev(ee)), p(dev(ww)), p(dev(lab, torch.int32)), N, S, E, kind, float(margin), float(scale), 1.0,
                     p(cosine), None, None, p(la), p(demb), p(gw), None, p(ws), stream())
        torch.cuda.synchronize()
        for t in (la, dt, ct, ws, gw):       # nothing was launched: nothing was written
            assert (t == SENTINEL).all(), what


def test_worst_ratios_are_reported():
    """Runs last in this file: the worst error / bound ratio per quantity over everything above."""
    print("margin_softmax worst error/bound ratios:", {k: "%.4f" % v for k, v in sorted(WORST.items())})
    for k, v in WORST.items():
        report("margin_softmax[worst]", "err_over_bound[%s]" % k, v)
    assert all(v <= 1.0 for v in WORST.values())
