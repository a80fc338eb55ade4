"""Host checks of tests/margin_refs.py (no GPU): the closed-form gradients against autograd, the fp32 restatement in both summation
orders inside the bounds, the ambiguity caps of every GPU input, and planted defects in the host model of the kernel, each of which
must break a bound."""
import numpy as np
import pytest

from tests import margin_refs as R

CASES = [(k, m, s) for (k, m) in R.KINDS for s in R.SCALES]


def _case_id(c):
    return "%s-s%g" % (R.kind_id(c[:2]), c[2])


@pytest.fixture(scope="module")
def planted():
    return R.planted_batch()


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_closed_form_gradients_are_autograd(case, planted):
    kind, margin, scale = case
    for e, w, lab in (R.batch(7, 65, 63), R.batch(3, 5, 3), planted[:3], R.e1_batch()):
        an = R.analyse(e, w, lab, kind, margin, scale)
        loss, ge, gw = R.autograd(e, w, lab, kind, margin, scale)
        assert abs(loss - an["loss"]) < 1e-10
        assert np.abs(ge - an["demb"]).max() < 1e-10 * max(1.0, np.abs(ge).max())
        assert np.abs(gw - an["grad_w"]).max() < 1e-10 * max(1.0, np.abs(gw).max())


def test_the_planted_batch_holds_what_it_says(planted):
    e, w, lab, what = planted
    an = R.analyse(e, w, lab, R.ANGULAR, 0.5, 30.0)
    c = an["c"]
    assert not an["part"][list(what["out"])].any() and an["part"].sum() == 5
    assert (c[what["zero_row"]] == 0).all() and (c[:, what["zero_col"]] == 0).all()
    assert (an["demb"][what["zero_row"]] == 0).all() and (an["grad_w"][:, what["zero_col"]] == 0).all()
    assert (an["demb"][list(what["out"])] == 0).all()
    a, b = what["twins"]
    assert (c[:, a] == c[:, b]).all() and an["pred_ref"][what["twin_row"]] == a and lab[what["twin_row"]] == b
    th = R.constants(R.ANGULAR, 0.5)[2]
    hi, lo = what["branches"]
    assert c[hi, lab[hi]] > th + 0.03 and c[lo, lab[lo]] < th - 0.03
    assert abs(c[what["floor_row"], lab[what["floor_row"]]] - 1.0) < 1e-12
    fr = list(an["rows"]).index(what["floor_row"])
    cm, sm = R.constants(R.ANGULAR, 0.5)[:2]
    assert abs(an["f"][fr] - (cm + sm / R.SIN_FLOOR)) < 1e-9          # the floor is in force


@pytest.mark.parametrize("case", CASES, ids=_case_id)
@pytest.mark.parametrize("rev", [False, True], ids=["ascending", "descending"])
def test_fp32_restatement_is_inside_the_bounds(case, rev, planted):
    kind, margin, scale = case
    inputs = [("N%d-S%d-E%d-s%d" % c, R.batch(*c)) for c in R.SMALL[:3]] + [("planted", planted[:3])]
    for name, (e, w, lab) in inputs:
        for gs in (1.0, 1024.0):
            out = R.margin_f32(e, w, lab, kind, margin, scale, rev=rev, grad_scale=gs)
            bad, r, an = R.check(out, e, w, lab, kind, margin, scale, gs)
            assert not bad, (name, bad)
            assert all(v <= 1.0 for v in r.values()), (name, gs, r)


def test_caps_hold_for_every_gpu_input():
    for name, cap, e, w, lab in R.gpu_inputs():
        pred_amb, branch_amb = R.ambiguity(e, w, lab)
        print(name, "ambiguous pred rows", pred_amb * len(e), "ambiguous branch rows", branch_amb * len(e))
        assert pred_amb <= R.CAPS[cap][0] and branch_amb <= R.CAPS[cap][1], name
        an = R.analyse(e, w, lab, R.ANGULAR, 0.5, 1.0)
        assert np.abs(an["cy"] - R.constants(R.ANGULAR, 0.5)[2]).min() >= 0.03, name
    e, w, lab, _ = R.planted_batch()
    assert R.ambiguity(e, w, lab)[1] == 0.0     # (the twins tie the argmax of every row they top: admissible either way, the first is asked for)


@pytest.mark.parametrize("wrong", R.WRONG)
def test_a_planted_defect_breaks_a_bound(wrong, planted):
    """Each defect on the input that shows it: the angular ones need both branches and the floor (the planted batch)."""
    e, w, lab = planted[:3] if wrong in ("wrong_side", "no_floor") else R.batch(7, 65, 63)
    # (at scale 30 the floored row, c_iy = 1, has p_y = 1 to rounding and so no gradient to amplify: the floor shows at scale 1)
    kind, margin, scale = R.ANGULAR, 0.5, 1.0 if wrong == "no_floor" else 30.0
    good = R.margin_f32(e, w, lab, kind, margin, scale)
    bad0, r0, _ = R.check(good, e, w, lab, kind, margin, scale)
    assert not bad0 and all(v <= 1.0 for v in r0.values())
    out = R.margin_f32(e, w, lab, kind, margin, scale, wrong=wrong)
    bad, r, _ = R.check(out, e, w, lab, kind, margin, scale)
    with np.errstate(invalid="ignore"):
        broken = [k for k, v in r.items() if not v <= 1.0]
    print(wrong, r)
    assert not bad and broken, (wrong, r)
    if wrong == "no_projection":
        assert broken == ["demb"]


def test_loss_object_matches_the_statement():
    from voicemap_amd.utils import MarginSoftmaxLoss
    e, w, lab = R.batch(7, 65, 63)
    for kind, name, margin in ((R.NONE, "none", 0.0), (R.COSINE, "cosine", 0.35), (R.ANGULAR, "angular", 0.5)):
        loss = MarginSoftmaxLoss(name, margin=margin, scale=30.0)
        an = R.analyse(e, w, lab, kind, margin, 30.0)
        c = an["c"]
        assert abs(loss(c, lab) - an["loss"]) < 1e-6
        assert loss.get_config() == {"kind": name, "margin": float(margin), "scale": 30.0}
    with pytest.raises(ValueError):
        MarginSoftmaxLoss("arc")
    with pytest.raises(ValueError):
        MarginSoftmaxLoss("angular", margin=2.0)
    with pytest.raises(ValueError):
        MarginSoftmaxLoss("angular", scale=0.0)
