"""-m gpu: the fp32 tail of the training step -- gradient norm and Adam (csrc/optim.hip), Dense, siamese head, both losses
(csrc/tail.hip), slab sums (csrc/reduce.hip) and column sums (colreduce_* in csrc/bnpool.hip) -- at the sizes training uses, at every
edge of the unrolled loops and at the loss clips.  Every reference is float64 from the definition (or the oracle in float32 where the
reference itself computes in float32: the clipped losses); output buffers start as NaN, and buffers with a length carry a sentinel tail
that is checked after the launch.  Bounds are derived (tests/tail_refs.py), not tuned."""
import numpy as np
import pytest
import torch

from oracle import voicemap_oracle as O
from tests import tail_refs as R
from tests.gpu_util import L, dev, max_err, p, padded, quant, rel_err, report, stream, DTYPES

pytestmark = pytest.mark.gpu

S = R.S
SENT = 12345.0
TAIL = 300          # sentinel elements behind every sized buffer


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def with_tail(a, n):
    """device copy of a[:n] followed by TAIL sentinel elements"""
    t = torch.full((n + TAIL,), SENT, device="cuda")
    t[:n] = torch.as_tensor(np.asarray(a, dtype=np.float32)[:n])
    return t


def tail_ok(t, n):
    return bool((t[n:] == SENT).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def sq_ws(n):
    return torch.full((L().query("vm_sqnorm_workspace_bytes", n) // 8,), float("nan"), dtype=torch.float64, device="cuda")


def grad_sqnorm(G, n, ws=None):
    ws = sq_ws(n) if ws is None else ws
    sq = nan(1)
    L().call("vm_grad_sqnorm", p(G), n, p(ws), p(sq), stream())
    return sq


def adam(P_, G_, M_, V_, n, t, clipnorm=1.0, prescale=1.0, sq=None, parts=None, skip=0, skipped=None):
    L().call("vm_adam_clip_step", p(P_), p(G_), p(M_), p(V_), n, R.lr_t(t), R.B1, R.B2, R.EPS, clipnorm, prescale, p(sq), p(parts), skip,
             p(skipped), stream())


# ==========================================================================================================
# 1. vm_grad_sqnorm
# ==========================================================================================================
def test_cfg_a_flat_size_is_what_the_engine_allocates():
    n = R.n_cfg_a()
    assert n == R.n_cfg_a_from_architecture() and 8 * S < n < 16 * S     # the main loop runs once per thread, then the tail loop


@pytest.mark.parametrize("n", R.sqnorm_sizes())
def test_grad_sqnorm_counts_every_element_once(n):
    """g = 1 everywhere: float(n) exactly (float64 partials, n < 2^24); one 3 among zeros: exactly 9, wherever it sits -- at both ends
    and within one element of every multiple of S, 7S, 8S (the grid's stride, the main loop's entry condition and its step)."""
    assert n < 2 ** 24
    ws = sq_ws(n)
    G = torch.full((n + TAIL,), float("nan"), device="cuda")     # an element read past n poisons the sum
    G[:n] = 1.0
    assert grad_sqnorm(G, n, ws).item() == float(n)
    G[:n] = 0.0
    for j in R.hot_indices(n):
        G[j] = 3.0
        got = grad_sqnorm(G, n, ws).item()
        G[j] = 0.0
        assert got == 9.0, (n, j, got)


@pytest.mark.parametrize("n", R.sqnorm_sizes())
def test_grad_sqnorm_values_and_both_forms(n):
    """Magnitudes that vary along the buffer against the float64 sum: the device adds in float64 and rounds once, 2 x 2^-24 relative.
    The partials-only form + vm_adam_clip_step publishes the same bits as the final kernel."""
    r = np.random.default_rng(101)
    g = R.graded_gradient(r, n)
    ref = float(np.sum(g.astype(np.float64) ** 2))
    G = torch.full((n + TAIL,), float("nan"), device="cuda")
    G[:n] = torch.as_tensor(g)
    ws = sq_ws(n)
    sq = grad_sqnorm(G, n, ws)
    err = abs(sq.item() - ref)
    report("step_tail.sqnorm", "n=%d rel err" % n, err / ref)
    assert err <= 2 * R.U32 * ref, (n, sq.item(), ref)
    ws2, sq2 = sq_ws(n), nan(1)
    L().call("vm_grad_sqnorm", p(G), n, p(ws2), None, stream())
    P_, M_, V_ = with_tail(np.zeros(n), n), with_tail(np.zeros(n), n), with_tail(np.zeros(n), n)
    adam(P_, G, M_, V_, n, 1, sq=sq2, parts=ws2)
    assert same_bits(sq, sq2) and torch.equal(ws, ws2)
    assert tail_ok(P_, n) and tail_ok(M_, n) and tail_ok(V_, n)


# ==========================================================================================================
# 2. vm_adam_clip_step
# ==========================================================================================================
def _adam_inputs(r, n, norm):
    pv = r.standard_normal(n).astype(np.float32)
    g = r.standard_normal(n)
    g = (g * (norm / np.linalg.norm(g))).astype(np.float32)
    m0 = (r.standard_normal(n) * 0.01).astype(np.float32)
    v0 = (r.random(n) * 1e-3).astype(np.float32)
    return pv, g, m0, v0


def _check_adam(tag, n, dev_pmv, ref_pmv, m0, g_scaled, m_roundings):
    (P_, M_, V_), (pr, mr, vr) = dev_pmv, ref_pmv
    pd, md, vd = (t[:n].cpu().numpy() for t in (P_, M_, V_))
    assert np.isfinite(pd).all() and np.isfinite(md).all() and np.isfinite(vd).all()
    figs = (max_err(pd, pr), rel_err(md, mr), rel_err(vd, vr))
    excess = float((np.abs(md.astype(np.float64) - mr) - R.adam_m_bound(m0, g_scaled, m_roundings)).max())
    report("step_tail.adam", tag + " max_err p", figs[0])
    report("step_tail.adam", tag + " rel_err m", figs[1])
    report("step_tail.adam", tag + " rel_err v", figs[2])
    assert figs[0] < 2e-6 and figs[1] < 1e-5 and figs[2] < 1e-5, (tag, figs)
    assert excess <= 0.0, (tag, "an element of m is outside its rounding bound by", excess)
    assert tail_ok(P_, n) and tail_ok(M_, n) and tail_ok(V_, n), tag


@pytest.mark.parametrize("n", R.sqnorm_sizes())
def test_adam_every_element_at_every_size(n):
    """Every element of p, m, v against O.adam_step in float64, iteration 7.  Below the clip (norm 0.5: the gradient enters unscaled)
    m is b1 * m0 + (1 - b1) * g: three fp32 roundings, |m - m_ref| <= 4 x 2^-24 (|b1 m0| + |(1 - b1) g|) per element.  Above the clip
    (norm 30) g is first multiplied by clipnorm / norm, itself computed in fp32 from the fp32 norm: (float) of the sum, sqrtf and the
    division put at most 2.5 x 2^-24 on the factor and the product one more, so 4 + 3.5 -> 8 x 2^-24 there."""
    r = np.random.default_rng(102)
    for norm, roundings in ((0.5, 4), (30.0, 8)):
        pv, g, m0, v0 = _adam_inputs(r, n, norm)
        gn = float(np.linalg.norm(g.astype(np.float64)))
        st = R.adam_state(6, m0, v0)
        ref = R.adam_oracle(st, pv, g)
        P_, G_, M_, V_ = (with_tail(a, n) for a in (pv, g, m0, v0))
        ws = sq_ws(n)
        L().call("vm_grad_sqnorm", p(G_), n, p(ws), None, stream())
        adam(P_, G_, M_, V_, n, 7, sq=nan(1), parts=ws)
        gs = g.astype(np.float64) * (1.0 / gn if gn >= 1.0 else 1.0)
        _check_adam("n=%d norm=%g" % (n, norm), n, (P_, M_, V_), ref, m0, gs, roundings)


def test_adam_clip_threshold_no_clip_and_zero_gradient():
    """cfg-A's size.  The same gradient scaled to norm 0.999 (unscaled: the 4 x 2^-24 bound) and 1.001 (clipped: 8 x 2^-24, see above);
    clipnorm = 0 with neither sqnorm nor partials against AdamState(clipnorm=None); g = 0 (norm 0): finite, p moves by the m term."""
    n = R.n_cfg_a()
    r = np.random.default_rng(103)
    pv, g1, m0, v0 = _adam_inputs(r, n, 1.0)
    for norm, roundings in ((0.999, 4), (1.001, 8)):
        g = (g1.astype(np.float64) * norm).astype(np.float32)
        gn = float(np.linalg.norm(g.astype(np.float64)))
        assert (gn >= 1.0) == (norm > 1.0)
        ref = R.adam_oracle(R.adam_state(6, m0, v0), pv, g)
        P_, G_, M_, V_ = (with_tail(a, n) for a in (pv, g, m0, v0))
        ws, sq = sq_ws(n), nan(1)
        L().call("vm_grad_sqnorm", p(G_), n, p(ws), None, stream())
        adam(P_, G_, M_, V_, n, 7, sq=sq, parts=ws)
        assert (np.sqrt(sq.item()) >= 1.0) == (norm > 1.0)      # the device takes the same side of the threshold
        _check_adam("cfgA norm=%g" % norm, n, (P_, M_, V_), ref, m0, g.astype(np.float64) / (gn if gn >= 1.0 else 1.0), roundings)
    # no clip at all: a large gradient goes through unscaled
    g = (g1.astype(np.float64) * 30.0).astype(np.float32)
    ref = R.adam_oracle(R.adam_state(6, m0, v0, clipnorm=None), pv, g)
    P_, G_, M_, V_ = (with_tail(a, n) for a in (pv, g, m0, v0))
    adam(P_, G_, M_, V_, n, 7, clipnorm=0.0)
    _check_adam("cfgA clipnorm=0", n, (P_, M_, V_), ref, m0, g, 4)
    # zero gradient
    z = np.zeros(n, np.float32)
    ref = R.adam_oracle(R.adam_state(6, m0, v0), pv, z)
    P_, G_, M_, V_ = (with_tail(a, n) for a in (pv, z, m0, v0))
    ws, sq = sq_ws(n), nan(1)
    L().call("vm_grad_sqnorm", p(G_), n, p(ws), None, stream())
    adam(P_, G_, M_, V_, n, 7, sq=sq, parts=ws)
    assert sq.item() == 0.0
    _check_adam("cfgA g=0", n, (P_, M_, V_), ref, m0, z, 4)
    assert np.array_equal(M_[:n].cpu().numpy(), np.float32(R.B1) * m0)


def test_adam_fresh_state_and_20_step_trajectory():
    """m = v = 0, t = 1, then 20 steps on one buffer with a new gradient per step and lr_t recomputed per step, against the oracle run
    for the same 20 steps.  The bound after 20 steps is measured, not derived: the same trajectory in float32 numpy on the CPU (the
    reference arithmetic) against the same oracle, times 4.
    Measured on an MI355X, device / float32 numpy: max_err p 1.32e-06 / 1.32e-06, rel_err m 8.91e-08 / 8.91e-08, rel_err v
    1.04e-07 / 1.04e-07 (the kernel's fp32 operations are numpy's, in the same order); allowed: 4 x the float32 numpy figure."""
    n = 8 * S + 100
    r = np.random.default_rng(104)
    pv = r.standard_normal(n).astype(np.float32)
    z = np.zeros(n, np.float32)
    P_, M_, V_ = with_tail(pv, n), with_tail(z, n), with_tail(z, n)
    st = R.adam_state(0)
    p64, (p32, m32, v32) = pv.astype(np.float64), (pv, z, z)
    ws = sq_ws(n)
    for t in range(1, 21):
        g = (r.standard_normal(n) * (3.0 / np.sqrt(n) if t % 3 else 0.5 / np.sqrt(n))).astype(np.float32)   # clipped and unclipped steps
        G_ = with_tail(g, n)
        L().call("vm_grad_sqnorm", p(G_), n, p(ws), None, stream())
        adam(P_, G_, M_, V_, n, t, sq=nan(1), parts=ws)
        p64, m64, v64 = R.adam_oracle(st, p64, g)
        p32, m32, v32 = R.adam_step_f32(p32, g, m32, v32, t)
        if t == 1:
            _check_adam("fresh state t=1", n, (P_, M_, V_), (p64, m64, v64), z, g.astype(np.float64) / max(1.0, float(np.linalg.norm(g.astype(np.float64)))), 8)
    pd, md, vd = (x[:n].cpu().numpy() for x in (P_, M_, V_))
    figs_dev = (max_err(pd, p64), rel_err(md, m64), rel_err(vd, v64))
    figs_cpu = (max_err(p32, p64), rel_err(m32, m64), rel_err(v32, v64))
    for nm, a, b in zip(("max_err p", "rel_err m", "rel_err v"), figs_dev, figs_cpu):
        report("step_tail.adam20", nm + " device", a)
        report("step_tail.adam20", nm + " float32 numpy", b)
        assert a <= 4 * b, (nm, a, b)
    assert tail_ok(P_, n) and tail_ok(M_, n) and tail_ok(V_, n)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("where", ["main-loop", "tail-loop"])
def test_adam_engine_form_skips_a_non_finite_step(bad, where):
    """engine.py optimizer_step's call (f16 storage): sqnorm_parts + skip_nonfinite + skipped.  n = 8S + 100: indices below 8S are read
    by sqnorm_partial_kernel's 8-wide loop, 8S + 50 only by its tail loop."""
    n = 8 * S + 100
    j = 3 * S + 77 if where == "main-loop" else 8 * S + 50
    r = np.random.default_rng(105)
    pv, g, m0, v0 = _adam_inputs(r, n, 30.0 * 4096.0)
    pre = 1.0 / 4096.0
    # finite gradient: equal to the plain form bit for bit, counter unchanged
    Pa, Ga, Ma, Va = (with_tail(a, n) for a in (pv, g, m0, v0))
    adam(Pa, Ga, Ma, Va, n, 7, prescale=pre, sq=grad_sqnorm(Ga, n))
    Pb, Mb, Vb = (with_tail(a, n) for a in (pv, m0, v0))
    ws, sq, cnt = sq_ws(n), nan(1), torch.full((1,), 7, dtype=torch.int32, device="cuda")
    L().call("vm_grad_sqnorm", p(Ga), n, p(ws), None, stream())
    adam(Pb, Ga, Mb, Vb, n, 7, prescale=pre, sq=sq, parts=ws, skip=1, skipped=cnt)
    assert torch.equal(Pa, Pb) and torch.equal(Ma, Mb) and torch.equal(Va, Vb) and cnt.item() == 7 and np.isfinite(sq.item())
    assert not torch.equal(Pb[:n], torch.as_tensor(pv).cuda())
    # one non-finite element: nothing moves, the counter does, the published norm is non-finite
    Ga[j] = bad
    before = (Pb.clone(), Mb.clone(), Vb.clone())
    sq.fill_(0.0)
    L().call("vm_grad_sqnorm", p(Ga), n, p(ws), None, stream())
    adam(Pb, Ga, Mb, Vb, n, 7, prescale=pre, sq=sq, parts=ws, skip=1, skipped=cnt)
    assert same_bits(Pb, before[0]) and same_bits(Mb, before[1]) and same_bits(Vb, before[2])
    assert cnt.item() == 8 and not np.isfinite(sq.item())
    # without the switch it goes through, as in Keras
    adam(Pb, Ga, Mb, Vb, n, 7, prescale=pre, sq=sq, parts=ws, skip=0, skipped=None)
    assert not torch.isfinite(Pb[:n]).all() and cnt.item() == 8 and tail_ok(Pb, n)


# ==========================================================================================================
# 3. vm_dense_fwd / vm_dense_bwd
# ==========================================================================================================
def _dense_case(rows, ni, no, seed):
    r = np.random.default_rng(seed)
    return tuple(r.standard_normal(s).astype(np.float32) for s in [(rows, ni), (ni, no), (no,), (rows, no)])


def _within(tag, got, ref, bound):
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), tag + ": an output element was not written"
    ex = float((np.abs(got - ref) - bound).max())
    report("step_tail.dense", tag + " frobenius", rel_err(got, ref))
    assert ex <= 0.0, (tag, "outside the dot-product bound by", ex, "at", np.unravel_index(np.argmax(np.abs(got - ref) - bound), ref.shape))


def _dense_all_forms(rows, ni, no, seed):
    x, w, b, dout = _dense_case(rows, ni, no, seed)
    x64, w64, b64, d64 = (a.astype(np.float64) for a in (x, w, b, dout))
    ax, aw, ad = np.abs(x64), np.abs(w64), np.abs(d64)
    X, W, B, D = dev(x), dev(w), dev(b), dev(dout)
    tag = "(%d,%d,%d)" % (rows, ni, no)
    out = nan(rows * no + TAIL)
    out[rows * no:] = SENT
    L().call("vm_dense_fwd", p(X), p(W), p(B), rows, ni, no, p(out), stream())
    _within(tag + " fwd", out[:rows * no].view(rows, no), x64 @ w64 + b64, R.dot_bound(ni, ax @ aw + np.abs(b64)))
    out0 = nan(rows * no + TAIL)
    out0[rows * no:] = SENT
    L().call("vm_dense_fwd", p(X), p(W), None, rows, ni, no, p(out0), stream())
    _within(tag + " fwd b=NULL", out0[:rows * no].view(rows, no), x64 @ w64, R.dot_bound(ni, ax @ aw))
    assert tail_ok(out, rows * no) and tail_ok(out0, rows * no)
    gw, gb, din = nan(ni * no + TAIL), nan(no + TAIL), nan(rows * ni + TAIL)
    gw[ni * no:], gb[no:], din[rows * ni:] = SENT, SENT, SENT
    L().call("vm_dense_bwd", p(X), p(W), p(D), rows, ni, no, p(gw), p(gb), p(din), stream())
    refs = (x64.T @ d64, d64.sum(0), d64 @ w64.T)
    bounds = (R.dot_bound(rows, ax.T @ ad), R.dot_bound(rows, ad.sum(0)), R.dot_bound(no, ad @ aw.T))
    _within(tag + " grad_w", gw[:ni * no].view(ni, no), refs[0], bounds[0])
    _within(tag + " grad_b", gb[:no], refs[1], bounds[1])
    _within(tag + " din", din[:rows * ni].view(rows, ni), refs[2], bounds[2])
    assert tail_ok(gw, ni * no) and tail_ok(gb, no) and tail_ok(din, rows * ni)
    # the two partial forms give the same bits and leave the absent outputs' neighbours alone
    din2 = nan(rows * ni + TAIL)
    din2[rows * ni:] = SENT
    L().call("vm_dense_bwd", p(X), p(W), p(D), rows, ni, no, None, None, p(din2), stream())
    gw2, gb2 = nan(ni * no + TAIL), nan(no + TAIL)
    gw2[ni * no:], gb2[no:] = SENT, SENT
    L().call("vm_dense_bwd", p(X), p(W), p(D), rows, ni, no, p(gw2), p(gb2), None, stream())
    assert torch.equal(din, din2) and torch.equal(gw, gw2) and torch.equal(gb, gb2)
    return out[:rows * no].view(rows, no), gw[:ni * no].view(ni, no), gb[:no], din[:rows * ni].view(rows, ni), refs, (x64 @ w64 + b64)


@pytest.mark.parametrize("rows,ni,no", R.DENSE_TRIPLES)
def test_dense_loop_structure(rows, ni, no):
    """Per element |out - ref| <= (K + 2) 2^-24 (|x| @ |w| + |b|), K the reduction length: the worst case of an fp32 dot product in any
    order.  With N(0, 1) operands a dropped or doubled term is ~ 1 against a bound of ~ K^1.5 x 6e-8."""
    out, gw, gb, din, refs, fref = _dense_all_forms(rows, ni, no, 106)
    if (rows, ni, no) == (10, 72, 33):      # the shape tests/test_gpu_kernels.py has always run: its Frobenius bound too
        assert rel_err(out.cpu().numpy(), fref) < 1e-6 and rel_err(gw.cpu().numpy(), refs[0]) < 1e-6
        assert rel_err(gb.cpu().numpy(), refs[1]) < 1e-6 and rel_err(din.cpu().numpy(), refs[2]) < 1e-6


@pytest.mark.parametrize("rows", [70000, 65536])
def test_dense_row_chunk_loop(rows):
    """grid.y holds 65 535 rows: the forward and the input gradient go in chunks; every row past the first chunk is written."""
    _dense_all_forms(rows, 16, 8, 107)


# ==========================================================================================================
# 4. siamese head and losses
# ==========================================================================================================
HW_UE, HB = 1.5, -21.0        # a = hw d + hb with d >= 0: every a >= -21 can be placed


def _band_values(r, pairs):
    """pre-activations cycling through: regular |a| <= 6, saturated high a in [20, 30], saturated low a in [-21, -20]; nothing with
    8 < |a| < 20 (there one ulp of p moves the logit by 2^-24 / (1 - p): a test of expf).  Labels alternate inside each band."""
    band = np.arange(pairs) % 3
    a = np.where(band == 0, r.uniform(-6, 6, pairs), np.where(band == 1, r.uniform(20, 30, pairs), r.uniform(-21, -20, pairs)))
    y = ((np.arange(pairs) // 3) % 2).astype(np.float32)
    return a, y, band


def _head_inputs(seed, pairs, e, head, a):
    r = np.random.default_rng(seed)
    hw = np.array([[HW_UE]], np.float32) if head == "uniform_euclidean" else r.uniform(0.2, 1.0, (e, 1)).astype(np.float32)
    hb = np.array([HB], np.float32)
    emb = R.pairs_with_chosen_a(r, a, e, head, hw, hb).astype(np.float32)
    return emb, hw, hb


def _head_launch(emb, hw, hb, y, pairs, e, head, loss, gs, split):
    from voicemap_amd.engine import HEADS, LOSSES
    E_, HW_, HB_, Y_ = dev(emb), dev(hw), dev(hb), dev(y)
    pred, la, demb, ghw, ghb, ws = nan(pairs), nan(2), nan(2 * pairs, e), nan(hw.size), nan(1), nan(4 * pairs)
    if split:
        L().call("vm_siamese_head_loss", p(E_), p(HW_), p(HB_), p(Y_), pairs, e, HEADS[head], LOSSES[loss], gs, p(pred), None, p(demb),
                 None, None, p(ws), stream())
        assert torch.isnan(la).all() and torch.isnan(ghw).all() and torch.isnan(ghb).all()
        L().call("vm_siamese_head_reduce", p(E_), p(ws), pairs, e, HEADS[head], p(la), p(ghw), p(ghb), stream())
    else:
        L().call("vm_siamese_head_loss", p(E_), p(HW_), p(HB_), p(Y_), pairs, e, HEADS[head], LOSSES[loss], gs, p(pred), p(la), p(demb),
                 p(ghw), p(ghb), p(ws), stream())
    return pred, la, demb, ghw, ghb, ws


def _check_head(tag, outs, emb, hw, hb, y, band, pairs, e, head, loss, gs):
    pred, la, demb, ghw, ghb, ws = (t.cpu().numpy().astype(np.float64) for t in outs)
    ws = ws.reshape(pairs, 4)
    ref = R.head_oracle(emb, hw, hb, y, head, loss)
    reg, hi, lo = band == 0, band == 1, band == 2
    sat = hi | lo
    # -- pred and accuracy
    assert np.isfinite(pred).all() and np.isfinite(ws).all()
    assert (pred[hi] == 1.0).all() and (np.abs(pred[lo] - ref["pred"][lo]) <= 1e-5 * ref["pred"][lo]).all(), tag
    assert rel_err(pred[reg], ref["pred"][reg]) < 1e-5, tag
    hit = (np.rint(ref["pred"]) == y).astype(np.float64)
    assert np.array_equal(ws[:, 1], hit) and abs(la[1] - ref["acc"]) < 1e-6, tag
    # -- per-pair loss: float64 oracle; BCE at the clip: the float32 oracle (logit 15.9424 high, -16.1181 low)
    want = ref["loss_pair"].copy()
    if loss == "bce":
        want[sat] = R.bce_pair_f32(ref["pred"][sat], y[sat])
        assert (np.abs(ws[sat, 0] - want[sat]) <= 1e-5 * np.abs(want[sat])).all(), (tag, ws[sat, 0][:6], want[sat][:6])
    else:
        assert (np.abs(ws[sat, 0] - want[sat]) <= 2e-5 * np.maximum(1.0, np.abs(want[sat]))).all(), tag
    assert (np.abs(ws[reg, 0] - want[reg]) <= 2e-5 * np.maximum(1.0, np.abs(want[reg]))).all(), tag
    assert abs(la[0] - want.mean()) < 2e-5 * max(1.0, abs(want.mean())), (tag, la[0], want.mean())
    # -- dL/da per pair.  p carries an absolute error of 2^-24 near 1, which (1 - p) inherits: 4 x 2^-24 / pairs on top of 1e-4 relative
    dlda = ws[:, 2] / gs
    d64 = np.linalg.norm(emb[:pairs].astype(np.float64) - emb[pairs:].astype(np.float64), axis=1) if head == "uniform_euclidean" else np.zeros(pairs)
    tol = 1e-4 * np.abs(ref["dlda"]) + 4 * R.U32 / pairs
    de, dr = demb / gs, ref["demb"]
    if loss == "bce":
        assert (ws[sat, 2] == 0.0).all() and (ws[sat, 3] == 0.0).all(), tag
        assert (demb[:pairs][sat] == 0.0).all() and (demb[pairs:][sat] == 0.0).all(), tag
        assert (np.abs(dlda[reg] - ref["dlda"][reg]) <= tol[reg]).all(), tag
        dr = dr.copy()
        dr[:pairs][sat], dr[pairs:][sat] = 0.0, 0.0     # clip_by_value passes no gradient outside [eps, 1 - eps]
    else:
        assert (np.abs(dlda - ref["dlda"]) <= tol).all(), (tag, np.abs(dlda - ref["dlda"]).max())
    assert (np.abs(ws[:, 3] / gs - dlda * d64) <= 1e-5 * np.abs(dlda * d64) + 1e-30).all(), tag
    # -- gradients, the tolerances tests/test_gpu_kernels.py has always used
    assert rel_err(de, dr) < 1e-4, (tag, rel_err(de, dr))
    rows = np.concatenate([reg, reg])
    assert (np.linalg.norm(de[rows] - dr[rows], axis=1) <= 1e-4 * np.linalg.norm(dr[rows], axis=1) + 1e-12).all(), tag
    assert rel_err(ghw / gs, ref["ghw"]) < 1e-4 and rel_err(ghb / gs, ref["ghb"]) < 1e-4, tag


HEAD_SHAPES = [(1, 64), (3, 1), (4, 8), (5, 63), (255, 65), (256, 128), (257, 256), (1000, 64), (6, 256), (257, 1), (1000, 8), (5, 128)]


@pytest.mark.parametrize("head", ["uniform_euclidean", "weighted_l1"])
@pytest.mark.parametrize("loss", ["contrastive", "bce"])
@pytest.mark.parametrize("pairs,e", HEAD_SHAPES)
def test_siamese_head_bands(head, loss, pairs, e):
    """Chosen pre-activations in the regular band and at both clips, both labels in each, per pair from ws.  pred: exactly 1 in the
    high band (1 + expf(-20) rounds to 1), exactly rounding to 0 in the low band and within 1e-5 of float64 there (p ~ 1e-9 is an
    ordinary fp32 number); accuracy exact.  The one-call form and head_loss(loss_acc = NULL) + head_reduce give the same bits."""
    r = np.random.default_rng(108)
    a, y, band = _band_values(r, pairs)
    emb, hw, hb = _head_inputs(108, pairs, e, head, a)
    gs = 4096.0 if pairs % 2 else 1.0
    one = _head_launch(emb, hw, hb, y, pairs, e, head, loss, gs, split=False)
    two = _head_launch(emb, hw, hb, y, pairs, e, head, loss, gs, split=True)
    for x, z, nm in zip(one, two, ("pred", "loss_acc", "demb", "grad_hw", "grad_hb", "ws")):
        assert same_bits(x, z), nm
    _check_head("%s %s %dx%d" % (head, loss, pairs, e), one, emb, hw, hb, y, band, pairs, e, head, loss, gs)


@pytest.mark.parametrize("loss", ["contrastive", "bce"])
@pytest.mark.parametrize("pairs,e", [(5, 64), (257, 8)])
def test_siamese_head_identical_twins(loss, pairs, e):
    """d == 0.  uniform_euclidean: the oracle's demb row is non-finite (sqrt'(0)), so is the kernel's; the other pairs' rows are what
    they are without that pair; an optimizer step with skip_nonfinite on a gradient buffer holding the row is skipped.  weighted_l1:
    sign(0) = 0, the row is exactly 0."""
    from voicemap_amd.engine import HEADS, LOSSES
    r = np.random.default_rng(109)
    twin = pairs // 2
    emb = r.normal(0, 0.4, (2 * pairs, e)).astype(np.float32)
    emb[pairs + twin] = emb[twin]
    y = (np.arange(pairs) % 2).astype(np.float32)
    others = np.arange(pairs) != twin
    rows = np.concatenate([others, others])
    for head in ("uniform_euclidean", "weighted_l1"):
        hw = np.array([[0.5]], np.float32) if head == "uniform_euclidean" else r.uniform(0.1, 0.5, (e, 1)).astype(np.float32)
        hb = np.array([-0.5], np.float32)
        outs = _head_launch(emb, hw, hb, y, pairs, e, head, loss, 1.0, split=False)
        pred, la, demb, ghw, ghb, ws = (t.cpu().numpy().astype(np.float64) for t in outs)
        ref = R.head_oracle(emb, hw, hb, y, head, loss)
        assert rel_err(pred, ref["pred"]) < 1e-5 and abs(la[0] - ref["loss"]) < 2e-5 * max(1.0, abs(ref["loss"]))
        assert rel_err(demb[rows], ref["demb"][rows]) < 1e-4
        if head == "uniform_euclidean":
            assert not np.isfinite(ref["demb"][twin]).any() and not np.isfinite(ref["demb"][pairs + twin]).any()
            assert not np.isfinite(demb[twin]).any() and not np.isfinite(demb[pairs + twin]).any()
            assert np.isfinite(demb[rows]).all()
            n = demb.size
            G = outs[2].reshape(-1)
            pv = r.standard_normal(n).astype(np.float32)
            P_, M_, V_ = with_tail(pv, n), with_tail(np.zeros(n), n), with_tail(np.zeros(n), n)
            before = P_.clone()
            ws_sq, sq, cnt = sq_ws(n), nan(1), torch.zeros(1, dtype=torch.int32, device="cuda")
            L().call("vm_grad_sqnorm", p(G), n, p(ws_sq), None, stream())
            adam(P_, G, M_, V_, n, 1, sq=sq, parts=ws_sq, skip=1, skipped=cnt)
            assert cnt.item() == 1 and not np.isfinite(sq.item()) and same_bits(P_, before) and not M_[:n].any() and not V_[:n].any()
        else:
            assert (demb[twin] == 0.0).all() and (demb[pairs + twin] == 0.0).all() and np.isfinite(demb).all()
            assert rel_err(ghw, ref["ghw"]) < 1e-4 and rel_err(ghb, ref["ghb"]) < 1e-4


@pytest.mark.parametrize("head", ["uniform_euclidean", "weighted_l1"])
@pytest.mark.parametrize("loss", ["contrastive", "bce"])
def test_tail_fused_equals_unfused_at_the_clips_and_for_identical_twins(head, loss):
    """The same bands and a d == 0 pair through vm_tail_fwd_bwd + vm_tail_param_grads: bit for bit the unfused launches (vm_dense_fwd,
    vm_siamese_head_loss, vm_dense_bwd).  The dense layer is the identity (C = E), so the embeddings ARE the chosen ones (x * 1 + 0 is
    exact); the unfused path is checked against the oracle by test_siamese_head_bands."""
    from voicemap_amd.engine import HEADS, LOSSES
    pairs, c = 13, 64
    e = c
    r = np.random.default_rng(110)
    a, y, band = _band_values(r, pairs)
    gmax_h, hw, hb = _head_inputs(110, pairs, e, head, a)
    gmax_h[pairs + 12] = gmax_h[12]                      # the last pair: identical twins
    n = 2 * pairs
    D_W, D_B, HW_, HB_, Y_ = dev(np.eye(c, e, dtype=np.float32)), dev(np.zeros(e, np.float32)), dev(hw), dev(hb), dev(y)
    gmax, gidx = dev(gmax_h), torch.zeros(n, c, dtype=torch.int32, device="cuda")
    gs = 4096.0
    emb, pred, demb, dgmax, ws = nan(n, e), nan(pairs), nan(n, e), nan(n, c), nan(4 * pairs)
    L().call("vm_tail_fwd_bwd", None, None, 0, p(gmax), p(gidx), p(D_W), p(D_B), p(HW_), p(HB_), p(Y_), pairs, c, e, HEADS[head],
             LOSSES[loss], gs, p(emb), p(pred), p(demb), p(dgmax), p(ws), stream())
    la, g_dw, g_db, g_hw, g_hb = nan(2), nan(c, e), nan(e), nan(hw.size), nan(1)
    L().call("vm_tail_param_grads", p(gmax), p(demb), p(emb), p(ws), pairs, c, e, HEADS[head], p(la), p(g_dw), p(g_db), p(g_hw), p(g_hb), stream())
    emb2, pred2, demb2, dgmax2, ws2 = nan(n, e), nan(pairs), nan(n, e), nan(n, c), nan(4 * pairs)
    la2, g_dw2, g_db2, g_hw2, g_hb2 = nan(2), nan(c, e), nan(e), nan(hw.size), nan(1)
    L().call("vm_dense_fwd", p(gmax), p(D_W), p(D_B), n, c, e, p(emb2), stream())
    L().call("vm_siamese_head_loss", p(emb2), p(HW_), p(HB_), p(Y_), pairs, e, HEADS[head], LOSSES[loss], gs, p(pred2), p(la2), p(demb2),
             p(g_hw2), p(g_hb2), p(ws2), stream())
    L().call("vm_dense_bwd", p(gmax), p(D_W), p(demb2), n, c, e, p(g_dw2), p(g_db2), p(dgmax2), stream())
    assert torch.equal(emb, gmax)
    for x, z, nm in ((emb, emb2, "emb"), (pred, pred2, "pred"), (demb, demb2, "demb"), (dgmax, dgmax2, "dgmax"), (la, la2, "loss_acc"), (ws, ws2, "ws"),
                     (g_dw, g_dw2, "grad dense w"), (g_db, g_db2, "grad dense b"), (g_hw, g_hw2, "grad head w"), (g_hb, g_hb2, "grad head b")):
        assert same_bits(x, z), nm
    # and the fused outputs are the banded ones: saturated BCE rows exactly zero, the twin row non-finite (euclidean) or zero (l1)
    dm = demb.cpu().numpy()
    sat = np.flatnonzero((band != 0) & (np.arange(pairs) != 12))
    if loss == "bce":
        assert (dm[sat] == 0.0).all() and (dm[pairs + sat] == 0.0).all() and (dgmax.cpu().numpy()[sat] == 0.0).all()
    assert band[12] == 0 and (pred.cpu().numpy()[band == 1] == 1.0).all()
    if head == "uniform_euclidean":
        assert not np.isfinite(dm[12]).any() and np.isfinite(dm[:12]).all()
    else:
        assert (dm[12] == 0.0).all() and np.isfinite(dm).all()


def _softmax(logits, labels, gs=1.0, with_grad=True):
    rows, nc = logits.shape
    prob, dl = nan(rows * nc + TAIL), nan(rows * nc + TAIL)
    prob[rows * nc:], dl[rows * nc:] = SENT, SENT
    la, ws = nan(2), nan(2 * rows)
    L().call("vm_softmax_cce", p(dev(logits)), p(dev(labels, torch.int32)), rows, nc, gs, p(prob), p(la), p(dl) if with_grad else None, p(ws), stream())
    assert tail_ok(prob, rows * nc) and tail_ok(dl, rows * nc)
    return (prob[:rows * nc].view(rows, nc).cpu().numpy().astype(np.float64), la.cpu().numpy().astype(np.float64),
            dl[:rows * nc].view(rows, nc).cpu().numpy().astype(np.float64), ws.cpu().numpy().astype(np.float64).reshape(2, rows))


def _cce_oracle(logits, labels, dtype=torch.float64):
    lt = torch.tensor(logits, dtype=dtype, requires_grad=True)
    pr = torch.softmax(lt, -1)
    oh = torch.nn.functional.one_hot(torch.tensor(labels, dtype=torch.int64), logits.shape[1]).to(dtype)
    per = np.array([float(O.categorical_crossentropy(oh[i:i + 1], pr[i:i + 1]).detach()) for i in range(len(labels))])
    (g,) = torch.autograd.grad(O.categorical_crossentropy(oh, pr), [lt])
    return pr.detach().numpy().astype(np.float64), per, g.numpy().astype(np.float64), float(O.categorical_accuracy(oh, pr))


SOFTMAX_CLASSES = [1, 2, 255, 256, 257, 251, 1172]


@pytest.mark.parametrize("rows", [1, 255, 257])
@pytest.mark.parametrize("nc", SOFTMAX_CLASSES)
def test_softmax_cce_sizes(nc, rows):
    """Logits in [-4, 4]: every probability is inside [1e-7, 1 - 1e-7] when there are two classes or more (>= e^-8 / 1172), so the
    float64 oracle applies; one class: the probability is 1, past the clip: the float32 oracle's loss, a zero gradient."""
    r = np.random.default_rng(111)
    logits = np.clip(r.normal(0, 2, (rows, nc)), -4, 4).astype(np.float32)
    labels = r.integers(0, nc, rows).astype(np.int32)
    prob, la, dl, ws = _softmax(logits, labels, gs=4096.0)
    pr, per, g, acc = _cce_oracle(logits, labels)
    assert rel_err(prob, pr) < 1e-5 and (np.abs(prob.sum(1) - 1.0) <= nc * R.U32).all()
    if nc == 1:
        per = _cce_oracle(logits, labels, torch.float32)[1]
        assert (dl == 0.0).all() and (np.abs(ws[0] - per) <= 1e-5 * per).all()
    else:
        assert rel_err(dl / 4096.0, g) < 1e-4
        assert (np.linalg.norm(dl / 4096.0 - g, axis=1) <= 1e-4 * np.linalg.norm(g, axis=1)).all()
    assert (np.abs(ws[0] - per) <= 1e-5 * np.maximum(1.0, np.abs(per))).all()
    assert np.array_equal(ws[1], (logits.argmax(1) == labels).astype(np.float64))
    assert abs(la[0] - per.mean()) < 1e-5 * max(1.0, abs(per.mean())) and abs(la[1] - acc) < 1e-6


@pytest.mark.parametrize("nc", SOFTMAX_CLASSES)
def test_softmax_cce_clips_and_large_logits(nc):
    """Row 0: the label's probability below 1e-7 (loss -log(1e-7), the whole gradient row exactly 0; needs two classes).  Row 1: above
    1 - 1e-7 (the float32 oracle: -log(1 - 2^-23); row exactly 0).  Rows 2, 3: logits of +-80 and of 1e4 (no overflow, the row sums to
    1).  Row 4: regular, so the mean mixes clipped and unclipped rows."""
    r = np.random.default_rng(112)
    rows = 5
    logits = np.clip(r.normal(0, 1, (rows, nc)), -3, 3).astype(np.float32)
    labels = r.integers(0, nc, rows).astype(np.int32)
    if nc >= 2:
        logits[0, labels[0]] = -40.0
    logits[1, labels[1]] = 40.0
    logits[2] = np.where(r.random(nc) < 0.5, 80.0, -80.0)
    logits[2, labels[2]] = 80.0
    logits[3] = 0.0
    logits[3, labels[3]] = 1e4
    logits[3, (labels[3] + nc // 2) % nc] = 1e4
    prob, la, dl, ws = _softmax(logits, labels)
    pr, per, g, acc = _cce_oracle(logits, labels)
    per32 = _cce_oracle(logits, labels, torch.float32)[1]
    assert np.isfinite(prob).all() and np.isfinite(dl).all() and np.isfinite(ws).all()
    assert rel_err(prob, pr) < 1e-5 and (np.abs(prob.sum(1) - 1.0) <= nc * R.U32).all()
    clipped = [0, 1] if nc >= 2 else [0, 1, 2, 3, 4]      # one class: every row has probability 1
    for i in clipped:
        assert (dl[i] == 0.0).all(), i
        assert abs(ws[0, i] - per32[i]) <= 1e-5 * abs(per32[i]), (i, ws[0, i], per32[i])
    if nc == 1:
        assert abs(la[0] - per32.mean()) <= 1e-5 * per32.mean()
    if nc >= 2:
        assert abs(ws[0, 0] + np.log(1e-7)) < 1e-5 * 16.2
        want = per.copy()
        want[clipped] = per32[clipped]
        for i in (2, 3, 4):
            assert abs(ws[0, i] - per[i]) <= 1e-5 * max(1.0, abs(per[i])), i
            assert np.linalg.norm(dl[i] - g[i]) <= 1e-4 * np.linalg.norm(g[i]), i
        assert abs(la[0] - want.mean()) < 1e-5 * max(1.0, want.mean())
    assert np.array_equal(ws[1], (logits.argmax(1) == labels).astype(np.float64))


@pytest.mark.parametrize("ties", [(70, 300), (300, 70), (600, 90, 900), (5, 261), (1171, 0), (64, 63), (255, 256, 257)])
def test_softmax_cce_first_maximum_wins(ties):
    """Equal maxima in different 64-lane waves and different 256-strides of the class loop: the hit goes to the first index, as argmax
    in the oracle.  Each tied index is the label of one row."""
    nc = 1172
    r = np.random.default_rng(113)
    rows = len(ties)
    logits = np.clip(r.normal(0, 1, (rows, nc)), -3, 3).astype(np.float32)
    logits[:, list(ties)] = 5.0
    labels = np.array(ties, np.int32)
    prob, la, dl, ws = _softmax(logits, labels)
    pr, per, g, acc = _cce_oracle(logits, labels)
    want = (labels == min(ties)).astype(np.float64)
    assert np.array_equal(logits.argmax(1), np.full(rows, min(ties)))
    assert np.array_equal(ws[1], want) and abs(la[1] - want.mean()) < 1e-6 and abs(acc - want.mean()) < 1e-12
    assert rel_err(prob, pr) < 1e-5 and rel_err(dl, g) < 1e-4


@pytest.mark.parametrize("nc", SOFTMAX_CLASSES)
def test_softmax_probabilities_only(nc):
    """labels = NULL: the probabilities, and nothing else is written."""
    r = np.random.default_rng(114)
    rows = 3
    logits = np.clip(r.normal(0, 2, (rows, nc)), -4, 4).astype(np.float32)
    prob = nan(rows * nc + TAIL)
    prob[rows * nc:] = SENT
    la, ws, dl = torch.full((2,), SENT, device="cuda"), torch.full((2 * rows,), SENT, device="cuda"), torch.full((rows * nc,), SENT, device="cuda")
    L().call("vm_softmax_cce", p(dev(logits)), None, rows, nc, 1.0, p(prob), p(la), p(dl), p(ws), stream())
    assert (la == SENT).all() and (ws == SENT).all() and (dl == SENT).all() and tail_ok(prob, rows * nc)
    pr = torch.softmax(torch.tensor(logits, dtype=torch.float64), -1).numpy()
    assert rel_err(prob[:rows * nc].view(rows, nc).cpu().numpy(), pr) < 1e-5
    prob2 = nan(rows, nc)
    L().call("vm_softmax_cce", p(dev(logits)), None, rows, nc, 1.0, p(prob2), None, None, None, stream())
    assert torch.equal(prob2.reshape(-1), prob[:rows * nc])


# ==========================================================================================================
# 5. reductions
# ==========================================================================================================
# slab_sum's regime per case, from its rule (tests/tail_refs.py slab_regime restates it; the CPU file pins this table):
#   F = 8: 256 elements, 1 workgroup -> rch = min(2048, slabs / 4, 16).  slabs 1, 3, 4, 7 (slabs / 4 <= 1): single launch, its 4-wide loop
#   from 4 slabs.  8, 9: two partial rows of 4 / 5 slabs.  31: 7 rows of 5 (the last has 1).  32: 8 rows of 4.  33: 8 rows of 5, row 7 empty.  64: 16 rows
#   of 4.  65: 16 rows of 5, rows 13..15 empty.  67: 16 rows of 5, rows 14, 15 empty.  130: 16 rows of 9 (8-wide loop + 1), row 15
#   empty.  1000: 16 rows of 63 (7 x 8 + 7), the last 55.
#   F = 2048: 65 536 elements, 256 workgroups -> single launch up to 64 slabs (1, 4, 5, 7, 64); 65: rch = min(8, 16, 16) = 8 rows of 9.
@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("f,n", [(8, s) for s in R.CONV1_WGRAD_SLABS_F8] + [(2048, s) for s in R.CONV1_WGRAD_SLABS_F2048])
def test_conv1_wgrad_slab_sum_regimes(dt, f, n):
    """vm_conv1_wgrad with one slab per window.  Each slab element is an fp32 dot product of length L (bound as for Dense, K = L), the
    slab sum is float64 rounded once: (L + 3) 2^-24 sum |x||du| per element."""
    vm, tdt = DTYPES[dt]
    r = np.random.default_rng(115)
    l = 40
    x = r.standard_normal((n, l)).astype(np.float32)
    du = quant(r.standard_normal((n, l, f), dtype=np.float32), dt)
    xp = np.zeros((n, l + 31), np.float32)
    xp[:, 15:15 + l] = x
    ws = nan(L().query("vm_conv1_wgrad_workspace_bytes", n, f) // 4 + 16)
    nel = 32 * f
    gw = nan(nel + TAIL)
    gw[nel:] = SENT
    L().call("vm_conv1_wgrad", p(dev(xp)), p(padded(du, tdt)), n, l, f, vm, p(ws), p(gw), stream())
    xt, adu = torch.tensor(xp, dtype=torch.float64), du.abs()
    ref = torch.stack([torch.einsum("nl,nlf->f", xt[:, k:k + l], du) for k in range(32)]).numpy()
    mag = torch.stack([torch.einsum("nl,nlf->f", xt[:, k:k + l].abs(), adu) for k in range(32)]).numpy()
    got = gw[:nel].view(32, f).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and tail_ok(gw, nel)
    ex = float((np.abs(got - ref) - (l + 3) * R.U32 * mag).max())
    report("step_tail.slab_sum", "%s F=%d slabs=%d frobenius" % (dt, f, n), rel_err(got, ref))
    assert ex <= 0.0, (R.slab_regime(n, nel), "outside the bound by", ex)


FUSE_DEFAULT = 17     # the library's default vm_set_tuning("fuse_finalize") mask (tests/test_gpu_replay.py pins it): bit 2, the column sums' own
                      # fused finalize, is OFF by default


@pytest.mark.parametrize("c", R.COLSUM_C)
@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_cancelling_columns(rows, c):
    """vm_colsum and vm_colsum_strided (row_step 4: the rows between are NaN here -- the kernel may not read them) on columns whose sum
    cancels (N(0, 1) plus a +-1e4 pair): float64 on the device, one rounding: 2^-24 |ref| + rows 2^-53 sum |x|.  vm_set_tuning exposes the
    finalize switch (fuse_finalize bit 2): the default two-launch form and the fused one, the same bits."""
    r = np.random.default_rng(116)
    x = R.cancelling_columns(r, rows, c)
    x64 = x.astype(np.float64)
    ref, bound = x64.sum(0), R.colsum_bound(np.abs(x64).sum(0), x64.sum(0), rows)
    if rows >= 4096:    # what fp32 accumulation would give is outside the bound: the bound can tell float64 from fp32 (host arithmetic only)
        assert (np.abs(np.cumsum(x, axis=0, dtype=np.float32)[-1].astype(np.float64) - ref) > bound).any()
    X1 = dev(x)
    X4 = torch.full((rows, 4, c), float("nan"), device="cuda")
    X4[:, 0, :] = X1
    ws = torch.full((L().query("vm_colreduce_workspace_bytes", 1, c) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    outs = []
    try:
        for fuse in (FUSE_DEFAULT, FUSE_DEFAULT | 4):
            L().call("vm_set_tuning", b"fuse_finalize", fuse)
            for step in (1, 4):
                out = nan(c + TAIL)
                out[c:] = SENT
                if step == 1:
                    L().call("vm_colsum", p(X1), rows, c, p(out), p(ws), stream())
                    out_s = nan(c + TAIL)
                    out_s[c:] = SENT
                    L().call("vm_colsum_strided", p(X1), rows, 1, c, p(out_s), p(ws), stream())
                    assert torch.equal(out, out_s)
                else:
                    L().call("vm_colsum_strided", p(X4), rows, 4, c, p(out), p(ws), stream())
                got = out[:c].cpu().numpy().astype(np.float64)
                assert np.isfinite(got).all() and tail_ok(out, c), (fuse, step)
                ex = float((np.abs(got - ref) - bound).max())
                assert ex <= 0.0, (fuse, step, "outside the bound by", ex)
                outs.append(out)
    finally:
        L().call("vm_set_tuning", b"fuse_finalize", FUSE_DEFAULT)
    assert all(torch.equal(outs[0], o) for o in outs[1:])
