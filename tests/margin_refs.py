"""Reference helpers of the margin-softmax tests (tests/test_gpu_margin_loss.py and tests/test_gpu_margin_step.py on the device,
tests/test_margin_refs_cpu.py on the host): the float64 statement of the loss with its closed-form gradients (numpy), the same loss
in torch for autograd, an fp32 numpy restatement in two summation orders, the test inputs and error bounds derived by counting
roundings.  Pure numpy / torch: nothing here touches the HIP library or a GPU.

The loss (include/voicemap_hip.h, vm_margin_softmax).  emb (N, E), w (E, S), labels (N); a label outside [0, S) takes its row out.
    c_ic = e_i . w_c / (|e_i| |w_c|) clamped to [-1, 1] (the clamp passes the gradient), 0 for a zero row or column;
    NONE c' = c_iy;  COSINE c' = c_iy - margin;  ANGULAR (cos_m, sin_m, th = -cos_m, mm = margin sin_m rounded to fp32 from double):
    c_iy > th: c' = c cos_m - sin_t sin_m, f = cos_m + sin_m c / max(sin_t, 2^-6), else c' = c - mm, f = 1;
    z = scale c with scale c' at the label;  loss = mean_i (logsumexp z_i - z_iy), acc = mean_i [first argmax_c c_ic == y_i];
    g = (scale / N) (softmax(z) - onehot) (* f at the label);  demb_i = (sum_c g_ic w_hat_c - (sum_c g_ic c_ic) e_hat_i) / |e_i|;
    grad_w[:, c] = (sum_i g_ic e_hat_i - (sum_i g_ic c_ic) w_hat_c) / |w_c|.

The argmax and the angular branch are discontinuous, so a result is compared in two stages (``check``): its ``pred`` must be
ADMISSIBLE (the float64 cosine at pred within the bound of the row maximum, and the reference's choice wherever the gap to the
runner-up exceeds the bound); the hits are then counted WITH the kernel's pred.  A row whose float64 c_iy is within the bound of th
is ambiguous at the branch.  The inputs of the GPU tests have no ambiguous row at all (small shapes) or at most 1 % rows with an
ambiguous pred and none at the branch (limit shapes) -- ``CAPS``; tests/test_margin_refs_cpu.py asserts it for every GPU input.
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
TINY = 2.0 ** -125
NONE, COSINE, ANGULAR = 0, 1, 2     # VM_MARGIN_*
SIN_FLOOR = 2.0 ** -6               # VM_MARGIN_SIN_FLOOR
# (kind, margin): the cases every shape is run under
KINDS = [(NONE, 0.0), (COSINE, 0.35), (ANGULAR, 0.2), (ANGULAR, 0.5)]
SCALES = [30.0, 1.0]

# (N, S, E, seed): standard-normal fp32 embeddings and class weights, uniform labels.
SMALL = [(3, 5, 3, 0), (7, 65, 63, 0), (64, 256, 64, 0), (65, 257, 65, 0), (33, 1000, 33, 0)]
LIMITS = [(256, 16384, 64, 0), (1024, 1172, 256, 0), (1024, 1172, 256, 1)]
CAPS = {"small": (0.0, 0.0), "limit": (0.01, 0.0)}      # (share of rows with an ambiguous pred, with an ambiguous branch) allowed


def kind_id(k):
    return ("none", "cosine", "angular")[k[0]] + ("" if k[0] == NONE else "-m%g" % k[1])


def batch(N, S, E, seed=0):
    """(emb (N, E), w (E, S) fp32 standard normal, labels (N,) int32 uniform over the classes)."""
    rng = np.random.default_rng(1000 * seed + 7)
    return (rng.standard_normal((N, E)).astype(np.float32), rng.standard_normal((E, S)).astype(np.float32),
            rng.integers(0, S, N).astype(np.int32))


def planted_batch():
    """(7, 65, 63) with the plants of the GPU test put in: (emb, w, labels, what), ``what`` naming the rows / columns.
    rows 0, 1: labels -1 and S;  row 2: all zeros;  column 9: all zeros;  column 21 = column 20 (row 3 is built as column 20's
    direction: its first maximum is 20, the two cosines bit-equal);  rows 4, 5: a (cos(phi) w_hat_y + sin(phi) u) with phi = 0.005
    and 3.0, clear of pi - m on both sides for the margins used (pi - 0.5 = 2.64), so both angular branches run;  row 6: phi = 0
    (c_iy = 1: the floor is in force).  At phi = 0 the cosine has no gradient in e_i or w_y, so whatever multiplies it cannot show;
    row 4 sits under the floor too (sin_t = 0.005 < 2^-6) with a gradient that does: the floored factor is 64 c, the unfloored 200 c.
    The random rows of every other input take the unfloored upper branch."""
    N, S, E = 7, 65, 63
    e, w, lab = batch(N, S, E, 3)
    rng = np.random.default_rng(99)
    lab = lab.copy()
    lab[0], lab[1] = -1, S
    e[2] = 0
    w[:, 9] = 0
    w[:, 21] = w[:, 20]
    e[3] = 1.5 * w[:, 20]
    lab[3] = 21
    for row, phi, y in ((4, 0.005, 30), (5, 3.0, 31), (6, 0.0, 32)):
        wy = w[:, y].astype(np.float64)
        wy /= np.linalg.norm(wy)
        u = rng.standard_normal(E)
        u -= (u @ wy) * wy
        u /= np.linalg.norm(u)
        e[row] = (2.0 * (math.cos(phi) * wy + math.sin(phi) * u)).astype(np.float32)
        lab[row] = y
    return e, w, lab, {"out": (0, 1), "zero_row": 2, "zero_col": 9, "twins": (20, 21), "twin_row": 3, "branches": (4, 5), "floor_row": 6}


def e1_batch():
    """E = 1: every cosine is +-1 and every row ties; a plant, not a random case."""
    e = np.array([[0.5], [-2.0], [3.0], [-0.25]], np.float32)
    w = np.array([[1.0, -1.0, 2.0, -0.5, 4.0]], np.float32)
    return e, w, np.array([0, 1, 3, 2], np.int32)


def gpu_inputs():
    """Every (name, cap kind, emb, w, labels) the GPU kernel tests compare inside the bounds; the cap kind is a key of CAPS."""
    out = [("N%d-S%d-E%d-s%d" % c, "small", *batch(*c)) for c in SMALL]
    out += [("N%d-S%d-E%d-s%d" % c, "limit", *batch(*c)) for c in LIMITS]
    return out


def constants(kind, margin):
    """cos_m, sin_m, th, mm as the entry point forms them: in double from the fp32 margin, rounded once to fp32."""
    m = float(np.float32(margin))
    f = lambda v: float(np.float32(v))
    return f(math.cos(m)), f(math.sin(m)), f(-math.cos(m)), f(m * math.sin(m)), m


def cosines64(emb, w):
    """(c (N, S) float64 clamped, n (N), m (S), e_hat, w_hat) with the zero rule."""
    e, w = np.asarray(emb, np.float64), np.asarray(w, np.float64)
    n, m = np.sqrt((e * e).sum(1)), np.sqrt((w * w).sum(0))
    ehat = np.where(n[:, None] > 0, e / np.where(n > 0, n, 1.0)[:, None], 0.0)
    what = np.where(m[None, :] > 0, w / np.where(m > 0, m, 1.0)[None, :], 0.0)
    return np.clip(ehat @ what, -1.0, 1.0), n, m, ehat, what


def target(c, kind, margin):
    """(c', f) of the label cosines c (float64 array)."""
    cos_m, sin_m, th, mm, m = constants(kind, margin)
    if kind == NONE:
        return c.copy(), np.ones_like(c)
    if kind == COSINE:
        return c - m, np.ones_like(c)
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    hi = c > th
    return (np.where(hi, c * cos_m - sin_t * sin_m, c - mm),
            np.where(hi, cos_m + sin_m * c / np.maximum(sin_t, SIN_FLOOR), 1.0))


def analyse(emb, w, labels, kind, margin, scale, pred=None, cos=None):
    """The float64 statement and the bounds.  ``pred``: the argmax to count the hits with (a kernel's; default the reference's);
    ``cos``: cosines64(emb, w) where the caller keeps it (it depends on neither the kind nor the scale).

    Bounds, u = 2^-24 (first order, constants rounded up):
    c     d_ic: E products summed with fmaf in any order, |dd| <= E u sum_t |e w| <= E u n m (Cauchy-Schwarz);  n and m: a sum of E
          non-negative terms ((E + 1) u), halved by sqrtf, which rounds once: each (E + 3) / 2 u;  their product and the division: 2 u.
          |dc| <= E u + (E + 5) u |c| <= bc = 2 (E + 8) u (absolute; the clamp only moves a value towards the true one).
    c'    COSINE: bc + u.  ANGULAR, c > th: v = 1 - c^2 moves by dv = 2 |c| bc + 2 u, sin_t by ds = min(dv / sin_t, sqrt(dv)) + u;
          c' by cos_m bc + sin_m ds + 4 u (the two constants, the product, the fmaf).  Otherwise bc + 2 u.
    z     scale (that bound) + u |z|.
    l_i   logsumexp is 1-Lipschitz in the largest |dz|, the label's logit enters once more: dz_max + dz_y;  the argument z - zmax
          (|.| <= 2 scale) rounds once, expf 2 u, the S terms in any nesting S u, logf 2 u:  (2 scale + S + 4) u + 3 u (|log Z| + |z_y - zmax|).
    loss  the mean of the l_i bounds + (N + 2) u |loss| (N terms in any nesting, the division).
    acc   exact once pred is given.
    g     p_c moves relatively by rp = 2 dz_max' + (2 scale + S + 8) u (dz_max' = max(dz_max, dz_y); softmax: dp_c <= p_c (dz_c + sum_k p_k dz_k));
          c != y: dg = coef p_c (rp + 3 u).  At the label g = coef (p_y - 1) f:  dg = coef ((p_y rp + 2 u) |f| + (1 - p_y) df) + 3 u |g|,
          df = sin_m dq + 3 u |f|, q = c / s, s = max(sin_t, floor):  dq = bc / s_lo + |c| dS / s_lo^2 + 3 u |q| with dS = max(0, min(ds,
          sin_t + ds - floor)) (nothing while both sides sit on the floor) and s_lo = max(floor, s - dS): the amplification by 1 / max(sin_t, floor).
    demb  K = max(N, S) + E + 8 covers the chain of the sum in any nesting, the norms and the divisions.  With Gd = dg + K u |g|:
          dA_i = sum_c (Gd_ic |c_ic| + |g_ic| bc);   |ddemb_i[t]| <= (sum_c Gd_ic |w_hat_c[t]| + (dA_i + K u |A_i|) |e_hat_i[t]|) / n_i.
    grad_w  likewise with dB_c = sum_i (Gd_ic |c_ic| + |g_ic| bc):  (sum_i Gd_ic |e_hat_i[t]| + (dB_c + K u |B_c|) |w_hat_c[t]|) / m_c.
    """
    u = U32
    lab = np.asarray(labels).astype(np.int64)
    c, n, m, ehat, what = cosines64(emb, w) if cos is None else cos
    N, S = c.shape
    E = ehat.shape[1]
    bc = 2 * (E + 8) * u
    part = (lab >= 0) & (lab < S)
    rows = np.flatnonzero(part)
    y = lab[rows]
    # stage 1: the argmax and the branch
    pred_ref = c.argmax(1)
    top2 = np.sort(np.partition(c, S - 2, axis=1)[:, -2:], axis=1)
    pred_amb = top2[:, 1] - top2[:, 0] <= 2 * bc
    cos_m, sin_m, th, mm, mf = constants(kind, margin)
    cy = c[rows, y]
    branch_amb = np.zeros(N, bool)
    if kind == ANGULAR:
        branch_amb[rows] = np.abs(cy - th) <= bc
    pred = pred_ref if pred is None else np.asarray(pred).astype(np.int64)
    # the loss
    cp, f = target(cy, kind, margin)
    z = scale * c
    z[rows, y] = scale * cp
    zmax = z.max(1, keepdims=True)
    ex = np.exp(z - zmax)
    Z = ex.sum(1)
    p = ex / Z[:, None]
    l = np.zeros(N)
    l[rows] = np.log(Z[rows]) - (z[rows, y] - zmax[rows, 0])
    loss = l.sum() / N
    acc = float((pred[rows] == y).sum()) / N
    # c', z, l bounds
    if kind == ANGULAR:
        sin_t = np.sqrt(np.maximum(0.0, 1.0 - cy * cy))
        dv = 2 * np.abs(cy) * bc + 2 * u
        ds = np.minimum(dv / np.maximum(sin_t, TINY), np.sqrt(dv)) + u
        hi = cy > th
        bcp = np.where(hi, cos_m * bc + sin_m * ds + 4 * u, bc + 2 * u)
        s = np.maximum(sin_t, SIN_FLOOR)
        dS = np.maximum(0.0, np.minimum(ds, sin_t + ds - SIN_FLOOR))
        s_lo = np.maximum(SIN_FLOOR, s - dS)
        dq = bc / s_lo + np.abs(cy) * dS / (s_lo * s_lo) + 3 * u * np.abs(cy / s)
        df = np.where(hi, sin_m * dq + 3 * u * np.abs(f), 0.0)
    else:
        bcp = np.full(len(rows), bc + 2 * u)
        df = np.zeros(len(rows))
    dz = scale * bc + u * scale
    dzy = scale * bcp + u * np.abs(scale * cp)
    lb = np.zeros(N)
    lb[rows] = dz + dzy + (2 * scale + S + 4) * u + 3 * u * (np.abs(np.log(Z[rows])) + np.abs(z[rows, y] - zmax[rows, 0]))
    loss_b = lb.sum() / N + (N + 2) * u * abs(loss) + TINY
    # gradients
    coef = scale / N
    g = np.zeros((N, S))
    dg = np.zeros((N, S))
    g[rows] = coef * p[rows]
    rp = 2 * np.maximum(dz, dzy) + (2 * scale + S + 8) * u
    dg[rows] = coef * p[rows] * (rp + 3 * u)[:, None]
    py = p[rows, y]
    g[rows, y] = coef * (py - 1.0) * f
    dg[rows, y] = coef * ((py * rp + 2 * u) * np.abs(f) + (1.0 - py) * df) + 3 * u * np.abs(g[rows, y])
    K = max(N, S) + E + 8
    Gd = dg + K * u * np.abs(g)
    A, B = (g * c).sum(1), (g * c).sum(0)
    dA = (Gd * np.abs(c) + np.abs(g) * bc).sum(1)
    dB = (Gd * np.abs(c) + np.abs(g) * bc).sum(0)
    inv_n = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)
    inv_m = np.where(m > 0, 1.0 / np.where(m > 0, m, 1.0), 0.0)
    demb = (g @ what.T - A[:, None] * ehat) * inv_n[:, None]
    grad_w = (ehat.T @ g - B[None, :] * what) * inv_m[None, :]
    demb_b = (Gd @ np.abs(what).T + (dA + K * u * np.abs(A))[:, None] * np.abs(ehat)) * inv_n[:, None] + TINY
    gw_b = (np.abs(ehat).T @ Gd + (dB + K * u * np.abs(B))[None, :] * np.abs(what)) * inv_m[None, :] + TINY
    return {"c": c, "pred_ref": pred_ref, "pred_amb": pred_amb, "branch_amb": branch_amb, "part": part, "loss": float(loss), "acc": acc,
            "p": p, "z": z, "g": g, "demb": demb, "grad_w": grad_w, "prob": _softmax64(scale * c), "f": f, "cy": cy, "rows": rows,
            "bounds": {"c": bc, "loss": loss_b, "demb": demb_b, "grad_w": gw_b, "prob": 2 * (scale * bc + (scale + S + 8) * u)}}


def _softmax64(z):
    ex = np.exp(z - z.max(1, keepdims=True))
    return ex / ex.sum(1, keepdims=True)


def ambiguity(emb, w, labels, margins=(0.2, 0.5)):
    """(share of rows with an ambiguous pred, share with an ambiguous angular branch, worst over the margins) of an input."""
    amb_b = 0.0
    for mg in margins:
        an = analyse(emb, w, labels, ANGULAR, mg, 1.0)
        amb_b = max(amb_b, an["branch_amb"].mean())
    return an["pred_amb"].mean(), amb_b


def admissible(pred, an):
    """Stage 1: is a result's argmax admissible against the analysis ``an``?  Returns a list of complaints (empty: yes)."""
    bad = []
    c, bc = an["c"], an["bounds"]["c"]
    pred = np.asarray(pred).astype(np.int64)
    for i in range(len(c)):
        j, r = pred[i], an["pred_ref"][i]
        if j < 0 or j >= c.shape[1]:
            bad.append("pred[%d] = %d is no class" % (i, j))
        elif j != r and (not an["pred_amb"][i] or c[i, r] - c[i, j] > 2 * bc):
            bad.append("pred[%d] = %d, the reference takes %d (c %r against %r)" % (i, j, r, c[i, j], c[i, r]))
    return bad


def ratios(out, an, grad_scale=1.0):
    """max |out - reference| / bound per output present in ``out`` (each <= 1 inside the bounds); ``an``: the analysis evaluated with
    out's pred.  acc is exact: its entry is 0 or inf."""
    b = an["bounds"]
    r = {}
    if "cosine" in out:
        r["cosine"] = float(np.abs(np.asarray(out["cosine"], np.float64) - an["c"]).max() / b["c"])
    if "prob" in out:
        r["prob"] = float((np.abs(np.asarray(out["prob"], np.float64) - an["prob"]) / (b["prob"] * an["prob"] + TINY)).max())
    if "loss" in out:
        r["loss"] = abs(out["loss"] - an["loss"]) / b["loss"]
        r["acc"] = 0.0 if abs(out["acc"] - an["acc"]) <= 2 * U32 else float("inf")
    for k in ("demb", "grad_w"):
        if out.get(k) is not None:
            r[k] = float((np.abs(np.asarray(out[k], np.float64) / grad_scale - an[k]) / b[k]).max())
    return r


def check(out, emb, w, labels, kind, margin, scale, grad_scale=1.0, cos=None):
    """Both stages for a result ``out`` (pred, and any of cosine, prob, loss + acc, demb, grad_w): (complaints, ratios, the analysis)."""
    an = analyse(emb, w, labels, kind, margin, scale, out["pred"], cos)
    bad = admissible(out["pred"], an)
    if bad:
        return bad, {}, an
    return bad, ratios(out, an, grad_scale), an


# ---- the same loss in torch (autograd) -----------------------------------------------------------------------------------------
def margin_loss_torch(e, w, labels, kind, margin, scale):
    """The float64 loss on torch tensors (differentiable in e and w).  The clamp passes the gradient; where sin_t is under the floor
    the target's derivative is the floored f by definition, so there c' is attached with that slope."""
    lab = np.asarray(labels).astype(np.int64)
    N, S = e.shape[0], w.shape[1]
    sse, ssw = (e * e).sum(1), (w * w).sum(0)
    n = torch.sqrt(torch.where(sse > 0, sse, torch.ones_like(sse)))   # (sqrt has no gradient at 0: a zero row / column is masked before it)
    m = torch.sqrt(torch.where(ssw > 0, ssw, torch.ones_like(ssw)))
    ok = (sse[:, None] > 0) & (ssw[None, :] > 0)
    raw = torch.where(ok, (e @ w) / (n[:, None] * m[None, :]), torch.zeros(N, S, dtype=e.dtype))
    c = raw + (raw.clamp(-1.0, 1.0) - raw).detach()
    part = (lab >= 0) & (lab < S)
    rows = np.flatnonzero(part)
    if len(rows) == 0:
        return (e * 0).sum()
    y = lab[rows]
    cy = c[rows, y]
    cos_m, sin_m, th, mm, mf = constants(kind, margin)
    if kind == NONE:
        cp = cy
    elif kind == COSINE:
        cp = cy - mf
    else:
        cd = cy.detach()
        sin_t = torch.sqrt(torch.clamp(1.0 - cy * cy, min=0.0) + (cd.abs() >= 1).to(e.dtype) * 1e-300)
        smooth = cy * cos_m - sin_t * sin_m
        floored = (cd * cos_m - torch.sqrt(torch.clamp(1.0 - cd * cd, min=0.0)) * sin_m) + (cos_m + sin_m * cd / SIN_FLOOR) * (cy - cd)
        hi = torch.where(sin_t.detach() > SIN_FLOOR, smooth, floored)
        cp = torch.where(cd > th, hi, cy - mm)
    z = scale * c[rows]
    onehot = torch.zeros_like(z)
    onehot[np.arange(len(rows)), y] = 1.0
    z = z * (1 - onehot) + (scale * cp)[:, None] * onehot
    return (torch.logsumexp(z, 1) - z[np.arange(len(rows)), y]).sum() / N


def autograd(emb, w, labels, kind, margin, scale):
    e = torch.tensor(np.asarray(emb), dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(np.asarray(w), dtype=torch.float64, requires_grad=True)
    loss = margin_loss_torch(e, wt, labels, kind, margin, scale)
    ge, gw = torch.autograd.grad(loss, [e, wt])
    return float(loss.detach()), ge.numpy(), gw.numpy()


# ---- fp32 restatement ----------------------------------------------------------------------------------------------------------
WRONG = ("no_projection", "margin_all", "wrong_side", "no_floor", "no_div_n")


def _fsum(x, rev, axis):
    """An fp32 sum along an axis taken one element at a time, ascending or descending."""
    x = np.asarray(x, np.float32)
    x = np.flip(x, axis) if rev else x
    return np.cumsum(x, axis=axis, dtype=np.float32).take(-1, axis=axis)


def margin_f32(emb, w, labels, kind, margin, scale, rev=False, grad_scale=1.0, wrong=None):
    """The kernel's arithmetic in fp32 numpy (a host model of it), every sum one element at a time, ascending or (``rev``) descending:
    the E components, the S classes, the N rows.  ``wrong``: a deliberately wrong variant the bounds must catch -- "no_projection"
    (the -(sum_c g c) e_hat term of demb dropped), "margin_all" (the margin applied to every class), "wrong_side" (the angular branch
    taken on the wrong side of th), "no_floor" (sin_t not floored), "no_div_n" (the division by N missing).
    Returns cosine, prob, pred, loss, acc, demb, grad_w."""
    f = np.float32
    e, w = np.asarray(emb, f), np.asarray(w, f)
    lab = np.asarray(labels).astype(np.int64)
    N, E = e.shape
    S = w.shape[1]
    n, m = np.sqrt(_fsum(e * e, rev, 1)), np.sqrt(_fsum(w * w, rev, 0))
    dot = _fsum(e[:, :, None] * w[None, :, :], rev, 1) if N * E * S <= 1 << 24 else None
    if dot is None:
        dot = np.zeros((N, S), f)
        for t in (range(E - 1, -1, -1) if rev else range(E)):
            dot = dot + e[:, t:t + 1] * w[t:t + 1, :]
    ok = (n[:, None] > 0) & (m[None, :] > 0)
    den = np.where(ok, n[:, None] * m[None, :], f(1))
    c = np.where(ok, np.clip(dot / den, f(-1), f(1)), f(0)).astype(f)
    pred = c.argmax(1)
    sc = f(scale)
    zu = sc * c
    eu = np.exp(zu - zu.max(1, keepdims=True)).astype(f)
    prob = eu / _fsum(eu, rev, 1)[:, None]
    cos_m, sin_m, th, mm, mf = (f(v) for v in constants(kind, margin))
    part = (lab >= 0) & (lab < S)
    rows = np.flatnonzero(part)
    y = lab[rows]

    def tgt(cy):
        if kind == NONE:
            return cy, np.ones_like(cy)
        if kind == COSINE:
            return cy - mf, np.ones_like(cy)
        sin_t = np.sqrt(np.maximum(f(0), f(1) - cy * cy)).astype(f)
        hi = (cy <= th) if wrong == "wrong_side" else (cy > th)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = cy / (sin_t if wrong == "no_floor" else np.maximum(sin_t, f(SIN_FLOOR)))
        return (np.where(hi, cy * cos_m - sin_t * sin_m, cy - mm).astype(f), np.where(hi, cos_m + sin_m * q, f(1)).astype(f))

    z = zu.copy()
    if wrong == "margin_all":
        z[rows] = sc * tgt(c[rows])[0]
    cp, fy = tgt(c[rows, y])
    z[rows, y] = sc * cp
    zmax = z.max(1, keepdims=True)
    ex = np.exp(z - zmax).astype(f)
    Z = _fsum(ex, rev, 1)
    l = np.zeros(N, f)
    l[rows] = np.log(Z[rows]) - (z[rows, y] - zmax[rows, 0])
    norm = f(1) if wrong == "no_div_n" else f(N)
    loss = _fsum(l, rev, 0) / norm
    acc = f((pred[rows] == y).sum()) / f(N)
    g = np.zeros((N, S), f)
    coef = sc / norm
    g[rows] = coef * (ex[rows] / Z[rows, None])
    g[rows, y] = coef * (ex[rows, y] / Z[rows] - f(1)) * fy
    inv_n = np.where(n > 0, f(1) / np.where(n > 0, n, f(1)), f(0)).astype(f)
    ehat = (e * inv_n[:, None]).astype(f)
    gm = np.where(m[None, :] > 0, g / np.where(m > 0, m, f(1))[None, :], f(0)).astype(f)
    A = _fsum(g * c, rev, 1)
    B = _fsum(g * c, rev, 0)
    acc_e = np.zeros((N, E), f)
    for cc in (range(S - 1, -1, -1) if rev else range(S)):
        acc_e = acc_e + gm[:, cc:cc + 1] * w[None, :, cc]
    if wrong != "no_projection":
        acc_e = acc_e - A[:, None] * ehat
    demb = f(grad_scale) * (acc_e * inv_n[:, None])
    acc_w = np.zeros((E, S), f)
    for i in (range(N - 1, -1, -1) if rev else range(N)):
        acc_w = acc_w + ehat[i][:, None] * g[i][None, :]
    what = np.where(m[None, :] > 0, w / np.where(m > 0, m, f(1))[None, :], f(0)).astype(f)
    grad_w = f(grad_scale) * np.where(m[None, :] > 0, (acc_w - B[None, :] * what) / np.where(m > 0, m, f(1))[None, :], f(0))
    return {"cosine": c, "prob": prob, "pred": pred, "loss": float(loss), "acc": float(acc), "demb": demb.astype(f), "grad_w": grad_w.astype(f)}


# ---- the training step in float64 ---------------------------------------------------------------------------------------------
def margin_step_oracle(arch, p, state, x, labels, kind, margin, scale, drop_masks=None):
    """One margin-softmax training step in float64, put together like tests/triplet_refs.py's: O.encoder_forward (training, the whole
    batch one tower) + the loss above on (embeddings, head.kernel) + autograd + the moving-statistic updates + O.adam_step.  The
    head's bias takes no part: its gradient is zero and Adam leaves it where it is."""
    from collections import OrderedDict
    from oracle import voicemap_oracle as O
    names = O.param_names(arch, head="classifier")
    leaf = OrderedDict((nm, v.detach().clone().requires_grad_(nm in names)) for nm, v in p.items())
    c = {}
    e = O.encoder_forward(arch, leaf, x, True, drop_masks, c)
    loss = margin_loss_torch(e, leaf["head.kernel"], labels, kind, margin, scale)
    gl = torch.autograd.grad(loss, [leaf[nm] for nm in names], allow_unused=True)
    grads = OrderedDict((nm, torch.zeros_like(leaf[nm]) if g is None else g.detach()) for nm, g in zip(names, gl))
    new_p = OrderedDict((nm, v.detach().clone()) for nm, v in p.items())
    O.apply_moving_updates(new_p, (c,), len(arch.blocks), arch.bn_eps, arch.bn_momentum, True, "fresh")
    if state is not None:
        tr = O.adam_step(state, OrderedDict((nm, new_p[nm]) for nm in names), grads)
        for nm in names:
            new_p[nm] = tr[nm]
    return {"loss": float(loss.detach()), "e": e.detach(), "grads": grads, "params": new_p}
