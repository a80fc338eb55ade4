"""Reference helpers of the prototypical-loss tests (tests/test_gpu_proto_loss.py and tests/test_gpu_proto_step.py on the device,
tests/test_proto_refs_cpu.py on the host): the float64 statement of the loss (torch, autograd for the gradients), its closed-form
gradients, an fp32 numpy restatement in two summation orders, the test inputs and error bounds derived by counting roundings.  Pure
numpy / torch: nothing here touches the HIP library or a GPU.

The loss (include/voicemap_hip.h, vm_proto_loss).  emb (k n + m, E): rows [0, k n) the support set, class-major, then m queries.
    p_c = mean of class c's n support rows          l[j, c] = -alpha sum_t (q_j[t] - p_c[t])^2
    L = mean_j (logsumexp_c l[j] - l[j, y_j])       acc = mean_j [first argmax_c l[j] == y_j]
    with r = softmax(l) - onehot(y):  dL/dq_j = (2 alpha / m) sum_c r[j, c] p_c,   dL/dp_c = (2 alpha / m) sum_j r[j, c] (q_j - p_c),
    every support row of class c receives dL/dp_c / n.
"""
import numpy as np
import torch

U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
TINY = 2.0 ** -125          # an fp32 exp() that underflows (flushed or denormal) is off by less than this, absolutely

# (k, n, m, E, alpha): the shapes of tests/test_gpu_proto_loss.py.  alpha is not 1 everywhere, so that a gradient that drops it differs.
CASES = [(2, 1, 1, 1, 1.0), (2, 1, 3, 64, 0.5), (5, 1, 5, 64, 1.0), (5, 5, 25, 128, 2.0), (3, 2, 7, 33, 0.5), (20, 5, 40, 64, 1.0),
         (64, 2, 128, 64, 1.0), (65, 1, 67, 31, 0.75), (128, 1, 130, 128, 1.0), (16, 16, 16, 256, 1.5)]


def case_id(c):
    return "k%d-n%d-m%d-E%d" % c[:4]


def episode(k, n, m, E, seed=0, scale=1.0, labels=None):
    """(emb (k n + m, E) fp32, labels (m,) int32): class centres N(0, 0.3^2), members centre + N(0, 0.3^2) -- the softmax is neither
    uniform nor one-hot; labels random and unbalanced (class c with weight ~ c + 1) unless given."""
    rng = np.random.default_rng(1000 * k + 100 * n + 10 * m + E + seed)
    centres = rng.normal(0, 0.3, (k, E))
    if labels is None:
        w = np.arange(1, k + 1, dtype=np.float64)
        labels = rng.choice(k, size=m, p=w / w.sum())
    labels = np.asarray(labels, dtype=np.int32)
    sup = np.repeat(centres, n, axis=0) + rng.normal(0, 0.3, (k * n, E))
    qry = centres[labels] + rng.normal(0, 0.3, (m, E))
    return (np.concatenate([sup, qry]) * scale).astype(np.float32), labels


def proto_ref(emb, labels, k, n, alpha):
    """The float64 statement: dict of numpy float64 arrays -- logits (m, k), soft (m, k), loss_rows (m,), loss, pred (m,) first
    argmax, acc, demb (k n + m, E) by autograd."""
    e = torch.tensor(np.asarray(emb), dtype=torch.float64, requires_grad=True)
    y = torch.tensor(np.asarray(labels), dtype=torch.int64)
    m = len(y)
    p = e[:k * n].reshape(k, n, -1).mean(1)
    q = e[k * n:]
    lg = -alpha * ((q[:, None, :] - p[None]) ** 2).sum(-1)
    rows = torch.logsumexp(lg, 1) - lg[torch.arange(m), y]
    loss = rows.mean()
    (g,) = torch.autograd.grad(loss, e)
    lgn = lg.detach().numpy()
    pred = lgn.argmax(1)          # numpy: the first maximum
    return {"logits": lgn, "soft": torch.softmax(lg, 1).detach().numpy(), "loss_rows": rows.detach().numpy(), "loss": float(loss.detach()),
            "pred": pred, "acc": float((pred == np.asarray(labels)).mean()), "demb": g.numpy()}


def proto_closed(emb, labels, k, n, alpha):
    """The closed-form gradients of the module docstring in float64: demb (k n + m, E)."""
    e = np.asarray(emb, dtype=np.float64)
    m = len(labels)
    p = e[:k * n].reshape(k, n, -1).mean(1)
    q = e[k * n:]
    lg = -alpha * ((q[:, None] - p[None]) ** 2).sum(-1)
    s = np.exp(lg - lg.max(1, keepdims=True))
    s /= s.sum(1, keepdims=True)
    r = s - np.eye(k)[np.asarray(labels)]
    gq = 2 * alpha / m * (r @ p)
    gp = 2 * alpha / m * (r.T @ q - r.sum(0)[:, None] * p)
    return np.concatenate([np.repeat(gp / n, n, 0), gq])


def proto_f32(emb, labels, k, n, alpha, rev=False, grad_scale=1.0, wrong=None):
    """The same arithmetic in fp32 numpy, every sum one element at a time, ascending or (``rev``) descending: support rows, the E
    components, the classes, the queries.  ``wrong``: a deliberately wrong variant the bounds must catch -- "proto_n_plus_1" (the
    prototype divided by n + 1), "grad_no_alpha" (alpha dropped from the gradient), "support_no_n" (a support gradient not divided by
    n).  Returns logits, loss, acc, demb like proto_ref."""
    f = np.float32
    e = np.asarray(emb, dtype=f)
    y = np.asarray(labels)
    m, E = len(y), e.shape[1]
    order = (lambda cnt: range(cnt - 1, -1, -1)) if rev else (lambda cnt: range(cnt))
    p = np.zeros((k, E), f)
    for i in order(n):
        p = p + e[i:k * n:n]
    p = p / f(n + 1 if wrong == "proto_n_plus_1" else n)
    q = e[k * n:]
    d2 = np.zeros((m, k), f)
    for t in order(E):
        d = q[:, None, t] - p[None, :, t]
        d2 = d2 + d * d
    lg = (-f(alpha)) * d2
    mx = lg.max(1, keepdims=True)
    ex = np.exp(lg - mx, dtype=f)
    S = np.zeros((m, 1), f)
    for c in order(k):
        S = S + ex[:, c:c + 1]
    r = ex / S
    r[np.arange(m), y] -= f(1)
    rows = np.log(S[:, 0], dtype=f) - (lg[np.arange(m), y] - mx[:, 0])
    loss = f(0)
    for j in order(m):
        loss = loss + rows[j]
    coef = f(2) * f(1.0 if wrong == "grad_no_alpha" else alpha) / f(m)
    gq = np.zeros((m, E), f)
    for c in order(k):
        gq = gq + r[:, c:c + 1] * p[c][None]
    gp = np.zeros((k, E), f)
    for j in order(m):
        gp = gp + r[j][:, None] * (q[j][None] - p)
    gs = coef * gp / f(1 if wrong == "support_no_n" else n)
    pred = lg.argmax(1)
    return {"logits": lg, "loss": float(loss / f(m)), "acc": float((pred == y).mean()), "pred": pred,
            "demb": f(grad_scale) * np.concatenate([np.repeat(gs, n, 0), coef * gq])}


def proto_bounds(emb, labels, k, n, alpha, ref=None):
    """Worst-case |fp32 result - float64 result| of every output for ANY order of the sums, from the logit bound on.  u = 2^-24.

    logits   |dl[j, c]| <= B[j, c] = alpha (E + n + 6) u sum_t (|q_j[t]| + A_c[t])^2,  A_c = mean |support rows of c|:
             p_c[t] carries n roundings (n - 1 adds, one division) of at most u A_c[t] each; the difference, its square and the E
             adds give a relative (E + 2) u of every term; d^2's sensitivity to p doubles the n u; alpha and the sign add 2 more.
    soft     s_c = exp(l_c - max) / S.  The logit errors move the numerator by a factor e^{+-B} and S by one inside e^{+-Bj}
             (Bj = max_c B[j, c]): 2 Bj in the exponent.  l_c - max is rounded once: u g_c with g_c = max - l_c.  exp: 4 u (a
             few ulp), the k adds of S: k u, the division: u, slack for second-order terms: 3 u.  So
             |ds_c| <= s_c expm1(2 Bj + u g_c + (k + 8) u) + TINY.
    loss     a row is log S - (l_y - max) = logsumexp(l) - l_y: 1-Lipschitz in each of the two -> 2 Bj.  S's relative error is
             u sum_c s_c g_c + (k + 5) u with sum_c s_c g_c <= H(s) <= log k; logf: 4 u log k; l_y - max: u g_y; the final
             subtraction: u (row + g_y + log k).  Together 2 Bj + u (k + 8 + 6 log k + 2 g_y + 2 row).  The mean over m rows in any
             order: (m + 2) u mean(row) on top of the mean of the row bounds.
    acc      a query's argmax may differ only if a class other than the reference's first maximum lies within B[j, c] + B[j, c*] of
             it: acc moves by at most (such queries) / m, + (m + 2) u for the mean.
    demb     r = s - onehot: |dr_c| <= |ds_c| + u |r_c|.
             query rows, (2 alpha / m) sum_c r_c p_c[t]: dr_c |p_c| + |r_c| n u A_c (the prototype's roundings) + (k + 2) u
             |r_c| |p_c| (the dot product) + 4 u (the coefficient's two roundings, its product, grad_scale), and |p_c[t]| <= A_c[t]:
                 (2 alpha / m) sum_c (|ds_c| + (k + n + 7) u |r_c|) A_c[t]
             support rows, (2 alpha / (m n)) sum_j r[j, c] (q_j[t] - p_c[t]): the difference is off by (n + 1) u (|q| + A_c), the sum
             over m queries by (m + 2) u, the coefficient, the division by n and grad_scale by 5 u:
                 (2 alpha / (m n)) sum_j (|ds[j, c]| + (m + n + 9) u |r[j, c]|) (|q_j[t]| + A_c[t])
    Returns dict(logits (m, k), soft (m, k), loss, acc, demb (k n + m, E), ambiguous (m,) bool)."""
    ref = ref or proto_ref(emb, labels, k, n, alpha)
    e = np.abs(np.asarray(emb, dtype=np.float64))
    y = np.asarray(labels)
    m, E = len(y), e.shape[1]
    u = U32
    A = e[:k * n].reshape(k, n, E).mean(1)
    aq = e[k * n:]
    B = alpha * (E + n + 6) * u * ((aq[:, None] + A[None]) ** 2).sum(-1)
    Bj = B.max(1)
    lg, s, rows = ref["logits"], ref["soft"], ref["loss_rows"]
    g = lg.max(1, keepdims=True) - lg
    ds = s * np.expm1(2 * Bj[:, None] + u * g + (k + 8) * u) + TINY
    gy = g[np.arange(m), y]
    row_b = 2 * Bj + u * (k + 8 + 6 * np.log(k) + 2 * gy + 2 * rows)
    loss_b = row_b.mean() + (m + 2) * u * rows.mean()
    top = ref["pred"]
    gap = lg[np.arange(m), top][:, None] - lg
    close = gap <= B + B[np.arange(m), top][:, None]
    close[np.arange(m), top] = False
    amb = close.any(1)
    r = np.abs(s - np.eye(k)[y])
    gq = (2 * alpha / m) * ((ds + (k + n + 7) * u * r) @ A)
    w = ds + (m + n + 9) * u * r                                              # (m, k)
    gs = (2 * alpha / (m * n)) * (w.T @ aq + w.sum(0)[:, None] * A)            # (k, E)
    return {"logits": B, "soft": ds, "loss": loss_b, "acc": amb.sum() / m + (m + 2) * u, "ambiguous": amb,
            "demb": np.concatenate([np.repeat(gs, n, 0), gq])}


def ratios(out, ref, bnd, grad_scale=1.0):
    """max |out - ref| / bound per output (each <= 1 when ``out`` is inside the bounds); ``out`` holds logits, loss, acc, demb."""
    w = {"logits": float((np.abs(out["logits"] - ref["logits"]) / bnd["logits"]).max()),
         "loss": abs(out["loss"] - ref["loss"]) / bnd["loss"],
         "acc": abs(out["acc"] - ref["acc"]) / bnd["acc"]}
    if out.get("demb") is not None:
        w["demb"] = float((np.abs(np.asarray(out["demb"], dtype=np.float64) / grad_scale - ref["demb"]) / bnd["demb"]).max())
    return w


def proto_loss_torch(e, labels, k, n, alpha):
    """The float64 loss on a torch tensor of embeddings (differentiable): (loss, logits)."""
    y = torch.as_tensor(np.asarray(labels), dtype=torch.int64)
    p = e[:k * n].reshape(k, n, -1).mean(1)
    lg = -alpha * ((e[k * n:, None, :] - p[None]) ** 2).sum(-1)
    return (torch.logsumexp(lg, 1) - lg[torch.arange(len(y)), y]).mean(), lg


def proto_step_oracle(arch, p, state, x, labels, k, n, alpha=1.0, drop_masks=None):
    """One prototypical training step in float64, put together like the oracle's classifier_train_step: O.encoder_forward (training,
    the whole episode one tower) + the loss above + autograd + the moving-statistic updates + O.adam_step.  ``p``: the parameters of
    a bare encoder (O.init_params(arch, head=None))."""
    from collections import OrderedDict
    from oracle import voicemap_oracle as O
    names = O.param_names(arch, head=None)
    leaf = OrderedDict((nm, v.detach().clone().requires_grad_(nm in names)) for nm, v in p.items())
    c = {}
    e = O.encoder_forward(arch, leaf, x, True, drop_masks, c)
    loss, lg = proto_loss_torch(e, labels, k, n, alpha)
    gl = torch.autograd.grad(loss, [leaf[nm] for nm in names])
    grads = OrderedDict((nm, g.detach()) for nm, g in zip(names, gl))
    new_p = OrderedDict((nm, v.detach().clone()) for nm, v in p.items())
    O.apply_moving_updates(new_p, (c,), len(arch.blocks), arch.bn_eps, arch.bn_momentum, True, "fresh")
    if state is not None:
        tr = O.adam_step(state, OrderedDict((nm, new_p[nm]) for nm in names), grads)
        for nm in names:
            new_p[nm] = tr[nm]
    lgn = lg.detach().numpy()
    return {"loss": float(loss.detach()), "acc": float((lgn.argmax(1) == np.asarray(labels)).mean()), "logits": lgn, "e": e.detach(),
            "grads": grads, "params": new_p}
