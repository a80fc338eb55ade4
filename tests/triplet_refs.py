"""Reference helpers of the triplet-loss tests (tests/test_gpu_triplet_loss.py and tests/test_gpu_triplet_step.py on the device,
tests/test_triplet_refs_cpu.py on the host): the float64 statement of both minings with its closed-form gradient (numpy), the same
loss in torch for autograd, an fp32 numpy restatement in two summation orders, the test inputs and error bounds derived by counting
roundings.  Pure numpy / torch: nothing here touches the HIP library or a GPU.

The loss (include/voicemap_hip.h, vm_triplet_loss).  emb (N, E), label (N); a row with label < 0 takes no part.
    s_ij = sum_t (e_i[t] - e_j[t])^2, d = sqrt(s);  P_a = {j != a, same label}, N_a = {j, other label};  valid iff both non-empty.
    HARD  hp = first of P_a by (s descending, j ascending), hn = first of N_a by (s, j) ascending; x_a = margin + d_hp - d_hn (soft: no
          margin); hinge max(0, x) with weight [x > 0], or softplus(x) with weight sigmoid(x); mean over the V valid anchors.
    ALL   every (a, p, n): hinge = sum of the active x / A (A = their number, a constant), soft = mean of softplus over the T triplets.
    Gradient: with C[a, j] the signed sum of the weights of the triplets in which j is a's positive (+) or negative (-), already
    divided by V, A or T:  demb[i] = sum_j (C[i, j] + C[j, i]) (e_i - e_j) / d_ij over the pairs with s_ij > 0.

Selections and hinge activity are discontinuous, so a result is compared in two stages (``check``): its hard_pos / hard_neg must be
ADMISSIBLE (the float64 s of the chosen row within the bound of the float64 optimum, and the reference's own choice wherever the gap
to the runner-up exceeds the bound); the float64 loss and gradient are then evaluated WITH those indices.  A triplet (in HARD: an
anchor) whose float64 |x| is within its bound is AMBIGUOUS: it may count either way, and the bounds widen by what it can contribute.
The inputs of the GPU tests are chosen so that the small shapes have no ambiguity at all and the limit shapes at most 1 % ambiguous
selections and 1e-3 ambiguous triplets (``CAPS``; tests/test_triplet_refs_cpu.py asserts it for every GPU input).
"""
import numpy as np
import torch

U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
TINY = 2.0 ** -125
HARD, ALL = 0, 1            # VM_TRIPLET_HARD, VM_TRIPLET_ALL
VARIANTS = [(HARD, 0), (HARD, 1), (ALL, 0), (ALL, 1)]     # (mining, soft)
MARGIN = 1.0

# (P, K, E, seed): standard-normal fp32 embeddings, class-major labels.  The last two are the limits (N = 1024; E = 256).
SMALL = [(2, 2, 1, 0), (3, 2, 5, 0), (12, 4, 64, 0), (12, 4, 64, 1)]
LIMITS = [(256, 4, 64, 0), (64, 4, 256, 0)]
CAPS = {"small": (0.0, 0.0), "limit": (0.01, 1e-3)}      # (share of ambiguous selections, share of ambiguous triplets) allowed


def variant_id(v):
    return ("hard", "all")[v[0]] + ("-hinge", "-soft")[v[1]]


def pk_batch(P, K, E, seed=0):
    """(emb (P K, E) fp32 standard normal, labels (P K,) int32 class-major 0..P-1 each K times)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((P * K, E)).astype(np.float32), np.repeat(np.arange(P), K).astype(np.int32)


def wave_batch(seed=2):
    """N = 65, E = 65: one past a wave in both dimensions; 13 classes of 5 (seeds 0 and 1 have an ambiguous triplet, seed 2 none)."""
    rng = np.random.default_rng(100 + seed)
    return rng.standard_normal((65, 65)).astype(np.float32), np.repeat(np.arange(13), 5).astype(np.int32)


def ragged_batch(seed=0):
    """N = 23, E = 33, rows shuffled: classes of 1, 2, 3 and 5 rows twice over (labels 10..17; 10 and 14 are singletons: invalid anchors
    that still serve as negatives) and one row with label -1.  Returns (emb, labels)."""
    rng = np.random.default_rng(200 + seed)
    lab = np.concatenate([np.repeat(np.arange(10, 18), [1, 2, 3, 5, 1, 2, 3, 5]), [-1]]).astype(np.int32)
    lab = lab[rng.permutation(len(lab))]
    return rng.standard_normal((23, 33)).astype(np.float32), lab


def gpu_inputs():
    """Every (name, kind, emb, labels) the GPU kernel tests compare inside the bounds; kind is a key of CAPS."""
    out = [("P%d-K%d-E%d-s%d" % c, "small", *pk_batch(*c)) for c in SMALL]
    out.append(("N65-E65", "small", *wave_batch()))
    out.append(("ragged-N23-E33", "small", *ragged_batch()))
    out += [("P%d-K%d-E%d-s%d" % c, "limit", *pk_batch(*c)) for c in LIMITS]
    return out


def masks(labels):
    lab = np.asarray(labels).astype(np.int64)
    part = lab >= 0
    same = lab[:, None] == lab[None, :]
    both = part[:, None] & part[None, :]
    pos = both & same & ~np.eye(len(lab), dtype=bool)
    neg = both & ~same
    return pos, neg


def sq_dists(e):
    """(N, N) sum_t (e_i[t] - e_j[t])^2 in e's dtype by the direct form, in row chunks."""
    N = len(e)
    s = np.empty((N, N), e.dtype)
    for i in range(0, N, 16):
        s[i:i + 16] = np.square(e[i:i + 16, None, :] - e[None, :, :]).sum(-1)
    return s


def select(s, pos, neg):
    """hp (first maximum of s over pos), hn (first minimum over neg), valid; -1 where not valid."""
    valid = pos.any(1) & neg.any(1)
    hp = np.where(pos, s, -np.inf).argmax(1)
    hn = np.where(neg, s, np.inf).argmin(1)
    return np.where(valid, hp, -1), np.where(valid, hn, -1), valid


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    t = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, t) / (1.0 + t)


def analyse(emb, labels, mining, soft, margin, hp=None, hn=None):
    """The float64 statement and the bounds.  ``hp`` / ``hn``: the indices to evaluate HARD with (a kernel's; default the reference's).

    Bounds, u = 2^-24 (first order, constants rounded up):
    s     a difference rounds once (its square: 2 u), the fused multiply-adds and the E non-negative terms in any order add (E - 1) u,
          the butterfly nothing more:  |ds| <= (E + 3) u s.  Two values compare reliably when they differ by more than the sum of
          their bounds.
    d     sqrtf halves the relative error of s and rounds once: (E + 5) / 2 u d; (E + 5) u d is used, as for the caps.
    x     margin + d_p - d_n: the two distance bounds and the two additions' roundings, 2 u (margin + d_p + d_n).
    loss  max(0, x) and softplus are 1-Lipschitz: a term moves by its x bound, plus 12 u l for expf, log1pf and the additions; a sum of
          n terms taken in any nesting adds n u: the longest chain is (an anchor's triplets) + N.  An ambiguous term is inside its x
          bound either way (the hinge is continuous).  ALL-hinge divides by A: m ambiguous triplets move it by m / (A - m), relatively.
    share m ambiguous terms move it by m / (V or T), + 4 u.
    demb  |dC| of a pair: soft, sigmoid' <= 1/4: sum over its triplets of (x bound / 4 + 8 u g) / norm; hinge: its ambiguous triplets /
          norm; the sum of up to N weights N u |C|.  The division by d: (E + 5) u; the difference e_i - e_j: u; the sum over j: N u;
          W[i][j] + W[j][i], the division by the norm, grad_scale, slack: 9 u.  With |e_i[t] - e_j[t]| <= |e_i[t]| + |e_j[t]|:
              sum_j ((2 N + E + 15) u (|C_ij| + |C_ji|) + dC_ij + dC_ji [+ m / (A - m) (|C_ij| + |C_ji|)]) / d_ij (|e_i[t]| + |e_j[t]|)
    """
    e = np.asarray(emb, dtype=np.float64)
    N, E = e.shape
    u = U32
    pos, neg = masks(labels)
    s = sq_dists(e)
    d = np.sqrt(s)
    invd = np.where(s > 0, 1.0 / np.where(s > 0, d, 1.0), 0.0)
    bs = (E + 3) * u * s
    hp_ref, hn_ref, valid = select(s, pos, neg)
    # runner-up gaps of the reference's selections
    sel_amb = np.zeros((N, 2), bool)
    for col, mask, sign in ((0, pos, -1.0), (1, neg, 1.0)):
        key = np.where(mask, sign * s, np.inf)              # ascending: the selected one first
        order = np.argsort(key, axis=1, kind="stable")[:, :2]
        k0, k1 = key[np.arange(N), order[:, 0]], key[np.arange(N), order[:, 1]]
        b0, b1 = bs[np.arange(N), order[:, 0]], bs[np.arange(N), order[:, 1]]
        with np.errstate(invalid="ignore"):   # (an anchor without a runner-up: inf - inf)
            sel_amb[:, col] = valid & np.isfinite(k1) & (k1 - k0 <= b0 + b1)
    hp = hp_ref if hp is None else np.asarray(hp).astype(np.int64)
    hn = hn_ref if hn is None else np.asarray(hn).astype(np.int64)
    V = int(valid.sum())
    C, dC = np.zeros((N, N)), np.zeros((N, N))
    bd = lambda dd: (E + 5) * u * dd
    out = {"hp_ref": hp_ref, "hn_ref": hn_ref, "valid": valid, "V": V, "sel_amb": sel_amb, "s": s, "bs": bs, "pos": pos, "neg": neg}
    rows = np.flatnonzero(valid)
    if mining == HARD:
        dp, dn = d[rows, hp[rows]], d[rows, hn[rows]]
        m = 0.0 if soft else margin
        x = m + dp - dn
        bx = bd(dp) + bd(dn) + 2 * u * (m + dp + dn)
        amb = np.abs(x) <= bx
        l = _softplus(x) if soft else np.maximum(x, 0)
        g = _sigmoid(x) if soft else (x > 0).astype(np.float64)
        norm = max(1, V)
        C[rows, hp[rows]] += g / norm
        C[rows, hn[rows]] -= g / norm
        dg = (bx / 4 + 8 * u * g) if soft else amb.astype(np.float64)
        dC[rows, hp[rows]] += dg / norm
        dC[rows, hn[rows]] += dg / norm
        loss = l.sum() / norm
        share = float((x > 0).sum()) / norm
        loss_b = (bx + 12 * u * l).sum() / norm + (N + 4) * u * loss + TINY
        n_amb, n_terms, rel = int(amb.sum()), V, 0.0
        out.update(x=x, T=V, A=int((x > 0).sum()))
    else:
        m = 0.0 if soft else margin
        per = []
        T = A = n_amb = 0
        for a in rows:
            Pa, Na = np.flatnonzero(pos[a]), np.flatnonzero(neg[a])
            dP, dN = d[a, Pa][:, None], d[a, Na][None, :]
            X = m + dP - dN
            BX = bd(dP) + bd(dN) + 2 * u * (m + dP + dN)
            per.append((a, Pa, Na, X, BX))
            T += X.size
            A += int((X > 0).sum())
            n_amb += int((np.abs(X) <= BX).sum())
        norm = max(1, T if soft else A)
        loss = loss_b = 0.0
        longest = 0
        for a, Pa, Na, X, BX in per:
            Lm = _softplus(X) if soft else np.maximum(X, 0)
            G = _sigmoid(X) if soft else (X > 0).astype(np.float64)
            dG = (BX / 4 + 8 * u * G) if soft else (np.abs(X) <= BX).astype(np.float64)
            C[a, Pa] += G.sum(1) / norm
            C[a, Na] -= G.sum(0) / norm
            dC[a, Pa] += dG.sum(1) / norm
            dC[a, Na] += dG.sum(0) / norm
            loss += Lm.sum() / norm
            loss_b += (BX + 12 * u * Lm).sum() / norm
            longest = max(longest, X.size)
        rel = 0.0 if soft or n_amb == 0 else n_amb / max(1, A - n_amb)
        loss_b += (longest + N + 4) * u * loss + rel * loss + TINY
        share = A / T if T else 0.0
        n_terms = T
        out.update(T=T, A=A)
    Cs = np.abs(C) + np.abs(C).T
    B = (((2 * N + E + 15) * u + rel) * Cs + dC + dC.T) * invd
    ae = np.abs(e)
    M = (C + C.T) * invd
    out.update(loss=float(loss), share=float(share), C=C, demb=M.sum(1)[:, None] * e - M @ e, n_amb=n_amb, n_terms=n_terms,
               bounds={"loss": loss_b, "share": (n_amb / n_terms if n_terms else 0.0) + 4 * u,
                       "demb": B.sum(1)[:, None] * ae + B @ ae + TINY})
    return out


def ambiguity(emb, labels, margin=MARGIN):
    """(share of ambiguous selections, share of ambiguous triplets or anchors, worst over the four variants) of an input."""
    sel = trip = 0.0
    for mining, soft in VARIANTS:
        an = analyse(emb, labels, mining, soft, margin)
        sel = max(sel, an["sel_amb"].sum() / max(1, 2 * an["V"]))
        trip = max(trip, an["n_amb"] / max(1, an["n_terms"]))
    return sel, trip


def admissible(hp, hn, an):
    """Stage 1: are a result's selections admissible against the analysis ``an``?  Returns a list of complaints (empty: yes)."""
    bad = []
    s, bs, valid = an["s"], an["bs"], an["valid"]
    for name, idx, ref, col, mask in (("hard_pos", hp, an["hp_ref"], 0, an["pos"]), ("hard_neg", hn, an["hn_ref"], 1, an["neg"])):
        idx = np.asarray(idx).astype(np.int64)
        if not (idx[~valid] == -1).all():
            bad.append("%s: an invalid anchor has an index" % name)
        for a in np.flatnonzero(valid):
            j, r = idx[a], ref[a]
            if j < 0 or j >= len(s) or not mask[a, j]:
                bad.append("%s[%d] = %d is no candidate" % (name, a, j))
            elif j != r and (not an["sel_amb"][a, col] or abs(s[a, j] - s[a, r]) > bs[a, j] + bs[a, r]):
                bad.append("%s[%d] = %d, the reference takes %d (s %r against %r)" % (name, a, j, r, s[a, j], s[a, r]))
    return bad


def ratios(out, an, grad_scale=1.0):
    """max |out - reference| / bound per output (each <= 1 inside the bounds); ``out``: loss, share and (optionally) demb; ``an``: the
    analysis evaluated with out's indices."""
    b = an["bounds"]
    w = {"loss": abs(out["loss"] - an["loss"]) / b["loss"], "share": abs(out["share"] - an["share"]) / b["share"]}
    if out.get("demb") is not None:
        w["demb"] = float((np.abs(np.asarray(out["demb"], dtype=np.float64) / grad_scale - an["demb"]) / b["demb"]).max())
    return w


def check(out, emb, labels, mining, soft, margin, grad_scale=1.0):
    """Both stages for a result ``out`` (hp, hn, loss, share[, demb]): (complaints about the selections, ratios, the analysis)."""
    an = analyse(emb, labels, mining, soft, margin, out["hp"], out["hn"])
    bad = admissible(out["hp"], out["hn"], an)
    if bad:   # indices that are no candidates cannot be evaluated
        return bad, {}, an
    return bad, ratios(out, an, grad_scale), an


# ---- the same loss in torch (autograd) -----------------------------------------------------------------------------------------
def triplet_loss_torch(e, labels, mining, soft, margin, hp=None, hn=None):
    """The float64 loss on a torch tensor of embeddings (differentiable); the selections (given, or the reference's) and A constant."""
    pos, neg = masks(labels)
    diff = e[:, None, :] - e[None, :, :]
    s = (diff * diff).sum(-1)
    ok = s > 0
    d = torch.where(ok, torch.sqrt(torch.where(ok, s, torch.ones_like(s))), torch.zeros_like(s))   # d = 0 with no gradient at s = 0
    sn = s.detach().numpy()
    hp_ref, hn_ref, valid = select(sn, pos, neg)
    hp = hp_ref if hp is None else np.asarray(hp)
    hn = hn_ref if hn is None else np.asarray(hn)
    rows = np.flatnonzero(valid)
    m = 0.0 if soft else margin
    term = torch.nn.functional.softplus if soft else torch.relu
    if len(rows) == 0:
        return (e * 0).sum()
    if mining == HARD:
        x = m + d[rows, hp[rows]] - d[rows, hn[rows]]
        return term(x).sum() / len(rows)
    a, p, n = (np.concatenate(v) for v in zip(*[(np.full(pos[r].sum() * neg[r].sum(), r), np.repeat(np.flatnonzero(pos[r]), neg[r].sum()),
                                                  np.tile(np.flatnonzero(neg[r]), pos[r].sum())) for r in rows]))
    x = m + d[a, p] - d[a, n]
    return term(x).sum() / (len(x) if soft else max(1, int((x.detach() > 0).sum())))


def autograd(emb, labels, mining, soft, margin):
    e = torch.tensor(np.asarray(emb), dtype=torch.float64, requires_grad=True)
    loss = triplet_loss_torch(e, labels, mining, soft, margin)
    (g,) = torch.autograd.grad(loss, e)
    return float(loss.detach()), g.numpy()


# ---- fp32 restatement ----------------------------------------------------------------------------------------------------------
WRONG = ("hardest_pos_min", "self_positive", "pos_grad_sign", "mean_over_n", "all_norm_t")


def _fsum(x, rev, axis=None):
    """An fp32 sum taken one element at a time, ascending or descending."""
    x = np.asarray(x, np.float32)
    if axis is None:
        x = x.reshape(-1)
        return np.cumsum(x[::-1] if rev else x, dtype=np.float32)[-1] if x.size else np.float32(0)
    x = np.flip(x, axis) if rev else x
    return np.cumsum(x, axis=axis, dtype=np.float32).take(-1, axis=axis)


def triplet_f32(emb, labels, mining, soft, margin, rev=False, grad_scale=1.0, wrong=None):
    """The same arithmetic in fp32 numpy, every sum one element at a time, ascending or (``rev``) descending: the E components, an
    anchor's triplets, the anchors, the rows j of the gradient.  ``wrong``: a deliberately wrong variant the bounds must catch --
    "hardest_pos_min" (the hardest positive taken as the minimum), "self_positive" (the anchor admitted as its own positive),
    "pos_grad_sign" (the positive row's gradient with the wrong sign), "mean_over_n" (HARD: the mean over N instead of V),
    "all_norm_t" (ALL hinge normalised by T instead of A).  Returns hp, hn, loss, share, demb."""
    f = np.float32
    e = np.asarray(emb, dtype=f)
    N, E = e.shape
    comps = range(E - 1, -1, -1) if rev else range(E)
    s = np.zeros((N, N), f)
    for t in comps:
        df = e[:, None, t] - e[None, :, t]
        s = s + df * df
    d = np.sqrt(s)
    pos, neg = masks(labels)
    if wrong == "self_positive":
        pos = pos | (np.eye(N, dtype=bool) & (np.asarray(labels) >= 0)[:, None])
    hp, hn, valid = select(s, pos, neg)
    if wrong == "hardest_pos_min":
        hp = np.where(valid, np.where(pos, s, np.inf).argmin(1), -1)
    rows = np.flatnonzero(valid)
    m = f(0.0 if soft else margin)
    W = np.zeros((N, N), f)
    sp = lambda x: (np.maximum(x, f(0)) + np.log1p(np.exp(-np.abs(x)))).astype(f)
    sg = lambda x: (np.where(x >= 0, f(1), np.exp(-np.abs(x))) / (f(1) + np.exp(-np.abs(x)))).astype(f)
    safe = lambda w, dd: np.where(dd > 0, w / np.where(dd > 0, dd, f(1)), f(0)).astype(f)
    if mining == HARD:
        dp, dn = d[rows, hp[rows]], d[rows, hn[rows]]
        x = (m + dp) - dn
        l = sp(x) if soft else np.maximum(x, f(0))
        g = sg(x) if soft else (x > 0).astype(f)
        W[rows, hp[rows]] = safe(g, dp)
        W[rows, hn[rows]] = safe(-g, dn)
        cnt, act = len(rows), int((x > 0).sum())
        norm = N if wrong == "mean_over_n" else max(1, cnt)
        lsum = _fsum(l, rev)
    else:
        parts, cnt, act = [], 0, 0
        for a in rows:
            Pa, Na = np.flatnonzero(pos[a]), np.flatnonzero(neg[a])
            dP, dN = d[a, Pa][:, None], d[a, Na][None, :]
            X = (m + dP) - dN
            G = sg(X) if soft else (X > 0).astype(f)
            parts.append(_fsum(sp(X) if soft else np.maximum(X, f(0)), rev))
            W[a, Pa] = safe(_fsum(G, rev, 1), dP[:, 0])
            W[a, Na] = safe(-_fsum(G, rev, 0), dN[0])
            cnt += X.size
            act += int((X > 0).sum())
        norm = max(1, cnt if soft or wrong == "all_norm_t" else act)
        lsum = _fsum(parts, rev)
    Wt = np.where(W > 0, -W, W).T if wrong == "pos_grad_sign" else W.T
    Msym = W + Wt
    acc = np.zeros((N, E), f)
    for j in (range(N - 1, -1, -1) if rev else range(N)):
        acc = acc + Msym[:, j:j + 1] * (e - e[j][None])
    return {"hp": hp, "hn": hn, "loss": float(lsum / f(norm)), "share": float(f(act) / f(cnt)) if cnt else 0.0,
            "demb": f(grad_scale) * (acc / f(norm))}


# ---- the training step in float64 ---------------------------------------------------------------------------------------------
def triplet_step_oracle(arch, p, state, x, labels, mining, soft, margin, hp=None, hn=None, drop_masks=None):
    """One triplet training step in float64, put together like tests/proto_refs.py's: O.encoder_forward (training, the whole batch one
    tower) + the loss above (with the given selections) + autograd + the moving-statistic updates + O.adam_step."""
    from collections import OrderedDict
    from oracle import voicemap_oracle as O
    names = O.param_names(arch, head=None)
    leaf = OrderedDict((nm, v.detach().clone().requires_grad_(nm in names)) for nm, v in p.items())
    c = {}
    e = O.encoder_forward(arch, leaf, x, True, drop_masks, c)
    loss = triplet_loss_torch(e, labels, mining, soft, margin, hp, hn)
    gl = torch.autograd.grad(loss, [leaf[nm] for nm in names])
    grads = OrderedDict((nm, g.detach()) for nm, g in zip(names, gl))
    new_p = OrderedDict((nm, v.detach().clone()) for nm, v in p.items())
    O.apply_moving_updates(new_p, (c,), len(arch.blocks), arch.bn_eps, arch.bn_momentum, True, "fresh")
    if state is not None:
        tr = O.adam_step(state, OrderedDict((nm, new_p[nm]) for nm in names), grads)
        for nm in names:
            new_p[nm] = tr[nm]
    return {"loss": float(loss.detach()), "e": e.detach(), "grads": grads, "params": new_p}
