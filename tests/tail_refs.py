"""Reference helpers of the step-tail tests (tests/test_gpu_step_tail.py on the device, tests/test_step_tail_refs_cpu.py on the
host): sizes and loop edges read from the kernels, float64 / float32 reference arithmetic, derived error bounds.  Pure numpy / torch:
nothing here touches the HIP library or a GPU."""
import math

import numpy as np
import torch

from oracle import voicemap_oracle as O

U32 = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
U64 = 2.0 ** -53

# ---- csrc/optim.hip ------------------------------------------------------------------------------------------
SQ_BLOCKS = 256
S = SQ_BLOCKS * 256         # elements one pass of sqnorm_partial_kernel's grid covers; its main loop takes 8 passes at a time

CFG_A_BLOCKS = [(32, 128, 4), (3, 256, 2), (3, 384, 2), (3, 512, 2)]   # bench.py: F = 128, E = 64, uniform_euclidean head
CFG_A_E = 64


def n_cfg_a():
    """Length of the flat parameter buffer of the bench configuration (HipEncoderEngine.n_flat), from the layout the engine uses."""
    from voicemap_amd.engine import flat_layout
    return flat_layout(CFG_A_BLOCKS, CFG_A_E, "uniform_euclidean")[2]


def n_cfg_a_from_architecture():
    """The same number from the architecture alone: Keras trainable tensors, each padded to 64 elements."""
    al = lambda n: (n + 63) // 64 * 64
    n, cin = 0, 1
    for k, c, _ in CFG_A_BLOCKS:
        n += al(k * cin * c) + 3 * al(c)      # kernel, bias, gamma, beta
        cin = c
    return n + al(cin * CFG_A_E) + al(CFG_A_E) + al(1) + al(1)


def sqnorm_sizes():
    return [1, 255, 256, 257, S - 1, S, S + 1, 7 * S, 7 * S + 1, 8 * S - 1, 8 * S, 8 * S + 1, 16 * S + 12345, n_cfg_a(), 3 * 8 * S + 7]


def hot_indices(n):
    """0, n - 1 and every index within one of a multiple of S, 7S or 8S that is < n."""
    out = {0, n - 1}
    for step in (S, 7 * S, 8 * S):
        for k in range(step, n + 2, step):
            out.update(j for j in (k - 1, k, k + 1) if 0 <= j < n)
    return sorted(out)


def graded_gradient(rng, n):
    """N(0, 1) x 10^(-3..0), the decade changing every 1000 elements: the sum is not dominated by one region of the buffer."""
    dec = 10.0 ** -((np.arange(n) // 1000) % 4).astype(np.float64)
    return (rng.standard_normal(n) * dec).astype(np.float32)


# ---- Adam ------------------------------------------------------------------------------------------------------
B1, B2, EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-7))   # what the kernel receives (fp32 scalars)


def lr_t(t, lr=1e-3):
    return lr * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)


def adam_state(iterations, m=None, v=None, clipnorm=1.0):
    st = O.AdamState(beta_1=B1, beta_2=B2, epsilon=EPS, clipnorm=clipnorm, iterations=iterations)
    if m is not None:
        st.m["w"], st.v["w"] = torch.tensor(m, dtype=torch.float64), torch.tensor(v, dtype=torch.float64)
    return st


def adam_oracle(st, p, g):
    """One O.adam_step in float64 on flat arrays; returns (p, m, v) as numpy float64 and advances st."""
    out = O.adam_step(st, {"w": torch.as_tensor(np.asarray(p), dtype=torch.float64)}, {"w": torch.as_tensor(np.asarray(g), dtype=torch.float64)})["w"]
    return out.numpy(), st.m["w"].numpy(), st.v["w"].numpy()


def adam_step_f32(p, g, m, v, t, clipnorm=1.0):
    """The reference arithmetic: the same update in float32 numpy (the norm summed in float64 and rounded once, as Keras' float32 graph
    rounds it at least once)."""
    f = np.float32
    sq = f(np.sum(g.astype(np.float64) ** 2))
    if clipnorm and clipnorm > 0:
        norm = np.sqrt(sq)
        if norm >= f(clipnorm):
            g = g * (f(clipnorm) / norm)
    b1, b2 = f(B1), f(B2)
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * g * g
    p = p - f(lr_t(t)) * m / (np.sqrt(v) + f(EPS))
    return p.astype(f), m.astype(f), v.astype(f)


def adam_m_bound(m0, g_scaled, roundings=4):
    """|m - m_ref| per element: b1 * m0, (1 - b1) * g and their sum are three fp32 roundings of at most 2^-24 of the larger magnitude
    each; 4 x 2^-24 of the sum of magnitudes covers them."""
    return roundings * U32 * (np.abs(B1 * np.asarray(m0, np.float64)) + np.abs((1.0 - B1) * np.asarray(g_scaled, np.float64)))


# ---- Dense -------------------------------------------------------------------------------------------------------
DENSE_KS = 16

DENSE_TRIPLES = [  # (rows, n_in, n_out): forward slices are ceil(n_in / 16) long, weight-gradient slices ceil(rows / 16); 8-wide main loops
    (1, 1, 1), (1, 512, 64), (1, 500, 1172), (7, 5, 33), (7, 113, 1), (16, 112, 63), (16, 512, 1172), (127, 113, 64), (127, 200, 65),
    (128, 128, 65), (128, 5, 251), (129, 200, 128), (129, 500, 63), (256, 512, 64), (256, 500, 251), (256, 1, 128), (1000, 512, 64),
    (1000, 128, 33), (1000, 113, 1), (10, 72, 33)]


def dot_bound(k, absprod):
    """Worst-case error of an fp32 dot product of length k in any summation order, plus one more rounding for the bias / final add:
    (k + 2) x 2^-24 x sum |x||w| (Higham, Accuracy and Stability, eq. 3.5: gamma_k <= k u / (1 - k u); the +2 absorbs the denominator
    for k u << 1 and the bias add)."""
    return (k + 2) * U32 * np.asarray(absprod, dtype=np.float64)


def dense_slices(n, ks=DENSE_KS):
    """(lo, hi) of each of the ks reduction slices the dense kernels cut a length-n reduction into."""
    per = (n + ks - 1) // ks
    return [(min(n, q * per), min(n, q * per + per)) for q in range(ks)]


# ---- siamese head ------------------------------------------------------------------------------------------------
def pairs_with_chosen_a(rng, a, e, head, hw, hb):
    """Embeddings (2 * pairs, e) in float64 whose head pre-activation is a[b] for pair b.  uniform_euclidean: e2 = e1 + d u with
    |u| = 1, d = (a - hb) / hw (needs d >= 0); weighted_l1: e2 = e1 + s u with s = (a - hb) / sum_j hw_j |u_j|."""
    a = np.asarray(a, dtype=np.float64)
    pairs = a.size
    hw = np.asarray(hw, dtype=np.float64).ravel()
    hb = float(np.asarray(hb).ravel()[0])
    e1 = rng.normal(0, 0.4, (pairs, e))
    u = rng.standard_normal((pairs, e))
    u[np.abs(u) < 0.05] = 0.05        # no component so small that rounding e1 + d u to fp32 could flip its sign
    if head == "uniform_euclidean":
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        d = (a - hb) / hw[0]
    else:
        d = (a - hb) / (np.abs(u) @ hw)
    assert (d >= 0).all(), "a below the head bias cannot be reached with a positive head weight"
    return np.concatenate([e1, e1 + d[:, None] * u])


def head_oracle(emb, hw, hb, y, head, loss, dtype=torch.float64):
    """O.siamese_head + the loss, per pair and with gradients: dict of numpy arrays (pred, loss per pair, mean loss, accuracy,
    demb, grad_hw, grad_hb, dlda = d mean-loss / d pre-activation per pair)."""
    pairs = len(y)
    et = torch.tensor(np.asarray(emb), dtype=dtype, requires_grad=True)
    prm = {"head.kernel": torch.tensor(np.asarray(hw), dtype=dtype, requires_grad=True),
           "head.bias": torch.tensor(np.asarray(hb), dtype=dtype, requires_grad=True)}
    pr = O.siamese_head(prm, et[:pairs], et[pairs:], head)
    yt = torch.tensor(np.asarray(y), dtype=dtype)[:, None]
    fn = O.contrastive_loss if loss == "contrastive" else O.binary_crossentropy
    per = torch.stack([fn(yt[b:b + 1], pr[b:b + 1]) for b in range(pairs)])
    lo = fn(yt, pr)
    ge, gw, gb = torch.autograd.grad(lo, [et, prm["head.kernel"], prm["head.bias"]])
    # d loss / d a through the loss alone (the head bias enters a with weight 1, so a one-pair loss differentiated by the bias is dL/da)
    dlda = np.zeros(pairs)
    for b in range(pairs):
        pb = pr[b:b + 1].detach().clone().requires_grad_(True)
        (gp,) = torch.autograd.grad(fn(yt[b:b + 1], pb), [pb])
        pv = float(pb.detach())
        dlda[b] = float(gp) * pv * (1.0 - pv) / pairs
    return {"pred": pr.detach().numpy()[:, 0].astype(np.float64), "loss_pair": per.detach().numpy().astype(np.float64), "loss": float(lo.detach()),
            "acc": float(O.binary_accuracy(yt, pr)), "demb": ge.numpy().astype(np.float64), "ghw": gw.numpy().ravel().astype(np.float64),
            "ghb": gb.numpy().astype(np.float64), "dlda": dlda}


def bce_pair_f32(p32, y):
    """O.binary_crossentropy in float32, one value per pair: what a float32 graph (the reference, and the kernel) computes at the clip."""
    pt = torch.tensor(np.asarray(p32, dtype=np.float32))
    yt = torch.tensor(np.asarray(y, dtype=np.float32))
    return np.array([float(O.binary_crossentropy(yt[b:b + 1], pt[b:b + 1])) for b in range(len(pt))], dtype=np.float64)


# ---- slab_sum (csrc/reduce.hip) -------------------------------------------------------------------------------------
SLAB_RCH = 16
C1_K = 32                   # taps of the first convolution: vm_conv1_wgrad sums n_windows slabs of C1_K * F elements


def slab_regime(slabs, nel):
    """slab_sum's dispatch restated: ("single", 1) for one launch, ("two-stage", partial rows, slabs per partial row, empty rows)."""
    blocks = -(-nel // 256)
    rch = -(-2048 // blocks)
    rch = min(rch, slabs // 4, SLAB_RCH)
    if slabs <= 64 and blocks >= 256:
        rch = 1
    if rch <= 1:
        return ("single", 1)
    per = -(-slabs // rch)
    empty = sum(1 for y in range(rch) if y * per >= slabs)
    return ("two-stage", rch, per, empty)


CONV1_WGRAD_SLABS_F8 = [1, 3, 4, 7, 8, 9, 31, 32, 33, 64, 65, 67, 130, 1000]
CONV1_WGRAD_SLABS_F2048 = [1, 4, 5, 7, 64, 65]

# ---- column sums ---------------------------------------------------------------------------------------------------
COLSUM_ROWS = [1, 31, 32, 33, 511, 512, 513, 2049, 131072]
COLSUM_C = [8, 32, 64, 96, 136, 512]


def cancelling_columns(rng, rows, c):
    """N(0, 1) with one +1e4 / -1e4 pair per column (when there are two rows to hold it): the column sums are O(sqrt(rows)) next to
    partial sums of 1e4, so accumulating in fp32 loses what float64 keeps."""
    x = rng.standard_normal((rows, c), dtype=np.float32)
    if rows >= 2:
        i = rng.integers(0, rows, c)
        j = (i + 1 + rng.integers(0, rows - 1, c)) % rows
        x[i, np.arange(c)] = 1e4
        x[j, np.arange(c)] = -1e4
    return x


def colsum_bound(x64_abs_sum, ref, rows):
    """The device adds float64 and rounds once to fp32: 2^-24 |ref| + rows 2^-53 sum |x|."""
    return U32 * np.abs(ref) + rows * U64 * x64_abs_sum
