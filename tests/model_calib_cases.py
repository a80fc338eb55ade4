"""Builders and guarded device calls for the calibration of speaker-model trials (vm_speaker_trial_calib_sums,
vm_plda_speaker_trial_calib_sums; voicemap_amd/enrolment.py), shared by test_model_calib_cpu.py and test_gpu_model_calib.py.

The device calls run with guard words around ``calib`` and around a workspace of exactly the queried size.  The reference scores of the
GPU tests are the device's own ``scores`` matrix of vm_[plda_]speaker_identify -- the header states that the calibration mode sums those
bits, and other test files hold that matrix to the numpy twins -- normalised, where there are statistics, by
``enrolment.normalise_trials_numpy``: only the new epilogue and its reduction are under test."""
import numpy as np
import torch

GUARD_D, GUARD_F = -1.2345e300, -7.75e30
EUC, COS, DOT = 0, 1, 2
# moderate; a = 0; saturating (|z| > 750: exp underflows); |z| about 40 -- the triples of test_gpu_calibration.py
ABT = [(-0.3, 1.0, -0.5), (0.0, 0.3, 0.7), (-0.25, 1000.0, 0.0), (-0.01, 40.0, 1.5)]
EXACT = [0, 1, 3, 4, 5, 6, 7]   # the columns of a (2, 8) result that are exact on the integer plant: everything but L


def cuda(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


# ---- host cases --------------------------------------------------------------------------------------------------------------------
def literal_sums(scores, trial, q_label, a, b, tau, magnitude=False):
    """The statement of the header as a literal double loop over (m, s), in Python floats (float64): the (2, 8) sums.  ``magnitude``:
    the sums of the terms' absolute values instead (what a rounding bound on a sum in another order is relative to)."""
    import math
    out = np.zeros((2, 8))
    s32 = np.asarray(scores, dtype=np.float32)
    M, S = s32.shape
    for m in range(M):
        for s in range(S):
            if not trial[m, s]:
                continue
            c = 0 if s == int(q_label[m]) else 1
            x = float(s32[m, s])
            if not math.isfinite(x):
                out[c, 1] += 1
                continue
            z = a * x + b + tau
            t = -z if c == 0 else z
            e = math.exp(-abs(t))
            d = 1.0 + e
            w = e / (d * d)
            p = 1.0 / d if t >= 0.0 else e / d
            terms = (1, 0, max(t, 0.0) + math.log1p(e), p, p * x, w, w * x, (w * x) * x)
            out[c] += [abs(v) for v in terms] if magnitude else terms
    return out


def small_corpus(seed=0, E=5):
    """(emb, label, q, q_label, S): 6 speakers of 3, 0, 1, 4, 2, 1 rows -- a speaker with no rows and two single-file speakers (no own
    trial under leave-one-out) -- queried by the enrolled rows themselves; the queries keep their labels but for one set to -1."""
    r = np.random.default_rng(seed)
    sizes = [3, 0, 1, 4, 2, 1]
    label = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    emb = (r.normal(0, 1, (len(sizes), E))[label] + r.normal(0, 0.7, (len(label), E))).astype(np.float32)
    q_label = label.copy()
    q_label[1] = -1
    return emb, label, emb.copy(), q_label, len(sizes)


def plant(M, S, E, seed, one_speaker=False):
    """The integer plant (euclidean kind): every row has ONE active component, e0 = seed % E, holding 12 x a small integer, so with
    speakers of 1 - 4 rows every mean (and every leave-one-out mean of 1 - 3 rows) is an integer, every score |12 k - mean| a small
    integer, and at a = b = tau = 0 p = 1/2, w = 1/4: the counts and P0, P1, W0, W1, W2 are exact in float64 in any order.
    Speakers 0 .. S - 1 get (s % 4) + 1 rows but speaker S - 2 (where S >= 3), which gets none, and speaker 0, which gets ONE (no own
    trial under leave-one-out).  Queries: the enrolled rows first (their own labels), then foreign rows; one query is labelled -1 and
    one S + 3 (neither has a target trial).  ``one_speaker``: every enrolled row -- at most 4 -- and every query label is speaker 0."""
    r = np.random.default_rng(seed)
    sizes = [(s % 4) + 1 for s in range(S)]
    sizes[0] = 1
    if S >= 3:
        sizes[S - 2] = 0
    if one_speaker:
        sizes = [4] + [0] * (S - 1)
    label = np.repeat(np.arange(S), sizes).astype(np.int32)
    e0 = seed % E
    emb = np.zeros((len(label), E), np.float32)
    emb[:, e0] = 12 * r.integers(-5, 6, len(label))
    q = np.zeros((M, E), np.float32)
    q[:, e0] = 12 * r.integers(-5, 6, M)
    q_label = r.integers(0, S, M).astype(np.int32)
    k = min(M, len(label))
    perm = r.permutation(len(label))[:k]
    q[:k], q_label[:k] = emb[perm], label[perm]
    if one_speaker:
        q_label[:] = 0
    if M >= 3:
        q_label[M - 1], q_label[M - 2] = -1, S + 3
    return emb, label, q, q_label


def clusters(N, E, speakers, seed, noise=1.0):
    r = np.random.default_rng(seed)
    spk = r.integers(0, speakers, N).astype(np.int32)
    emb = r.normal(0, 1, (speakers, E))[spk] + r.normal(0, noise, (N, E))
    return emb.astype(np.float32), spk


def plda_case(D, seed, N=300, speakers=37, noise=1.0):
    """(model, PLDA-space rows (N, P) fp32, labels): a two-covariance model drawn at random (tests/plda_cases.py) and rows drawn from
    its own covariances -- the within-speaker part scaled by ``noise``, so that speakers can be made to overlap -- projected on the
    host."""
    from tests import plda_cases as PC
    from voicemap_amd import plda as PL
    rng = np.random.default_rng(seed)
    mu, Phi_b, Phi_w = rng.normal(size=D), PC.random_spd(rng, D), PC.random_spd(rng, D)
    spk = rng.integers(0, speakers, N).astype(np.int32)
    Lb, Lw = np.linalg.cholesky(Phi_b), np.linalg.cholesky(Phi_w)
    x = mu[None, :] + (rng.normal(size=(speakers, D)) @ Lb.T)[spk] + noise * (rng.normal(size=(N, D)) @ Lw.T)
    model = PL.PldaModel.from_covariances(mu, Phi_b, Phi_w)
    return model, np.ascontiguousarray(model.project_numpy(x.astype(np.float32)), dtype=np.float32), spk


def synthetic_stats(scores, trial, loo, seed):
    """Six statistics arrays around the distribution of the trial scores (they need not come from a cohort): mu near the median,
    1 / sigma within a factor 2 of the scores' own; the own pair only under leave-one-out."""
    r = np.random.default_rng(seed)
    M, S = scores.shape
    s = scores[trial].astype(np.float64)
    med, sd = float(np.median(s)), float(s.std())
    mu = lambda n: (med + r.normal(0, 0.1 * sd, n)).astype(np.float32)
    rs = lambda n: (1.0 / (sd * r.uniform(0.5, 2.0, n))).astype(np.float32)
    return (mu(M), rs(M), mu(S), rs(S)) + ((mu(M), rs(M)) if loo else (None, None))


def target_mask(q_label, S):
    return np.arange(S)[None, :] == np.asarray(q_label).reshape(-1, 1)


# ---- guarded device calls ------------------------------------------------------------------------------------------------------------
def _guarded(name, ws_query, ws_dims, head, tail, abt, stats, keep):
    """One call of a ``*_trial_calib_sums`` entry point: ``head`` the arguments up to leave_one_out, the six statistics (host arrays or
    None), (a, b, tau), then the guarded ``calib`` and workspace."""
    from tests.gpu_util import L, stream
    sd = [None if t is None else cuda(np.asarray(t, np.float32)) for t in (stats if stats is not None else (None,) * 6)]
    out = torch.full((4 + 16 + 4,), GUARD_D, dtype=torch.float64, device="cuda")
    words = (L().query(ws_query, *ws_dims) + 3) // 4
    ws = torch.full((8 + words + 8,), GUARD_F, dtype=torch.float32, device="cuda")
    L().call(name, *head, *tail, *[None if t is None else t.data_ptr() for t in sd], float(abt[0]), float(abt[1]), float(abt[2]),
             out.data_ptr() + 32, ws.data_ptr() + 32, stream())
    torch.cuda.synchronize()
    o, g = out.cpu().numpy(), ws.cpu().numpy()
    del keep
    assert np.all(o[:4] == GUARD_D) and np.all(o[20:] == GUARD_D), "words around calib were written"
    assert np.all(g[:8] == np.float32(GUARD_F)) and np.all(g[8 + words:] == np.float32(GUARD_F)), "words around the workspace were written"
    return o[4:20].reshape(2, 8).copy()


def geo_sums(q, q_label, sums, msum, count, kind, loo, abt=(0.0, 0.0, 0.0), stats=None, M=None):
    """vm_speaker_trial_calib_sums: host rows / labels, device sums / msum / count -> (2, 8) numpy.  ``M``: fewer rows than ``q`` holds."""
    M, E = q.shape[0] if M is None else M, q.shape[1]
    S = int(count.shape[0])
    qd, ld = cuda(q, torch.float32), cuda(q_label, torch.int32)
    return _guarded("vm_speaker_trial_calib_sums", "vm_speaker_trial_calib_sums_workspace_bytes", (M, E, S),
                    (qd.data_ptr(), ld.data_ptr(), M, E, sums.data_ptr(), msum.data_ptr(), count.data_ptr(), S, kind), (int(loo),), abt, stats,
                    (qd, ld))


def plda_sums(q, q_label, sums, count, tables, loo, abt=(0.0, 0.0, 0.0), stats=None):
    """vm_plda_speaker_trial_calib_sums: host PLDA-space rows / labels, device sums / count / tables -> (2, 8) numpy."""
    M, P = q.shape
    S, D, n_max = int(count.shape[0]), int(tables["G"].shape[0]), int(tables["C"].shape[0]) - 1
    qd, ld = cuda(q, torch.float32), cuda(q_label, torch.int32)
    return _guarded("vm_plda_speaker_trial_calib_sums", "vm_plda_speaker_trial_calib_sums_workspace_bytes", (M, D, S),
                    (qd.data_ptr(), ld.data_ptr(), M, P, D, sums.data_ptr(), count.data_ptr(), S) + tuple(tables[k].data_ptr() for k in
                                                                                                        ("A", "beta", "C", "G")) + (n_max,),
                    (int(loo),), abt, stats, (qd, ld))


def device_scores(q, q_label, sums, msum, count, kind, loo, tables=None):
    """((M, S) fp32 scores of vm_[plda_]speaker_identify, its trial mask): NaN exactly where the cell is no trial -- a trial whose score
    is NaN would be missed here, so callers that plant NaN rows take the mask from ``trial_mask``."""
    from voicemap_amd import enrolment as EN
    out = EN._identify(cuda(q, torch.float32), cuda(q_label, torch.int32), sums, msum, count, kind, tables, loo, return_scores=True)
    s = out["scores"].cpu().numpy()
    s.setflags(write=False)
    return s, ~np.isnan(s)


def trial_mask(q_label, count, loo, n_max=None):
    """The (M, S) trial mask of the header from the counts alone: a model exists iff it has n > 0 rows (PLDA: 1 <= n <= n_max), n the
    count less one in the own cell under leave-one-out."""
    count = np.asarray(count).astype(np.int64)
    S = len(count)
    n = np.broadcast_to(count[None, :], (len(q_label), S)).copy()
    if loo:
        n -= target_mask(q_label, S)
    return (n >= 1) & (n <= (np.iinfo(np.int64).max if n_max is None else n_max))
