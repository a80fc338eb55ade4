"""Times the PLDA back end (voicemap_amd/plda.py, csrc/plda.hip) and what score kind VM_SCORE_PLDA costs the all-pairs histogram pass.

  python tools/plda_time.py [--rows 104014] [--dim 64] [--speakers 921] [--repeats 10] [--warmup 2] [--other-lib PATH]
                            [--out profiles/plda_time.txt]

The cache: `rows` x `dim` fp32 rows of `speakers` speakers drawn from a seeded two-covariance model (the size of train-clean-360's
104 014 files under a 64-wide encoder).  Rows of the report:
  fit_plda               the whole fit -- two passes of vm_speaker_sums + vm_scatter_f64, two vm_plda_project calls, the host's
                         eigenproblems and 10 EM iterations -- host clock around the call, which ends in read-backs (a synchronise)
  vm_scatter_f64, vm_speaker_sums, vm_plda_project (stage 1, with length normalisation; stage 2, with the row term), project
                         the single calls between HIP events
  vm_pair_score_hist     ONE pass over all rows (one window of 4096 bins placed by verification.sampled_window) between HIP events:
                         VM_SCORE_PLDA on the projected rows (P = dim + 4) against VM_DIST_DOT, euclidean and cosine on the raw rows,
                         and VM_SCORE_PLDA on the rows of a model fitted with lda_dim = dim - 1 (P = dim: no further 64-component
                         stage), the kinds taken in turn inside every repeat
  --other-lib PATH       another build of libvoicemap_hip.so (the parent commit's) loaded beside this one: its euclidean and cosine
                         passes on the same rows, alternating with this build's inside every repeat, and the counts compared
Nothing here is a threshold: the file records what was seen."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from voicemap_amd import _lib, plda, verification as V  # noqa: E402
from voicemap_amd.retrieval import EmbeddingCache  # noqa: E402


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    ts = np.asarray(ts, dtype=np.float64)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def corpus(N, E, S, seed=0):
    """(rows (N, E) fp32, speaker codes): unit between-speaker covariance, within-speaker noise of standard deviation 3 in E / 8
    rotated directions and 0.5 in the rest, a mean away from the origin."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(E, E)))
    sd = np.where(np.arange(E) < max(1, E // 8), 3.0, 0.5)
    spk = np.sort(rng.integers(0, S, N))
    x = rng.normal(size=E) + rng.normal(size=(S, E))[spk] + (rng.normal(size=(N, E)) * sd) @ Q.T
    return x.astype(np.float32), spk


def hist_call(cdll, cache, kind, window, bins=4096):
    """() -> one vm_pair_score_hist pass of ``cdll`` over all rows; .hist holds the counts."""
    dev = cache.emb.device
    hist = torch.zeros(1, 2, bins + 3, dtype=torch.int64, device=dev)
    ws = torch.empty(cdll.vm_pair_score_hist_workspace_bytes(cache.n, cache.E) + 256, dtype=torch.uint8, device=dev)
    win = np.ascontiguousarray(np.asarray([window], dtype=np.int64))
    st = torch.cuda.current_stream(dev).cuda_stream

    def call():
        hist.zero_()
        rc = cdll.vm_pair_score_hist(cache.emb.data_ptr(), cache.speaker_dev.data_ptr(), cache.n, cache.E, kind, None, 0, cache.n,
                                     win.ctypes.data, 1, bins, hist.data_ptr(), ws.data_ptr(), st)
        assert rc == 0, rc
    call.hist, call.keep = hist, (ws, win)
    return call


def bind(path):
    """Another build of the library, with the two entry points this tool calls bound from this tree's header."""
    cdll = ctypes.CDLL(path)
    for name in ("vm_pair_score_hist", "vm_pair_score_hist_workspace_bytes"):
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return cdll


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=104014)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--speakers", type=int, default=921)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--other-lib", default="")
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert torch.cuda.is_available(), "plda_time.py measures on the GPU"
    lib = _lib.lib()
    N, E = a.rows, a.dim
    x, spk = corpus(N, E, a.speakers)
    raw = EmbeddingCache(torch.from_numpy(x).cuda(), spk)
    lines = ["card: %s; %d rows x %d, %d speakers; %d repeats after %d warm-ups" % (torch.cuda.get_device_name(0), N, E, a.speakers, a.repeats,
                                                                                    a.warmup),
             "%-58s %12s %12s %12s" % ("", "median ms", "min ms", "max ms")]
    row = lambda name, t: lines.append("%-58s %12.3f %12.3f %12.3f" % ((name,) + stats(t)))

    # ---- the fit and the projection
    fits = []
    for k in range(a.warmup + min(a.repeats, 5)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model = plda.fit_plda(raw)
        torch.cuda.synchronize()
        if k >= a.warmup:
            fits.append((time.perf_counter() - t0) * 1e3)
    row("fit_plda (host clock; 2 x sums + scatter, 2 x project, EM)", fits)
    label, S = plda.dense_labels(spk)
    lab_t = torch.from_numpy(label).cuda()
    mean1, A1, mean2, A2, quad = model._on(raw.emb.device)
    from voicemap_amd.enrolment import speaker_sums
    y = plda.device_project(raw.emb, mean1, A1, model.length_norm)
    calls = (("vm_scatter_f64 (%d x %d)" % (N, E), lambda: plda.device_scatter(raw.emb, lab_t, mean1)),
             ("vm_speaker_sums (euclidean kind, %d speakers)" % S, lambda: speaker_sums(raw.emb, lab_t, S, _lib.VM_DIST_EUCLIDEAN)),
             ("vm_plda_project stage 1 (%d -> %d, length norm)" % (E, model.A1.shape[0]),
              lambda: plda.device_project(raw.emb, mean1, A1, model.length_norm)),
             ("vm_plda_project stage 2 (%d -> P = %d, row term)" % (model.A1.shape[0], model.P),
              lambda: plda.device_project(y, mean2, A2, False, quad, model.c0)),
             ("PldaModel.project (both calls)", lambda: model.project(raw.emb)))
    for name, fn in calls:
        for _ in range(a.warmup):
            fn()
        row(name, [events(fn) for _ in range(a.repeats)])
    proj = model.project(raw)

    # ---- one histogram pass per kind, the kinds in turn inside every repeat
    proj1 = plda.fit_plda(raw, lda_dim=E - 1).project(raw)   # one LDA direction fewer: the row term takes the freed column
    kinds = (("plda, P = %d" % proj.E, proj, _lib.VM_SCORE_PLDA), ("dot_product, E = %d" % E, raw, _lib.VM_DIST_DOT),
             ("euclidean, E = %d" % E, raw, _lib.VM_DIST_EUCLIDEAN), ("cosine, E = %d" % E, raw, _lib.VM_DIST_COSINE),
             ("plda, lda_dim = %d, P = %d" % (E - 1, proj1.E), proj1, _lib.VM_SCORE_PLDA))
    passes = []
    for name, cache, kind in kinds:
        lo, hi = V.bounds(cache, kind)
        window = V.sampled_window(cache, kind, None, lo, hi)
        passes.append(("vm_pair_score_hist, " + name, hist_call(lib.cdll, cache, kind, window), []))
    other = []
    if a.other_lib:
        cdll = bind(a.other_lib)
        for k in (2, 3):
            name, call, _ = passes[k]
            other.append((name + ", other build", hist_call(cdll, kinds[k][1], kinds[k][2], tuple(call.keep[1][0])), [], call))
    everything = [(n, c, t) for n, c, t in passes] + [(n, c, t) for n, c, t, _ in other]
    for _ in range(a.warmup):
        for _, call, _ in everything:
            call()
    for _ in range(a.repeats):
        for _, call, ts in everything:
            ts.append(events(call))
    for name, _, ts in everything:
        row(name, ts)
    med = {name: stats(ts)[0] for name, _, ts in everything}
    names = [n for n, _, _ in passes]
    lines.append("plda / dot_product: %.4f (the instruction count says %d / %d = %.4f plus the finishing add)"
                 % (med[names[0]] / med[names[1]], proj.E, E, proj.E / E))
    lines.append("plda with lda_dim = %d / dot_product: %.4f (P = %d: the same stages as the dot kind)" % (E - 1, med[names[4]] / med[names[1]], proj1.E))
    for name, call, _, mine in other:
        assert torch.equal(call.hist, mine.hist), "the two builds count differently"
        lines.append("%s / this build: %.4f (counts equal)" % (name, med[name] / med[name.replace(", other build", "")]))
    pairs = N * (N - 1) // 2
    lines.append("pairs per pass: %d; %.1f G pairs / s (plda)" % (pairs, pairs / med[names[0]] / 1e6))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
