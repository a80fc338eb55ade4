"""Times vm_vbx (csrc/vbx.hip) beside vm_ahc (csrc/cluster.hip) on the same rows.

  python tools/vbx_time.py [--recordings 64] [--windows 1024] [--dim 63] [--models 16] [--iters 10] [--repeats 10] [--warmup 2]
                           [--out profiles/vbx_time.txt]

The batch: `recordings` recordings of `windows` windows each, rows of width P = 4 ceil((dim + 1) / 4) drawn around 2 to 4 seeded centres
per recording (tools/ahc_time.py's), a random psi in [0.1, 10].  Rows, whole calls between HIP events, one call per timing, after
warm-ups: median and spread
  vm_ahc            PLDA score kind, average linkage, merged down to `models` clusters per recording
  vm_vbx            `models` speakers per recording from that clustering's labels, `iters` iterations with the stop rule off (epsilon =
                    -inf: every recording runs them all), one chain per recording
  vm_vbx at D = 1   the same call reading one column: what is left is the forward-backward, the priors and the per-row passes, nothing
                    that scales with D -- its share of the full call is quoted as the sequential step's share (an upper estimate: the
                    exp pass and the row maxima are in it too)
Nothing here is a threshold: the file records what was seen.  A call that fails ends the run: nothing is launched after it."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.ahc_time import batch, timed  # noqa: E402
from voicemap_amd import _lib  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--recordings", type=int, default=64)
    p.add_argument("--windows", type=int, default=1024)
    p.add_argument("--dim", type=int, default=63)
    p.add_argument("--models", type=int, default=16)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert torch.cuda.is_available(), "vbx_time.py measures on the GPU"
    lib = _lib.lib()
    R, n, D, K = a.recordings, a.windows, a.dim, a.models
    P = 4 * ((D + 1 + 3) // 4)
    N, sq, em = R * n, R * n * n, R * n * K
    rows = torch.from_numpy(batch(R, n, P)).cuda()
    psi = np.exp(np.random.RandomState(1).uniform(np.log(0.1), np.log(10.0), D))
    mod = torch.from_numpy(np.concatenate([psi, np.sqrt(1.0 + 2.0 * psi), (1.0 + 2.0 * psi) / psi])).cuda()
    steps = np.arange(R + 1, dtype=np.int64)
    tab = torch.from_numpy(np.concatenate([steps * n, steps * n * n, steps * n * K])).cuda()
    row0, mat0, em0 = tab[:R + 1], tab[R + 1:2 * R + 2], tab[2 * R + 2:]
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device="cuda")
    f64 = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
    ma, mb, ms, lab, nc, out, run = i32(N), i32(N), i32(N), i32(N), i32(R), i32(N), i32(R)
    mh = torch.empty(N, dtype=torch.float32, device="cuda")
    gamma, pi, elbo = f64(em), f64(R * 64), f64(R * a.iters)
    target = torch.full((R,), K, dtype=torch.int32, device="cuda")
    ws_a = lib.workspace("vm_ahc_workspace_bytes", N, P, R, sq, device="cuda")
    ws_v = lib.workspace("vm_vbx_workspace_bytes", N, D, R, em, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    # lib.call raises on a failed call and torch raises on a failed synchronisation: either ends the run here, before the next launch
    def ahc():
        lib.call("vm_ahc", rows.data_ptr(), N, P, row0.data_ptr(), mat0.data_ptr(), R, sq, _lib.VM_SCORE_PLDA, _lib._ENUMS["VM_LINK_AVERAGE"],
                 float("nan"), target.data_ptr(), ma.data_ptr(), mb.data_ptr(), mh.data_ptr(), ms.data_ptr(), lab.data_ptr(), nc.data_ptr(),
                 ws_a.data_ptr(), st)

    def vbx(d=D):
        lib.call("vm_vbx", rows.data_ptr(), N, P, d, row0.data_ptr(), em0.data_ptr(), R, em, nc.data_ptr(), lab.data_ptr(), None,
                 mod.data_ptr(), mod[D:].data_ptr(), mod[2 * D:].data_ptr(), 0.99, 0.3, 17.0, 5.0, float("-inf"), a.iters, None, None,
                 out.data_ptr(), gamma.data_ptr(), pi.data_ptr(), elbo.data_ptr(), run.data_ptr(), ws_v.data_ptr(), st)

    t_ahc = timed(ahc, a.repeats, a.warmup)
    assert int(nc.min().item()) == int(nc.max().item()) == K
    t_vbx = timed(vbx, a.repeats, a.warmup)
    runs = run.cpu().numpy()
    alive = float((pi.view(R, 64)[:, :K] > 1e-7).sum(1).double().mean().item())
    t_one = timed(lambda: vbx(1), a.repeats, a.warmup)
    runs_one = run.cpu().numpy()
    lines = ["card: %s; %d recordings x %d windows x P = %d (%d rows); vm_ahc: PLDA scores, average linkage down to %d clusters; vm_vbx: K = %d, "
             "D = %d, %d iterations (no stop), loop_prob 0.99, fa 0.3, fb 17; %d repeats after %d warm-ups"
             % (torch.cuda.get_device_name(0), R, n, P, N, K, K, D, a.iters, a.repeats, a.warmup),
             "%-36s %12s %12s %12s %16s" % ("", "median ms", "min ms", "max ms", "us / recording"),
             "%-36s %12.3f %12.3f %12.3f %16.1f" % (("vm_ahc",) + t_ahc + (t_ahc[0] * 1e3 / R,)),
             "%-36s %12.3f %12.3f %12.3f %16.1f" % (("vm_vbx",) + t_vbx + (t_vbx[0] * 1e3 / R,)),
             "%-36s %12.3f %12.3f %12.3f %16.1f" % (("vm_vbx at D = 1",) + t_one + (t_one[0] * 1e3 / R,)),
             "vm_vbx / vm_ahc (medians): %.3f" % (t_vbx[0] / t_ahc[0]),
             "the sequential step's share of vm_vbx (the D = 1 call over the full call, an upper estimate): %.1f %%; per iteration and "
             "row: %.3f us of %.3f us" % (100.0 * t_one[0] / t_vbx[0], t_one[0] * 1e3 / (a.iters * n), t_vbx[0] * 1e3 / (a.iters * n)),
             "speakers left with a prior above 1e-7 after %d iterations: %.2f of %d on average; iterations run: %d .. %d, at D = 1: %d .. %d (-2: a recording that degenerated)"
             % (a.iters, alive, K, int(runs.min()), int(runs.max()), int(runs_one.min()), int(runs_one.max()))]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
