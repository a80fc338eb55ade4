"""Times vm_reseg (csrc/reseg.hip) beside vm_ahc (csrc/cluster.hip) on the batch of tools/ahc_time.py.

  python tools/reseg_time.py [--recordings 256] [--windows 800] [--dim 64] [--models 4] [--iters 3] [--repeats 10] [--warmup 2]
                             [--out profiles/reseg_time.txt]

The batch: `recordings` recordings of `windows` windows each, embeddings of width `dim` drawn around 2 to 4 seeded centres per recording
(tools/ahc_time.py's).  Rows, whole calls between HIP events, one call per timing, after warm-ups: median and spread
  vm_ahc      cosine, average linkage, merged down to `models` clusters per recording
  vm_reseg    cosine, `models` models per recording from that clustering's labels, `iters` iterations, one chain per recording,
              emissions kept in the workspace
  vm_reseg, every tenth label moved
              the same call on labels of which every tenth row's is moved to the next cluster: more for the decode to undo
and the ratio of the first two.  The file also says how many decodes the recordings ran: a recording stops at its first unchanged
decode, so `iters` is a ceiling.
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
    p.add_argument("--recordings", type=int, default=256)
    p.add_argument("--windows", type=int, default=800)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--models", type=int, default=4)
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--switch-cost", type=float, default=0.1)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert torch.cuda.is_available(), "reseg_time.py measures on the GPU"
    lib = _lib.lib()
    R, n, E, K = a.recordings, a.windows, a.dim, a.models
    N, sq, em = R * n, R * n * n, R * n * K
    emb = torch.from_numpy(batch(R, n, E)).cuda()
    steps = np.arange(R + 1, dtype=np.int64)
    tab = torch.from_numpy(np.concatenate([steps * n, steps * n * n, steps * n * K])).cuda()
    row0, mat0, em0 = tab[:R + 1], tab[R + 1:2 * R + 2], tab[2 * R + 2:]
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device="cuda")
    ma, mb, ms, lab, nc, out, run, chg = i32(N), i32(N), i32(N), i32(N), i32(R), i32(N), i32(R), i32(R)
    mh = torch.empty(N, dtype=torch.float32, device="cuda")
    cost = torch.empty(R, dtype=torch.float64, device="cuda")
    target = torch.full((R,), K, dtype=torch.int32, device="cuda")
    ws_a = lib.workspace("vm_ahc_workspace_bytes", N, E, R, sq, device="cuda")
    ws_r = lib.workspace("vm_reseg_workspace_bytes", N, E, R, em, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    # lib.call raises on a failed call and torch raises on a failed synchronisation: either ends the run here, before the next launch
    def ahc():
        lib.call("vm_ahc", emb.data_ptr(), N, E, row0.data_ptr(), mat0.data_ptr(), R, sq, _lib.DIST["cosine"], _lib._ENUMS["VM_LINK_AVERAGE"],
                 float("nan"), target.data_ptr(), ma.data_ptr(), mb.data_ptr(), mh.data_ptr(), ms.data_ptr(), lab.data_ptr(), nc.data_ptr(),
                 ws_a.data_ptr(), st)

    def reseg(lab=lab):
        lib.call("vm_reseg", emb.data_ptr(), N, E, row0.data_ptr(), em0.data_ptr(), R, em, nc.data_ptr(), lab.data_ptr(), None,
                 _lib.DIST["cosine"], a.switch_cost, a.iters, out.data_ptr(), cost.data_ptr(), run.data_ptr(), chg.data_ptr(), None,
                 ws_r.data_ptr(), st)

    t_ahc = timed(ahc, a.repeats, a.warmup)
    assert int(nc.min().item()) == int(nc.max().item()) == K
    t_res = timed(reseg, a.repeats, a.warmup)
    runs = run.cpu().numpy()
    assert runs.min() >= 1
    moved = float((out != lab).float().mean().item())
    spoiled = torch.where(torch.arange(N, device="cuda") % 10 == 0, (lab + 1) % K, lab).contiguous()
    t_sp = timed(lambda: reseg(spoiled), a.repeats, a.warmup)
    runs_sp = run.cpu().numpy()
    lines = ["card: %s; %d recordings x %d windows x E = %d (%d rows), cosine; vm_ahc: average linkage down to %d clusters; vm_reseg: K = %d, "
             "iters = %d, switch_cost = %g; %d repeats after %d warm-ups"
             % (torch.cuda.get_device_name(0), R, n, E, N, K, K, a.iters, a.switch_cost, a.repeats, a.warmup),
             "%-36s %12s %12s %12s %16s" % ("", "median ms", "min ms", "max ms", "us / recording"),
             "%-36s %12.3f %12.3f %12.3f %16.1f" % (("vm_ahc",) + t_ahc + (t_ahc[0] * 1e3 / R,)),
             "%-36s %12.3f %12.3f %12.3f %16.1f" % (("vm_reseg",) + t_res + (t_res[0] * 1e3 / R,)),
             "%-36s %12.3f %12.3f %12.3f %16.1f" % (("vm_reseg, every tenth label moved",) + t_sp + (t_sp[0] * 1e3 / R,)),
             "vm_reseg / vm_ahc (medians): %.3f" % (t_res[0] / t_ahc[0]),
             "decodes run per recording: min %d, mean %.2f, max %d; rows whose label the decode changed: %.2f %%"
             % (int(runs.min()), float(runs.mean()), int(runs.max()), 100.0 * moved),
             "with every tenth label moved: min %d, mean %.2f, max %d decodes" % (int(runs_sp.min()), float(runs_sp.mean()), int(runs_sp.max()))]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
