"""Times the triplet training step (batch hard and batch all) against the prototypical training step at the bench configuration, in
one process.

  python tools/triplet_time.py [--p 64] [--k 4] [--proto-k 64] [--proto-n 2] [--steps 40] [--blocks 9] [--warmup 8] [--out FILE]

cfg-A (filters 128, embedding 64, dropout 0), f16 storage, p * k raw 3 s int16 windows resident on the device, decimated and whitened
on the GPU.  All three steps run the SAME one-tower encoder work over the same windows (engine.train_step_resident: replayed from the
third step on); they differ in the head, each two launches without parameters: vm_triplet_loss on the windows as p speakers x k
utterances (hinge, margin 0.2) against vm_proto_loss on them as a (proto-k, proto-n, rest) episode.  HIP events around blocks of
`steps` steps, the three kinds of block interleaved (A B C A B C ...), medians over `blocks` blocks each; the loss launches alone are
timed the same way on the embeddings the last step left.  The yardstick is the prototypical step measured in the same run.  Prints
one JSON line (and writes it, with a readable summary, to --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.proto_time import CFG_A, interleaved  # noqa: E402
from voicemap_amd.engine import HipEncoderEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=64)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--proto-k", type=int, default=64)
    ap.add_argument("--proto-n", type=int, default=2)
    ap.add_argument("--margin", type=float, default=0.2)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    N = a.p * a.k
    pk, pn = a.proto_k, a.proto_n
    m = N - pk * pn
    raw_len = int(16000 * a.seconds)
    g = torch.Generator(device="cuda").manual_seed(0)
    raw = (torch.randn(N, raw_len, device="cuda", generator=g) * 0.05 * 32767).clamp(-32767, 32767).to(torch.int16)
    r = np.random.default_rng(0)
    y_proto = torch.as_tensor(r.integers(0, pk, m).astype(np.int32)).cuda()
    y_trip = torch.as_tensor(np.repeat(np.arange(a.p), a.k).astype(np.int32)).cuda()
    # one engine per step kind, the same seed: each records its own program
    eng = {nm: HipEncoderEngine(CFG_A, 64, dropout=0.0, head=None, dtype=a.dtype, seed=1) for nm in ("hard", "all", "proto")}
    l0 = (raw_len + 3) // 4
    pl = {nm: e.plan(N, l0, True) for nm, e in eng.items()}
    loss = {"hard": ("triplet", 0, 0, a.margin), "all": ("triplet", 1, 0, a.margin), "proto": ("prototypical", pk, pn, 1.0)}
    tgt = {"hard": y_trip, "all": y_trip, "proto": y_proto}
    for nm in ("hard", "all"):
        eng[nm]._triplet_bufs(pl[nm])

    def step(nm):
        return lambda: eng[nm].train_step_resident(pl[nm], N, tgt[nm], loss=loss[nm], raw=raw, drop_masks=None, input_ready=True)

    names = {"hard": "triplet_hard_step", "all": "triplet_all_step", "proto": "prototypical_step"}
    t = interleaved({names[nm]: step(nm) for nm in ("hard", "all", "proto")}, a.steps, a.blocks, a.warmup)
    replayed = {names[nm]: len(eng[nm]._programs.recorded()) for nm in eng}
    heads = {"triplet_hard_launches": lambda: eng["hard"].triplet_head(pl["hard"], y_trip, 0, 0, a.margin),
             "triplet_all_launches": lambda: eng["all"].triplet_head(pl["all"], y_trip, 1, 0, a.margin),
             "proto_loss_launches": lambda: eng["proto"].prototypical_head(pl["proto"], y_proto, pk, pn, 1.0)}
    t.update(interleaved(heads, 200, a.blocks, 20))
    torch.cuda.synchronize()
    med = {nm: float(np.median(v)) for nm, v in t.items()}
    out = {"card": torch.cuda.get_device_name(0), "dtype": a.dtype, "windows": N, "seconds": a.seconds, "p": a.p, "k": a.k,
           "margin": a.margin, "proto_episode": [pk, pn, m], "steps_per_block": a.steps, "blocks": a.blocks, "warmup": a.warmup,
           "median_ms": med, "min_ms": {nm: float(min(v)) for nm, v in t.items()}, "max_ms": {nm: float(max(v)) for nm, v in t.items()},
           "recorded_programs": replayed,
           "step_ratio_hard_over_proto": med["triplet_hard_step"] / med["prototypical_step"],
           "step_ratio_all_over_proto": med["triplet_all_step"] / med["prototypical_step"],
           "skipped_steps": {names[nm]: eng[nm].skipped_steps() for nm in eng},
           "loss_scale": {names[nm]: eng[nm].loss_scale for nm in eng},
           "loss_and_share": {names[nm]: [float(v) for v in pl[nm]["loss_acc"].cpu()] for nm in eng}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/triplet_time.py: %s, %s storage, %d windows of %g s as %d speakers x %d (hinge, margin %g); prototypical episode "
                    "(k, n, m) = (%d, %d, %d)\n" % (out["card"], a.dtype, N, a.seconds, a.p, a.k, a.margin, pk, pn, m))
            f.write("medians over %d interleaved blocks of %d steps (loss launches: blocks of 200 calls), ms [min .. max]\n" % (a.blocks, a.steps))
            for nm in t:
                f.write("  %-28s %.4f  [%.4f .. %.4f]\n" % (nm, med[nm], out["min_ms"][nm], out["max_ms"][nm]))
            f.write("triplet step / prototypical step: batch hard %.4f, batch all %.4f\n"
                    % (out["step_ratio_hard_over_proto"], out["step_ratio_all_over_proto"]))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
