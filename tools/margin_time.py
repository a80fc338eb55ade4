"""Times the classifier's training step under the margin softmax against the softmax classifier's step at the bench configuration,
in one process.

  python tools/margin_time.py [--windows 256] [--classes 1172] [--steps 40] [--blocks 9] [--warmup 8] [--out FILE]

cfg-A (filters 128, embedding 64, dropout 0), f16 storage, `windows` raw 3 s int16 windows resident on the device, decimated and
whitened on the GPU, `classes` = 1172 (the speakers of train-clean-100 + 360).  Both steps run the SAME one-tower encoder work over
the same windows (engine.train_step_resident: replayed from the third step on) and hold the same head parameters; they differ in the
head: vm_margin_softmax (additive angular, margin 0.2, scale 30; one entry point, three launches) against vm_dense_fwd +
vm_softmax_cce + vm_dense_bwd.  HIP events around blocks of `steps` steps, the two kinds of block interleaved (A B A B ...), medians
over `blocks` blocks each; the head launches alone are timed the same way on the embeddings the last step left.  The two heads compute
different losses: the figures are a record, not a comparison either has to win.  Prints one JSON line (and writes it, with a readable
summary, to --out)."""
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
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--classes", type=int, default=1172)
    ap.add_argument("--kind", type=int, default=2)
    ap.add_argument("--margin", type=float, default=0.2)
    ap.add_argument("--scale", type=float, default=30.0)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    N, S = a.windows, a.classes
    raw_len = int(16000 * a.seconds)
    g = torch.Generator(device="cuda").manual_seed(0)
    raw = (torch.randn(N, raw_len, device="cuda", generator=g) * 0.05 * 32767).clamp(-32767, 32767).to(torch.int16)
    y = torch.as_tensor(np.random.default_rng(0).integers(0, S, N).astype(np.int32)).cuda()
    # one engine per step kind, the same seed: each records its own program
    eng = {nm: HipEncoderEngine(CFG_A, 64, dropout=0.0, head="classifier", num_classes=S, dtype=a.dtype, seed=1) for nm in ("margin", "softmax")}
    l0 = (raw_len + 3) // 4
    pl = {nm: e.plan(N, l0, True) for nm, e in eng.items()}
    loss = {"margin": ("margin", a.kind, a.margin, a.scale), "softmax": None}
    eng["margin"]._margin_bufs(pl["margin"])

    def step(nm):
        return lambda: eng[nm].train_step_resident(pl[nm], N, y, loss=loss[nm], raw=raw, drop_masks=None, input_ready=True)

    names = {"margin": "margin_softmax_step", "softmax": "softmax_classifier_step"}
    t = interleaved({names[nm]: step(nm) for nm in ("margin", "softmax")}, a.steps, a.blocks, a.warmup)
    replayed = {names[nm]: len(eng[nm]._programs.recorded()) for nm in eng}
    heads = {"margin_head_launches": lambda: eng["margin"].margin_head(pl["margin"], y, a.kind, a.margin, a.scale),
             "dense_softmax_dense_launches": lambda: eng["softmax"].classifier_head(pl["softmax"], y)}
    t.update(interleaved(heads, 200, a.blocks, 20))
    torch.cuda.synchronize()
    med = {nm: float(np.median(v)) for nm, v in t.items()}
    out = {"card": torch.cuda.get_device_name(0), "dtype": a.dtype, "windows": N, "classes": S, "seconds": a.seconds, "kind": a.kind,
           "margin": a.margin, "scale": a.scale, "steps_per_block": a.steps, "blocks": a.blocks, "warmup": a.warmup,
           "median_ms": med, "min_ms": {nm: float(min(v)) for nm, v in t.items()}, "max_ms": {nm: float(max(v)) for nm, v in t.items()},
           "recorded_programs": replayed,
           "step_ratio_margin_over_softmax": med["margin_softmax_step"] / med["softmax_classifier_step"],
           "head_ratio_margin_over_softmax": med["margin_head_launches"] / med["dense_softmax_dense_launches"],
           "skipped_steps": {names[nm]: eng[nm].skipped_steps() for nm in eng},
           "loss_scale": {names[nm]: eng[nm].loss_scale for nm in eng},
           "loss_and_accuracy": {names[nm]: [float(v) for v in pl[nm]["loss_acc"].cpu()] for nm in eng}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/margin_time.py: %s, %s storage, %d windows of %g s, %d classes; margin head kind %d, margin %g, scale %g\n"
                    % (out["card"], a.dtype, N, a.seconds, S, a.kind, a.margin, a.scale))
            f.write("medians over %d interleaved blocks of %d steps (head launches: blocks of 200 calls), ms [min .. max]\n" % (a.blocks, a.steps))
            for nm in t:
                f.write("  %-30s %.4f  [%.4f .. %.4f]\n" % (nm, med[nm], out["min_ms"][nm], out["max_ms"][nm]))
            f.write("margin step / softmax step: %.4f;  margin head / dense + softmax + dense: %.4f\n"
                    % (out["step_ratio_margin_over_softmax"], out["head_ratio_margin_over_softmax"]))
            f.write(line + "\n")


if __name__ == "__main__":
    main()
