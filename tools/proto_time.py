"""Times the prototypical training step against the classifier training step at the bench configuration, in one process.

  python tools/proto_time.py [--windows 256] [--k 64] [--n 2] [--classes 1172] [--steps 40] [--blocks 9] [--warmup 8] [--out FILE]

cfg-A (filters 128, embedding 64, dropout 0), f16 storage, `windows` raw 3 s int16 windows resident on the device, decimated and
whitened on the GPU.  Both steps run the SAME one-tower encoder work over the same windows (engine.train_step_resident: replayed from
the third step on); they differ in the head: vm_proto_loss (two launches, no parameters) on a (k, n, windows - k n) episode against
Dense(classes) + softmax CE + its backward (five launches, a (64, classes) weight matrix in the optimizer).  HIP events around blocks
of `steps` steps, the two kinds of block interleaved (A B A B ...), medians over `blocks` blocks each; the loss launches alone are
timed the same way on the embeddings the last step left.  Prints one JSON line (and writes it, with a readable summary, to --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from voicemap_amd.engine import HipEncoderEngine  # noqa: E402

CFG_A = [(32, 128, 4), (3, 256, 2), (3, 384, 2), (3, 512, 2)]


def block_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def interleaved(fns, steps, blocks, warmup):
    """{name: [ms per call of every block]}: all functions warmed up, then one block of each in turn, `blocks` times."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {nm: [] for nm in fns}
    for _ in range(blocks):
        for nm, fn in fns.items():
            out[nm].append(block_ms(fn, steps))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--windows", type=int, default=256)
    p.add_argument("--k", type=int, default=64)
    p.add_argument("--n", type=int, default=2)
    p.add_argument("--classes", type=int, default=1172)
    p.add_argument("--seconds", type=float, default=3.0)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--blocks", type=int, default=9)
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--dtype", default="f16")
    p.add_argument("--out", default="")
    a = p.parse_args()
    N, k, n = a.windows, a.k, a.n
    m = N - k * n
    raw_len = int(16000 * a.seconds)
    g = torch.Generator(device="cuda").manual_seed(0)
    raw = (torch.randn(N, raw_len, device="cuda", generator=g) * 0.05 * 32767).clamp(-32767, 32767).to(torch.int16)
    r = np.random.default_rng(0)
    y_proto = torch.as_tensor(r.integers(0, k, m).astype(np.int32)).cuda()
    y_cls = torch.as_tensor(r.integers(0, a.classes, N).astype(np.int32)).cuda()
    proto = HipEncoderEngine(CFG_A, 64, dropout=0.0, head=None, dtype=a.dtype, seed=1)
    cls = HipEncoderEngine(CFG_A, 64, dropout=0.0, head="classifier", num_classes=a.classes, dtype=a.dtype, seed=1)
    l0 = (raw_len + 3) // 4
    pp, pc = proto.plan(N, l0, True), cls.plan(N, l0, True)
    loss = ("prototypical", k, n, 1.0)

    steps = {"prototypical_step": lambda: proto.train_step_resident(pp, N, y_proto, loss=loss, raw=raw, drop_masks=None, input_ready=True),
             "classifier_step": lambda: cls.train_step_resident(pc, N, y_cls, loss=None, raw=raw, drop_masks=None, input_ready=True)}
    t = interleaved(steps, a.steps, a.blocks, a.warmup)
    replayed = {"prototypical_step": len(proto._programs.recorded()), "classifier_step": len(cls._programs.recorded())}
    heads = {"proto_loss_launches": lambda: proto.prototypical_head(pp, y_proto, k, n, 1.0),
             "classifier_head_launches": lambda: cls.classifier_head(pc, y_cls)}
    t.update(interleaved(heads, 200, a.blocks, 20))
    torch.cuda.synchronize()
    med = {nm: float(np.median(v)) for nm, v in t.items()}
    out = {"card": torch.cuda.get_device_name(0), "dtype": a.dtype, "windows": N, "seconds": a.seconds, "k": k, "n": n, "m": m,
           "classes": a.classes, "steps_per_block": a.steps, "blocks": a.blocks, "warmup": a.warmup,
           "median_ms": med, "min_ms": {nm: float(min(v)) for nm, v in t.items()}, "max_ms": {nm: float(max(v)) for nm, v in t.items()},
           "recorded_programs": replayed, "step_ratio_proto_over_classifier": med["prototypical_step"] / med["classifier_step"],
           "skipped_steps": {"prototypical_step": proto.skipped_steps(), "classifier_step": cls.skipped_steps()},
           "loss_scale": {"prototypical_step": proto.loss_scale, "classifier_step": cls.loss_scale},
           "proto_loss": float(pp["loss_acc"][0].item()), "proto_loss_finite": bool(torch.isfinite(pp["loss_acc"]).all().item())}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tools/proto_time.py: %s, %s storage, %d windows of %g s; episode (k, n, m) = (%d, %d, %d); classifier %d classes\n"
                    % (out["card"], a.dtype, N, a.seconds, k, n, m, a.classes))
            f.write("medians over %d interleaved blocks of %d steps (loss launches: blocks of 200 calls), ms [min .. max]\n" % (a.blocks, a.steps))
            for nm in t:
                f.write("  %-28s %.4f  [%.4f .. %.4f]\n" % (nm, med[nm], out["min_ms"][nm], out["max_ms"][nm]))
            f.write("prototypical step / classifier step = %.4f\n" % out["step_ratio_proto_over_classifier"])
            f.write(line + "\n")


if __name__ == "__main__":
    main()
