"""Times speaker identification and the model-trial histogram (csrc/enrol.hip) at train-clean-360's size against the same numbers from
torch in float64 on the same card.

  python tools/enrol_time.py [--rows 104014] [--speakers 921] [--dim 64] [--calls 20] [--warmup 5]

Ours: vm_speaker_identify (ranks, best, true scores; no score matrix) + vm_speaker_trial_hist (one 4096-bin pass), leave-one-out,
euclidean.  The yardstick: the prototype matrix, torch.cdist in float64, the own cell recomputed from sums - row, scores rounded to fp32,
the rank by comparison counts (no argsort), argmin, and the same 4096-bin class histogram by integer binning + bincount, in row blocks
that fit memory.  HIP events around `calls` calls after `warmup` warm-ups, one process.  Prints both times, their parts, the card and
the float64 rate of our two passes (M x S x E subtract + multiply-add pairs each)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from voicemap_amd import enrolment as EN  # noqa: E402
from voicemap_amd import verification as V  # noqa: E402


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=104014)
    p.add_argument("--speakers", type=int, default=921)
    p.add_argument("--dim", type=int, default=64)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--block", type=int, default=16384, help="rows per block of the torch yardstick")
    a = p.parse_args()
    N, S, E = a.rows, a.speakers, a.dim
    r = np.random.default_rng(0)
    label = np.concatenate([np.arange(S), r.integers(0, S, N - S)]).astype(np.int32)
    r.shuffle(label)
    emb = torch.as_tensor((r.normal(0, 1, (S, E))[label] + r.normal(0, 1.0, (N, E))).astype(np.float32)).cuda()
    lab = torch.as_tensor(label).cuda()
    t_sums = timed(lambda: EN.speaker_sums(emb, lab, S, 0), 3, 1)
    sums, msum, count = EN.speaker_sums(emb, lab, S, 0)
    win = [V.pass1_window(0.0, 24.0)]
    keep = {}

    def ours_identify():
        keep["id"] = EN.speaker_identify(emb, lab, sums, msum, count, 0, True)

    def ours_hist():
        keep["h"] = EN.speaker_trial_hist(emb, lab, sums, msum, count, 0, True, win, 4096)

    lo, sh = win[0]
    idx = torch.arange(S, device="cuda")[None, :]
    lab64 = lab.long()

    def torch_scores(b0, b1):
        q = emb[b0:b1].double()
        l = lab64[b0:b1]
        n = count.double()
        d = torch.cdist(q, sums / n[:, None])
        n1 = n[l] - 1
        own = torch.linalg.vector_norm(q - (sums[l] - q) / n1[:, None], dim=1)
        d[torch.arange(b1 - b0, device="cuda"), l] = own
        return d.float(), l

    def torch_identify():
        ranks, best = [], []
        for b0 in range(0, N, a.block):
            d, l = torch_scores(b0, min(N, b0 + a.block))
            t = d.gather(1, l[:, None])
            ranks.append(((d < t) | ((d == t) & (idx < l[:, None]))).sum(1))
            best.append(d.argmin(1))
        keep["tr"], keep["tb"] = torch.cat(ranks), torch.cat(best)

    def torch_hist():
        h = torch.zeros(2 * 4099, dtype=torch.int64, device="cuda")
        for b0 in range(0, N, a.block):
            d, l = torch_scores(b0, min(N, b0 + a.block))
            u = d.view(torch.int32).long() & 0xFFFFFFFF
            k = torch.where(u >= 0x80000000, u ^ 0xFFFFFFFF, u | 0x80000000)
            b = (k - lo) >> sh
            slot = torch.where(k < lo, torch.full_like(b, 4096), torch.where(b < 4096, b, torch.full_like(b, 4097)))
            cls = (idx != l[:, None]).long()
            h += torch.bincount((cls * 4099 + slot).reshape(-1), minlength=2 * 4099)
        keep["th"] = h

    t_id, t_h = timed(ours_identify, a.calls, a.warmup), timed(ours_hist, a.calls, a.warmup)
    y_id, y_h = timed(torch_identify, a.calls, a.warmup), timed(torch_hist, a.calls, a.warmup)
    # the two sides computed the same thing: ranks of all rows but the near-ties of one fp32 ulp, the histogram's totals
    rk = keep["id"]["rank"].long()
    same_rank = float((rk == keep["tr"]).double().mean().item())
    hd = keep["h"].reshape(-1)
    out = {"card": torch.cuda.get_device_name(0), "rows": N, "speakers": S, "dim": E, "calls": a.calls, "warmup": a.warmup,
           "speaker_sums_ms": t_sums, "ours_identify_ms": t_id, "ours_trial_hist_ms": t_h, "ours_ms": t_id + t_h,
           "torch_f64_identify_ms": y_id, "torch_f64_hist_ms": y_h, "torch_f64_ms": y_id + y_h, "speedup": (y_id + y_h) / (t_id + t_h),
           "f64_sub_fma_pairs_per_s": 2.0 * N * S * E / ((t_id + t_h) * 1e-3),
           "f64_flops_per_s": 3.0 * 2.0 * N * S * E / ((t_id + t_h) * 1e-3),
           "ranks_equal_share": same_rank, "rank1_accuracy": float((rk == 0).double().mean().item()),
           "hist_total": int(hd.sum().item()), "torch_hist_total": int(keep["th"].sum().item()),
           "hist_equal_bins_share": float((hd == keep["th"]).double().mean().item())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
