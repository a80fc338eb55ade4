"""Timing of whole-utterance embedding (HipEncoderEngine.embed_varlen) for cfg-A (128 filters, embedding 64) in f16 storage, against the
fixed-window embed-only figure of the same engine in the same process.  Prints ONE JSON line.

* Workload: --files recordings (default 2048) resident in HBM as int16, lengths drawn from a LibriSpeech-like distribution --
  0.8 x Normal(14 s, 2.5 s) + 0.2 x Uniform(1 s, 35 s), clipped to [1 s, 35 s], seed 0 -- embedded whole, downsampling 4.
* Yardstick: embed_from_offsets of 256 windows of 3 s from the same buffer (bench.py's inference batch).
* Both in audio-seconds per second; the target is whole / fixed >= 0.8.  Also the padded-row overhead, the bucket count, the
  distinct bucket lengths and the plans the engine holds.

Host clock around whole calls after a warm-up (synchronised), in several blocks: median and spread."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SR, DS = 16000, 4


def lengths(n, seed=0):
    r = np.random.default_rng(seed)
    s = np.where(r.random(n) < 0.8, r.normal(14.0, 2.5, n), r.uniform(1.0, 35.0, n))
    return (np.clip(s, 1.0, 35.0) * SR).astype(np.int64)


def timed(fn, reps, blocks):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return {"median_ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out)), "blocks": blocks, "reps": reps}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--fixed-reps", type=int, default=20)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("utterance_embed_bench needs a GPU")
    from oracle import voicemap_oracle as O
    from voicemap_amd.engine import HipEncoderEngine
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    arch = O.EncoderArch.baseline(128, 64, dropout=0.0)
    eng = HipEncoderEngine(arch.blocks, 64, dropout=0.0, head=None, dtype=a.dtype, seed=0)
    rl = lengths(a.files)
    offs = np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.int64)
    total = int(rl.sum())
    g = torch.Generator(device=dev).manual_seed(0)
    audio = (torch.randn(total, device=dev, generator=g) * 1600.0).clamp_(-32768, 32767).to(torch.int16)
    seconds = total / SR

    whole = timed(lambda: eng.embed_varlen(audio, offs, rl, DS), a.reps, a.blocks)
    bp = eng.last_bucket_plan
    T = 3 * SR
    starts = torch.as_tensor(offs[np.nonzero(rl >= T)[0][:256]], device=dev)
    assert starts.numel() == 256
    fixed = timed(lambda: eng.embed_from_offsets(audio, starts, T, DS, True, windows_per_tower=1), a.fixed_reps, a.blocks)
    rate_whole = seconds / (whole["median_ms"] * 1e-3)
    rate_fixed = 256 * 3.0 / (fixed["median_ms"] * 1e-3)
    out = {
        "workload": "whole-utterance embedding, cfg-A %s, %d recordings, %.0f s of audio; lengths 0.8 x N(14 s, 2.5 s) + 0.2 x U(1 s, 35 s), "
                    "clipped to [1, 35] s, seed 0; downsampling 4" % (a.dtype, a.files, seconds),
        "embed_varlen": whole,
        "audio_s_per_s_whole": rate_whole,
        "fixed_window_embed_256x3s": fixed,
        "audio_s_per_s_fixed_3s": rate_fixed,
        "ratio_whole_over_fixed": rate_whole / rate_fixed,
        "target_ratio": 0.8,
        "target_met": bool(rate_whole / rate_fixed >= 0.8),
        "padded_row_overhead": bp.pad_overhead,
        "buckets": len(bp.buckets),
        "bucket_lengths": len(bp.shapes),
        "engine_plans": eng.plan_count(),
        "row_budget": bp.row_budget,
        "device": torch.cuda.get_device_name(dev),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
