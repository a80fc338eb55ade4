"""Times vm_crop_augment_decimate_whiten (csrc/augment.hip) at cfg-A's batch beside vm_crop_decimate_whiten at the same shape in the
same process.

  python tools/augment_time.py [--windows 256] [--raw-len 48000] [--ds 4] [--repeats 30] [--warmup 5] [--out profiles/augment_time.txt]

Rows: the plain launch; the augmented launch with K = 0 / 2 babble voices and no RIR; then R in {1024, 4096, 8192} taps on HALF the
windows (K = 2) and on ALL of them (K = 0).  Every row: `repeats` single launches between HIP events after `warmup` warm-ups, median and
spread (min, max) in microseconds.  The FIR's own time is the row minus the same K without an RIR; its fp32 rate is the multiply-add
count (windows with an RIR x L0 x R) over that time, against the VALU issue bound of the card (CUs x 4 SIMDs x 32 lanes x clock: one fp32
FMA per lane per clock, packed FMAs counted as two).  Resident int16 corpus of 64 M samples, random offsets."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from voicemap_amd import _lib  # noqa: E402
from voicemap_amd.augment import synth_rir_bank  # noqa: E402


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--windows", type=int, default=256)
    p.add_argument("--raw-len", type=int, default=48000)
    p.add_argument("--ds", type=int, default=4)
    p.add_argument("--repeats", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--step-ms", type=float, default=2.55, help="the training step this is set against (cfg-A: 2.5-2.6 ms)")
    p.add_argument("--out", default="")
    a = p.parse_args()
    lib = _lib.lib()
    n, T, ds = a.windows, a.raw_len, a.ds
    L0 = (T + ds - 1) // ds
    r = np.random.RandomState(0)
    total = 1 << 26
    audio = torch.from_numpy(r.randint(-8000, 8000, total).astype(np.int16)).cuda()
    offs = torch.from_numpy(r.randint(0, total - T, n).astype(np.int64)).cuda()
    noff = torch.from_numpy(r.randint(0, total - T, (n, 2)).astype(np.int64)).cuda()
    snr = torch.full((n,), 10.0, device="cuda")
    gain = torch.ones(n, device="cuda")
    out = torch.empty(n, L0 + 31, device="cuda")
    ws0 = torch.empty(lib.query("vm_decimate_whiten_workspace_bytes", n) // 8, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.query("vm_crop_augment_workspace_bytes", n, L0) // 8 + 1, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    wpt = n // 2

    def plain():
        lib.call("vm_crop_decimate_whiten", audio.data_ptr(), 1, offs.data_ptr(), n, T, ds, 1, 0.038021, wpt, out.data_ptr(), ws0.data_ptr(), st)

    def aug(K, rirs, rid):
        def f():
            lib.call("vm_crop_augment_decimate_whiten", audio.data_ptr(), 1, offs.data_ptr(), n, T, ds, 1, 0.038021, wpt,
                     audio.data_ptr() if K else None, 1, noff.data_ptr() if K else None, K, snr.data_ptr(), gain.data_ptr(),
                     None if rirs is None else rirs.data_ptr(), 0 if rirs is None else rirs.shape[0], 0 if rirs is None else rirs.shape[1],
                     None if rirs is None else rid.data_ptr(), out.data_ptr(), ws.data_ptr(), st)
        return f

    rows = [("vm_crop_decimate_whiten (plain)", 0, 0, 0, timed(plain, a.repeats, a.warmup))]
    base = {}
    for K in (0, 2):
        base[K] = timed(aug(K, None, None), a.repeats, a.warmup)
        rows.append(("augment K=%d R=0" % K, K, 0, 0, base[K]))
    half = torch.from_numpy(np.where(np.arange(n) % 2 == 0, np.arange(n) % 8, -1).astype(np.int32)).cuda()
    every = torch.from_numpy((np.arange(n) % 8).astype(np.int32)).cuda()
    for R in (1024, 4096, 8192):
        rirs = torch.from_numpy(synth_rir_bank(8, max_taps=R, seed=R)).cuda()
        rows.append(("augment K=2 R=%d on half" % R, 2, R, n // 2, timed(aug(2, rirs, half), a.repeats, a.warmup)))
        rows.append(("augment K=0 R=%d on all" % R, 0, R, n, timed(aug(0, rirs, every), a.repeats, a.warmup)))
    prop = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(prop, "clock_rate", 2400000)) * 1e3
    bound = prop.multi_processor_count * 4 * 32 * clock_hz     # fp32 FMAs per second, one per lane per clock
    lines = ["card: %s, %d CUs, %.0f MHz; %d windows x %d samples, ds %d (L0 %d), int16 corpus; %d repeats after %d warm-ups"
             % (torch.cuda.get_device_name(0), prop.multi_processor_count, clock_hz / 1e6, n, T, ds, L0, a.repeats, a.warmup),
             "VALU issue bound taken: %.1f T fp32 FMA/s (CUs x 4 SIMDs x 32 lanes x clock)" % (bound / 1e12),
             "%-34s %10s %10s %10s %12s %12s %10s %10s" % ("launch", "median us", "min us", "max us", "FIR us", "GFMA/s", "of bound", "of step")]
    res = []
    for name, K, R, nr, (med, lo, hi) in rows:
        fir = med - base[K][0] if R else 0.0
        rate = nr * L0 * R / (fir * 1e-6) if R and fir > 0 else 0.0
        lines.append("%-34s %10.1f %10.1f %10.1f %12s %12s %10s %9.1f%%"
                     % (name, med, lo, hi, "%.1f" % fir if R else "-", "%.0f" % (rate / 1e9) if R else "-",
                        "%.1f%%" % (100 * rate / bound) if R else "-", 100 * med * 1e-3 / a.step_ms))
        res.append({"launch": name, "median_us": med, "min_us": lo, "max_us": hi, "fir_us": fir, "fir_fma_per_s": rate})
    text = "\n".join(lines)
    print(text)
    print(json.dumps({"card": torch.cuda.get_device_name(0), "rows": res, "fma_bound_per_s": bound, "step_ms": a.step_ms}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
