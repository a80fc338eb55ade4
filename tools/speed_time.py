"""Times one factor of speed perturbation (vm_resample_i16, csrc/speed.hip) over a generated resident corpus beside a plain
device-to-device copy that moves the same number of bytes, in the same process.

  python tools/speed_time.py [--samples 1073741824] [--repeats 5] [--warmup 2] [--out profiles/speed_perturb_time.txt]

The corpus: full-scale int16 noise in utterances of 2 to 35 s at 16 kHz back to back.  Rows: the default design at 10/9 (speed 0.9: the
64-bit accumulator, phase_abs_max 71012) and at 10/11 (speed 1.1: the 32-bit one, 61532).  Every row: ``repeats`` single calls between
HIP events after ``warmup`` warm-ups, median and spread in milliseconds; the bytes the pass has to move (2 B read per input sample, 2 B
written per output sample; the tables and the taps are noise beside them); the copy floor = those bytes over the HBM rate (8.0 TB/s by
specification) and the share of it achieved; and a ``copy_`` of half those bytes (a copy reads and writes every byte) with the ratio of
the two times.  The MAC count is outputs x taps per phase."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from voicemap_amd import _lib, speed  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


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
        ts.append(a.elapsed_time(b))
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def utterance_lengths(total, seed=0, rate=16000):
    r = np.random.RandomState(seed)
    lens = []
    while sum(lens) < total:
        lens.append(int(r.randint(2 * rate, 35 * rate + 1)))
    lens[-1] -= sum(lens) - total
    if lens[-1] < 2 * rate and len(lens) > 1:   # the remainder joins the utterance before it
        last = lens.pop()
        lens[-1] += last
    return np.array(lens, dtype=np.int64)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, default=1 << 30)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert torch.cuda.is_available(), "speed_time.py measures on the GPU"
    lib = _lib.lib()
    lens = utterance_lengths(a.samples)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    n = len(lens)
    audio = torch.randint(-32768, 32768, (a.samples,), dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for factor in (0.9, 1.1):
        U, D = speed.ratio(factor)
        taps = speed.design_taps(U, D)
        T, pam = len(taps) // U, speed.phase_abs_max(taps, U)
        n_out = speed.output_length(lens, U, D)
        base = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
        total = int(base[-1])
        tab = torch.from_numpy(np.concatenate([offs, lens, base, base[:-1]])).cuda()
        taps_d = torch.from_numpy(taps.astype(np.int32)).cuda()
        out = torch.empty(total, dtype=torch.int16, device="cuda")
        e = tab.element_size()

        def resample():
            lib.call("vm_resample_i16", audio.data_ptr(), tab.data_ptr(), tab.data_ptr() + n * e, tab.data_ptr() + 2 * n * e, n, U, D,
                     taps_d.data_ptr(), T, 15, pam, tab.data_ptr() + (3 * n + 1) * e, out.data_ptr(), st)

        nbytes = 2 * a.samples + 2 * total
        t = timed(resample, a.repeats, a.warmup)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda").random_(0, 255)
        cp = torch.empty_like(src)
        c = timed(lambda: cp.copy_(src), a.repeats, a.warmup)
        del src, cp
        clipped = int(((out == 32767) | (out == -32768)).sum().item())
        rows.append((factor, U, D, pam, "int64" if pam > speed.NARROW_MAX else "int32", total, nbytes, t, c, clipped))
        del out, tab
    lines = ["card: %s; %d int16 samples of full-scale noise in %d utterances of %.1f..%.1f s; default design (32 taps per phase, shift 15); "
             "%d repeats after %d warm-ups; copy floor at %.1f TB/s"
             % (torch.cuda.get_device_name(0), a.samples, n, lens.min() / 16000.0, lens.max() / 16000.0, a.repeats, a.warmup,
                HBM_BYTES_PER_S / 1e12),
             "%-6s %-6s %-6s %12s %10s %10s %10s %10s %10s %9s %9s | %10s %10s %8s" % ("speed", "U/D", "acc", "outputs", "MB moved", "median ms", "min ms",
                                                                                       "max ms", "floor ms", "of floor", "GMAC/s", "copy med", "copy GB/s", "x copy")]
    res = []
    for factor, U, D, pam, acc, total, nbytes, (med, lo, hi), (cm, cl, ch), clipped in rows:
        floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
        lines.append("%-6g %-6s %-6s %12d %10.1f %10.3f %10.3f %10.3f %10.3f %8.1f%% %9.0f | %10.3f %10.0f %8.2f"
                     % (factor, "%d/%d" % (U, D), acc, total, nbytes / 1e6, med, lo, hi, floor_ms, 100.0 * floor_ms / med, total * 32 / med / 1e6,
                        cm, nbytes / cm / 1e6, med / cm))
        res.append({"factor": factor, "U": U, "D": D, "phase_abs_max": pam, "accumulator": acc, "outputs": total, "bytes_moved": nbytes,
                    "median_ms": med, "min_ms": lo, "max_ms": hi, "copy_floor_ms": floor_ms, "share_of_copy_floor": floor_ms / med,
                    "copy_median_ms": cm, "time_over_copy": med / cm, "clipped_outputs": clipped})
    text = "\n".join(lines)
    print(text)
    print(json.dumps({"card": torch.cuda.get_device_name(0), "samples": a.samples, "utterances": n, "rows": res}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
