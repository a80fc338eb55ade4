"""Times vm_vad_frames and vm_vad_compact (csrc/vad.hip) on a generated resident corpus beside a plain device-to-device copy that moves
the same number of bytes, in the same process.

  python tools/vad_time.py [--samples 67108864] [--repeats 30] [--warmup 5] [--out profiles/vad_time.txt]

The corpus: int16 utterances of 2 to 35 s at 16 kHz back to back, bursts of noise at speech level between pauses at +-2 (a quarter of
every utterance on average), so the default policy trims something.  Rows: vm_vad_frames (its two launches: the energy pass over the
corpus and the decide pass over the frames), vm_vad_compact, and for each a ``copy_`` of half the row's bytes (a copy reads and writes
every byte: the same bytes moved).  Every row: `repeats` single calls between HIP events after `warmup` warm-ups, median and spread
(min, max) in microseconds, the bytes the pass has to move over the median, and the ratio of its time to its copy's.

Bytes counted (what the algorithm needs, not what the cache system did): frames pass = 2 B per sample read + per frame 8 B of energy
written and read back, 1 B of mask and 8 B of dst written; compact = 2 B read and 2 B written per KEPT sample + per frame 1 B of mask
and, per kept frame, 8 B of dst read.  The per-utterance tables are noise beside these."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from voicemap_amd import _lib  # noqa: E402
from voicemap_amd.vad import VadPolicy  # noqa: E402


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


def corpus(total, seed=0, rate=16000):
    """(int16 buffer of ``total`` samples, offsets, lens): utterances of 2 to 35 s; segments of 0.1 to 1.5 s, every fourth on average
    a pause."""
    r = np.random.RandomState(seed)
    lens = []
    while sum(lens) < total:
        lens.append(int(r.randint(2 * rate, 35 * rate + 1)))
    lens[-1] -= sum(lens) - total
    if lens[-1] < 2 * rate:   # the remainder joins the utterance before it
        last = lens.pop()
        lens[-1] += last
    lens = np.array(lens, dtype=np.int64)
    seg = r.randint(rate // 10, 3 * rate // 2, size=2 * total // rate + 16)
    seg = seg[:np.searchsorted(np.cumsum(seg), total) + 1]
    loud = np.repeat(r.random_sample(seg.size) >= 0.25, seg)[:total]
    x = np.where(loud, r.randint(-6000, 6001, total), r.randint(-2, 3, total)).astype(np.int16)
    return x, np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), lens


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, default=1 << 26)
    p.add_argument("--repeats", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert torch.cuda.is_available(), "vad_time.py measures on the GPU"
    lib = _lib.lib()
    pol = VadPolicy()
    x, offs, lens = corpus(a.samples)
    n, Fr = len(lens), pol.frame
    fb = np.concatenate([[0], np.cumsum((lens + Fr - 1) // Fr)]).astype(np.int64)
    frames = int(fb[-1])
    audio = torch.from_numpy(x).cuda()
    tab = torch.from_numpy(np.concatenate([offs, lens, fb])).cuda()
    o_d, l_d, fb_d = tab[:n], tab[n:2 * n], tab[2 * n:]
    energy = torch.empty(frames, dtype=torch.int64, device="cuda")
    dst = torch.empty(frames, dtype=torch.int64, device="cuda")
    mask = torch.empty(frames, dtype=torch.uint8, device="cuda")
    new_lens = torch.empty(n, dtype=torch.int64, device="cuda")
    info = torch.empty(n, 4, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def frames_pass():
        lib.call("vm_vad_frames", audio.data_ptr(), o_d.data_ptr(), l_d.data_ptr(), fb_d.data_ptr(), n, Fr, pol.rel, pol.floor_energy,
                 pol.min_run, pol.hang, pol.keep(), energy.data_ptr(), mask.data_ptr(), dst.data_ptr(), new_lens.data_ptr(), info.data_ptr(), st)

    frames_pass()
    torch.cuda.synchronize()
    nl = new_lens.cpu().numpy()
    kept, kept_frames = int(nl.sum()), int(mask.sum().item())
    no_d = torch.from_numpy(np.concatenate([[0], np.cumsum(nl)[:-1]]).astype(np.int64)).cuda()
    out = torch.empty(kept, dtype=torch.int16, device="cuda")

    def compact_pass():
        lib.call("vm_vad_compact", audio.data_ptr(), o_d.data_ptr(), l_d.data_ptr(), fb_d.data_ptr(), mask.data_ptr(), dst.data_ptr(),
                 no_d.data_ptr(), n, Fr, out.data_ptr(), st)

    bytes_frames = 2 * a.samples + frames * (8 + 8 + 1 + 8)
    bytes_compact = 4 * kept + frames + 8 * kept_frames
    rows = []
    for name, fn, nbytes in (("vm_vad_frames", frames_pass, bytes_frames), ("vm_vad_compact", compact_pass, bytes_compact)):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda").random_(0, 255)
        cp = torch.empty_like(src)
        t = timed(fn, a.repeats, a.warmup)
        c = timed(lambda: cp.copy_(src), a.repeats, a.warmup)
        rows.append((name, nbytes, t, c))
        del src, cp
    lines = ["card: %s; %d int16 samples in %d utterances of %.1f..%.1f s, %d frames of %d; kept %.1f%% of the samples, %d of %d frames; "
             "%d repeats after %d warm-ups" % (torch.cuda.get_device_name(0), a.samples, n, lens.min() / 16000.0, lens.max() / 16000.0, frames,
                                               Fr, 100.0 * kept / a.samples, kept_frames, frames, a.repeats, a.warmup),
             "%-16s %12s %10s %10s %10s %10s | %10s %10s %10s %10s | %8s" % ("call", "MB moved", "median us", "min us", "max us", "GB/s",
                                                                            "copy med", "copy min", "copy max", "copy GB/s", "x copy")]
    res = []
    for name, nbytes, (med, lo, hi), (cm, cl, ch) in rows:
        lines.append("%-16s %12.1f %10.1f %10.1f %10.1f %10.0f | %10.1f %10.1f %10.1f %10.0f | %8.2f"
                     % (name, nbytes / 1e6, med, lo, hi, nbytes / med / 1e3, cm, cl, ch, nbytes / cm / 1e3, med / cm))
        res.append({"call": name, "bytes_moved": nbytes, "median_us": med, "min_us": lo, "max_us": hi, "copy_median_us": cm,
                    "copy_min_us": cl, "copy_max_us": ch, "time_over_copy": med / cm})
    text = "\n".join(lines)
    print(text)
    print(json.dumps({"card": torch.cuda.get_device_name(0), "samples": a.samples, "utterances": n, "frames": frames, "kept_samples": kept,
                      "rows": res}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
