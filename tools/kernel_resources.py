"""Compare the kernel resource reports of two builds of libvoicemap_hip.so.

Build each tree with the compiler's report switched on and keep what it prints:

  VM_EXTRA_HIPCC_FLAGS=-Rpass-analysis=kernel-resource-usage python -m voicemap_amd.build --force 2> build.log

  python tools/kernel_resources.py parent.log this.log [--only pairdist_kernel,pair_hist_kernel,...]

Prints one line per kernel instantiation (demangled): SGPRs, VGPRs, AGPRs, scratch, occupancy, spills and LDS bytes of both builds, `same`
or `DIFF`, and the instantiations only one build has.  The exit status is 1 when an instantiation both builds have differs.
"""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")
SHORT = ("sgpr", "vgpr", "agpr", "scratch", "occ", "sspill", "vspill", "lds")


def parse(path):
    """mangled kernel name -> tuple of FIELDS values of one build log."""
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]*\])?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            out[cur][m.group(1).strip()] = m.group(2)
    return {k: tuple(v.get(f, "?") for f in FIELDS) for k, v in out.items()}


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, (re.sub(r"\(.*", "", s) for s in r.stdout.splitlines())))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv):
    only = None
    if "--only" in argv:
        k = argv.index("--only")
        only = argv[k + 1].split(",")
        argv = argv[:k] + argv[k + 2:]
    a, b = parse(argv[0]), parse(argv[1])
    names = sorted(set(a) | set(b))
    if only:
        names = [n for n in names if any(o in n for o in only)]
    dm = demangle(names)
    fmt = lambda t: " ".join("%s=%s" % kv for kv in zip(SHORT, t))
    diff = 0
    for n in sorted(names, key=lambda n: dm[n]):
        if n in a and n in b:
            same = a[n] == b[n]
            diff += not same
            print("%-62s %s  %s" % (dm[n], "same" if same else "DIFF", fmt(b[n]) if same else fmt(a[n]) + "  ->  " + fmt(b[n])))
        else:
            print("%-62s %s  %s" % (dm[n], "only in " + (argv[0] if n in a else argv[1]), fmt(a.get(n) or b[n])))
    print("%d instantiations in both builds, %d differ" % (sum(n in a and n in b for n in names), diff))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
