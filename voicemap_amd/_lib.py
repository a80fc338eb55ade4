"""ctypes binding of libvoicemap_hip.so (the C ABI declared in include/voicemap_hip.h).

There is NO fallback: if the shared library is missing (and cannot be built because hipcc is absent) the
import of the product path fails loudly.  The oracle under ``oracle/`` is never imported from here.
"""
import ctypes
import os
import re

# torch must be imported BEFORE the shared library is loaded: the wheel bundles its own libamdhip64.so / HSA
# runtime, and the process must end up with ONE HIP runtime (ours then binds to the copy torch already mapped,
# so torch's streams and allocations are valid in our launches).  Loading ours first leaves two runtimes and
# hipGetDevice fails with "no ROCm-capable device is detected".
import torch  # noqa: F401
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VOICEMAP_HIP_LIB") or os.path.join(_HERE, "lib", "libvoicemap_hip.so")  # env: A/B experiments
HEADER_PATH = os.path.join(_HERE, "..", "include", "voicemap_hip.h")

ABI_VERSION = 11  # include/voicemap_hip.h vm_abi_version(): checked when the library is loaded

P, I, L, F, D = c_void_p, c_int, c_int64, c_float, c_double
_SCALARS = {"int": I, "int64_t": L, "float": F, "double": D}


def _ctype(decl, fn, is_arg):
    """The ctypes type of one declared argument (`type name`) or return type of ``fn``; a type the binding has no rule for raises."""
    words = decl.replace("*", " * ").split()
    base = [w for w in words if w not in ("*", "const")]
    if is_arg and len(base) > 1:
        base.pop()   # the parameter's name
    base, stars = " ".join(base), words.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base == "char" and "const" in words:
        return c_char_p
    if stars == 2 and base == "void" and "const" not in words:
        return ctypes.POINTER(c_void_p)   # an out-handle
    if stars >= 1 and re.fullmatch(r"\w+", base):
        return P
    raise TypeError("include/voicemap_hip.h: %s: no ctypes type for %r" % (fn, decl.strip()))


def parse_header(src):
    """(name -> (restype, argtypes) of every ``ret vm_name(args);`` prototype, name -> value of every enum constant) of a header."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    enums = {k: int(v) for body in re.findall(r"\benum\s*\{([^}]*)\}", src) for k, v in re.findall(r"(\w+)\s*=\s*(-?\d+)", body)}
    sigs = {}
    for ret, fn, args in re.findall(r"([\w\s*]+?)\b(vm_\w+)\s*\(([^()]*)\)\s*;", src):
        args = [] if args.strip() in ("", "void") else args.split(",")
        sigs[fn] = (_ctype(ret, fn, False), [_ctype(a, fn, True) for a in args])
    return sigs, enums


# name -> (restype, argtypes) of every function the header declares: the header is the one statement of the ABI (the kernels are
# compiled against it), the binding is read from it
with open(HEADER_PATH) as _f:
    SIGNATURES, _ENUMS = parse_header(_f.read())
VM_F32, VM_BF16, VM_F32S, VM_F16 = (_ENUMS[k] for k in ("VM_F32", "VM_BF16", "VM_F32S", "VM_F16"))
VM_LOSS_CONTRASTIVE, VM_LOSS_BCE = _ENUMS["VM_LOSS_CONTRASTIVE"], _ENUMS["VM_LOSS_BCE"]
VM_HEAD_UNIFORM_EUCLIDEAN, VM_HEAD_WEIGHTED_L1 = _ENUMS["VM_HEAD_UNIFORM_EUCLIDEAN"], _ENUMS["VM_HEAD_WEIGHTED_L1"]
VM_DIST_EUCLIDEAN, VM_DIST_COSINE, VM_DIST_DOT = (_ENUMS[k] for k in ("VM_DIST_EUCLIDEAN", "VM_DIST_COSINE", "VM_DIST_DOT"))
VM_SCORE_WEIGHTED_L1, VM_SCORE_NEG_EUCLIDEAN = _ENUMS["VM_SCORE_WEIGHTED_L1"], _ENUMS["VM_SCORE_NEG_EUCLIDEAN"]
VM_SCORE_PLDA = _ENUMS["VM_SCORE_PLDA"]
DIST = {"euclidean": VM_DIST_EUCLIDEAN, "cosine": VM_DIST_COSINE, "dot_product": VM_DIST_DOT}   # the one distance-name table
# ... and the scorers that also take PLDA-space rows (voicemap_amd/plda.py): pairwise retrieval, clustering
PAIR_DIST = {**DIST, "plda": VM_SCORE_PLDA}


def header_functions(path=HEADER_PATH):
    """Names of all functions declared in include/voicemap_hip.h."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vm_[a-z0-9_]+)\s*\(", src)))


class VoicemapHipError(RuntimeError):
    pass


class _Lib:
    def __init__(self, path=None):
        if path is None:
            path = LIB_PATH
            if not os.path.exists(path):
                from . import build as _build
                _build.build(verbose=False)  # raises if hipcc is missing too
        self.path = path
        self.cdll = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(self.cdll, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        self._program_table = False   # not asked yet (program_table())
        self.tuning_epoch = 0   # bumped by every vm_set_tuning through call(): recorded launch sequences (engine.py) are keyed on it
        self.abi = self.cdll.vm_abi_version()
        if self.abi != ABI_VERSION:  # a stale prebuilt library: its entry points take different arguments
            raise VoicemapHipError("%s reports ABI %d, this package binds ABI %d -- rebuild it (python -m voicemap_amd.build --force)"
                                   % (path, self.abi, ABI_VERSION))
        # experiments: kernel-selection knobs for a whole process (a pytest run under another knob value): VOICEMAP_TUNE="key=value,..."
        for kv in [t for t in os.environ.get("VOICEMAP_TUNE", "").split(",") if t.strip()]:
            k, v = kv.split("=")
            self.call("vm_set_tuning", k.strip().encode(), int(v))

    def call(self, name, *args):
        """Call an int-returning entry point; raise with vm_last_error() on failure."""
        if name == "vm_set_tuning":
            self.tuning_epoch += 1
        rc = getattr(self.cdll, name)(*args)
        if rc != 0:
            msg = self.cdll.vm_last_error()
            raise VoicemapHipError("%s failed (%d): %s" % (name, rc, msg.decode() if msg else ""))

    def query(self, name, *args):
        return getattr(self.cdll, name)(*args)

    def workspace(self, name, *args, device):
        """A byte tensor on ``device`` of the size the ``..._workspace_bytes`` query ``name`` gives for ``args``, plus 256 bytes of slack."""
        return torch.empty(self.query(name, *args) + 256, dtype=torch.uint8, device=device)

    def program_table(self):
        """(name -> function id, name -> "PILFD" argument types) of vm_program_run, or None when the loaded library was generated from
        another table than this binding's (tools/gen_program_run.py: ids are positions in the name-sorted list of int-returning entry
        points whose arguments are pointers / int / int64 / float / double)."""
        if self._program_table is False:
            import zlib
            code = {P: "P", I: "I", L: "L", F: "F", D: "D"}
            tab = [(n, "".join(code[a] for a in SIGNATURES[n][1])) for n in sorted(SIGNATURES)
                   if SIGNATURES[n][0] is I and n != "vm_program_run" and all(a in code for a in SIGNATURES[n][1])]
            h = zlib.crc32(";".join("%s:%s" % t for t in tab).encode()) & 0x7FFFFFFF
            ok = self.cdll.vm_program_table_hash() == h
            self._program_table = ({n: k for k, (n, _) in enumerate(tab)}, dict(tab)) if ok else None
        return self._program_table


_LIB = None


def program_table():
    """lib().program_table()"""
    return lib().program_table()


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _Lib()
    return _LIB


def load(path):
    """Another build of the library (A/B tools: the parent commit's), bound from this tree's header like the package's own."""
    return _Lib(path)


def use(other):
    """Make ``lib()`` -- and with it every wrapper of the package -- return ``other`` (``load``'s or ``lib()``'s); returns the one before."""
    global _LIB
    before, _LIB = lib(), other
    return before
