"""ctypes binding of libvitgan_hip.so (C ABI: include/vitgan_hip.h).

There is no CPU fallback: if the library is missing every operator raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VITGAN_HIP_LIB", os.path.join(_HERE, "libvitgan_hip.so"))  # override: kernel experiments only
CSRC = os.path.join(_HERE, "csrc")

HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "vitgan_hip.h"))

c_void_p, c_int, c_float, c_ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
_SCALARS = {"int": c_int, "float": c_float, "long long": c_ll, "unsigned long long": C.c_ulonglong}
_POINTEES = set(_SCALARS) | {"void", "double", "unsigned", "unsigned char"}  # what a plain address may point at
_TYPED_POINTERS = {"long long*": C.POINTER(c_ll), "void**": C.POINTER(c_void_p)}  # out-parameters filled through byref()
# The spectral table is kept twice by the caller, as bytes on the host and as the same bytes on the device, and the calls take both:
# one of the two is a device address, so neither is bound as a pointer to the ctypes struct.
_BYTE_TABLES = ("table_host", "table_dev")


class HeaderError(ValueError):
    pass


class Header:
    """What the binding needs of the C header: ``structs`` {name: ctypes.Structure class}, ``prototypes`` {function: (return type,
    [(type, parameter)])} as C text, ``signatures`` {function: (restype, [ctypes of the arguments])}, ``defines`` {name: int} and the two
    enumerations kept as defines, ``lr_kinds`` (VG_LR_*) and ``tel_fields`` (VG_TEL_* but the row width VG_TEL_NF).  It reads the constructs
    include/vitgan_hip.h uses and raises HeaderError, naming the offender, on anything else."""

    def __init__(self, text: str):
        self.structs, self.prototypes, self.signatures, self.defines = {}, {}, {}, {}
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        text = re.sub(r"^[ \t]*#[ \t]*ifdef __cplusplus\n.*?^[ \t]*#[ \t]*endif[^\n]*$", "", text, flags=re.S | re.M)  # extern "C" { and }
        for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(VG_\w+)[ \t]*(.*)$", text, flags=re.M):
            if not re.fullmatch(r"-?\d+", value.strip()):
                raise HeaderError(f"#define {name}: {value.strip()!r} is not an integer")
            self.defines[name] = int(value)
        text = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)

        def struct(m):
            self._struct(m.group(1) or m.group(3), m.group(2), m.group(3))
            return ""
        text = re.sub(r"\btypedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
        *statements, rest = text.split(";")
        for st in statements + [rest]:
            if st.strip():
                self._prototype(" ".join(st.split()), terminated=st is not rest)
        self.lr_kinds = self._enum("VG_LR_")
        self.tel_fields = tuple(self._enum("VG_TEL_", reserved="VG_TEL_NF"))

    @staticmethod
    def _declarator(decl: str, where: str):
        """'const float* lr_dev' -> ('const float*', 'lr_dev', None);  'long long gin[2]' -> ('long long', 'gin', 2)"""
        m = re.fullmatch(r"(.*?)(\w+)\s*(?:\[\s*(\d+)\s*\])?", decl.strip())
        if not m or not re.fullmatch(r"[\w\s*]*", m.group(1)):
            raise HeaderError(f"{where}: cannot read the declaration {decl.strip()!r}")
        return re.sub(r"\s*\*\s*", "*", " ".join(m.group(1).split())), m.group(2), m.group(3) and int(m.group(3))

    def _ctype(self, ctext: str, name: str, where: str, parameter: bool):
        base = " ".join(re.sub(r"\bconst\b", "", ctext).replace("*", " ").split())
        if "*" not in ctext:
            t = _SCALARS.get(base) or (None if parameter else self.structs.get(base))  # a nested struct is held by value
        elif parameter and ctext in _TYPED_POINTERS:
            t = _TYPED_POINTERS[ctext]
        elif parameter and base in self.structs and ctext.count("*") == 1:
            t = c_void_p if name in _BYTE_TABLES else C.POINTER(self.structs[base])
        else:
            t = c_void_p if base in _POINTEES else None
        if t is None:
            raise HeaderError(f"{where}: no ctypes mapping for the type {ctext!r} of {name!r}")
        return t

    def _struct(self, tag: str, body: str, name: str) -> None:
        if tag != name:
            raise HeaderError(f"struct {name}: tag {tag!r} differs from the typedef name")
        fields = []
        *decls, rest = body.split(";")
        if rest.strip():
            raise HeaderError(f"struct {name}: field {rest.strip()!r} has no ';'")
        for decl in decls:
            first, *more = (self._declarator(x, f"struct {name}") for x in decl.split(","))  # 'long long gin[2], gmid[2]': one type
            if any(ctext for ctext, _, _ in more):
                raise HeaderError(f"struct {name}: cannot read the declaration {decl.strip()!r}")
            for _, field, count in [first] + more:
                t = self._ctype(first[0], field, f"struct {name}", parameter=False)
                fields.append((field, t * count if count else t))
        self.structs[name] = type(name, (C.Structure,), {"_fields_": fields})

    def _prototype(self, st: str, terminated: bool) -> None:
        fn = (re.search(r"\bvg_\w+", st) or re.search(r"\w+", st)).group(0)
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(vg_\w+)\s*\(([^()]*)\)", st)
        if not m or not terminated:
            raise HeaderError(f"{fn}: cannot split the prototype {st[:120]!r}" + ("" if terminated else " (no ';')"))
        ret = " ".join(m.group(1).split())
        if ret not in _SCALARS:
            raise HeaderError(f"{fn}: no ctypes mapping for the return type {ret!r}")
        params = [] if m.group(3).strip() == "void" else [self._declarator(p, fn) for p in m.group(3).split(",")]
        if any(count is not None or not ctext for ctext, _, count in params):
            raise HeaderError(f"{fn}: cannot read the parameter list ({m.group(3).strip()})")
        self.prototypes[fn] = (ret, [(ctext, p) for ctext, p, _ in params])
        self.signatures[fn] = (_SCALARS[ret], [self._ctype(ctext, p, fn, parameter=True) for ctext, p, _ in params])

    def _enum(self, prefix: str, reserved: str = None) -> dict:
        """{lower-cased suffix: value} of the ``#define prefix*`` group (without ``reserved``), which must number 0..n-1 without a gap"""
        group = sorted((v, k[len(prefix):].lower()) for k, v in self.defines.items() if k.startswith(prefix) and k != reserved)
        for i, (v, name) in enumerate(group):
            if v != i:
                raise HeaderError(f"{prefix}{name.upper()} = {v}: the {prefix}* indices must run 0..n-1 without a gap, expected {i}")
        if group and reserved is not None and len(group) >= self.defines.get(reserved, 0):
            raise HeaderError(f"{reserved} = {self.defines.get(reserved)} does not lie above the {len(group)} {prefix}* indices")
        return {name: v for v, name in group}


with open(HEADER) as _f:
    _HEADER = Header(_f.read())
globals().update(_HEADER.structs)  # VgVitDims, VgVitNet, ...: one ctypes.Structure per typedef struct, fields in the header's order
_SIGNATURES = _HEADER.signatures
ABI_VERSION = _HEADER.defines["VG_ABI_VERSION"]
TEL_NF = _HEADER.defines["VG_TEL_NF"]  # floats per telemetry row; TEL_FIELDS names them by index (the slots above are reserved)
TEL_FIELDS, LR_KINDS = _HEADER.tel_fields, _HEADER.lr_kinds

_lib: Optional[C.CDLL] = None


def build(verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into libvitgan_hip.so (hipcc cross-compiles without a GPU)."""
    jobs = str(min(6, os.cpu_count() or 1))
    r = subprocess.run(["make", "-C", CSRC, "-j", jobs], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode != 0:
        raise RuntimeError("libvitgan_hip.so build failed")
    return LIB_PATH


def bind(handle: C.CDLL, names=None) -> C.CDLL:
    """Give the entry points of the header (``names``: only those - a build of another ABI version may lack the rest) their restype /
    argtypes on ``handle``: this library, or another build of it loaded beside it."""
    for name in _SIGNATURES if names is None else names:
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _SIGNATURES[name]
    return handle


def lib() -> C.CDLL:
    """The loaded library; raises loudly when it has not been built."""
    global _lib
    if _lib is None:
        # torch bundles its own libamdhip64; it must be loaded FIRST so that this library binds to the
        # same HIP runtime instance (same SONAME) - otherwise torch's device pointers are foreign to it.
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension is the only compute path of this package. "
                "Build it with `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).")
        handle = bind(C.CDLL(LIB_PATH))
        if handle.vg_abi_version() != ABI_VERSION:
            raise RuntimeError("libvitgan_hip.so ABI version mismatch; rebuild")
        _lib = handle
    return _lib


_ctx = None


def context() -> c_void_p:
    """Process-wide execution context (second stream + events) for concurrent weight-gradient work."""
    global _ctx
    if _ctx is None:
        h = c_void_p()
        call("vg_ctx_create", C.byref(h))
        _ctx = h
    return _ctx


class HipError(RuntimeError):
    pass


def check(rc: int, what: str) -> None:
    if rc != 0:
        kind = "argument validation" if rc < 0 else "hipError_t"
        raise HipError(f"{what} failed: {kind} {rc}")


def call(name: str, *args, what: Optional[str] = None) -> None:
    """One status-returning entry point, by name; ``what`` replaces the name in the error text.  Resolved through lib() every time."""
    check(getattr(lib(), name)(*args), what or name)


def ptr(t):
    """A tensor's device pointer (None stays NULL)."""
    return None if t is None else c_void_p(t.data_ptr())


def stream() -> c_void_p:
    """The current torch stream as the ABI's ``void* stream``."""
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)
