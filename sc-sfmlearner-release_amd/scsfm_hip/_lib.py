"""ctypes binding of the C ABIs declared in include/: one loader over scsfm_hip/libraries.py's table.

``get()`` returns the product library, libscsfm_hip.so (hipcc, gfx950), and nothing else: if the
shared object is missing it is built in-tree with hipcc, and if that is impossible the call raises
-- there is no CPU or eager fallback anywhere in this package.  ``get_<name>()`` does the same for every other row; each
row also gives ``<NAME>_HEADER``, ``<NAME>_LIB_PATH`` and ``<NAME>_ABI_VERSION`` (the loss library's carry no prefix).

The libraries (shared object, sources, header, what it computes):
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

# torch bundles its own HIP runtime (torch/lib/libamdhip64.so) while libscsfm_hip.so is linked
# against the one under /opt/rocm.  Both carry the same SONAME, so whichever is loaded first serves
# the whole process: importing torch first makes the kernels launch on the very runtime that owns
# torch's streams and allocations.  (Loaded the other way round, the first launch fails with
# hipErrorNoDevice.)
import torch  # noqa: F401  (must precede ctypes.CDLL below)

from .libraries import ALL, BY_NAME, CATALOGUE, EVERY, HERE, LATER, LIBRARIES, REGISTRY, ROWS, SINCE, SUMMARY, TABLE  # noqa: F401  (ALL, CATALOGUE, EVERY, HERE, LATER, LIBRARIES, ROWS: as before)

__doc__ = (__doc__ or "") + SUMMARY + "\n" + SINCE + "\n"

HEADER = BY_NAME[""].header
# SCSFM_HIP_LIB points at a library built elsewhere (tuning variants, a system-wide install)
LIB_PATH = os.environ.get("SCSFM_HIP_LIB") or BY_NAME[""].lib
ABI_VERSION = BY_NAME[""].abi

_CTYPES = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
           "float": ctypes.c_float}
_DECL = re.compile(r"^(int|size_t)\s+(scsfm_\w+)\s*\(([^)]*)\)\s*;", re.M | re.S)


def parse_header(path=HEADER):
    """-> {name: (restype, [argtypes])} for every function the header declares."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, args in _DECL.findall(text):
        argtypes = []
        args = " ".join(args.split())
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    argtypes.append(ctypes.c_void_p)
                else:
                    argtypes.append(_CTYPES[a.split()[0]])
        out[name] = (_CTYPES[ret], argtypes)
    return out


class ScsfmError(RuntimeError):
    pass


class CLib:
    """A loaded implementation of the C ABI of ``header`` (default include/scsfm_hip.h).  Every declared symbol must be
    present and ``<prefix>abi_version()`` must return ``abi``; the source id is read from ``<prefix>source_id``."""

    def __init__(self, path, header=HEADER, abi=ABI_VERSION, prefix="scsfm_"):
        self.path = path
        self._dll = ctypes.CDLL(path)
        self.decls = parse_header(header)
        self._fn = {}
        self._prefix = prefix
        for name, (ret, argtypes) in self.decls.items():
            try:
                fn = getattr(self._dll, name)
            except AttributeError as e:
                raise ScsfmError(f"{path} does not export {name} (declared in {header})") from e
            fn.restype = ret
            fn.argtypes = argtypes
            self._fn[name] = fn
        if self._fn[prefix + "abi_version"]() != abi:
            raise ScsfmError(f"{path}: ABI version mismatch")

    def source_id(self):
        """The source hash compiled into the binary (scsfm_hip/build.py: lib_source_id)."""
        buf = ctypes.create_string_buffer(64)
        self._fn[self._prefix + "source_id"](buf, 64)
        return buf.value.decode()

    def call(self, name, *args):
        """Invoke an int-returning entry point; raise on a non-zero status."""
        rc = self._fn[name](*args)
        if rc != 0:
            kind = "rejected argument" if rc == -1 else "hipError_t"
            raise ScsfmError(f"{name} failed with status {rc} ({kind})")

    def size(self, name, *args):
        return int(self._fn[name](*args))


_lock = threading.Lock()  # one for the process: loading, building included, is serial


def _load(row) -> CLib:
    """Ties the binary to the sources next to it BEFORE loading it: the source id compiled into the shared object is
    read from the file (scsfm_hip.build.binary_source_id -- a stale binary may lack symbols or carry another ABI number,
    which the strict loader below would report as an error instead of rebuilding), and a missing or stale library is
    built with hipcc under a file lock, so that the N ranks of a torchrun job that all arrive here at once compile
    once.  Without hipcc a stale library is refused.  A loss library named by SCSFM_HIP_LIB (a tuning variant, a
    system-wide install) is taken as it is."""
    from . import build as _build
    name = row.name
    path, own = (row.lib, True) if name else (LIB_PATH, "SCSFM_HIP_LIB" not in os.environ)
    if own and _build.lib_is_stale(name):
        have = _build.binary_source_id(path)
        try:
            _build.build_lib(name)
        except Exception as e:
            what = f"was built from other sources ({have}) than the tree's ({_build.lib_source_id(name)})" if have \
                else "is missing (or carries no source id)"
            raise ScsfmError(f"{path} {what} and cannot be built here: {e}") from e
    lib = CLib(path, row.header, row.abi, row.prefix)
    if own and lib.source_id() != _build.lib_source_id(name):
        raise ScsfmError(f"{path}: its source id {lib.source_id()} is not the tree's {_build.lib_source_id(name)}")
    return lib


def _getter(row):
    lib = None  # the cache: once loaded, a call is this lookup and a return (the training step's host path)

    def get() -> CLib:
        nonlocal lib
        if lib is None:
            with _lock:
                if lib is None:
                    lib = _load(row)
        return lib
    get.__name__ = get.__qualname__ = f"get_{row.name}" if row.name else "get"
    get.__doc__ = f"""{os.path.basename(row.lib)} (one per process): {row.what} (include/{os.path.basename(row.header)}).
    Built in-tree with hipcc when it is missing or stale; raises when that is impossible (see ``_load``)."""
    return get


get = _getter(TABLE[0])
for _row in REGISTRY[1:]:
    globals().update({
        f"{_row.name.upper()}_HEADER": _row.header,
        f"{_row.name.upper()}_LIB_PATH": _row.lib,
        f"{_row.name.upper()}_ABI_VERSION": _row.abi,
        f"get_{_row.name}": _getter(_row),
    })
del _row
