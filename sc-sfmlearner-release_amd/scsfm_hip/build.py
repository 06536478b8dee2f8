"""Build the HIP libraries of scsfm_hip/libraries.py's table (gfx950) in-tree with hipcc.

    python -m scsfm_hip.build        (from sc-sfmlearner-release_amd/)

Each shared object is plain HIP + a C ABI; none links against torch.  They are written next to this file so that they
travel with the source tree to the GPU box.  They are separate targets with separate source ids, so that an edit of the
nets' or the evaluation's kernels leaves the loss library's id (to which recorded PMC counters are tied) unchanged.

``lib_sources(name)``, ``lib_deps(name)``, ``lib_source_id(name)``, ``lib_is_stale(name)`` and ``build_lib(name)`` work
on any row, by its short name.  The loss library's own names carry no prefix (``sources``, ``source_id(extra)``,
``build(extra=...)``: it alone takes tuning flags); every other row gets ``<name>_sources``, ``<name>_deps``,
``<name>_source_id``, ``<name>_is_stale``, ``build_<name>``, ``<NAME>_CSRC`` and ``<NAME>_LIB`` from the loop below.

Safe for N processes at once (torchrun: every rank calls ``_lib.get()`` lazily, and ``*.so`` is git-ignored, so a fresh
clone on an 8-GPU node has no library): the build runs under an exclusive ``flock`` on ``libscsfm_hip.so.lock``, the
compiler writes to a name unique to the process and the result is moved into place atomically; a process that gets the
lock after another one has built finds a binary whose compiled-in source id matches and does not compile again.

The libraries (shared object, sources, header, what it computes):
"""
from __future__ import annotations

import contextlib
import fcntl
import functools
import glob
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

from .libraries import ALL, BY_NAME, CATALOGUE, EVERY, HERE, INCLUDE, LATER, LIBRARIES, REGISTRY, ROWS, SINCE, SUMMARY, TABLE, find  # noqa: F401  (ALL, CATALOGUE, EVERY, LATER, LIBRARIES, ROWS: as before)

__doc__ = (__doc__ or "") + SUMMARY + "\n" + SINCE + "\n"

CSRC = BY_NAME[""].csrc
LIB = BY_NAME[""].lib
LOCK = LIB + ".lock"
LOG = LIB + ".buildlog"
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", f"--offload-arch={ARCH}", "-munsafe-fp-atomics",
         "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
         # the SLP vectoriser pairs unrelated scalar fp32 chains into v_pk_* with 4 v_mov per packed op (+5 % VALU
         # in the tiled pass); the 2-wide math that pays is written with vector types in csrc/scsfm_ssim.h
         "-fno-slp-vectorize"]
# the id a binary carries is embedded behind this marker, so that it can be read without loading the library
ID_MARKER = b"scsfm-source-id:"


def lib_sources(name):
    return sorted(glob.glob(os.path.join(find(name).csrc, "*.hip")))


# What a row's sources include from outside its own directory and header, by a relative path (no -I): the two trackers'
# point-to-plane ICP core.  It belongs to no row; the ids of the rows that include it cover it.
ICP_CORE = os.path.join(os.path.dirname(HERE), "csrc_icp", "scsfm_icp.h")
SHARED_DEPS = {"track": [ICP_CORE], "sim3": [ICP_CORE]}


def lib_deps(name):
    row = find(name)
    return lib_sources(name) + sorted(glob.glob(os.path.join(row.csrc, "*.h"))) + [row.header] + SHARED_DEPS.get(name, [])


def _hash(files, extra=()):
    h = hashlib.sha256()
    for path in files:
        h.update(os.path.basename(path).encode())
        h.update(open(path, "rb").read())
    h.update(" ".join(FLAGS).encode())
    if extra:
        h.update(b"\0extra:" + " ".join(extra).encode())
    return h.hexdigest()[:16]


def lib_source_id(name):
    """First 16 hex digits of the sha256 over everything the library is built from: its own sources (names and contents,
    sorted), its header, what SHARED_DEPS names for it and the compiler flags / target architecture.  It is compiled into
    the binary (<prefix>source_id) so that a loaded .so can be tied to the sources next to it."""
    return _hash(lib_deps(name))


def binary_source_id(path=LIB):
    """The source id compiled into the shared object at ``path``, read from the file (no dlopen: a stale or foreign
    binary may lack symbols the loader insists on).  None if there is no such file or it carries no id."""
    try:
        blob = open(path, "rb").read()
    except OSError:
        return None
    i = blob.find(ID_MARKER)
    if i < 0:
        return None
    j = i + len(ID_MARKER)
    return blob[j:j + 16].decode("ascii", "replace")


def lib_is_stale(name):
    """True when the in-tree library is missing or was built from other sources / flags than the tree's."""
    return binary_source_id(find(name).lib) != lib_source_id(name)


def build_lib(name, force=False, verbose=True):
    """Compile every .hip file of the row's source directory into its shared object.  Raises on failure.  Returns the
    library's path.  Without ``force`` nothing is compiled when the binary in place already carries the tree's source
    id -- also when that became true while this process was waiting for the lock (N ranks asking at once: one
    compiles)."""
    if not name:
        return build(force, verbose)  # (the loss library includes nothing from include/ by name: no -I)
    return _build(find(name).lib, lib_source_id(name), lib_sources(name), ("-I", INCLUDE), force, verbose)


# The loss library.  It alone takes ``extra`` compiler flags (tuning knobs), which its source id then covers.

sources = functools.partial(lib_sources, "")
deps = functools.partial(lib_deps, "")
is_stale = functools.partial(lib_is_stale, "")


def source_id(extra=()):
    """lib_source_id("") -- including any ``extra`` flags (-D tuning knobs) of a non-default build, so that a tuning
    variant can never carry the default library's id (bench.py ties PMC counters to a library by this id)."""
    files = deps()
    if any("SCSFM_WITH_MARCH" in e or "variants" in e for e in extra):
        # tuning builds compile the experimental kernels of variants/src/ in: an edit there must change the id too (round-5
        # advisor finding: PMC counters could be attributed to a stale variant binary)
        vsrc = os.path.join(os.path.dirname(os.path.dirname(HERE)), "variants", "src")
        files = files + sorted(p for p in glob.glob(os.path.join(vsrc, "*")) if os.path.isfile(p))
    return _hash(files, extra)


def build(force=False, verbose=True, extra=()):
    """build_lib("").  ``extra``: further compiler flags (tuning knobs); the binary then carries source_id(extra), which
    differs from the tree's default id, so the loader treats it as stale for the default configuration and rebuilds on
    the next plain get()."""
    extra = tuple(extra)
    return _build(LIB, source_id(extra), sources(), extra, force, verbose)


# Every other row, under its own names.
for _row in REGISTRY[1:]:
    globals().update({
        f"{_row.name.upper()}_CSRC": _row.csrc,
        f"{_row.name.upper()}_LIB": _row.lib,
        f"{_row.name}_sources": functools.partial(lib_sources, _row.name),
        f"{_row.name}_deps": functools.partial(lib_deps, _row.name),
        f"{_row.name}_source_id": functools.partial(lib_source_id, _row.name),
        f"{_row.name}_is_stale": functools.partial(lib_is_stale, _row.name),
        f"build_{_row.name}": functools.partial(build_lib, _row.name),
    })
del _row


@contextlib.contextmanager
def _build_lock(lock=None):
    fd = os.open(lock or LOCK, os.O_CREAT | os.O_RDWR, 0o644)
    try:
        fcntl.flock(fd, fcntl.LOCK_EX)
        yield
    finally:
        try:
            fcntl.flock(fd, fcntl.LOCK_UN)
        finally:
            os.close(fd)


def _build(lib, want, srcs, extra, force, verbose):
    if not force and binary_source_id(lib) == want:
        return lib
    with _build_lock(lib + ".lock"):
        # (another process may have built while this one waited for the lock)
        if not force and binary_source_id(lib) == want:
            return lib
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        name = os.path.basename(lib)
        if not os.path.exists(hipcc):
            raise RuntimeError(f"hipcc not found: {name} cannot be built on this machine")
        fd, tmp = tempfile.mkstemp(prefix=name[:-len(".so")] + ".", suffix=f".{os.getpid()}.tmp", dir=HERE)
        os.close(fd)
        try:
            cmd = [hipcc, *FLAGS, f'-DSCSFM_SOURCE_ID="{want}"', *extra, "-o", tmp, *srcs]
            if verbose:
                print("[scsfm_hip.build]", " ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
            os.chmod(tmp, 0o755)
            os.replace(tmp, lib)
            with open(lib + ".buildlog", "a") as f:  # who built what (tests/test_build_race.py counts the lines)
                f.write(f"{want} {os.getpid()}\n")
        finally:
            if os.path.exists(tmp):
                os.unlink(tmp)
    return lib


if __name__ == "__main__":
    for _row in REGISTRY:
        build_lib(_row.name, force="--force" in sys.argv)
    for _row in REGISTRY:
        print(_row.lib)
