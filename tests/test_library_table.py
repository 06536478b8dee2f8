"""scsfm_hip/libraries.py's table as a whole (no compiler, no GPU): sixteen rows with names, outputs, headers and
prefixes of their own; every library hashes only its own sources, so no two source ids agree and no edit of one library
changes another's id (the all-pairs form of what the per-library tests assert for the libraries that came before them);
every header declares its version and its source id under the row's prefix; the names scsfm_hip.build and
scsfm_hip._lib give each row are there and are the row's; and build() reports every row once."""
import os
import sys

from scsfm_hip import _lib, build
from scsfm_hip.libraries import TABLE, Library

NAMES = ("", "nets", "eval", "odom", "enc", "stem", "snip", "prep", "vis", "dvis", "val", "enceval", "decb", "wrw", "vlog",
         "dgrad")


def test_sixteen_rows_each_with_files_of_its_own():
    assert tuple(row.name for row in TABLE) == NAMES
    assert all(isinstance(row, Library) and row.abi >= 1 and row.tag and row.what for row in TABLE)
    for column in ("csrc", "header", "lib", "prefix"):
        assert len({getattr(row, column) for row in TABLE}) == 16, column
    pkg = os.path.dirname(os.path.abspath(build.__file__))
    for row in TABLE:
        stem = "scsfm_" + (row.name or "hip")
        assert row.csrc == os.path.join(os.path.dirname(pkg), "csrc_" + row.name if row.name else "csrc")
        assert row.header == os.path.join(build.INCLUDE, stem + ".h") and os.path.isfile(row.header), row.name
        assert row.lib == os.path.join(pkg, "lib" + stem + ".so")
        assert row.prefix == ("scsfm_" + row.name + "_" if row.name else "scsfm_")


def test_every_library_hashes_only_its_own_sources():
    ids = {}
    for row in TABLE:
        srcs, deps = build.lib_sources(row.name), build.lib_deps(row.name)
        assert srcs and all(p.startswith(row.csrc + os.sep) and p.endswith(".hip") for p in srcs), row.name
        assert deps[:len(srcs)] == srcs and deps[-1] == row.header, row.name
        assert all(p.startswith(row.csrc + os.sep) or p == row.header for p in deps), row.name
        ids[row.name] = build.lib_source_id(row.name)
        assert len(ids[row.name]) == 16 and int(ids[row.name], 16) >= 0
    assert len(set(ids.values())) == len(TABLE)


def test_every_header_declares_its_version_and_source_id():
    for row in TABLE:
        decls = _lib.parse_header(row.header)
        assert row.prefix + "abi_version" in decls and row.prefix + "source_id" in decls, row.name
        assert all(name.startswith(row.prefix) for name in decls), row.name


def test_the_names_of_every_row_are_the_rows():
    for row in TABLE:
        p = row.name + "_" if row.name else ""
        assert getattr(build, p.upper() + "CSRC") == row.csrc and getattr(build, p.upper() + "LIB") == row.lib
        assert getattr(build, p + "sources")() == build.lib_sources(row.name)
        assert getattr(build, p + "deps")() == build.lib_deps(row.name)
        assert getattr(build, p + "source_id")() == build.lib_source_id(row.name)
        assert getattr(build, p + "is_stale")() == build.lib_is_stale(row.name)
        assert callable(getattr(build, "build_" + row.name if row.name else "build"))
        assert getattr(_lib, p.upper() + "HEADER") == row.header
        assert getattr(_lib, p.upper() + "ABI_VERSION") == row.abi
        assert getattr(_lib, p.upper() + "LIB_PATH") == (os.environ.get("SCSFM_HIP_LIB") or row.lib if not row.name
                                                         else row.lib)
        getter = getattr(_lib, "get_" + row.name if row.name else "get")
        assert callable(getter) and row.what in getter.__doc__
    assert build.LOCK == build.LIB + ".lock" and build.LOG == build.LIB + ".buildlog" and build.ARCH == "gfx950"
    assert build.HERE == os.path.dirname(os.path.abspath(build.__file__))
    assert build.source_id(()) == build.lib_source_id("")
    assert all(isinstance(t, type) for t in (_lib.CLib, _lib.ScsfmError)) and callable(_lib.parse_header)


def test_build_reports_every_row_once():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as G
    assert sorted(G.REPORT_ORDER) == sorted(NAMES)
