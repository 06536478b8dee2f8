"""ctypes binding of the C ABI declared in include/scsfm_hip.h.

``get()`` returns the product library, libscsfm_hip.so (hipcc, gfx950), and nothing else: if the
shared object is missing it is built in-tree with hipcc, and if that is impossible the call raises
-- there is no CPU or eager fallback anywhere in this package.
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

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_hip.h")
# SCSFM_HIP_LIB points at a library built elsewhere (tuning variants, a system-wide install)
LIB_PATH = os.environ.get("SCSFM_HIP_LIB") or os.path.join(HERE, "libscsfm_hip.so")

ABI_VERSION = 9  # include/scsfm_hip.h

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
        """The source hash compiled into the binary (scsfm_hip/build.py: source_id / nets_source_id)."""
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


_lock = threading.Lock()
_lib = None


def get() -> CLib:
    """The HIP library (singleton).  Ties the binary to the sources next to it BEFORE loading it: the source id compiled
    into libscsfm_hip.so is read from the file (scsfm_hip.build.binary_source_id -- a stale binary may lack symbols or
    carry another ABI number, which the strict loader below would report as an error instead of rebuilding), and a
    missing or stale library is built with hipcc under a file lock, so that the N ranks of a torchrun job that all
    arrive here at once compile once.  Without hipcc a stale library is refused.  A library named by SCSFM_HIP_LIB (a
    tuning variant, a system-wide install) is taken as it is."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                from . import build as _build
                own = "SCSFM_HIP_LIB" not in os.environ
                if own and _build.is_stale():
                    have = _build.binary_source_id(LIB_PATH)
                    try:
                        _build.build()
                    except Exception as e:
                        what = f"was built from other sources ({have}) than the tree's ({_build.source_id()})" if have \
                            else "is missing (or carries no source id)"
                        raise ScsfmError(f"{LIB_PATH} {what} and cannot be built here: {e}") from e
                lib = CLib(LIB_PATH)
                if own and lib.source_id() != _build.source_id():
                    raise ScsfmError(f"{LIB_PATH}: its source id {lib.source_id()} is not the tree's {_build.source_id()}")
                _lib = lib
    return _lib


NETS_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_nets.h")
NETS_LIB_PATH = os.path.join(HERE, "libscsfm_nets.so")
NETS_ABI_VERSION = 1  # include/scsfm_nets.h
_nets = None


def get_nets() -> CLib:
    """The nets library, libscsfm_nets.so (singleton): the fused glue of the depth decoder (include/scsfm_nets.h).
    Built in-tree with hipcc when it is missing or stale, under the same file-lock scheme as ``get()``; raises when that
    is impossible."""
    global _nets
    if _nets is None:
        with _lock:
            if _nets is None:
                from . import build as _build
                if _build.nets_is_stale():
                    have = _build.binary_source_id(NETS_LIB_PATH)
                    try:
                        _build.build_nets()
                    except Exception as e:
                        raise ScsfmError(f"{NETS_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(NETS_LIB_PATH, NETS_HEADER, NETS_ABI_VERSION, "scsfm_nets_")
                if lib.source_id() != _build.nets_source_id():
                    raise ScsfmError(f"{NETS_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.nets_source_id()}")
                _nets = lib
    return _nets


EVAL_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_eval.h")
EVAL_LIB_PATH = os.path.join(HERE, "libscsfm_eval.so")
EVAL_ABI_VERSION = 1  # include/scsfm_eval.h
_eval = None


def get_eval() -> CLib:
    """The evaluation library, libscsfm_eval.so (singleton): depth evaluation with median scaling
    (include/scsfm_eval.h).  Built in-tree with hipcc when it is missing or stale, under the same file-lock scheme as
    ``get()``; raises when that is impossible."""
    global _eval
    if _eval is None:
        with _lock:
            if _eval is None:
                from . import build as _build
                if _build.eval_is_stale():
                    have = _build.binary_source_id(EVAL_LIB_PATH)
                    try:
                        _build.build_eval()
                    except Exception as e:
                        raise ScsfmError(f"{EVAL_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(EVAL_LIB_PATH, EVAL_HEADER, EVAL_ABI_VERSION, "scsfm_eval_")
                if lib.source_id() != _build.eval_source_id():
                    raise ScsfmError(f"{EVAL_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.eval_source_id()}")
                _eval = lib
    return _eval


ODOM_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_odom.h")
ODOM_LIB_PATH = os.path.join(HERE, "libscsfm_odom.so")
ODOM_ABI_VERSION = 1  # include/scsfm_odom.h
_odom = None


def get_odom() -> CLib:
    """The odometry library, libscsfm_odom.so (singleton): the pose chain of test_vo.py and KITTI odometry evaluation
    (include/scsfm_odom.h).  Built in-tree with hipcc when it is missing or stale, under the same file-lock scheme as
    ``get()``; raises when that is impossible."""
    global _odom
    if _odom is None:
        with _lock:
            if _odom is None:
                from . import build as _build
                if _build.odom_is_stale():
                    have = _build.binary_source_id(ODOM_LIB_PATH)
                    try:
                        _build.build_odom()
                    except Exception as e:
                        raise ScsfmError(f"{ODOM_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(ODOM_LIB_PATH, ODOM_HEADER, ODOM_ABI_VERSION, "scsfm_odom_")
                if lib.source_id() != _build.odom_source_id():
                    raise ScsfmError(f"{ODOM_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.odom_source_id()}")
                _odom = lib
    return _odom


ENC_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_enc.h")
ENC_LIB_PATH = os.path.join(HERE, "libscsfm_enc.so")
ENC_ABI_VERSION = 1  # include/scsfm_enc.h
_enc = None


def get_enc() -> CLib:
    """The encoder library, libscsfm_enc.so (singleton): the ResNet encoder's fused BatchNorm / ReLU / residual add and
    max-pool (include/scsfm_enc.h).  Built in-tree with hipcc when it is missing or stale, under the same file-lock
    scheme as ``get()``; raises when that is impossible."""
    global _enc
    if _enc is None:
        with _lock:
            if _enc is None:
                from . import build as _build
                if _build.enc_is_stale():
                    have = _build.binary_source_id(ENC_LIB_PATH)
                    try:
                        _build.build_enc()
                    except Exception as e:
                        raise ScsfmError(f"{ENC_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(ENC_LIB_PATH, ENC_HEADER, ENC_ABI_VERSION, "scsfm_enc_")
                if lib.source_id() != _build.enc_source_id():
                    raise ScsfmError(f"{ENC_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.enc_source_id()}")
                _enc = lib
    return _enc


STEM_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_stem.h")
STEM_LIB_PATH = os.path.join(HERE, "libscsfm_stem.so")
STEM_ABI_VERSION = 1  # include/scsfm_stem.h
_stem = None


def get_stem() -> CLib:
    """The stem library, libscsfm_stem.so (singleton): the ResNet stem's BatchNorm / ReLU fused with its max-pool
    (include/scsfm_stem.h).  Built in-tree with hipcc when it is missing or stale, under the same file-lock scheme as
    ``get()``; raises when that is impossible."""
    global _stem
    if _stem is None:
        with _lock:
            if _stem is None:
                from . import build as _build
                if _build.stem_is_stale():
                    have = _build.binary_source_id(STEM_LIB_PATH)
                    try:
                        _build.build_stem()
                    except Exception as e:
                        raise ScsfmError(f"{STEM_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(STEM_LIB_PATH, STEM_HEADER, STEM_ABI_VERSION, "scsfm_stem_")
                if lib.source_id() != _build.stem_source_id():
                    raise ScsfmError(f"{STEM_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.stem_source_id()}")
                _stem = lib
    return _stem


SNIP_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_snip.h")
SNIP_LIB_PATH = os.path.join(HERE, "libscsfm_snip.so")
SNIP_ABI_VERSION = 1  # include/scsfm_snip.h
_snip = None


def get_snip() -> CLib:
    """The snippet library, libscsfm_snip.so (singleton): test_pose.py's 5-frame snippet pose evaluation
    (include/scsfm_snip.h).  Built in-tree with hipcc when it is missing or stale, under the same file-lock scheme as
    ``get()``; raises when that is impossible."""
    global _snip
    if _snip is None:
        with _lock:
            if _snip is None:
                from . import build as _build
                if _build.snip_is_stale():
                    have = _build.binary_source_id(SNIP_LIB_PATH)
                    try:
                        _build.build_snip()
                    except Exception as e:
                        raise ScsfmError(f"{SNIP_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(SNIP_LIB_PATH, SNIP_HEADER, SNIP_ABI_VERSION, "scsfm_snip_")
                if lib.source_id() != _build.snip_source_id():
                    raise ScsfmError(f"{SNIP_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.snip_source_id()}")
                _snip = lib
    return _snip


PREP_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_prep.h")
PREP_LIB_PATH = os.path.join(HERE, "libscsfm_prep.so")
PREP_ABI_VERSION = 1  # include/scsfm_prep.h
_prep = None


def get_prep() -> CLib:
    """The preparation library, libscsfm_prep.so (singleton): the resize and the Velodyne depth maps of
    data/prepare_train_data.py (include/scsfm_prep.h).  Built in-tree with hipcc when it is missing or stale, under the
    same file-lock scheme as ``get()``; raises when that is impossible."""
    global _prep
    if _prep is None:
        with _lock:
            if _prep is None:
                from . import build as _build
                if _build.prep_is_stale():
                    have = _build.binary_source_id(PREP_LIB_PATH)
                    try:
                        _build.build_prep()
                    except Exception as e:
                        raise ScsfmError(f"{PREP_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(PREP_LIB_PATH, PREP_HEADER, PREP_ABI_VERSION, "scsfm_prep_")
                if lib.source_id() != _build.prep_source_id():
                    raise ScsfmError(f"{PREP_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.prep_source_id()}")
                _prep = lib
    return _prep


VIS_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_vis.h")
VIS_LIB_PATH = os.path.join(HERE, "libscsfm_vis.so")
VIS_ABI_VERSION = 1  # include/scsfm_vis.h
_vis = None


def get_vis() -> CLib:
    """The visualisation library, libscsfm_vis.so (singleton): the input normalisation, the per-image maximum and the
    colour-mapped pictures of run_inference.py (include/scsfm_vis.h).  Built in-tree with hipcc when it is missing or
    stale, under the same file-lock scheme as ``get()``; raises when that is impossible."""
    global _vis
    if _vis is None:
        with _lock:
            if _vis is None:
                from . import build as _build
                if _build.vis_is_stale():
                    have = _build.binary_source_id(VIS_LIB_PATH)
                    try:
                        _build.build_vis()
                    except Exception as e:
                        raise ScsfmError(f"{VIS_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(VIS_LIB_PATH, VIS_HEADER, VIS_ABI_VERSION, "scsfm_vis_")
                if lib.source_id() != _build.vis_source_id():
                    raise ScsfmError(f"{VIS_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.vis_source_id()}")
                _vis = lib
    return _vis


DVIS_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_dvis.h")
DVIS_LIB_PATH = os.path.join(HERE, "libscsfm_dvis.so")
DVIS_ABI_VERSION = 1  # include/scsfm_dvis.h
_dvis = None


def get_dvis() -> CLib:
    """The depth visualisation library, libscsfm_dvis.so (singleton): the scaled prediction at the ground truth's size,
    the colour range and the magma pictures of eval_depth.py --vis_dir (include/scsfm_dvis.h).  Built in-tree with hipcc
    when it is missing or stale, under the same file-lock scheme as ``get()``; raises when that is impossible."""
    global _dvis
    if _dvis is None:
        with _lock:
            if _dvis is None:
                from . import build as _build
                if _build.dvis_is_stale():
                    have = _build.binary_source_id(DVIS_LIB_PATH)
                    try:
                        _build.build_dvis()
                    except Exception as e:
                        raise ScsfmError(f"{DVIS_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(DVIS_LIB_PATH, DVIS_HEADER, DVIS_ABI_VERSION, "scsfm_dvis_")
                if lib.source_id() != _build.dvis_source_id():
                    raise ScsfmError(f"{DVIS_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.dvis_source_id()}")
                _dvis = lib
    return _dvis


VAL_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_val.h")
VAL_LIB_PATH = os.path.join(HERE, "libscsfm_val.so")
VAL_ABI_VERSION = 1  # include/scsfm_val.h
_val = None


def get_val() -> CLib:
    """The validation library, libscsfm_val.so (singleton): the ground-truth validation metrics of train.py --with-gt
    (include/scsfm_val.h).  Built in-tree with hipcc when it is missing or stale, under the same file-lock scheme as
    ``get()``; raises when that is impossible."""
    global _val
    if _val is None:
        with _lock:
            if _val is None:
                from . import build as _build
                if _build.val_is_stale():
                    have = _build.binary_source_id(VAL_LIB_PATH)
                    try:
                        _build.build_val()
                    except Exception as e:
                        raise ScsfmError(f"{VAL_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(VAL_LIB_PATH, VAL_HEADER, VAL_ABI_VERSION, "scsfm_val_")
                if lib.source_id() != _build.val_source_id():
                    raise ScsfmError(f"{VAL_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.val_source_id()}")
                _val = lib
    return _val


ENCEVAL_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_enceval.h")
ENCEVAL_LIB_PATH = os.path.join(HERE, "libscsfm_enceval.so")
ENCEVAL_ABI_VERSION = 1  # include/scsfm_enceval.h
_enceval = None


def get_enceval() -> CLib:
    """The eval-mode encoder library, libscsfm_enceval.so (singleton): the ResNet encoder's BatchNorm from the running
    statistics fused with the ReLU / residual add, and the stem's max-pool (include/scsfm_enceval.h).  Built in-tree with
    hipcc when it is missing or stale, under the same file-lock scheme as ``get()``; raises when that is impossible."""
    global _enceval
    if _enceval is None:
        with _lock:
            if _enceval is None:
                from . import build as _build
                if _build.enceval_is_stale():
                    have = _build.binary_source_id(ENCEVAL_LIB_PATH)
                    try:
                        _build.build_enceval()
                    except Exception as e:
                        raise ScsfmError(f"{ENCEVAL_LIB_PATH} is stale or missing ({have}) and cannot be built here: "
                                         f"{e}") from e
                lib = CLib(ENCEVAL_LIB_PATH, ENCEVAL_HEADER, ENCEVAL_ABI_VERSION, "scsfm_enceval_")
                if lib.source_id() != _build.enceval_source_id():
                    raise ScsfmError(f"{ENCEVAL_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.enceval_source_id()}")
                _enceval = lib
    return _enceval


DECB_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_decb.h")
DECB_LIB_PATH = os.path.join(HERE, "libscsfm_decb.so")
DECB_ABI_VERSION = 1  # include/scsfm_decb.h
_decb = None


def get_decb() -> CLib:
    """The decoder-bias library, libscsfm_decb.so (singleton): the depth decoder's fused glue with the biases of its
    convolutions folded in (include/scsfm_decb.h).  Built in-tree with hipcc when it is missing or stale, under the same
    file-lock scheme as ``get()``; raises when that is impossible."""
    global _decb
    if _decb is None:
        with _lock:
            if _decb is None:
                from . import build as _build
                if _build.decb_is_stale():
                    have = _build.binary_source_id(DECB_LIB_PATH)
                    try:
                        _build.build_decb()
                    except Exception as e:
                        raise ScsfmError(f"{DECB_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(DECB_LIB_PATH, DECB_HEADER, DECB_ABI_VERSION, "scsfm_decb_")
                if lib.source_id() != _build.decb_source_id():
                    raise ScsfmError(f"{DECB_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.decb_source_id()}")
                _decb = lib
    return _decb


WRW_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_wrw.h")
WRW_LIB_PATH = os.path.join(HERE, "libscsfm_wrw.so")
WRW_ABI_VERSION = 1  # include/scsfm_wrw.h
_wrw = None


def get_wrw() -> CLib:
    """The weight-gradient library, libscsfm_wrw.so (singleton): the weight gradient of the depth decoder's low-channel
    3x3 convolutions on the fp32 matrix instruction (include/scsfm_wrw.h).  Built in-tree with hipcc when it is missing
    or stale, under the same file-lock scheme as ``get()``; raises when that is impossible."""
    global _wrw
    if _wrw is None:
        with _lock:
            if _wrw is None:
                from . import build as _build
                if _build.wrw_is_stale():
                    have = _build.binary_source_id(WRW_LIB_PATH)
                    try:
                        _build.build_wrw()
                    except Exception as e:
                        raise ScsfmError(f"{WRW_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(WRW_LIB_PATH, WRW_HEADER, WRW_ABI_VERSION, "scsfm_wrw_")
                if lib.source_id() != _build.wrw_source_id():
                    raise ScsfmError(f"{WRW_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.wrw_source_id()}")
                _wrw = lib
    return _wrw


VLOG_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_vlog.h")
VLOG_LIB_PATH = os.path.join(HERE, "libscsfm_vlog.so")
VLOG_ABI_VERSION = 1  # include/scsfm_vlog.h
_vlog = None


def get_vlog() -> CLib:
    """The validation-log library, libscsfm_vlog.so (singleton): the validation pictures of train.py --log-output
    (include/scsfm_vlog.h).  Built in-tree with hipcc when it is missing or stale, under the same file-lock scheme as
    ``get()``; raises when that is impossible."""
    global _vlog
    if _vlog is None:
        with _lock:
            if _vlog is None:
                from . import build as _build
                if _build.vlog_is_stale():
                    have = _build.binary_source_id(VLOG_LIB_PATH)
                    try:
                        _build.build_vlog()
                    except Exception as e:
                        raise ScsfmError(f"{VLOG_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(VLOG_LIB_PATH, VLOG_HEADER, VLOG_ABI_VERSION, "scsfm_vlog_")
                if lib.source_id() != _build.vlog_source_id():
                    raise ScsfmError(f"{VLOG_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.vlog_source_id()}")
                _vlog = lib
    return _vlog


DGRAD_HEADER = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include", "scsfm_dgrad.h")
DGRAD_LIB_PATH = os.path.join(HERE, "libscsfm_dgrad.so")
DGRAD_ABI_VERSION = 1  # include/scsfm_dgrad.h
_dgrad = None


def get_dgrad() -> CLib:
    """The tail-backward library, libscsfm_dgrad.so (singleton): the backward of the depth decoder's full-resolution
    tail (ELU / pad / disparity head) as one streaming kernel (include/scsfm_dgrad.h).  Built in-tree with hipcc when it
    is missing or stale, under the same file-lock scheme as ``get()``; raises when that is impossible."""
    global _dgrad
    if _dgrad is None:
        with _lock:
            if _dgrad is None:
                from . import build as _build
                if _build.dgrad_is_stale():
                    have = _build.binary_source_id(DGRAD_LIB_PATH)
                    try:
                        _build.build_dgrad()
                    except Exception as e:
                        raise ScsfmError(f"{DGRAD_LIB_PATH} is stale or missing ({have}) and cannot be built here: {e}") \
                            from e
                lib = CLib(DGRAD_LIB_PATH, DGRAD_HEADER, DGRAD_ABI_VERSION, "scsfm_dgrad_")
                if lib.source_id() != _build.dgrad_source_id():
                    raise ScsfmError(f"{DGRAD_LIB_PATH}: its source id {lib.source_id()} is not the tree's "
                                     f"{_build.dgrad_source_id()}")
                _dgrad = lib
    return _dgrad
