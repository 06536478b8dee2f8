"""Build libscsfm_hip.so, libscsfm_nets.so, libscsfm_eval.so, libscsfm_odom.so, libscsfm_enc.so, libscsfm_stem.so,
libscsfm_snip.so, libscsfm_prep.so, libscsfm_vis.so, libscsfm_dvis.so, libscsfm_val.so, libscsfm_enceval.so,
libscsfm_decb.so, libscsfm_wrw.so, libscsfm_vlog.so and libscsfm_dgrad.so (gfx950) in-tree with hipcc.

    python -m scsfm_hip.build        (from sc-sfmlearner-release_amd/)

Each shared object is plain HIP + a C ABI (include/scsfm_hip.h: the loss path from csrc/*.hip; include/scsfm_nets.h:
the depth decoder's fused glue from csrc_nets/*.hip; include/scsfm_eval.h: depth evaluation from csrc_eval/*.hip;
include/scsfm_odom.h: odometry testing and evaluation from csrc_odom/*.hip; include/scsfm_enc.h: the ResNet encoder's
fused BatchNorm / ReLU / residual / max-pool glue from csrc_enc/*.hip; include/scsfm_stem.h: the stem's BatchNorm / ReLU
fused with its max-pool from csrc_stem/*.hip; include/scsfm_snip.h: the 5-frame snippet pose evaluation from
csrc_snip/*.hip; include/scsfm_prep.h: the resize and the Velodyne depth maps of data/prepare_train_data.py from
csrc_prep/*.hip; include/scsfm_vis.h: the input normalisation, the per-image maximum and the colour-mapped pictures of
run_inference.py from csrc_vis/*.hip; include/scsfm_dvis.h: the scaled prediction, the colour range and the magma
pictures of eval_depth.py --vis_dir from csrc_dvis/*.hip; include/scsfm_val.h: the ground-truth validation metrics of
train.py --with-gt from csrc_val/*.hip; include/scsfm_enceval.h: the ResNet encoder's eval-mode BatchNorm / ReLU / residual /
max-pool glue from csrc_enceval/*.hip; include/scsfm_decb.h: the depth decoder's glue with the convolutions' biases folded
in from csrc_decb/*.hip; include/scsfm_wrw.h: the weight gradient of the depth decoder's low-channel convolutions from
csrc_wrw/*.hip; include/scsfm_vlog.h: the validation pictures of train.py --log-output from csrc_vlog/*.hip;
include/scsfm_dgrad.h: the backward of the depth decoder's full-resolution tail from csrc_dgrad/*.hip); none links
against torch.  They are written next to this file so that they travel with the source tree to the GPU box.  They
are separate targets with separate source ids, so that an edit of the nets' or the evaluation's kernels leaves the loss
library's id (to which recorded PMC counters are tied) unchanged.

Safe for N processes at once (torchrun: every rank calls ``_lib.get()`` lazily, and ``*.so`` is git-ignored, so a fresh
clone on an 8-GPU node has no library): the build runs under an exclusive ``flock`` on ``libscsfm_hip.so.lock``, the
compiler writes to a name unique to the process and the result is moved into place atomically; a process that gets the
lock after another one has built finds a binary whose compiled-in source id matches and does not compile again.
"""
from __future__ import annotations

import contextlib
import fcntl
import glob
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "csrc")
LIB = os.path.join(HERE, "libscsfm_hip.so")
LOCK = LIB + ".lock"
LOG = LIB + ".buildlog"
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include")
NETS_CSRC = os.path.join(os.path.dirname(HERE), "csrc_nets")
NETS_LIB = os.path.join(HERE, "libscsfm_nets.so")
EVAL_CSRC = os.path.join(os.path.dirname(HERE), "csrc_eval")
EVAL_LIB = os.path.join(HERE, "libscsfm_eval.so")
ODOM_CSRC = os.path.join(os.path.dirname(HERE), "csrc_odom")
ODOM_LIB = os.path.join(HERE, "libscsfm_odom.so")
ENC_CSRC = os.path.join(os.path.dirname(HERE), "csrc_enc")
ENC_LIB = os.path.join(HERE, "libscsfm_enc.so")
STEM_CSRC = os.path.join(os.path.dirname(HERE), "csrc_stem")
STEM_LIB = os.path.join(HERE, "libscsfm_stem.so")
SNIP_CSRC = os.path.join(os.path.dirname(HERE), "csrc_snip")
SNIP_LIB = os.path.join(HERE, "libscsfm_snip.so")
PREP_CSRC = os.path.join(os.path.dirname(HERE), "csrc_prep")
PREP_LIB = os.path.join(HERE, "libscsfm_prep.so")
VIS_CSRC = os.path.join(os.path.dirname(HERE), "csrc_vis")
VIS_LIB = os.path.join(HERE, "libscsfm_vis.so")
DVIS_CSRC = os.path.join(os.path.dirname(HERE), "csrc_dvis")
DVIS_LIB = os.path.join(HERE, "libscsfm_dvis.so")
VAL_CSRC = os.path.join(os.path.dirname(HERE), "csrc_val")
VAL_LIB = os.path.join(HERE, "libscsfm_val.so")
ENCEVAL_CSRC = os.path.join(os.path.dirname(HERE), "csrc_enceval")
ENCEVAL_LIB = os.path.join(HERE, "libscsfm_enceval.so")
DECB_CSRC = os.path.join(os.path.dirname(HERE), "csrc_decb")
DECB_LIB = os.path.join(HERE, "libscsfm_decb.so")
WRW_CSRC = os.path.join(os.path.dirname(HERE), "csrc_wrw")
WRW_LIB = os.path.join(HERE, "libscsfm_wrw.so")
VLOG_CSRC = os.path.join(os.path.dirname(HERE), "csrc_vlog")
VLOG_LIB = os.path.join(HERE, "libscsfm_vlog.so")
DGRAD_CSRC = os.path.join(os.path.dirname(HERE), "csrc_dgrad")
DGRAD_LIB = os.path.join(HERE, "libscsfm_dgrad.so")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", f"--offload-arch={ARCH}", "-munsafe-fp-atomics",
         "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
         # the SLP vectoriser pairs unrelated scalar fp32 chains into v_pk_* with 4 v_mov per packed op (+5 % VALU
         # in the tiled pass); the 2-wide math that pays is written with vector types in csrc/scsfm_ssim.h
         "-fno-slp-vectorize"]
# the id a binary carries is embedded behind this marker, so that it can be read without loading the library
ID_MARKER = b"scsfm-source-id:"


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def deps():
    return sources() + sorted(glob.glob(os.path.join(CSRC, "*.h"))) + \
        [os.path.join(INCLUDE, "scsfm_hip.h")]


def nets_sources():
    return sorted(glob.glob(os.path.join(NETS_CSRC, "*.hip")))


def nets_deps():
    return nets_sources() + sorted(glob.glob(os.path.join(NETS_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_nets.h")]


def eval_sources():
    return sorted(glob.glob(os.path.join(EVAL_CSRC, "*.hip")))


def eval_deps():
    return eval_sources() + sorted(glob.glob(os.path.join(EVAL_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_eval.h")]


def odom_sources():
    return sorted(glob.glob(os.path.join(ODOM_CSRC, "*.hip")))


def odom_deps():
    return odom_sources() + sorted(glob.glob(os.path.join(ODOM_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_odom.h")]


def enc_sources():
    return sorted(glob.glob(os.path.join(ENC_CSRC, "*.hip")))


def enc_deps():
    return enc_sources() + sorted(glob.glob(os.path.join(ENC_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_enc.h")]


def stem_sources():
    return sorted(glob.glob(os.path.join(STEM_CSRC, "*.hip")))


def stem_deps():
    return stem_sources() + sorted(glob.glob(os.path.join(STEM_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_stem.h")]


def snip_sources():
    return sorted(glob.glob(os.path.join(SNIP_CSRC, "*.hip")))


def snip_deps():
    return snip_sources() + sorted(glob.glob(os.path.join(SNIP_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_snip.h")]


def prep_sources():
    return sorted(glob.glob(os.path.join(PREP_CSRC, "*.hip")))


def prep_deps():
    return prep_sources() + sorted(glob.glob(os.path.join(PREP_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_prep.h")]


def vis_sources():
    return sorted(glob.glob(os.path.join(VIS_CSRC, "*.hip")))


def vis_deps():
    return vis_sources() + sorted(glob.glob(os.path.join(VIS_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_vis.h")]


def dvis_sources():
    return sorted(glob.glob(os.path.join(DVIS_CSRC, "*.hip")))


def dvis_deps():
    return dvis_sources() + sorted(glob.glob(os.path.join(DVIS_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_dvis.h")]


def val_sources():
    return sorted(glob.glob(os.path.join(VAL_CSRC, "*.hip")))


def val_deps():
    return val_sources() + sorted(glob.glob(os.path.join(VAL_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_val.h")]


def enceval_sources():
    return sorted(glob.glob(os.path.join(ENCEVAL_CSRC, "*.hip")))


def enceval_deps():
    return enceval_sources() + sorted(glob.glob(os.path.join(ENCEVAL_CSRC, "*.h"))) + \
        [os.path.join(INCLUDE, "scsfm_enceval.h")]


def decb_sources():
    return sorted(glob.glob(os.path.join(DECB_CSRC, "*.hip")))


def decb_deps():
    return decb_sources() + sorted(glob.glob(os.path.join(DECB_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_decb.h")]


def wrw_sources():
    return sorted(glob.glob(os.path.join(WRW_CSRC, "*.hip")))


def wrw_deps():
    return wrw_sources() + sorted(glob.glob(os.path.join(WRW_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_wrw.h")]


def vlog_sources():
    return sorted(glob.glob(os.path.join(VLOG_CSRC, "*.hip")))


def vlog_deps():
    return vlog_sources() + sorted(glob.glob(os.path.join(VLOG_CSRC, "*.h"))) + [os.path.join(INCLUDE, "scsfm_vlog.h")]


def dgrad_sources():
    return sorted(glob.glob(os.path.join(DGRAD_CSRC, "*.hip")))


def dgrad_deps():
    return dgrad_sources() + sorted(glob.glob(os.path.join(DGRAD_CSRC, "*.h"))) + \
        [os.path.join(INCLUDE, "scsfm_dgrad.h")]


def _hash(files, extra=()):
    h = hashlib.sha256()
    for path in files:
        h.update(os.path.basename(path).encode())
        h.update(open(path, "rb").read())
    h.update(" ".join(FLAGS).encode())
    if extra:
        h.update(b"\0extra:" + " ".join(extra).encode())
    return h.hexdigest()[:16]


def source_id(extra=()):
    """First 16 hex digits of the sha256 over everything the library is built from: every source file (names and
    contents, sorted) and the compiler flags / target architecture -- including any ``extra`` flags (-D tuning knobs)
    of a non-default build, so that a tuning variant can never carry the default library's id (bench.py ties PMC
    counters to a library by this id).  It is compiled into the binary (scsfm_source_id) so that a loaded .so can be
    tied to the sources next to it."""
    files = deps()
    if any("SCSFM_WITH_MARCH" in e or "variants" in e for e in extra):
        # tuning builds compile the experimental kernels of variants/src/ in: an edit there must change the id too (round-5
        # advisor finding: PMC counters could be attributed to a stale variant binary)
        vsrc = os.path.join(os.path.dirname(os.path.dirname(HERE)), "variants", "src")
        files = files + sorted(p for p in glob.glob(os.path.join(vsrc, "*")) if os.path.isfile(p))
    return _hash(files, extra)


def nets_source_id():
    """source_id() of libscsfm_nets.so: its own sources (csrc_nets/, include/scsfm_nets.h) and the compiler flags."""
    return _hash(nets_deps())


def eval_source_id():
    """source_id() of libscsfm_eval.so: its own sources (csrc_eval/, include/scsfm_eval.h) and the compiler flags."""
    return _hash(eval_deps())


def odom_source_id():
    """source_id() of libscsfm_odom.so: its own sources (csrc_odom/, include/scsfm_odom.h) and the compiler flags."""
    return _hash(odom_deps())


def enc_source_id():
    """source_id() of libscsfm_enc.so: its own sources (csrc_enc/, include/scsfm_enc.h) and the compiler flags."""
    return _hash(enc_deps())


def stem_source_id():
    """source_id() of libscsfm_stem.so: its own sources (csrc_stem/, include/scsfm_stem.h) and the compiler flags."""
    return _hash(stem_deps())


def snip_source_id():
    """source_id() of libscsfm_snip.so: its own sources (csrc_snip/, include/scsfm_snip.h) and the compiler flags."""
    return _hash(snip_deps())


def prep_source_id():
    """source_id() of libscsfm_prep.so: its own sources (csrc_prep/, include/scsfm_prep.h) and the compiler flags."""
    return _hash(prep_deps())


def vis_source_id():
    """source_id() of libscsfm_vis.so: its own sources (csrc_vis/, include/scsfm_vis.h) and the compiler flags."""
    return _hash(vis_deps())


def dvis_source_id():
    """source_id() of libscsfm_dvis.so: its own sources (csrc_dvis/, include/scsfm_dvis.h) and the compiler flags."""
    return _hash(dvis_deps())


def val_source_id():
    """source_id() of libscsfm_val.so: its own sources (csrc_val/, include/scsfm_val.h) and the compiler flags."""
    return _hash(val_deps())


def enceval_source_id():
    """source_id() of libscsfm_enceval.so: its own sources (csrc_enceval/, include/scsfm_enceval.h) and the flags."""
    return _hash(enceval_deps())


def decb_source_id():
    """source_id() of libscsfm_decb.so: its own sources (csrc_decb/, include/scsfm_decb.h) and the compiler flags."""
    return _hash(decb_deps())


def wrw_source_id():
    """source_id() of libscsfm_wrw.so: its own sources (csrc_wrw/, include/scsfm_wrw.h) and the compiler flags."""
    return _hash(wrw_deps())


def vlog_source_id():
    """source_id() of libscsfm_vlog.so: its own sources (csrc_vlog/, include/scsfm_vlog.h) and the compiler flags."""
    return _hash(vlog_deps())


def dgrad_source_id():
    """source_id() of libscsfm_dgrad.so: its own sources (csrc_dgrad/, include/scsfm_dgrad.h) and the compiler flags."""
    return _hash(dgrad_deps())


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


def is_stale():
    """True when the in-tree library is missing or was built from other sources / flags than the tree's."""
    return binary_source_id(LIB) != source_id()


def nets_is_stale():
    return binary_source_id(NETS_LIB) != nets_source_id()


def eval_is_stale():
    return binary_source_id(EVAL_LIB) != eval_source_id()


def odom_is_stale():
    return binary_source_id(ODOM_LIB) != odom_source_id()


def enc_is_stale():
    return binary_source_id(ENC_LIB) != enc_source_id()


def stem_is_stale():
    return binary_source_id(STEM_LIB) != stem_source_id()


def snip_is_stale():
    return binary_source_id(SNIP_LIB) != snip_source_id()


def prep_is_stale():
    return binary_source_id(PREP_LIB) != prep_source_id()


def vis_is_stale():
    return binary_source_id(VIS_LIB) != vis_source_id()


def dvis_is_stale():
    return binary_source_id(DVIS_LIB) != dvis_source_id()


def val_is_stale():
    return binary_source_id(VAL_LIB) != val_source_id()


def enceval_is_stale():
    return binary_source_id(ENCEVAL_LIB) != enceval_source_id()


def decb_is_stale():
    return binary_source_id(DECB_LIB) != decb_source_id()


def wrw_is_stale():
    return binary_source_id(WRW_LIB) != wrw_source_id()


def vlog_is_stale():
    return binary_source_id(VLOG_LIB) != vlog_source_id()


def dgrad_is_stale():
    return binary_source_id(DGRAD_LIB) != dgrad_source_id()


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


def build(force=False, verbose=True, extra=()):
    """Compile every .hip file under csrc/ into one shared object.  Raises on failure.  Returns the library's path.
    Without ``force`` nothing is compiled when the binary in place already carries the tree's source id -- also when
    that became true while this process was waiting for the lock (N ranks asking at once: one compiles).  ``extra``:
    further compiler flags (tuning knobs); the binary then carries source_id(extra), which differs from the tree's
    default id, so the loader treats it as stale for the default configuration and rebuilds on the next plain get()."""
    extra = tuple(extra)
    return _build(LIB, source_id(extra), sources(), extra, force, verbose)


def build_nets(force=False, verbose=True):
    """build() for libscsfm_nets.so: every .hip file under csrc_nets/, against include/scsfm_nets.h."""
    return _build(NETS_LIB, nets_source_id(), nets_sources(), ("-I", INCLUDE), force, verbose)


def build_eval(force=False, verbose=True):
    """build() for libscsfm_eval.so: every .hip file under csrc_eval/, against include/scsfm_eval.h."""
    return _build(EVAL_LIB, eval_source_id(), eval_sources(), ("-I", INCLUDE), force, verbose)


def build_odom(force=False, verbose=True):
    """build() for libscsfm_odom.so: every .hip file under csrc_odom/, against include/scsfm_odom.h."""
    return _build(ODOM_LIB, odom_source_id(), odom_sources(), ("-I", INCLUDE), force, verbose)


def build_enc(force=False, verbose=True):
    """build() for libscsfm_enc.so: every .hip file under csrc_enc/, against include/scsfm_enc.h."""
    return _build(ENC_LIB, enc_source_id(), enc_sources(), ("-I", INCLUDE), force, verbose)


def build_stem(force=False, verbose=True):
    """build() for libscsfm_stem.so: every .hip file under csrc_stem/, against include/scsfm_stem.h."""
    return _build(STEM_LIB, stem_source_id(), stem_sources(), ("-I", INCLUDE), force, verbose)


def build_snip(force=False, verbose=True):
    """build() for libscsfm_snip.so: every .hip file under csrc_snip/, against include/scsfm_snip.h."""
    return _build(SNIP_LIB, snip_source_id(), snip_sources(), ("-I", INCLUDE), force, verbose)


def build_prep(force=False, verbose=True):
    """build() for libscsfm_prep.so: every .hip file under csrc_prep/, against include/scsfm_prep.h."""
    return _build(PREP_LIB, prep_source_id(), prep_sources(), ("-I", INCLUDE), force, verbose)


def build_vis(force=False, verbose=True):
    """build() for libscsfm_vis.so: every .hip file under csrc_vis/, against include/scsfm_vis.h."""
    return _build(VIS_LIB, vis_source_id(), vis_sources(), ("-I", INCLUDE), force, verbose)


def build_dvis(force=False, verbose=True):
    """build() for libscsfm_dvis.so: every .hip file under csrc_dvis/, against include/scsfm_dvis.h."""
    return _build(DVIS_LIB, dvis_source_id(), dvis_sources(), ("-I", INCLUDE), force, verbose)


def build_val(force=False, verbose=True):
    """build() for libscsfm_val.so: every .hip file under csrc_val/, against include/scsfm_val.h."""
    return _build(VAL_LIB, val_source_id(), val_sources(), ("-I", INCLUDE), force, verbose)


def build_enceval(force=False, verbose=True):
    """build() for libscsfm_enceval.so: every .hip file under csrc_enceval/, against include/scsfm_enceval.h."""
    return _build(ENCEVAL_LIB, enceval_source_id(), enceval_sources(), ("-I", INCLUDE), force, verbose)


def build_decb(force=False, verbose=True):
    """build() for libscsfm_decb.so: every .hip file under csrc_decb/, against include/scsfm_decb.h."""
    return _build(DECB_LIB, decb_source_id(), decb_sources(), ("-I", INCLUDE), force, verbose)


def build_wrw(force=False, verbose=True):
    """build() for libscsfm_wrw.so: every .hip file under csrc_wrw/, against include/scsfm_wrw.h."""
    return _build(WRW_LIB, wrw_source_id(), wrw_sources(), ("-I", INCLUDE), force, verbose)


def build_vlog(force=False, verbose=True):
    """build() for libscsfm_vlog.so: every .hip file under csrc_vlog/, against include/scsfm_vlog.h."""
    return _build(VLOG_LIB, vlog_source_id(), vlog_sources(), ("-I", INCLUDE), force, verbose)


def build_dgrad(force=False, verbose=True):
    """build() for libscsfm_dgrad.so: every .hip file under csrc_dgrad/, against include/scsfm_dgrad.h."""
    return _build(DGRAD_LIB, dgrad_source_id(), dgrad_sources(), ("-I", INCLUDE), force, verbose)


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
    build(force="--force" in sys.argv)
    build_nets(force="--force" in sys.argv)
    build_eval(force="--force" in sys.argv)
    build_odom(force="--force" in sys.argv)
    build_enc(force="--force" in sys.argv)
    build_stem(force="--force" in sys.argv)
    build_snip(force="--force" in sys.argv)
    build_prep(force="--force" in sys.argv)
    build_vis(force="--force" in sys.argv)
    build_dvis(force="--force" in sys.argv)
    build_val(force="--force" in sys.argv)
    build_enceval(force="--force" in sys.argv)
    build_decb(force="--force" in sys.argv)
    build_wrw(force="--force" in sys.argv)
    build_vlog(force="--force" in sys.argv)
    build_dgrad(force="--force" in sys.argv)
    print(LIB)
    print(NETS_LIB)
    print(EVAL_LIB)
    print(ODOM_LIB)
    print(ENC_LIB)
    print(STEM_LIB)
    print(SNIP_LIB)
    print(PREP_LIB)
    print(VIS_LIB)
    print(DVIS_LIB)
    print(VAL_LIB)
    print(ENCEVAL_LIB)
    print(DECB_LIB)
    print(WRW_LIB)
    print(VLOG_LIB)
    print(DGRAD_LIB)
