"""The one table of the HIP libraries.  scsfm_hip/build.py compiles its rows, scsfm_hip/_lib.py loads them,
__graft_entry__.build() reports them and tests/hostsim/library.py compiles them for the host simulator.

A row holds what cannot be derived: the short name ("" for the loss library), the ABI version its header states, the
tag build() reports it under and one line on what it computes.  The source directory, the header, the shared object and
the symbol prefix follow from the short name.  ``TABLE`` is the sixteen rows whose number and order tests pin; a library
added since goes into ``LATER``, and ``BY_NAME`` covers both; their number and ``BY_NAME``'s keys are pinned as well, so
rows added after those go into ``NEWER``.  ``ROWS`` is those three together, pinned in its turn, so rows added since stand
in ``NEWEST``; ``EVERY``, pinned as ``ROWS + NEWEST``, is those four, so rows added since stand in ``NEXT``; ``ALL``, pinned
as ``EVERY + NEXT`` with twenty rows, is those five, so rows added since stand in ``BEYOND``; ``LIBRARIES``, pinned
as ``ALL + BEYOND`` with twenty-one rows, is those six, and ``SUMMARY`` lists them, one line each, pinned too; so rows added
since stand in ``FURTHER``.  ``CATALOGUE``, pinned as ``LIBRARIES + FURTHER`` with twenty-two rows, is those seven.

``ADDED`` ends the ratchet: it is the open-ended tuple.  Every library added from libscsfm_track.so on (libscsfm_conf.so
is the second, libscsfm_roll.so the third, libscsfm_sim3.so the fourth) is appended to it, and no test pins its length or its contents -- a test asserts that its own row is in it.  ``REGISTRY`` is
``CATALOGUE + ADDED``, every row: the loops that build, load and name the libraries run over it, and ``find(name)`` looks
a row up among all of them.  Imports nothing but os, so that scsfm_hip._lib can read it on import.
"""
from __future__ import annotations

import os
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include")


class Library(NamedTuple):
    name: str  # "" for the loss library
    abi: int   # what <prefix>abi_version() returns, as include/<header> states it
    tag: str   # __graft_entry__.build() prints "[<tag>] <path>: <n> entry points resolved"
    what: str

    @property
    def csrc(self):
        return os.path.join(os.path.dirname(HERE), "csrc_" + self.name if self.name else "csrc")

    @property
    def header(self):
        return os.path.join(INCLUDE, f"scsfm_{self.name or 'hip'}.h")

    @property
    def lib(self):
        return os.path.join(HERE, f"libscsfm_{self.name or 'hip'}.so")

    @property
    def prefix(self):
        return f"scsfm_{self.name}_" if self.name else "scsfm_"


TABLE = (
    Library("", 9, "build", "the loss path"),
    Library("nets", 1, "build", "the depth decoder's fused glue"),
    Library("eval", 1, "build", "depth evaluation with median scaling"),
    Library("odom", 1, "build", "the pose chain of test_vo.py and KITTI odometry evaluation"),
    Library("enc", 1, "build", "the ResNet encoder's fused BatchNorm / ReLU / residual / max-pool glue"),
    Library("stem", 1, "build", "the ResNet stem's BatchNorm / ReLU fused with its max-pool"),
    Library("snip", 1, "build", "the 5-frame snippet pose evaluation of test_pose.py"),
    Library("prep", 1, "build:prep", "the resize and the Velodyne depth maps of data/prepare_train_data.py"),
    Library("vis", 1, "build:vis", "the input normalisation, the per-image maximum and the colour-mapped pictures of "
                                   "run_inference.py"),
    Library("dvis", 1, "build:dvis", "the scaled prediction, the colour range and the magma pictures of eval_depth.py "
                                     "--vis_dir"),
    Library("val", 2, "val:build", "the validation pass of train.py: the ground-truth metrics of --with-gt and the "
                                   "per-batch table of --shard-validation"),
    Library("enceval", 1, "enceval:build", "the ResNet encoder's eval-mode BatchNorm / ReLU / residual / max-pool glue"),
    Library("decb", 1, "decb:build", "the depth decoder's glue with the convolutions' biases folded in"),
    Library("wrw", 1, "wrw:build", "the weight gradient of the depth decoder's low-channel 3x3 convolutions"),
    Library("vlog", 1, "vlog:build", "the validation pictures of train.py --log-output"),
    Library("dgrad", 1, "dgrad:build", "the backward of the depth decoder's full-resolution tail"),
)
# Rows added after the table of sixteen was fixed: the same kind of row, built, loaded and reported in the same way.
LATER = (
    Library("fbn", 1, "fbn:build", "the backward of the ResNet encoder's BatchNorm with frozen statistics (train.py "
                                   "--freeze-bn)"),
)
BY_NAME = {row.name: row for row in TABLE + LATER}
# Rows added after LATER and the keys of BY_NAME were fixed in their turn.  build() reports these ahead of LATER's, in a
# wording of their own: "[<tag>] <path>: <n> entry points resolved (ABI <abi>)".
NEWER = (
    Library("opt", 1, "opt:build", "Adam over every parameter tensor in one launch (train.py --optimizer hip)"),
)
ROWS = TABLE + LATER + NEWER
# Rows added after ROWS was fixed as the sum of those three.  build() reports these directly behind NEWER's, in NEWER's
# wording.
NEWEST = (
    Library("pw", 1, "pw:build", "the weight and stride-2 data gradients of the encoders' 1x1 down-sample convolutions"),
)
EVERY = ROWS + NEWEST
# Rows added after EVERY was fixed as the sum of ROWS and NEWEST.  build() reports these directly behind LATER's lines, in
# NEWER's wording (the lines that end in "entry points resolved" are counted).
NEXT = (
    Library("fuse", 1, "fuse:build", "the TSDF fusion of predicted depth and poses and the surface points of "
                                     "reconstruct.py"),
)
ALL = EVERY + NEXT
# Rows added after ALL was fixed as the sum of EVERY and NEXT.  build() reports these directly behind dgrad's line, in
# NEWER's wording.
BEYOND = (
    Library("mesh", 1, "mesh:build", "the triangle mesh of a fused volume's surface by marching tetrahedra (reconstruct.py "
                                     "--mesh)"),
)
LIBRARIES = ALL + BEYOND
# Rows added after LIBRARIES was fixed as the sum of ALL and BEYOND, and SUMMARY as its lines.  build() reports these ahead
# of every other line, in a wording of their own: "[<tag>] <path>: ABI <abi>, <n> symbols of include/<header>".
FURTHER = (
    Library("cast", 1, "cast:build", "the ray cast of a fused volume from camera poses: depth, normals, colour and shaded "
                                     "pictures (reconstruct.py --render)"),
)
CATALOGUE = LIBRARIES + FURTHER
# Rows added after CATALOGUE was fixed as the sum of LIBRARIES and FURTHER.  The open-ended tuple: the next library is
# appended here.  build() reports these ahead of FURTHER's lines, in FURTHER's wording.
ADDED = (
    Library("track", 1, "track:build", "the frame-to-model tracking of predicted depth against the ray-cast model by "
                                       "point-to-plane ICP (reconstruct.py --refine-poses)"),
    Library("conf", 1, "conf:build", "the depth consistency of a frame with its neighbours as a per-pixel confidence and "
                                     "the TSDF fusion weighed by it (reconstruct.py --consistency-weight)"),
    Library("roll", 1, "roll:build", "the shift of a volume that follows the camera by whole voxels and the surface points "
                                     "that leave with it (reconstruct.py --follow)"),
    Library("sim3", 1, "sim3:build", "the frame-to-model tracking of predicted depth with a scale of its own per frame: "
                                     "point-to-plane ICP over seven degrees of freedom, the scale solved only where it is "
                                     "observable (reconstruct.py --refine-scale)"),
)
REGISTRY = CATALOGUE + ADDED
_FIND = {row.name: row for row in REGISTRY}


def find(name):
    """The row of the short name ``name``, among all rows."""
    return _FIND[name]


# one line per library of LIBRARIES, for the docstrings of build.py and _lib.py (FURTHER's rows: libscsfm_cast.so, csrc_cast/,
# include/scsfm_cast.h)
SUMMARY = "\n".join(f"    {os.path.basename(row.lib):22s} {os.path.basename(row.csrc) + '/':14s} "
                    f"include/{os.path.basename(row.header):16s} {row.what}" for row in LIBRARIES)
# the same lines for the rows added since SUMMARY was fixed (FURTHER and ADDED: cast, track, conf, ...), appended to those
# docstrings behind it
SINCE = "\n".join(f"    {os.path.basename(row.lib):22s} {os.path.basename(row.csrc) + '/':14s} "
                  f"include/{os.path.basename(row.header):16s} {row.what}" for row in FURTHER + ADDED)
