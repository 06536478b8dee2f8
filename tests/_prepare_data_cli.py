"""data/prepare_train_data.py with the two wrappers of scsfm_hip.prepare replaced by the host simulator, so that the
command-line program runs end to end without a GPU: in-process (``run(argv)``) or as a child,
``python tests/_prepare_data_cli.py <arguments of prepare_train_data.py>``.  Test infrastructure only."""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "sc-sfmlearner-release_amd")
for p in (HERE, PKG, os.path.join(PKG, "data")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import _hostsim_prep as hs  # noqa: E402
import prepare_train_data as cli  # noqa: E402
from scsfm_hip import prepare  # noqa: E402


def _resize(images, height, width, keep_rows=None):
    return torch.from_numpy(hs.resize_u8(images.numpy(), height, width, keep_rows))


def _depth(points, scan_off, P, height, width, bounds):
    return torch.from_numpy(hs.velodyne_depth(points.numpy(), scan_off.numpy(), P.numpy(), height, width, bounds))


def run(argv):
    saved = prepare.resize_u8, prepare.velodyne_depth
    prepare.resize_u8, prepare.velodyne_depth = _resize, _depth
    try:
        cli.run(cli.parser.parse_args(argv), torch.device("cpu"))
    finally:
        prepare.resize_u8, prepare.velodyne_depth = saved


if __name__ == "__main__":
    run(sys.argv[1:])
