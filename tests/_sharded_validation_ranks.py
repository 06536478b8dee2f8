"""Shared by tests/test_gpu_sharded_validation.py and the rank processes it spawns: seeded validation batches of case A's
shapes (tests/_validation_errors_cases.py) and one rank of a pass that is split over two processes on one GPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sc-sfmlearner-release_amd")
PINNED = 3
EMPTY, NAN_IMAGE = 4, 5  # of the seven batches of the two-rank pass: no ground truth at all; a NaN in image 1
SEVEN = (3, 3, 3, 3, 3, 3, 1)


def _paths():
    for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def batch(seed, B):
    """-> (gt[B, 37, 124], disp[B, 16, 52]) fp32 numpy, kitti: the shapes and value ranges of case A."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.05, 90.0, (B, 37, 124)).astype(np.float32)
    gt[rng.random(gt.shape) < 0.4] = 0
    return gt, rng.uniform(0.008, 1.6, (B, 16, 52)).astype(np.float32)


def seven_batches():
    """The two-rank pass: batch EMPTY has an empty ground truth (its row stays absent, as train.py's loop leaves it),
    batch NAN_IMAGE a NaN disparity under a valid ground-truth pixel of image 1 (its six columns are NaN)."""
    out = []
    for i, B in enumerate(SEVEN):
        gt, disp = batch(700 + i, B)
        if i == EMPTY:
            gt = gt[:0]
        if i == NAN_IMAGE:
            gt[1, 20, 60] = 9.0    # inside the crop box (rows 15:36, columns 4:119) and the depth range
            disp[1, 8, 25] = np.nan  # its nearest source pixel: floor(20 * 16 / 37) = 8, floor(60 * 52 / 124) = 25
        out.append((gt, disp))
    return out


def add_owned(table, batches, rank, world, device):
    """What train.validate_with_gt does with the batches ``rank`` owns."""
    from scsfm_hip.validation import owner
    for i, (gt, disp) in enumerate(batches):
        if owner(i, world, PINNED) != rank:
            continue
        if gt.size == 0:
            continue
        table.add_errors(i, torch.from_numpy(gt).to(device), torch.from_numpy(disp).to(device), "kitti", is_disp=True)


def rank_worker(rank, world, port, q):
    _paths()
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from scsfm_hip.validation import ValidationTable
    torch.set_num_threads(2)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        batches = seven_batches()
        table = ValidationTable(len(batches), device)
        add_owned(table, batches, rank, world, device)
        own = sorted(int(i) for i in torch.nonzero(table.table[:, 7]).flatten().tolist())
        values, count = table.finish()
        # (numpy: pickled by value through the queue)
        q.put((rank, {"values": values, "count": count, "own": own, "table": table.table.cpu().numpy().copy()}))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def statistics_worker(rank, world, port, q):
    """One rank of train.rank0_statistics on the host (gloo): a BatchNorm whose running statistics differ per rank."""
    _paths()
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    import train as T
    torch.set_num_threads(1)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        nets = [torch.nn.Sequential(torch.nn.Linear(2, 3), torch.nn.BatchNorm1d(3)) for _ in range(2)]
        for k, net in enumerate(nets):
            net[1].running_mean.fill_(10.0 * k + rank + 1)
            net[1].num_batches_tracked.fill_(100 * k + rank + 5)
        state = lambda: [[float(net[1].running_mean[0]), int(net[1].num_batches_tracked)] for net in nets]  # noqa: E731
        before = state()
        with T.rank0_statistics(nets, world):
            inside = state()
        alone = state()
        with T.rank0_statistics(nets, 1):  # a world of one: nothing is sent
            single = state()
        q.put((rank, {"before": before, "inside": inside, "after": alone, "single": single}))
        dist.barrier()
    finally:
        dist.destroy_process_group()
