"""Ground-truth validation metrics of training on the GPU: train.py --with-gt's ``validate_with_gt`` step (1 / disp, the
nearest resize to the ground truth's size) and ``loss_functions.compute_errors`` (mask and crop, clamp, torch.median
scaling, six error terms), through libscsfm_val.so (include/scsfm_val.h).

    res = depth_errors(gt, disp, "kitti", is_disp=True)   # one library call, no device-to-host copy
    abs_diff, abs_rel, sq_rel, a1, a2, a3 = batch_mean(res)

Per image the result is what the reference's tensor operations give -- the medians bit for bit, the thresholds' counts
exactly -- except that the three means are summed in double rather than in fp32, and that a NaN among the valid
predictions makes all six metrics NaN (the reference's three threshold shares are 0 there, its three means NaN).  There
is no CPU fallback: without a HIP device or the library this raises.

A whole validation pass (train.py --shard-validation) keeps its per-batch results on the device and may be split over
the data-parallel ranks by whole batches:

    batches = OwnedBatches(len(val_set), batch_size, rank, world, pinned=3)   # a DataLoader's batch_sampler
    table = ValidationTable(batches.n_batches, device)
    for i, (img, gt) in zip(batches.indices, loader):
        table.add_errors(i, gt, disp_net(img), "kitti")      # one library call into row i, no device-to-host copy
    values, count = table.finish()                            # one all-reduce, one library call, one copy

``owner`` gives every global batch to one rank, every rank writes only the rows of its batches, the rows of the others
stay zero, and ``x + 0.0 == x``: the summed table is the same bits whatever the world size, and it is reduced in row
order by the arithmetic of logger.AverageMeter.  So ``finish`` returns the same floats on every rank and in every world.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib

COLUMNS = ("abs_diff", "abs_rel", "sq_rel", "a1", "a2", "a3")
MIN_GT = 0.1      # valid = gt > 0.1 ...
CLAMP_LO = 1e-3   # ... pred.clamp(1e-3, max_depth)


@dataclass
class DepthErrors:
    metrics: torch.Tensor  # [B, 6] float64, COLUMNS order; NaN for an empty mask or a NaN among the valid predictions
    medians: torch.Tensor  # [B, 2] float32: torch.median of the valid GT and of the valid clamped prediction
    count: torch.Tensor    # [B] int32 valid pixels


def crop_and_cap(dataset, h, w):
    """-> (y1, y2, x1, x2, max_depth): the reference's crop box of an h x w ground-truth map and its depth cap."""
    if dataset == 'kitti':  # Garg/Eigen crop
        return int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w), 80
    if dataset == 'nyu':
        return int(0.09375 * h), int(0.98125 * h), int(0.0640625 * w), int(0.9390625 * w), 10
    # the reference leaves crop_mask unbound for any other name
    raise UnboundLocalError("dataset must be 'kitti' or 'nyu', got {!r}".format(dataset))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _depth_errors(gt, pred_or_disp, dataset, is_disp, row=None) -> DepthErrors:
    """depth_errors; with ``row`` (a device pointer to 8 doubles) through scsfm_val_depth_errors_row, which also stores
    the batch's mean there."""
    y1, y2, x1, x2, max_depth = crop_and_cap(dataset, gt.size(1), gt.size(2))
    src = pred_or_disp
    if src.dim() == 4 and src.size(1) == 1:
        src = src[:, 0]
    if gt.dim() != 3 or src.dim() != 3 or src.size(0) != gt.size(0):
        raise ValueError(f"gt must be [B, H, W] and the prediction [B, h, w], got {tuple(gt.shape)} and "
                         f"{tuple(pred_or_disp.shape)}")
    if gt.dtype != torch.float32 or src.dtype != torch.float32:
        raise TypeError(f"depth_errors takes float32 tensors, got {gt.dtype} and {src.dtype}")
    if not gt.is_cuda or src.device != gt.device:
        raise RuntimeError("depth_errors needs both tensors on one HIP device (there is no CPU fallback)")
    lib = _lib.get_val()
    gt, src = gt.contiguous(), src.contiguous()
    B, H, W = gt.shape
    h, w = src.shape[1:]
    dev = gt.device
    nbytes = lib.size("scsfm_val_workspace_bytes", B, H, W)
    if nbytes == 0:
        raise ValueError(f"a ground truth of {B} x {H} x {W} is beyond the library's range")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        metrics = torch.empty((B, 6), dtype=torch.float64, device=dev)
        medians = torch.empty((B, 2), dtype=torch.float32, device=dev)
        count = torch.empty(B, dtype=torch.int32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        args = (B, h, w, _ptr(src), int(bool(is_disp)), H, W, _ptr(gt), y1, y2, x1, x2, MIN_GT, float(max_depth), CLAMP_LO,
                _ptr(ws), nbytes, _ptr(metrics), _ptr(medians), _ptr(count))
        if row is None:
            lib.call("scsfm_val_depth_errors", *args, stream)
        else:
            lib.call("scsfm_val_depth_errors_row", *args, row, stream)
    return DepthErrors(metrics, medians, count)


@torch.no_grad()
def depth_errors(gt, pred_or_disp, dataset, is_disp=False) -> DepthErrors:
    """The validation errors of a batch: ``gt`` [B, H, W] and a prediction [B, h, w] (or [B, 1, h, w]) of any size --
    the library takes it at the ground truth's size by F.interpolate's nearest rule -- both fp32 on one HIP device.
    ``is_disp``: the prediction is the network's disparity, of which 1 / x is taken.  One library call."""
    return _depth_errors(gt, pred_or_disp, dataset, is_disp)


def batch_mean(result):
    """The six Python floats compute_errors returns: the sum over the batch divided by the batch size (a NaN image makes
    its columns NaN, as in the reference).  One device-to-host copy."""
    b = result.metrics.size(0)
    return [v / b for v in result.metrics.sum(0).tolist()]


# ---- a whole validation pass: who owns which batch, and the table of per-batch results on the device ----

ROW = 8     # doubles in a row of the table: seven values and the presence mark
VALUES = 7


def owner(i, world, pinned=0):
    """The rank that owns global batch ``i``: rank 0 the first ``pinned`` (the batches --log-output pictures: 3), the
    ranks in turn from there on."""
    return 0 if i < pinned else (i - pinned) % world


class OwnedBatches:
    """A ``batch_sampler``: of the batches the unshuffled loader forms of ``n_samples`` -- global batch i is the samples
    [i * batch_size, min((i + 1) * batch_size, n_samples)), the short last one included -- those ``rank`` owns, in
    ascending order.  No padding and no sample twice (torch's DistributedSampler does both): the ranks' batches together
    are exactly the unsharded loader's, each once, whatever the world size."""

    def __init__(self, n_samples, batch_size, rank, world, pinned=0):
        if batch_size <= 0 or world <= 0 or not 0 <= rank < world or n_samples < 0 or pinned < 0:
            raise ValueError(f"OwnedBatches({n_samples}, {batch_size}, {rank}, {world}, {pinned})")
        self.n_samples, self.batch_size = n_samples, batch_size
        self.n_batches = (n_samples + batch_size - 1) // batch_size
        self.indices = [i for i in range(self.n_batches) if owner(i, world, pinned) == rank]

    def __iter__(self):
        for i in self.indices:
            yield list(range(i * self.batch_size, min((i + 1) * self.batch_size, self.n_samples)))

    def __len__(self):
        return len(self.indices)


class ValidationTable:
    """The table of one validation pass, [n_batches, 8] float64 on ``device`` and zero: row i is global batch i's seven
    values and a 1.0 once it is written (include/scsfm_val.h).  ``add_*`` enqueue one library call and copy nothing to
    the host; ``finish`` sums the ranks' tables and reduces the sum on the device."""

    def __init__(self, n_batches, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ValidationTable needs a HIP device (there is no CPU fallback)")
        if n_batches < 0:
            raise ValueError(f"a table of {n_batches} rows")
        with torch.cuda.device(device):
            device = torch.device("cuda", torch.cuda.current_device())
        self.n_batches, self.device = n_batches, device
        self.table = torch.zeros((n_batches, ROW), dtype=torch.float64, device=device)
        self._mine = []  # the rows this process wrote, in the order it wrote them

    def _row(self, i):
        if not 0 <= i < self.n_batches:
            raise IndexError(f"batch {i} of a pass of {self.n_batches}")
        return ctypes.c_void_p(self.table.data_ptr() + i * ROW * self.table.element_size())

    @torch.no_grad()
    def add_errors(self, i, gt, pred_or_disp, dataset, is_disp=True) -> DepthErrors:
        """``depth_errors`` of global batch ``i`` and, by the same library call, the batch's mean into row ``i``."""
        if not gt.is_cuda or gt.device != self.device:
            raise RuntimeError("add_errors needs the tensors on the table's HIP device (there is no CPU fallback)")
        res = _depth_errors(gt, pred_or_disp, dataset, is_disp, self._row(i))
        self._mine.append(i)
        return res

    @torch.no_grad()
    def add_losses(self, i, photo, smooth, geom):
        """Three fp32 scalars on the device into row ``i`` as validate_without_gt's [photo, photo, smooth, geom]."""
        row = self._row(i)
        scalars = []
        for t in (photo, smooth, geom):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != self.device:
                raise RuntimeError("add_losses needs scalars on the table's HIP device (there is no CPU fallback)")
            if t.dtype != torch.float32 or t.numel() != 1:
                raise TypeError(f"add_losses takes float32 scalars, got {t.dtype} of {tuple(t.shape)}")
            scalars.append(t.detach())
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.get_val().call("scsfm_val_losses_row", *(_ptr(t) for t in scalars), row, stream)
        self._mine.append(i)

    def peek(self, i):
        """-> (row ``i``'s seven values, the running mean of the rows this process has written so far), as Python floats
        by AverageMeter's arithmetic.  One device-to-host copy: for the progress lines only."""
        rows = self.table.tolist()
        total, mean = [0.0] * VALUES, [0.0] * VALUES
        for n, r in enumerate(self._mine, 1):
            for k in range(VALUES):
                total[k] += rows[r][k]
                mean[k] = total[k] / n
        return rows[i][:VALUES], mean

    @torch.no_grad()
    def finish(self, group=None):
        """-> (the seven means over the pass's present rows, their number): the same floats on every rank, whatever the
        world size.  One all-reduce (in a world of more than one), one library call, one device-to-host copy."""
        if self.n_batches == 0:  # (on every rank alike)
            return [0.0] * VALUES, 0  # AverageMeter.avg before any update
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            if "nccl" in str(dist.get_backend(group)):
                dist.all_reduce(self.table, op=dist.ReduceOp.SUM, group=group)
            else:  # a backend that reduces host tensors only: the table goes through the host, once per pass
                host = self.table.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
                self.table.copy_(host)
        with torch.cuda.device(self.device):
            out = torch.empty(ROW, dtype=torch.float64, device=self.device)
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.get_val().call("scsfm_val_table_mean", self.n_batches, _ptr(self.table), _ptr(out), stream)
        vals = out.tolist()
        return vals[:VALUES], int(vals[VALUES])
