"""Ground-truth validation metrics of training on the GPU: train.py --with-gt's ``validate_with_gt`` step (1 / disp, the
nearest resize to the ground truth's size) and ``loss_functions.compute_errors`` (mask and crop, clamp, torch.median
scaling, six error terms), through libscsfm_val.so (include/scsfm_val.h).

    res = depth_errors(gt, disp, "kitti", is_disp=True)   # one library call, no device-to-host copy
    abs_diff, abs_rel, sq_rel, a1, a2, a3 = batch_mean(res)

Per image the result is what the reference's tensor operations give -- the medians bit for bit, the thresholds' counts
exactly -- except that the three means are summed in double rather than in fp32, and that a NaN among the valid
predictions makes all six metrics NaN (the reference's three threshold shares are 0 there, its three means NaN).  There
is no CPU fallback: without a HIP device or the library this raises.
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


@torch.no_grad()
def depth_errors(gt, pred_or_disp, dataset, is_disp=False) -> DepthErrors:
    """The validation errors of a batch: ``gt`` [B, H, W] and a prediction [B, h, w] (or [B, 1, h, w]) of any size --
    the library takes it at the ground truth's size by F.interpolate's nearest rule -- both fp32 on one HIP device.
    ``is_disp``: the prediction is the network's disparity, of which 1 / x is taken.  One library call."""
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
        lib.call("scsfm_val_depth_errors", B, h, w, _ptr(src), int(bool(is_disp)), H, W, _ptr(gt), y1, y2, x1, x2,
                 MIN_GT, float(max_depth), CLAMP_LO, _ptr(ws), nbytes, _ptr(metrics), _ptr(medians), _ptr(count), stream)
    return DepthErrors(metrics, medians, count)


def batch_mean(result):
    """The six Python floats compute_errors returns: the sum over the batch divided by the batch size (a NaN image makes
    its columns NaN, as in the reference).  One device-to-host copy."""
    b = result.metrics.size(0)
    return [v / b for v in result.metrics.sum(0).tolist()]
