"""Monocular depth evaluation on the GPU: eval_depth.py's DepthEvalEigen.evaluate_depth with eval_mono=True, through
libscsfm_eval.so (include/scsfm_eval.h).

    res = evaluate_depth(gt_depths, pred_depths, "kitti")
    print("\\n".join(res.report_lines()))

Per image: the prediction's inverse depth is resized to the GT's size (OpenCV INTER_LINEAR's generic path), the GT is
masked to (min_depth, max_depth) (and cropped for KITTI), the prediction is scaled by median(gt) / median(pred) and
clamped, and the eight error terms are reduced -- all on the device, for the whole set, without a host loop over images.
Only the mean over the images and the ratio statistics (N values) are taken on the host, with numpy, as the reference
takes them.  There is no CPU fallback: without a HIP device or the library this raises.
"""
from __future__ import annotations

import ctypes
import warnings
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

COLUMNS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "log10", "a1", "a2", "a3")
DATASET_COLUMNS = {"kitti": ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"),
                   "nyu": ("abs_rel", "log10", "rmse", "a1", "a2", "a3")}
MAX_DEPTH = {"kitti": 80.0, "nyu": 10.0}
# pixels of packed GT per call when ``chunk`` is not given: bounds the packed GT copy plus the compacted pairs
# (at most 2^26 * (4 + 8 + 8) bytes = 1.3 GB with float64 inputs)
CHUNK_PIXELS = 1 << 26


@dataclass
class DepthEvalResult:
    dataset: str
    metrics: np.ndarray    # [N, 8] float64, COLUMNS order; NaN for skipped images and empty masks
    ratio: np.ndarray      # [N] float64 (each value exact in the promoted dtype of GT and prediction)
    med_gt: np.ndarray     # [N] median of the valid GT
    med_pred: np.ndarray   # [N] median of the valid resized prediction
    count: np.ndarray      # [N] int32 valid pixels
    evaluated: np.ndarray  # [N] bool: False where the prediction's mean is exactly -1 (the reference skips those)
    ratios: np.ndarray     # the evaluated images' ratios in the promoted dtype (what the reference collects)
    mean: np.ndarray       # mean over the evaluated images, in DATASET_COLUMNS[dataset] order
    ratio_stats: tuple     # (median, std(ratios / median), mean, std) of ``ratios``

    @property
    def columns(self):
        return DATASET_COLUMNS[self.dataset]

    def report_lines(self):
        """The reference's printout after its progress bar, line by line (print them joined by newlines)."""
        med, std_rel, mean_r, std_r = self.ratio_stats
        cols = self.columns
        return [" Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, std_rel),
                " Scaling ratios | mean: {:0.3f} +- std: {:0.3f}".format(mean_r, std_r),
                "",
                "  " + ("{:>8} | " * len(cols)).format(*cols),
                ("&{: 8.3f}  " * len(cols)).format(*self.mean.tolist()) + "\\\\"]


def _as_tensor(x, device):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"depth maps must be float32 or float64, got {t.dtype}")
    return t.to(device)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def evaluate_depth(gt_depths, pred_depths, dataset, eval_mono=True, min_depth=1e-3, max_depth=None, chunk=None,
                   device=None) -> DepthEvalResult:
    """Evaluates predictions [N, h, w] against N ground-truth maps: a list of [H_i, W_i] tensors / arrays (ragged, as
    KITTI's) or one [N, H, W] tensor / array.  float32 and float64 are accepted for both, with numpy's promotion rules
    (include/scsfm_eval.h).  ``chunk``: images per library call (default: as many as hold CHUNK_PIXELS GT pixels); the
    results do not depend on it."""
    if dataset not in DATASET_COLUMNS:
        raise ValueError(f"dataset must be 'kitti' or 'nyu', got {dataset!r}")
    if not eval_mono:
        raise ValueError("only eval_mono=True (median scaling, the reference scripts' mode) is implemented")
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_depth needs a HIP device (there is no CPU fallback)")
    max_depth = MAX_DEPTH[dataset] if max_depth is None else float(max_depth)
    device = torch.device(device or "cuda")
    lib = _lib.get_eval()

    pred = _as_tensor(pred_depths, device).contiguous()
    if pred.dim() != 3:
        raise ValueError(f"pred_depths must be [N, h, w], got {tuple(pred.shape)}")
    N, h, w = pred.shape
    if isinstance(gt_depths, (list, tuple)):
        gts = [_as_tensor(g, device) for g in gt_depths]
    else:
        g = _as_tensor(gt_depths, device)
        if g.dim() != 3:
            raise ValueError(f"gt_depths must be a list of [H, W] maps or [N, H, W], got {tuple(g.shape)}")
        gts = list(g.unbind(0))
    if len(gts) != N:
        raise ValueError(f"{len(gts)} GT maps for {N} predictions")
    if any(g.dim() != 2 for g in gts) or len({g.dtype for g in gts}) != 1:
        raise ValueError("GT maps must be 2-D and of one dtype")
    gdt = gts[0].dtype
    sizes = np.array([g.shape for g in gts], np.int64).reshape(N, 2)
    hw = sizes[:, 0] * sizes[:, 1]
    slot = (hw + 3) // 4 * 4  # packed offsets stay multiples of 4 elements (vector loads)

    metrics = torch.empty((N, 8), dtype=torch.float64, device=device)
    stats = torch.empty((N, 3), dtype=torch.float64, device=device)
    count = torch.empty(N, dtype=torch.int32, device=device)
    flag = torch.empty(N, dtype=torch.int32, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    pf, gf = int(pred.dtype == torch.float64), int(gdt == torch.float64)
    i0 = 0
    while i0 < N:
        if chunk:
            i1 = min(N, i0 + int(chunk))
        else:
            i1 = i0 + max(1, int(np.searchsorted(np.cumsum(slot[i0:]), CHUNK_PIXELS, side="right")))
            i1 = min(i1, N)
        off = np.concatenate([[0], np.cumsum(slot[i0:i1])[:-1]]).astype(np.int64)
        total = int(off[-1] + hw[i1 - 1])
        buf = torch.empty(total, dtype=gdt, device=device)
        for k, g in enumerate(gts[i0:i1]):
            buf[off[k]:off[k] + hw[i0 + k]].view(g.shape).copy_(g)
        d_off = torch.from_numpy(off).to(device)
        d_h = torch.from_numpy(sizes[i0:i1, 0].astype(np.int32)).to(device)
        d_w = torch.from_numpy(sizes[i0:i1, 1].astype(np.int32)).to(device)
        max_hw = int(hw[i0:i1].max())
        nbytes = lib.size("scsfm_eval_workspace_bytes", i1 - i0, max_hw, total, pf, gf)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        lib.call("scsfm_eval_depth", i1 - i0, h, w, pf, _ptr(pred[i0:i1]), gf, _ptr(buf), _ptr(d_off), _ptr(d_h),
                 _ptr(d_w), max_hw, total, int(dataset == "kitti"), float(min_depth), max_depth, _ptr(ws), nbytes,
                 _ptr(metrics[i0:i1]), _ptr(stats[i0:i1]), _ptr(count[i0:i1]), _ptr(flag[i0:i1]), stream)
        i0 = i1

    metrics, stats = metrics.cpu().numpy(), stats.cpu().numpy()
    count, evaluated = count.cpu().numpy(), flag.cpu().numpy() == 1
    rdt = np.result_type(np.float32 if gdt == torch.float32 else np.float64,
                         np.float32 if pred.dtype == torch.float32 else np.float64)
    cols = [COLUMNS.index(c) for c in DATASET_COLUMNS[dataset]]
    ratios = stats[evaluated, 0].astype(rdt)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (an empty mask's NaN, as in the reference)
        mean = metrics[evaluated][:, cols].mean(0)
        med = np.median(ratios)
        ratio_stats = (med, np.std(ratios / med), np.mean(ratios), np.std(ratios))
    return DepthEvalResult(dataset, metrics, stats[:, 0], stats[:, 1], stats[:, 2], count, evaluated, ratios, mean,
                           ratio_stats)
