"""The 5-frame snippet pose evaluation of test_pose.py on the GPU through libscsfm_snip.so (include/scsfm_snip.h): every
snippet of every sequence folded, compensated and scored in one library call.

    res = evaluate_snippets([vec_09, vec_10], [gt_09, gt_10])      # [n - 1, 6] pair vectors, [n, 12] KITTI poses
    print("\\n".join(res.report_lines()))

vec[k] is pose_net(img_k, img_{k+1}): each distinct pair goes through the network once, however many snippets share it.
There is no CPU fallback: without a HIP device or the library this raises.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

ROTATION_MODES = {"euler": 0, "quat": 1}
MIN_LENGTH, MAX_LENGTH = 2, 16  # include/scsfm_snip.h


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("the snippet kernels need a HIP device (there is no CPU fallback)")
    return torch.device("cuda")


@dataclass
class SnippetResult:
    errors: np.ndarray       # [N, 2] float64: ATE, RE per snippet (unrounded)
    predictions: np.ndarray  # [N, L, 3, 4] float64: the folded poses, the first one the identity
    gt: np.ndarray           # [N, L, 3, 4] float64: the ground truth compensated by its first frame
    mean: np.ndarray         # [2] float64: over the errors rounded to float32, as the reference keeps them
    std: np.ndarray          # [2]

    def report_lines(self):
        """The reference's results block: the empty line, the title, the header, mean and std."""
        return ["", "Results", "\t {:>10}, {:>10}".format("ATE", "RE"),
                "mean \t {:10.4f}, {:10.4f}".format(*self.mean), "std \t {:10.4f}, {:10.4f}".format(*self.std)]


def evaluate_snippets(pose_vecs, gt_poses, seq_length=5, rotation_mode="euler") -> SnippetResult:
    """test_pose.py's loop over every snippet of every sequence.  ``pose_vecs``: a list of [n_s - 1, 6] tensors / arrays
    of one dtype (float32 or float64), row k the network's output for frames (k, k + 1); ``gt_poses``: a list of
    [n_s, 12] or [n_s, 3, 4] KITTI poses (converted to float64).  Both on the host or on the device.  Sequence s
    contributes n_s - seq_length + 1 snippets (none when it is shorter), in order."""
    if rotation_mode not in ROTATION_MODES:
        raise ValueError(f"rotation_mode must be 'euler' or 'quat', got {rotation_mode!r}")
    if not MIN_LENGTH <= int(seq_length) <= MAX_LENGTH:
        raise ValueError(f"seq_length must be in [{MIN_LENGTH}, {MAX_LENGTH}], got {seq_length}")
    seq_length = int(seq_length)
    device = _device()
    lib = _lib.get_snip()
    if len(pose_vecs) != len(gt_poses) or not len(gt_poses):
        raise ValueError(f"{len(pose_vecs)} sets of pose vectors for {len(gt_poses)} ground-truth trajectories")
    vecs = [v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)) for v in pose_vecs]
    if len({v.dtype for v in vecs}) != 1 or vecs[0].dtype not in (torch.float32, torch.float64):
        raise TypeError("pose vectors must be float32 or float64 tensors of one dtype")
    if any(v.dim() != 2 or v.shape[1] != 6 for v in vecs):
        raise ValueError("pose vectors must be [n - 1, 6]")
    dt = vecs[0].dtype

    def rows(x):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        return t.to(device=device, dtype=torch.float64).reshape(-1, 12)

    G = [rows(g) for g in gt_poses]
    for v, g in zip(vecs, G):
        if len(g) != len(v) + 1 and not (len(g) == 0 and len(v) == 0):
            raise ValueError(f"{len(v)} pose vectors need {len(v) + 1} ground-truth poses, got {len(g)}")
    lens = np.array([len(g) for g in G], np.int64)
    counts = np.maximum(lens - seq_length + 1, 0)
    total, n_snip, S = int(lens.sum()), int(counts.sum()), len(G)
    if n_snip == 0:
        raise ValueError(f"no sequence has {seq_length} frames: there is no snippet to evaluate")
    frame_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    snip_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    # [total, 6]: a sequence's n - 1 vectors and one unused row, so that vectors and poses share their offsets
    pad = torch.zeros((1, 6), dtype=dt, device=device)
    vec = torch.cat([x for v, n in zip(vecs, lens) if n for x in (v.to(device), pad)]).contiguous()
    gt = torch.cat(G).contiguous()
    assert vec.shape == (total, 6) and gt.shape == (total, 12)
    d_off, d_len, d_snip = (torch.from_numpy(a).to(device) for a in (frame_off, lens.astype(np.int32), snip_off))
    f64 = dict(dtype=torch.float64, device=device)
    pred, comp = torch.empty((n_snip, seq_length, 12), **f64), torch.empty((n_snip, seq_length, 12), **f64)
    errors, stats = torch.empty((n_snip, 2), **f64), torch.empty(4, **f64)
    nbytes = lib.size("scsfm_snip_workspace_bytes", S, seq_length, total)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    lib.call("scsfm_snip_eval", S, seq_length, int(dt == torch.float64), ROTATION_MODES[rotation_mode], _ptr(vec),
             _ptr(gt), _ptr(d_off), _ptr(d_len), _ptr(d_snip), total, n_snip, _ptr(pred), _ptr(comp), _ptr(errors),
             _ptr(stats), _ptr(ws), nbytes, stream)
    stats = stats.cpu().numpy()
    return SnippetResult(errors.cpu().numpy(), pred.cpu().numpy().reshape(n_snip, seq_length, 3, 4),
                         comp.cpu().numpy().reshape(n_snip, seq_length, 3, 4), stats[:2].copy(), stats[2:].copy())
