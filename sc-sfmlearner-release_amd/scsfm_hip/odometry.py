"""KITTI visual odometry on the GPU through libscsfm_odom.so (include/scsfm_odom.h): test_vo.py's pose fold as a scan and
kitti_eval/kitti_odometry.py's KittiEvalOdom.eval for a whole set of sequences in one library call.

    poses = chain_poses(pose_vecs)                          # [n, 6] -> float64 [n + 1, 3, 4]
    res = evaluate_odometry([gt_09, gt_10], [pred_09, pred_10], alignment="7dof", seqs=[9, 10])
    print("\\n".join(res.report_lines() + res.copy_block()))

There is no CPU fallback: without a HIP device or the library this raises.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

LENGTHS = (100, 200, 300, 400, 500, 600, 700, 800)
ALIGNMENTS = {None: 0, "scale": 1, "scale_7dof": 2, "7dof": 3, "6dof": 4}
ROTATION_MODES = {"euler": 0, "quat": 1}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("the odometry kernels need a HIP device (there is no CPU fallback)")
    return torch.device("cuda")


def _num(x):
    return str(np.float64(x))


def chain_poses_ragged(pose_vecs, rotation_mode="euler", return_local=False):
    """chain_poses for several sequences in one call: a list of [n_s, 6] tensors / arrays of one dtype (float32 or
    float64) -> a list of float64 [n_s + 1, 3, 4] device tensors (and, with ``return_local``, the list of
    pose_vec2mat matrices [n_s, 3, 4] in the input precision)."""
    if rotation_mode not in ROTATION_MODES:
        raise ValueError(f"rotation_mode must be 'euler' or 'quat', got {rotation_mode!r}")
    device = _device()
    lib = _lib.get_odom()
    vecs = [v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v)) for v in pose_vecs]
    if not vecs or len({v.dtype for v in vecs}) != 1 or vecs[0].dtype not in (torch.float32, torch.float64):
        raise TypeError("pose vectors must be float32 or float64 tensors of one dtype")
    if any(v.dim() != 2 or v.shape[1] != 6 for v in vecs):
        raise ValueError("pose vectors must be [n, 6]")
    dt = vecs[0].dtype
    lens = np.array([v.shape[0] for v in vecs], np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    out_off = (off + np.arange(len(vecs))).astype(np.int32)
    S, max_len, total = len(vecs), int(lens.max()), int(lens.sum())
    vec = torch.cat([v.to(device) for v in vecs]).contiguous() if total else torch.zeros((1, 6), dtype=dt, device=device)
    local = torch.empty((max(total, 1), 12), dtype=dt, device=device) if return_local else None
    poses = torch.empty((total + S, 12), dtype=torch.float64, device=device)
    d_off, d_len, d_out = (torch.from_numpy(a).to(device) for a in (off, lens, out_off))
    nbytes = lib.size("scsfm_odom_chain_workspace_bytes", S, max_len)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    lib.call("scsfm_odom_chain", S, max_len, int(dt == torch.float64), ROTATION_MODES[rotation_mode], _ptr(vec),
             _ptr(d_off), _ptr(d_len), _ptr(d_out), _ptr(local) if return_local else None, _ptr(poses), _ptr(ws), nbytes,
             stream)
    out = [poses[o:o + n + 1].view(-1, 3, 4) for o, n in zip(out_off.tolist(), lens.tolist())]
    if return_local:
        return out, [local[o:o + n].view(-1, 3, 4) for o, n in zip(off.tolist(), lens.tolist())]
    return out


def chain_poses(pose_vecs, rotation_mode="euler"):
    """test_vo.py's fold: [n, 6] pose vectors (tx ty tz rx ry rz, frame k -> k + 1) -> float64 [n + 1, 3, 4] global
    poses on the device, G_0 = I, G_k = G_{k-1} inv(pose_vec2mat(vec_k))."""
    return chain_poses_ragged([pose_vecs], rotation_mode)[0]


@dataclass
class OdomEvalResult:
    seqs: list               # sequence numbers (what the printout names)
    alignment: object        # None, "scale", "scale_7dof", "7dof" or "6dof"
    summary: np.ndarray      # [S, 7]: mean t_err, mean r_err, ATE, RPE translation, RPE rotation, scale, segments
    per_length: np.ndarray   # [S, 8, 3]: mean t_err, mean r_err, count for 100 .. 800 m
    segments: list           # per sequence [m, 5]: first_frame, r_err / len, t_err / len, len, speed
    gt_rel: list             # per sequence [n, 3, 4]: the ground truth re-based on its first frame
    aligned: list            # per sequence [n, 3, 4]: the re-based, aligned prediction

    def report_lines(self):
        """The reference's console lines, sequence after sequence."""
        out = []
        for seq, (t, r, ate, rpe_t, rpe_r, _, m) in zip(self.seqs, self.summary):
            out += ["Sequence: " + str(seq),
                    "Translational error (%):  " + (_num(t * 100) if m else "0"),
                    "Rotational error (deg/100m):  " + (_num(r / np.pi * 180 * 100) if m else "0.0"),
                    "ATE (m):  " + _num(ate),
                    "RPE (m):  " + _num(rpe_t),
                    "RPE (deg):  " + _num(rpe_r * 180 / np.pi)]
        return out

    def copy_block(self):
        out = ["-------------------- For Copying ------------------------------"]
        for s in self.summary:
            out += ["{0:.2f}".format(s[0] * 100), "{0:.2f}".format(s[1] / np.pi * 180 * 100)]
        return out

    def result_txt(self):
        out = ""
        for seq, (t, r, ate, rpe_t, rpe_r, _, _) in zip(self.seqs, self.summary):
            out += "Sequence: \t {} \n".format(seq)
            out += "Trans. err. (%): \t {:.3f} \n".format(t * 100)
            out += "Rot. err. (deg/100m): \t {:.3f} \n".format(r / np.pi * 180 * 100)
            out += "ATE (m): \t {:.3f} \n".format(ate)
            out += "RPE (m): \t {:.3f} \n".format(rpe_t)
            out += "RPE (deg): \t {:.3f} \n\n".format(rpe_r * 180 / np.pi)
        return out

    def segment_errors(self, i):
        """The text of errors/<seq>.txt for the i-th evaluated sequence."""
        return "".join("{} {} {} {} {}\n".format(int(f), _num(r), _num(t), int(L), repr(float(v)))
                       for f, r, t, L, v in self.segments[i])

    def avg_segment_errs(self, i):
        """{length: [mean t_err, mean r_err] or []} as the reference's compute_segment_error returns it."""
        return {L: ([float(t), float(r)] if c else []) for L, (t, r, c) in zip(LENGTHS, self.per_length[i])}


def evaluate_odometry(gt, pred, alignment=None, seqs=None) -> OdomEvalResult:
    """KittiEvalOdom.eval for lists of per-sequence poses ([n, 12] or [n, 3, 4], tensors or arrays, on the host or on the
    device; float64 is what the pose files hold, anything else is converted).  Frame i of a prediction belongs to frame
    i of its ground truth, whose surplus frames (if any) are ignored.  ``seqs``: the sequence numbers for the printout."""
    if alignment not in ALIGNMENTS:
        raise ValueError(f"alignment must be one of {list(ALIGNMENTS)}, got {alignment!r}")
    device = _device()
    lib = _lib.get_odom()
    if len(gt) != len(pred) or not len(gt):
        raise ValueError(f"{len(gt)} ground-truth trajectories for {len(pred)} predictions")

    def rows(x):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        return t.to(device=device, dtype=torch.float64).reshape(-1, 12)

    P = [rows(p) for p in pred]
    G = [rows(g)[:len(p)] for g, p in zip(gt, P)]
    if any(len(g) != len(p) or not len(p) for g, p in zip(G, P)):
        raise ValueError("every prediction needs at least one frame and a ground truth at least as long")
    seqs = list(range(len(P))) if seqs is None else list(seqs)
    lens = np.array([len(p) for p in P], np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    S, max_len, total = len(P), int(lens.max()), int(lens.sum())
    d_gt, d_pred = torch.cat(G).contiguous(), torch.cat(P).contiguous()
    d_off, d_len = torch.from_numpy(off).to(device), torch.from_numpy(lens).to(device)
    max_seg = lib.size("scsfm_odom_eval_max_segments", max_len)
    nbytes = lib.size("scsfm_odom_eval_workspace_bytes", S, max_len, total)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    f64 = dict(dtype=torch.float64, device=device)
    summary, per_length = torch.empty((S, 7), **f64), torch.empty((S, 8, 3), **f64)
    seg, n_seg = torch.empty((S, max_seg, 5), **f64), torch.empty(S, dtype=torch.int32, device=device)
    gt_rel, aligned = torch.empty((total, 12), **f64), torch.empty((total, 12), **f64)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    lib.call("scsfm_odom_eval", S, max_len, total, ALIGNMENTS[alignment], _ptr(d_gt), _ptr(d_pred), _ptr(d_off),
             _ptr(d_len), max_seg, _ptr(ws), nbytes, _ptr(summary), _ptr(per_length), _ptr(seg), _ptr(n_seg),
             _ptr(gt_rel), _ptr(aligned), stream)
    n_seg = n_seg.cpu().numpy()
    seg = seg[:, :max(int(n_seg.max()), 1)].cpu().numpy()
    gt_rel, aligned = gt_rel.cpu().numpy(), aligned.cpu().numpy()
    cut = lambda a: [a[o:o + n].reshape(-1, 3, 4) for o, n in zip(off, lens)]
    return OdomEvalResult(seqs, alignment, summary.cpu().numpy(), per_length.cpu().numpy(),
                          [seg[s, :n_seg[s]] for s in range(S)], cut(gt_rel), cut(aligned))
