"""Depth visualisation of eval_depth.py --vis_dir on the GPU through libscsfm_dvis.so (include/scsfm_dvis.h).

    canvases = composites(res, pred_depths, gt_depths, "kitti", photos)    # uint8 [2H, W, 3] each, on the device

The three pieces, each the reference's arithmetic under numpy 2 and matplotlib 3.10, bit for bit and byte for byte:
``scaled_depths`` is what the reference's evaluate_depth returns (the prediction's inverse depth resized to the ground
truth's size, back to depth, times the median ratio); ``depth_range`` is (min, 95th percentile) of a map's inverse depth;
``colourise`` is matplotlib's Normalize and the magma lookup.  ``composites`` puts them beside the photograph the way
eval_depth.py's main does.  The magma table is committed below as data (matplotlib is not needed at run time).  There is
no CPU fallback: without a HIP device or the library the wrappers raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

# uint8(float64(matplotlib.colormaps['magma'].colors) * 255), 256 entries of (R, G, B); tests/test_depth_vis_reference.py
# compares every entry with the installed matplotlib
MAGMA = np.frombuffer(bytes.fromhex(
    "00000300000400000601000701010901010b02020d02020f03031104031304041505041706051907051b08061d09071f"
    "0a07220b08240c09260d0a280e0a2a0f0b2c100c2f110c31120d33140d35150e38160e3a170f3c180f3f1a10411b1044"
    "1c10461e10491f114b20114d2211502311522511552611572811592a115c2b115e2d10602f1062301065321067341068"
    "350f6a370f6c390f6e3b0f6f3c0f713e0f72400f73420f74430f75450f76470f774810784a10794b10794d117a4f117b"
    "50127b52127c53137c55137d57147d58157e5a157e5b167e5d177e5e177f60187f61187f63197f651a80661a80681b80"
    "691c806b1c806c1d806e1e816f1e81711f81731f817420817621817721817922817a22817c23817e24817f2481812581"
    "8225818426818526818727818928818a28818c29808d29808f2a80912a80922b80942b80952c80972c7f992d7f9a2d7f"
    "9c2e7f9e2e7e9f2f7ea12f7ea3307ea4307da6317da7317da9327cab337cac337bae347bb0347bb1357ab3357ab53679"
    "b63679b83778b93778bb3877bd3977be3976c03a75c23a75c33b74c53c74c63c73c83d72ca3e72cb3e71cd3f70ce4070"
    "d0416fd1426ed3426dd4436dd6446cd7456bd9466ada4769dc4869dd4968de4a67e04b66e14c66e24d65e44e64e55063"
    "e65162e75262e85461ea5560eb5660ec585fed595fee5b5eee5d5def5e5df0605df1615cf2635cf3655cf3675bf4685b"
    "f56a5bf56c5bf66e5bf6705bf7715bf7735cf8755cf8775cf9795cf97b5df97d5dfa7f5efa805efa825ffb8460fb8660"
    "fb8861fb8a62fc8c63fc8e63fc9064fc9265fc9366fd9567fd9768fd9969fd9b6afd9d6bfd9f6cfda16efda26ffda470"
    "fea671fea873feaa74feac75feae76feaf78feb179feb37bfeb57cfeb77dfeb97ffebb80febc82febe83fec085fec286"
    "fec488fec689fec78bfec98dfecb8efdcd90fdcf92fdd193fdd295fdd497fdd698fdd89afdda9cfddc9dfddd9ffddfa1"
    "fde1a3fce3a5fce5a6fce6a8fce8aafceaacfcecaefceeb0fcf0b1fcf1b3fcf3b5fcf5b7fbf7b9fbf9bbfbfabdfbfcbf"),
    dtype=np.uint8).reshape(256, 3)

_NP = {torch.float32: np.float32, torch.float64: np.float64}
_device_tables = {}


def percentile_index(n, dtype):
    """(lo, hi, t) of np.percentile(a, 95) for n elements of ``dtype`` (np.float32 / np.float64), formed with numpy
    scalars of that type as numpy 2.2 forms them: the two order statistics and the weight of the upper one."""
    T = np.dtype(dtype).type
    vi = T(n - 1) * (T(95) / T(100))
    lo = int(np.floor(vi))
    return lo, min(lo + 1, n - 1), T(vi - T(lo))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check_device(t, what):
    if not torch.cuda.is_available() or not t.is_cuda:
        raise RuntimeError(f"{what} must live on a HIP device (there is no CPU fallback)")


class Ragged:
    """Maps of different sizes in one device buffer: image i is sizes[i] = (H, W), row-major, at element offset off[i]
    (a multiple of 4, the include/scsfm_eval.h convention)."""

    def __init__(self, sizes, dtype, device):
        self.sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
        if len(self.sizes) < 1 or (self.sizes < 1).any() or (self.sizes[:, 0] * self.sizes[:, 1] >= 1 << 31).any():
            raise ValueError("every map needs at least one pixel and fewer than 2^31")
        self.hw = self.sizes[:, 0] * self.sizes[:, 1]
        slot = (self.hw + 3) // 4 * 4
        self.off = np.concatenate([[0], np.cumsum(slot)[:-1]]).astype(np.int64)
        self.total = int(self.off[-1] + self.hw[-1])
        self.max_hw = int(self.hw.max())
        self.buf = torch.empty(self.total, dtype=dtype, device=device)
        self.d_off = torch.from_numpy(self.off).to(device)
        self.d_h = torch.from_numpy(self.sizes[:, 0].astype(np.int32)).to(device)
        self.d_w = torch.from_numpy(self.sizes[:, 1].astype(np.int32)).to(device)

    def __len__(self):
        return len(self.sizes)

    def map(self, i):
        return self.buf[self.off[i]:self.off[i] + self.hw[i]].view(int(self.sizes[i, 0]), int(self.sizes[i, 1]))

    def maps(self):
        return [self.map(i) for i in range(len(self))]

    @classmethod
    def pack(cls, maps):
        """A list of [H_i, W_i] device tensors (or one [N, H, W] tensor) of one floating dtype, copied into one buffer."""
        maps = list(maps.unbind(0)) if isinstance(maps, torch.Tensor) else list(maps)
        if not maps or any(not isinstance(m, torch.Tensor) or m.dim() != 2 for m in maps):
            raise ValueError("maps must be a non-empty list of 2-D tensors or one [N, H, W] tensor")
        _check_device(maps[0], "maps")
        if maps[0].dtype not in _NP or len({(m.dtype, m.device) for m in maps}) != 1:
            raise TypeError("maps must be float32 or float64, of one dtype, on one device")
        r = cls([m.shape for m in maps], maps[0].dtype, maps[0].device)
        for i, m in enumerate(maps):
            r.map(i).copy_(m)
        return r


def _ragged(maps):
    return maps if isinstance(maps, Ragged) else Ragged.pack(maps)


def scaled_depths(pred, ratios, sizes, dtype=None) -> Ragged:
    """What the reference's evaluate_depth returns for these predictions: pred [N, h, w] on the device (float32 or
    float64), resized through its inverse depth to sizes[i] = (H_i, W_i) and multiplied by ratios[i] in ``dtype`` -- the
    promotion of the ground truth's dtype and the prediction's (default: the prediction's)."""
    _check_device(pred, "pred")
    if pred.dtype not in _NP or pred.dim() != 3 or pred.numel() < 1:
        raise ValueError("pred must be float32 or float64 [N, h, w] with at least one pixel")
    dtype = dtype or pred.dtype
    if dtype not in _NP or (pred.dtype == torch.float64 and dtype != torch.float64):
        raise ValueError("the scaled prediction is float32 or float64 and never narrower than the prediction")
    pred = pred.contiguous()
    N, h, w = pred.shape
    with torch.cuda.device(pred.device):
        out = Ragged(sizes, dtype, pred.device)
        if len(out) != N:
            raise ValueError(f"{len(out)} sizes for {N} predictions")
        d_ratio = torch.from_numpy(np.asarray(ratios, np.float64).reshape(N).astype(_NP[dtype])).to(pred.device)
        _lib.get_dvis().call("scsfm_dvis_scaled_depth", N, h, w, int(pred.dtype == torch.float64), _ptr(pred),
                             int(dtype == torch.float64), _ptr(d_ratio), _ptr(out.d_off), _ptr(out.d_h), _ptr(out.d_w),
                             out.max_hw, _ptr(out.buf), _stream(pred.device))
    return out


def depth_range(maps):
    """(vmin, vmax) of every map's inverse depth 1 / (x + 1e-6): its minimum and np.percentile(., 95), in the maps'
    precision.  -> float64 [N, 2] on the device, each value the exact widening of one of that precision; both NaN for a
    map that holds a NaN.  ``maps``: a list of [H_i, W_i] device tensors, one [N, H, W] tensor or a Ragged."""
    r = _ragged(maps)
    device, T = r.buf.device, _NP[r.buf.dtype]
    f64 = int(r.buf.dtype == torch.float64)
    idx = [percentile_index(int(n), T) for n in r.hw]
    with torch.cuda.device(device):
        lib = _lib.get_dvis()
        d_lo = torch.tensor([i[0] for i in idx], dtype=torch.int32).to(device)
        d_hi = torch.tensor([i[1] for i in idx], dtype=torch.int32).to(device)
        d_t = torch.from_numpy(np.array([i[2] for i in idx], T)).to(device)
        nbytes = lib.size("scsfm_dvis_range_workspace_bytes", r.total, f64)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        out = torch.empty((len(r), 2), dtype=torch.float64, device=device)
        lib.call("scsfm_dvis_range", len(r), f64, _ptr(r.buf), _ptr(r.d_off), _ptr(r.d_h), _ptr(r.d_w), r.total,
                 _ptr(d_lo), _ptr(d_hi), _ptr(d_t), _ptr(ws), nbytes, _ptr(out), _stream(device))
    return out


def _table_on(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(MAGMA.copy()).to(device)
    return _device_tables[key]


def colourise(maps, ranges, out=None):
    """The magma picture of every map's inverse depth in ranges[i] = (vmin, vmax) (float64 [N, 2] on the device, as
    depth_range gives it -- possibly another set's).  ``out``: a list of uint8 views [H_i, W_i, 3] of ONE device buffer,
    unit stride along the last two axes (panels of wider canvases), written in place; default: fresh pictures.
    -> the list of pictures."""
    r = _ragged(maps)
    device = r.buf.device
    _check_device(ranges, "ranges")
    if ranges.dtype != torch.float64 or tuple(ranges.shape) != (len(r), 2):
        raise ValueError(f"ranges must be float64 [{len(r)}, 2]")
    ranges = ranges.contiguous()
    with torch.cuda.device(device):
        if out is None:
            flat = torch.empty(int(3 * r.hw.sum()), dtype=torch.uint8, device=device)
            ends = np.cumsum(3 * r.hw)
            out = [flat[e - 3 * n:e].view(int(s[0]), int(s[1]), 3) for e, n, s in zip(ends, r.hw, r.sizes)]
        if len(out) != len(r):
            raise ValueError(f"{len(out)} pictures for {len(r)} maps")
        store = out[0].untyped_storage()
        base = store.data_ptr()
        offs, pitches = [], []
        for o, s in zip(out, r.sizes):
            if o.dtype != torch.uint8 or tuple(o.shape) != (int(s[0]), int(s[1]), 3) or o.stride(2) != 1 or \
                    o.stride(1) != 3 or (s[0] > 1 and o.stride(0) < 3 * s[1]) or \
                    o.untyped_storage().data_ptr() != base:
                raise ValueError("every picture must be a uint8 [H, W, 3] view of one buffer with packed pixels")
            last = o.storage_offset() + (int(s[0]) - 1) * o.stride(0) + 3 * int(s[1])
            if last > store.nbytes():
                raise ValueError("a picture reaches past its buffer")
            offs.append(o.storage_offset())
            pitches.append(o.stride(0) if s[0] > 1 else 3 * int(s[1]))
        d_ooff = torch.tensor(offs, dtype=torch.int64).to(device)
        d_pitch = torch.tensor(pitches, dtype=torch.int32).to(device)
        _lib.get_dvis().call("scsfm_dvis_colourise", len(r), int(r.buf.dtype == torch.float64), _ptr(r.buf),
                             _ptr(r.d_off), _ptr(r.d_h), _ptr(r.d_w), r.max_hw, _ptr(ranges), _ptr(_table_on(device)),
                             ctypes.c_void_p(base), _ptr(d_ooff), _ptr(d_pitch), _stream(device))
    return out


def depth_pictures(maps):
    """The reference's depth_visualizer for every map: -> (ranges float64 [N, 2], [uint8 [H_i, W_i, 3]]), on the
    device."""
    r = _ragged(maps)
    ranges = depth_range(r)
    return ranges, colourise(r, ranges)


def depth_pair_pictures(preds, gts):
    """The reference's depth_pair_visualizer for every pair: both pictures in the ground truth's range.
    -> (ranges, prediction pictures, ground-truth pictures)."""
    p, g = _ragged(preds), _ragged(gts)
    ranges = depth_range(g)
    return ranges, colourise(p, ranges), colourise(g, ranges)


def _on(x, device):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device)


def evaluated_indices(res):
    """The predictions the reference visualises: those it evaluated (a mean of exactly -1 is skipped), in order."""
    return np.flatnonzero(np.asarray(res.evaluated))


def picture_sizes(res, gt_depths):
    """(H, W) of picture k = 0, 1, ...: the size of the ground-truth map the k-th evaluated prediction was resized to."""
    return [tuple(int(v) for v in gt_depths[i].shape[:2]) for i in evaluated_indices(res)]


def composites(res, pred_depths, gt_depths, dataset, photos, first=0):
    """The canvases eval_depth.py --vis_dir writes, numbers ``first`` .. ``first + len(photos) - 1``, as uint8 device
    tensors.  ``res``: the DepthEvalResult of evaluate_depth(gt_depths, pred_depths, dataset); ``pred_depths`` [N, h, w]
    and ``gt_depths`` (a list of [H_i, W_i] or [N, H, W]): arrays or tensors, on the host or the device -- only this
    chunk's maps are moved; ``photos``: this chunk's photographs, uint8 [H, W, 3] device tensors.

    Pictures are numbered over the evaluated predictions, as in the reference: picture k shows the k-th evaluated
    prediction (resized to ITS ground truth's size and scaled by its ratio), photograph k and, on NYU, ground truth k.
      kitti: [2H, W, 3]: the photograph above the prediction's picture in the prediction's own range;
      nyu:   [H, 3W, 3]: photograph, prediction's picture, ground truth's picture, both in the ground truth's range.
    The results do not depend on how the set is cut into chunks."""
    if dataset not in ("kitti", "nyu"):
        raise ValueError(f"dataset must be 'kitti' or 'nyu', got {dataset!r}")
    photos = list(photos)
    if not photos:
        return []
    _check_device(photos[0], "photos")
    device = photos[0].device
    ev = evaluated_indices(res)
    if first < 0 or first + len(photos) > len(ev):
        raise ValueError(f"pictures {first} .. {first + len(photos) - 1} of {len(ev)} evaluated predictions")
    idx = ev[first:first + len(photos)]
    sizes = [tuple(int(v) for v in gt_depths[i].shape[:2]) for i in idx]
    for k, (p, s) in enumerate(zip(photos, sizes)):
        if p.dtype != torch.uint8 or p.dim() != 3 or p.shape[2] != 3 or p.device != device:
            raise ValueError("photos must be uint8 [H, W, 3] tensors on one device")
        if tuple(p.shape[:2]) != s:
            raise ValueError(f"photograph {first + k} is {p.shape[0]} x {p.shape[1]} but its depth map is "
                             f"{s[0]} x {s[1]}")
    with torch.cuda.device(device):
        pred = torch.stack([_on(pred_depths[i], device) for i in idx])
        gdt = _on(gt_depths[0], "cpu").dtype if not isinstance(gt_depths[0], torch.Tensor) else gt_depths[0].dtype
        if gdt not in _NP or pred.dtype not in _NP:
            raise TypeError("depth maps must be float32 or float64")
        rdt = torch.promote_types(gdt, pred.dtype)
        scaled = scaled_depths(pred, np.asarray(res.ratio)[idx], sizes, rdt)
        nyu = dataset == "nyu"
        nbytes = np.array([(9 if nyu else 6) * h * w for h, w in sizes], np.int64)
        ends = np.cumsum(nbytes)
        flat = torch.empty(int(ends[-1]), dtype=torch.uint8, device=device)
        canvases = [flat[e - n:e].view(*((h, 3 * w, 3) if nyu else (2 * h, w, 3)))
                    for e, n, (h, w) in zip(ends, nbytes, sizes)]
        for c, p, (h, w) in zip(canvases, photos, sizes):
            (c[:, :w] if nyu else c[:h]).copy_(p)
        if nyu:
            gts = [_on(gt_depths[first + k], device) for k in range(len(photos))]
            if any(tuple(g.shape) != s for g, s in zip(gts, sizes)):
                raise ValueError("on NYU every ground-truth map has one size")
            gt = Ragged.pack(gts)
            ranges = depth_range(gt)
            colourise(scaled, ranges, [c[:, w:2 * w] for c, (h, w) in zip(canvases, sizes)])
            colourise(gt, ranges, [c[:, 2 * w:] for c, (h, w) in zip(canvases, sizes)])
        else:
            colourise(scaled, depth_range(scaled), [c[h:] for c, (h, w) in zip(canvases, sizes)])
    return canvases
