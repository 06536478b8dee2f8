"""Drop-in for the reference's ``loss_functions`` module, backed by hand-written HIP kernels.

Same public names, positional signatures, return arity and flag conventions as
/root/reference/loss_functions.py, so that ``from loss_functions import compute_smooth_loss,
compute_photo_and_geometry_loss, compute_errors`` (train.py:19) resolves here when this directory
precedes the reference on PYTHONPATH.

What changes underneath: one ``compute_pairwise_loss`` is 182 ATen kernels forward
+ 221 backward in the reference; here it is one fused HIP kernel forward and one backward
(csrc/scsfm_pair.hip).  ``compute_photo_and_geometry_loss`` puts all refs x scales x directions
behind a single autograd node that accumulates the depth gradients in place.  The 10000-pixel gate
of ``mean_on_mask`` is evaluated on the device, so the loss path never synchronises with the host;
a gated-off term is a zero that still carries a (zero-gradient) ``grad_fn``, where the reference
returns a fresh constant (loss_functions.py:128).

All tensors must be HIP ('cuda') tensors.  There is no CPU path in this package.
"""
from __future__ import division

import torch
import torch.nn.functional as F
from torch import nn

from inverse_warp import inverse_warp, inverse_warp2  # noqa: F401  (re-exported like the reference, :5)
from scsfm_hip import capi, config, ops, validation

device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


class SSIM(nn.Module):
    """clamp((1 - SSIM(x, y)) / 2, 0, 1) over reflect-padded 3x3 windows (loss_functions.py:11-42).
    Standalone HIP kernel (csrc/scsfm_aux.hip) with gradients to both inputs; inside the training
    loss the same arithmetic runs fused in the pair kernels."""

    def __init__(self):
        super(SSIM, self).__init__()
        self.C1 = 0.01 ** 2
        self.C2 = 0.03 ** 2

    def forward(self, x, y):
        return ops.SsimMap.apply(x, y)


compute_ssim_loss = SSIM().to(device)


def _scale_maps(tgt_depth, ref_depths, n_ref, num_scales, b, h, w):
    """The depth maps of every scale as the kernels take them (loss_functions.py:77-82).  A coarser scale whose maps are
    [b, 1, h >> k, w >> k] (what DispResNet emits) is passed as it is: the kernels index it through the nearest
    up-sampling's map and sum-pool the gradient (scsfm_pair_desc::depth_shift).  Any other shape is up-sampled with
    F.interpolate under autograd, as the reference does."""
    if num_scales == 1:  # (the usual step)
        maps = [tgt_depth[0]] + [ref_depths[i][0] for i in range(n_ref)]
        for d in maps:
            if d.shape[-1] != w or d.shape[-2] != h:  # scale 0 is never re-sampled (:77-79)
                capi.check_sizes(d, "depth", (b, 1, h, w))
        return maps[:1], maps[1:]

    def fused(s):
        maps = [tgt_depth[s]] + [ref_depths[i][s] for i in range(n_ref)]
        return capi.depth_shift(maps[0].shape, b, h, w) is not None and all(m.shape == maps[0].shape for m in maps)

    for d in [tgt_depth[0]] + [ref_depths[i][0] for i in range(n_ref)]:  # scale 0 is never re-sampled (:77-79)
        capi.check_sizes(d, "depth", (b, 1, h, w))
    keep = [s == 0 or fused(s) for s in range(num_scales)]

    def full_res(d, s):
        return d if keep[s] else F.interpolate(d, (h, w), mode='nearest')

    tgt_full = [full_res(tgt_depth[s], s) for s in range(num_scales)]
    ref_full = [full_res(ref_depths[i][s], s) for i in range(n_ref) for s in range(num_scales)]
    return tgt_full, ref_full


def compute_photo_and_geometry_loss(tgt_img, ref_imgs, intrinsics, tgt_depth, ref_depths, poses, poses_inv,
                                    max_scales, with_ssim, with_mask, with_auto_mask, padding_mode):
    """loss_functions.py:50-92 -> (photo_loss, geometry_loss), summed over refs, scales and both
    directions.  Scale s > 0 depth maps are nearest-upsampled to the image size (:81-82)."""
    num_scales = min(len(tgt_depth), max_scales)
    n_ref = len(ref_imgs)
    if n_ref == 0 or num_scales <= 0:
        return 0, 0  # the reference's accumulators stay the Python ints they start as (:52-53)
    b, _, h, w = tgt_img.size()
    flags = capi.make_flags(with_ssim, with_mask, with_auto_mask, padding_mode)

    tgt_full, ref_full = _scale_maps(tgt_depth, ref_depths, n_ref, num_scales, b, h, w)
    photo, geom, smooth = ops.PhotoGeometryLoss.apply(flags, n_ref, num_scales, tgt_img, intrinsics, *ref_imgs, *tgt_full,
                                                      *ref_full, *poses[:n_ref], *poses_inv[:n_ref])
    if smooth is not None:
        # the speculative forward evaluated compute_smooth_loss of these very frames on the way (third output of the same
        # autograd node): it waits for the call train.py:262-266 makes next, keyed on the tensor objects handed in here
        ops._SmoothStash.put([tgt_depth[0]] + [ref_depths[i][0] for i in range(n_ref)], [tgt_img] + list(ref_imgs[:n_ref]), smooth)
    return photo, geom


def compute_pairwise_loss(tgt_img, ref_img, tgt_depth, ref_depth, pose, intrinsic, with_ssim, with_mask,
                          with_auto_mask, padding_mode):
    """loss_functions.py:95-119 -> (reconstruction_loss, geometry_consistency_loss)."""
    flags = capi.make_flags(with_ssim, with_mask, with_auto_mask, padding_mode)
    return ops.PairwiseLoss.apply(flags, tgt_img, ref_img, tgt_depth, ref_depth, pose, intrinsic)


def mean_on_mask(diff, valid_mask):
    """sum(diff * mask) / sum(mask) if the expanded mask holds more than 10000 ones, else 0
    (loss_functions.py:123-129); the gate is evaluated on the device."""
    return ops.MaskedMean.apply(diff, valid_mask)


def compute_smooth_loss(tgt_depth, tgt_img, ref_depths, ref_imgs):
    """loss_functions.py:132-159: edge-aware smoothness of the mean-normalised depth at scale 0,
    summed over the target and every reference frame."""
    depths = [tgt_depth[0]] + [rd[0] for rd, _ in zip(ref_depths, ref_imgs)]
    imgs = [tgt_img] + [im for _, im in zip(ref_depths, ref_imgs)]
    waiting = ops._SmoothStash.take(depths, imgs)  # left by compute_photo_and_geometry_loss on the same tensors?
    if waiting is not None:
        return waiting
    return ops.SmoothLoss.apply(len(depths), *depths, *imgs)


# frames one launch of scsfm_smooth_multi_fwd_step holds (csrc/scsfm_smooth.hip: kMaxFrames)
MAX_FUSED_FRAMES = 8


def compute_total_loss(tgt_img, ref_imgs, intrinsics, tgt_depth, ref_depths, poses, poses_inv, max_scales, with_ssim,
                       with_mask, with_auto_mask, padding_mode, w_photo, w_smooth, w_geom):
    """Not in the reference: what train.py:259-268 computes -- compute_photo_and_geometry_loss,
    compute_smooth_loss and ``loss = w1*loss_1 + w2*loss_2 + w3*loss_3`` -- behind one autograd node.
    -> (loss, loss_1 photo, loss_2 smooth, loss_3 geometry); only ``loss`` carries gradient.  Same values and
    gradients as the three reference-style calls (tests), ~10 % less device time per step: autograd no longer
    runs scalar kernels for the weighted sum nor adds the two gradient contributions of every depth map."""
    num_scales = min(len(tgt_depth), max_scales)
    n_ref = len(ref_imgs)
    if n_ref == 0 or num_scales <= 0:
        raise ValueError("compute_total_loss needs at least one reference frame and one scale")
    b, _, h, w = tgt_img.size()
    flags = capi.make_flags(with_ssim, with_mask, with_auto_mask, padding_mode)

    if 1 + n_ref > MAX_FUSED_FRAMES:
        # the fused smooth forward / combine hold one launch's frames (8 = target + 7 references; the combine caps at
        # 16): longer sequences take the reference's call structure -- same values and gradients, three autograd nodes
        photo, geom = compute_photo_and_geometry_loss(tgt_img, ref_imgs, intrinsics, tgt_depth, ref_depths, poses, poses_inv,
                                                      max_scales, with_ssim, with_mask, with_auto_mask, padding_mode)
        smooth = compute_smooth_loss(tgt_depth, tgt_img, ref_depths, ref_imgs)
        loss = w_photo * photo + w_smooth * smooth + w_geom * geom
        return loss, photo.detach(), smooth.detach(), geom.detach()
    tgt_full, ref_full = _scale_maps(tgt_depth, ref_depths, n_ref, num_scales, b, h, w)
    return ops.StepLoss.apply(flags, n_ref, num_scales, float(w_photo), float(w_smooth), float(w_geom), tgt_img, intrinsics,
                              *ref_imgs, *tgt_full, *ref_full, *poses[:n_ref], *poses_inv[:n_ref])


@torch.no_grad()
def compute_errors(gt, pred, dataset):
    """loss_functions.py:162-205 -> [abs_diff, abs_rel, sq_rel, a1, a2, a3] (Python floats, batch
    means).  Validation-only.  fp32 tensors on a HIP device go through libscsfm_val.so
    (scsfm_hip/validation.py: one call per batch, one read-back); anything else -- CPU tensors, other
    dtypes, or config.errors_on_torch() -- takes the torch body below."""
    if (gt.is_cuda and pred.device == gt.device and gt.dtype == torch.float32 and pred.dtype == torch.float32
            and not config.errors_on_torch()):
        return validation.batch_mean(validation.depth_errors(gt, pred, dataset))
    return _compute_errors_torch(gt, pred, dataset)


def _compute_errors_torch(gt, pred, dataset):
    """compute_errors on PyTorch ops: boolean-mask gathers and per-image medians, the six metric sums
    accumulated on the device and read back once."""
    batch_size, h, w = gt.size()
    if dataset == 'kitti':  # Garg/Eigen crop
        y1, y2 = int(0.40810811 * h), int(0.99189189 * h)
        x1, x2 = int(0.03594771 * w), int(0.96405229 * w)
        max_depth = 80
    elif dataset == 'nyu':
        y1, y2 = int(0.09375 * h), int(0.98125 * h)
        x1, x2 = int(0.0640625 * w), int(0.9390625 * w)
        max_depth = 10
    else:
        # the reference leaves crop_mask unbound for any other name (:172-185)
        raise UnboundLocalError("dataset must be 'kitti' or 'nyu', got {!r}".format(dataset))
    crop_mask = torch.zeros(h, w, dtype=torch.bool, device=gt.device)
    crop_mask[y1:y2, x1:x2] = True
    totals = torch.zeros(6, dtype=torch.float32, device=gt.device)
    for current_gt, current_pred in zip(gt, pred):
        valid = (current_gt > 0.1) & (current_gt < max_depth) & crop_mask
        valid_gt = current_gt[valid]
        valid_pred = current_pred[valid].clamp(1e-3, max_depth)
        valid_pred = valid_pred * torch.median(valid_gt) / torch.median(valid_pred)
        thresh = torch.max(valid_gt / valid_pred, valid_pred / valid_gt)
        err = torch.abs(valid_gt - valid_pred)
        totals += torch.stack([err.mean(), (err / valid_gt).mean(), (err ** 2 / valid_gt).mean(),
                               (thresh < 1.25).float().mean(), (thresh < 1.25 ** 2).float().mean(),
                               (thresh < 1.25 ** 3).float().mean()]).float()
    return [v / batch_size for v in totals.tolist()]
