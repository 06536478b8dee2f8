"""Run-time knobs of the HIP loss path."""
from __future__ import annotations

# (w_photo, w_geom): the weights the training loop multiplies photo_loss and geometry_loss with
# (train.py:268, defaults -p 1 -c 0.5 of scripts/train_resnet18_depth_256.sh).  With a hint the
# forward of compute_photo_and_geometry_loss already runs the backward's tiled pass (speculative
# forward, see include/scsfm_hip.h: scsfm_pair_fwd_spec).  A wrong hint costs time, never
# correctness: the backward checks the actual upstream gradients on the device and recomputes --
# and leaves them in the device-side copy of the hint (scsfm_pair_desc::hint), so the step after
# a mis-speculated one already speculates on the weights the loop really uses.  set_weight_hint
# is therefore an optimisation of the FIRST step only.
_hint = (1.0, 0.5)
_hint_dev = {}  # device -> float64[2] tensor holding (w_photo, w_geom); rewritten by every backward


def set_weight_hint(w_photo, w_geom):
    """Tell the loss which upstream-gradient ratio to speculate on; ``None, None`` disables it."""
    global _hint
    if w_photo is None:
        # (the device tensors stay alive: a captured HIP graph may still hold their addresses; hint_tensor() hands
        # none out while speculation is off)
        _hint = None
        return
    # the upstream gradients arrive as fp32 tensors: compare against the fp32 roundings of the weights
    # (the device-side check is an exact equality of products)
    import numpy as np
    _hint = (float(np.float32(w_photo)), float(np.float32(w_geom)))
    for t in _hint_dev.values():
        t.copy_(t.new_tensor(_hint))


def weight_hint():
    return _hint


def hint_tensor(device):
    """The device-side (w_photo, w_geom) of ``device`` (created from the host hint on first use); None when speculation
    is disabled."""
    if _hint is None:
        return None
    import torch
    key = (device.type, device.index)
    t = _hint_dev.get(key)
    if t is None:
        t = torch.tensor(_hint, dtype=torch.float64, device=device)
        _hint_dev[key] = t
    return t


def check_window():
    """SCSFM_CHECK_WINDOW=1 (debugging): every speculative forward counts wraps of its fixed-point scatter cells and the
    call raises capi.WindowOverflow if there are any (synchronises; the runtime-flag kernel instantiation).  Read per
    call."""
    import os
    return os.environ.get("SCSFM_CHECK_WINDOW") == "1"


_smooth_rides = None


def smooth_rides_along():
    """Does the speculative forward of compute_photo_and_geometry_loss also evaluate the smooth loss of its frames (round 6:
    scsfm_pair_desc::smooth_ws; the compute_smooth_loss call that follows then finds its result waiting)?  Default on;
    SCSFM_SMOOTH_RIDE=0 (read once) or set_smooth_rides_along(False) restore the stand-alone smooth forward."""
    global _smooth_rides
    if _smooth_rides is None:
        import os
        _smooth_rides = os.environ.get("SCSFM_SMOOTH_RIDE", "1") != "0"
    return _smooth_rides


def set_smooth_rides_along(on):
    global _smooth_rides
    _smooth_rides = bool(on)


_errors_torch = None


def errors_on_torch():
    """Does loss_functions.compute_errors run its torch body (a Python loop over the batch: mask gathers, torch.median,
    some thirty small launches per image) also for fp32 tensors on a HIP device, instead of libscsfm_val.so?  Default
    off; SCSFM_ERRORS_TORCH=1 (read once) or set_errors_on_torch(True) force it (tools/bench_validation_errors.py's
    A/B)."""
    global _errors_torch
    if _errors_torch is None:
        import os
        _errors_torch = os.environ.get("SCSFM_ERRORS_TORCH", "0") == "1"
    return _errors_torch


def set_errors_on_torch(on):
    global _errors_torch
    _errors_torch = bool(on)


_decoder_bias = None


def decoder_bias_folded():
    """Does DepthDecoder.forward call its convolutions without their biases and hand these to the fused glue that
    follows (libscsfm_decb.so: forward_fused_bias), instead of letting ATen add and reduce them in passes of their own
    (forward_fused)?  Default on; SCSFM_DECODER_BIAS=0 (read once) or set_decoder_bias_folded(False) select
    forward_fused."""
    global _decoder_bias
    if _decoder_bias is None:
        import os
        _decoder_bias = os.environ.get("SCSFM_DECODER_BIAS", "1") != "0"
    return _decoder_bias


def set_decoder_bias_folded(on):
    global _decoder_bias
    _decoder_bias = None if on is None else bool(on)


_decoder_wrw = None


def decoder_wrw():
    """Do the depth decoder's low-channel 3x3 convolutions take their weight gradient from libscsfm_wrw.so
    (scsfm_hip.conv_wrw.conv3x3_valid) instead of MIOpen's weight-gradient path?  Default on; SCSFM_DECODER_WRW=0 (read
    once) or set_decoder_wrw(False) restore the plain convolution calls."""
    global _decoder_wrw
    if _decoder_wrw is None:
        import os
        _decoder_wrw = os.environ.get("SCSFM_DECODER_WRW", "1") != "0"
    return _decoder_wrw


def set_decoder_wrw(on):
    global _decoder_wrw
    _decoder_wrw = None if on is None else bool(on)


_decoder_dgrad = None


def decoder_dgrad():
    """Does the depth decoder's full-resolution tail (ELU / pad / disparity head at level 0) take its backward from
    libscsfm_dgrad.so (scsfm_hip.decoder_dgrad.head_tail) instead of the head's sigmoid backward, MIOpen's data gradient
    and the pad / ELU backward as launches of their own?  Default on; SCSFM_DECODER_DGRAD=0 (read once) or
    set_decoder_dgrad(False) restore those calls exactly."""
    global _decoder_dgrad
    if _decoder_dgrad is None:
        import os
        _decoder_dgrad = os.environ.get("SCSFM_DECODER_DGRAD", "1") != "0"
    return _decoder_dgrad


def set_decoder_dgrad(on):
    global _decoder_dgrad
    _decoder_dgrad = None if on is None else bool(on)


_conv1x1_bwd = None


def conv1x1_bwd():
    """Do the encoders' 1x1 down-sample convolutions and the pose decoder's squeeze take their weight gradient, and the
    stride-2 ones their input gradient, from libscsfm_pw.so (scsfm_hip.conv1x1.conv1x1) instead of MIOpen's backward
    paths?  Default on; SCSFM_CONV1X1_BWD=0 (read once) or set_conv1x1_bwd(False) restore the plain module calls."""
    global _conv1x1_bwd
    if _conv1x1_bwd is None:
        import os
        _conv1x1_bwd = os.environ.get("SCSFM_CONV1X1_BWD", "1") != "0"
    return _conv1x1_bwd


def set_conv1x1_bwd(on):
    global _conv1x1_bwd
    _conv1x1_bwd = None if on is None else bool(on)
