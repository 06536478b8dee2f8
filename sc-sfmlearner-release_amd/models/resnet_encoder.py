"""ResNet-18 / -50 encoder with the parameter names of torchvision's ``ResNet`` (conv1, bn1,
layer1..4.<i>.{conv,bn}<k>, downsample.{0,1}, fc), which is what the reference's checkpoints hold under
``encoder.encoder.*`` (models/resnet_encoder.py:17-61; utils.py:57-66).  ``fc`` and ``avgpool`` are
kept although the encoder never calls them -- they are in the state dict."""
from __future__ import absolute_import, division, print_function

import numpy as np
import torch
import torch.nn as nn


_encoder_ops = None


def _E():
    """scsfm_hip.encoder, imported on first use (a CPU-only run never loads it)"""
    global _encoder_ops
    if _encoder_ops is None:
        from scsfm_hip import encoder
        _encoder_ops = encoder
    return _encoder_ops


_encoder_eval_ops = None


def _EV():
    """scsfm_hip.encoder_eval, imported on first use (a CPU-only run never loads it)"""
    global _encoder_eval_ops
    if _encoder_eval_ops is None:
        from scsfm_hip import encoder_eval
        _encoder_eval_ops = encoder_eval
    return _encoder_eval_ops


_encoder_frozen_ops = None


def _EF():
    """scsfm_hip.encoder_frozen, imported on first use (a CPU-only run never loads it)"""
    global _encoder_frozen_ops
    if _encoder_frozen_ops is None:
        from scsfm_hip import encoder_frozen
        _encoder_frozen_ops = encoder_frozen
    return _encoder_frozen_ops


def _fused_applies(x, *bns):
    """CUDA fp32 contiguous NCHW activations through training-mode BatchNorms take the fused HIP glue
    (scsfm_hip.encoder); eval mode is ``_eval_applies``'s; CPU, fp64, channels_last and BatchNorms without affine
    parameters, running statistics or a fixed momentum run the ATen chain unchanged."""
    return x.is_cuda and _E().applies(x, *bns)


def _eval_applies(x, *bns):
    """CUDA fp32 contiguous NCHW activations through eval-mode BatchNorms with grad mode off take the fused eval-mode HIP
    glue (scsfm_hip.encoder_eval); eval mode with grad enabled is ``_frozen_applies``'s where the module was frozen and
    ATen's otherwise; SCSFM_EVAL_TORCH=1, CPU, fp64, channels_last and BatchNorms without affine parameters or running
    statistics run the ATen chain unchanged."""
    return x.is_cuda and _EV().applies(x, *bns)


def _frozen_applies(x, *bns, relu=True):
    """CUDA fp32 contiguous NCHW activations with grad mode on through BatchNorms that scsfm_hip.encoder_frozen.freeze
    holds in eval mode (train.py --freeze-bn) take the fused frozen-statistics HIP glue where a ReLU follows; a BatchNorm
    without one (the down-sample branch: nothing to fuse, and measured slower), a module that is merely in eval
    mode, SCSFM_FROZEN_TORCH=1, CPU, fp64 and channels_last run the ATen chain unchanged.  (The class is looked at only
    once the module is known not to be in training mode: the ordinary step pays one attribute test.)"""
    return x.is_cuda and not any(bn.training for bn in bns) and _EF().applies(x, *bns, relu=relu)


def _bn_act(x, bn, act, identity=None):
    """act(bn(x) [+ identity]), fused when the call qualifies (act is the module's in-place ReLU, or None): by
    scsfm_hip.encoder in training mode, else by scsfm_hip.encoder_frozen for a frozen module with grad mode on and a
    ReLU behind it, else by scsfm_hip.encoder_eval in eval mode under no_grad, else ATen"""
    if _fused_applies(x, bn) and (identity is None or _fused_applies(identity)):
        return _E().bn_act(x, bn, identity, relu=act is not None)
    if _frozen_applies(x, bn, relu=act is not None) and (identity is None or _frozen_applies(identity)):
        return _EF().bn_act(x, bn, identity, relu=act is not None)
    if _eval_applies(x, bn) and (identity is None or _eval_applies(identity)):
        return _EV().bn_act(x, bn, identity, relu=act is not None)
    out = bn(x)
    if identity is not None:
        out = out + identity
    return out if act is None else act(out)


_conv1x1_ops = None


def _PW():
    """scsfm_hip.conv1x1, imported on first use (a CPU-only run never loads it)"""
    global _conv1x1_ops
    if _conv1x1_ops is None:
        from scsfm_hip import conv1x1
        _conv1x1_ops = conv1x1
    return _conv1x1_ops


def _downsample(ds, x):
    """the down-sample branch nn.Sequential(conv, bn); the 1x1 convolution keeps its forward and takes its backward
    from scsfm_hip.conv1x1 where that applies (CUDA fp32 contiguous NCHW with grad mode on, a routed shape) and the
    blocks run the project's own glue: a BatchNorm in training mode, or one that scsfm_hip.encoder_frozen.freeze holds
    (SCSFM_FROZEN_TORCH=1 sends a frozen net down the ATen chain whole, this convolution's backward included); a module
    that is merely in eval mode keeps the plain call"""
    conv, bn = ds[0], ds[1]
    hip = x.is_cuda and (bn.training or (_EF().is_frozen(bn) and _EF().enabled()))
    y = _PW().conv(conv, x) if hip else conv(x)
    return _bn_act(y, bn, None)


def _conv3x3(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = _conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        identity = x if self.downsample is None else _downsample(self.downsample, x)
        out = _bn_act(self.conv1(x), self.bn1, self.relu)
        return _bn_act(self.conv2(out), self.bn2, self.relu, identity)

    def forward_reference(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + identity)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = _conv3x3(planes, planes, stride)  # stride on the 3x3 (torchvision "v1.5")
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x if self.downsample is None else _downsample(self.downsample, x)
        out = _bn_act(self.conv1(x), self.bn1, self.relu)
        out = _bn_act(self.conv2(out), self.bn2, self.relu)
        return _bn_act(self.conv3(out), self.bn3, self.relu, identity)

    def forward_reference(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


class ResNet(nn.Module):
    """The trunk; ``num_input_images`` frames are stacked on the channel axis of conv1
    (models/resnet_encoder.py:21-23)."""

    def __init__(self, block, layers, num_classes=1000, num_input_images=1):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(num_input_images * 3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)


_CFG = {18: (BasicBlock, [2, 2, 2, 2]), 50: (Bottleneck, [3, 4, 6, 3])}


def imagenet_weights_path(num_layers):
    """Local stand-in for the reference's model-zoo download: $SCSFM_IMAGENET_WEIGHTS/resnet<N>.pth or None."""
    import os
    root = os.environ.get("SCSFM_IMAGENET_WEIGHTS")
    if not root:
        return None
    path = os.path.join(root, "resnet{}.pth".format(num_layers))
    return path if os.path.exists(path) else None


class ResnetEncoder(nn.Module):
    """Five feature maps at strides 2..32 (models/resnet_encoder.py:64-97)."""

    def __init__(self, num_layers, pretrained, num_input_images=1):
        super().__init__()
        if num_layers not in _CFG:
            raise ValueError("{} is not a valid number of resnet layers".format(num_layers))
        block, layers = _CFG[num_layers]
        self.num_ch_enc = np.array([64, 64, 128, 256, 512])
        if num_layers > 34:
            self.num_ch_enc[1:] *= 4
        self.encoder = ResNet(block, layers, num_input_images=num_input_images)
        if pretrained:
            # the reference downloads ImageNet weights (models/resnet_encoder.py:53-59); offline they come from a
            # local torchvision state dict: $SCSFM_IMAGENET_WEIGHTS/resnet<N>.pth (train.py checks this at
            # argument-parsing time, before any dataset is touched)
            path = imagenet_weights_path(num_layers)
            if path is None:
                raise RuntimeError("ImageNet-pretrained weights are not reachable offline: set SCSFM_IMAGENET_WEIGHTS "
                                   "to a directory holding resnet{}.pth, or use --with-pretrain 0".format(num_layers))
            loaded = torch.load(path, map_location="cpu")
            # several stacked input frames: the first convolution's filters repeated and rescaled (:55-57)
            loaded['conv1.weight'] = torch.cat([loaded['conv1.weight']] * num_input_images, 1) / num_input_images
            self.encoder.load_state_dict(loaded)
        # never reached by forward(): frozen so that DistributedDataParallel does not wait for them
        for p in self.encoder.fc.parameters():
            p.requires_grad_(False)

    def forward(self, input_image):
        """The stem's BatchNorm / ReLU / max-pool and every block's BatchNorm / ReLU / residual add run as the fused HIP
        kernels of scsfm_hip.encoder where the call qualifies (``_fused_applies``: CUDA fp32 contiguous NCHW in training mode),
        of scsfm_hip.encoder_frozen (``_frozen_applies``: the same tensors with grad mode on through modules that
        ``freeze`` holds in eval mode; its stem is ``_bn_act`` followed by ``_maxpool``), or of scsfm_hip.encoder_eval
        (``_eval_applies``: the same tensors in eval mode with grad mode off), through the same modules' parameters and
        buffers; everything else is ``forward_reference``'s ATen chain."""
        e = self.encoder
        x = e.conv1(input_image)
        if _fused_applies(x, e.bn1) and _E().pool_applies(x):
            # the stem: one kernel writes f0 and the pooled map, one backward serves both
            f0, pooled = _E().bn_act(x, e.bn1, relu=True, pool=True)
        elif _eval_applies(x, e.bn1) and _EV().pool_applies(x):
            # ... and in eval mode one kernel without a backward
            f0, pooled = _EV().bn_act(x, e.bn1, relu=True, pool=True)
        else:
            f0 = _bn_act(x, e.bn1, e.relu)
            pooled = self._maxpool(f0)
        f1 = e.layer1(pooled)
        f2 = e.layer2(f1)
        f3 = e.layer3(f2)
        f4 = e.layer4(f3)
        self.features = [f0, f1, f2, f3, f4]
        return self.features

    def _maxpool(self, f0):
        e = self.encoder
        if f0.is_cuda and e.training and _E().pool_applies(f0):
            return _E().max_pool(f0)
        if f0.is_cuda and not e.training and _EV().pool_applies(f0):
            return _EV().max_pool(f0)
        return e.maxpool(f0)

    def forward_reference(self, input_image):
        """forward() by the ATen chain alone, whatever the input (what the fused path is tested against)"""
        e = self.encoder
        f0 = e.relu(e.bn1(e.conv1(input_image)))
        feats, x = [f0], e.maxpool(f0)
        for layer in (e.layer1, e.layer2, e.layer3, e.layer4):
            for block in layer:
                x = block.forward_reference(x)
            feats.append(x)
        return feats
