"""DispResNet: ResNet encoder + monodepth2-style decoder, disparity = 10 * sigmoid + 0.01 at four
scales (models/DispResNet.py:49-121).  State-dict layout: ``encoder.encoder.*`` and
``decoder.decoder.<k>`` with k = 0..9 the (upconv i, j) blocks for i = 4..0, j = 0..1 and k = 10..13
the disparity heads of scales 0..3."""
from __future__ import absolute_import, division, print_function

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .resnet_encoder import ResnetEncoder


class Conv3x3(nn.Module):
    def __init__(self, in_channels, out_channels, use_refl=True):
        super().__init__()
        self.pad = nn.ReflectionPad2d(1) if use_refl else nn.ZeroPad2d(1)
        self.conv = nn.Conv2d(int(in_channels), int(out_channels), 3)

    def forward(self, x):
        return self.conv(self.pad(x))


class ConvBlock(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = Conv3x3(in_channels, out_channels)
        self.nonlin = nn.ELU(inplace=True)

    def forward(self, x):
        return self.nonlin(self.conv(x))


class DepthDecoder(nn.Module):
    def __init__(self, num_ch_enc, scales=range(4), num_output_channels=1, use_skips=True):
        super().__init__()
        self.alpha, self.beta = 10, 0.01
        self.use_skips = use_skips
        self.scales = list(scales)
        self.num_ch_enc = num_ch_enc
        self.num_ch_dec = np.array([16, 32, 64, 128, 256])
        blocks, self._up, self._head = [], {}, {}
        for i in range(4, -1, -1):
            cin = self.num_ch_enc[-1] if i == 4 else self.num_ch_dec[i + 1]
            self._up[(i, 0)] = len(blocks)
            blocks.append(ConvBlock(cin, self.num_ch_dec[i]))
            cin = self.num_ch_dec[i] + (self.num_ch_enc[i - 1] if use_skips and i > 0 else 0)
            self._up[(i, 1)] = len(blocks)
            blocks.append(ConvBlock(cin, self.num_ch_dec[i]))
        for s in self.scales:
            self._head[s] = len(blocks)
            blocks.append(Conv3x3(self.num_ch_dec[s], num_output_channels))
        self.decoder = nn.ModuleList(blocks)
        self.sigmoid = nn.Sigmoid()

    def forward(self, feats):
        if self.fused_path_applies(feats):
            if self.bias_path_applies():
                return self.forward_fused_bias(feats)
            return self.forward_fused(feats)
        return self.forward_reference(feats)

    def bias_path_applies(self):
        """On the fused path, the biases of the convolutions are folded into the glue behind them (forward_fused_bias)
        when every one of them is a contiguous CUDA fp32 tensor, unless SCSFM_DECODER_BIAS=0 (scsfm_hip.config) selects
        forward_fused."""
        from scsfm_hip import config
        if not config.decoder_bias_folded():
            return False
        biases = [self._conv(k).bias for k in range(len(self.decoder))]
        return all(b is not None and b.is_cuda and b.dtype == torch.float32 and b.is_contiguous() for b in biases)

    def fused_path_applies(self, feats):
        """CUDA fp32 contiguous NCHW features and weights take the fused HIP glue (forward_fused); CPU, fp64 and
        channels_last run the reference chain (forward_reference) unchanged."""
        return all(f.is_cuda and f.dtype == torch.float32 and f.dim() == 4 and f.is_contiguous() for f in feats) and \
            all(self._conv(k).weight.dtype == torch.float32 and self._conv(k).weight.is_contiguous()
                for k in range(len(self.decoder)))

    def _conv(self, k):
        """the nn.Conv2d of block k (a ConvBlock's or a head's Conv3x3), called without its pad"""
        m = self.decoder[k]
        return m.conv.conv if isinstance(m, ConvBlock) else m.conv

    def forward_reference(self, feats):
        outputs = []
        x = feats[-1]
        for i in range(4, -1, -1):
            x = self.decoder[self._up[(i, 0)]](x)
            x = F.interpolate(x, scale_factor=2, mode="nearest")
            if self.use_skips and i > 0:
                x = torch.cat([x, feats[i - 1]], 1)
            x = self.decoder[self._up[(i, 1)]](x)
            if i in self._head:
                outputs.append(self.alpha * self.sigmoid(self.decoder[self._head[i]](x)) + self.beta)
        return outputs[::-1]

    def forward_fused(self, feats):
        """forward_reference with every reflection pad, ELU, upsampling and concatenation done by the HIP kernels of
        scsfm_hip.decoder: the same modules' convolutions (``Conv3x3.conv``, ``_conv``) receive the same padded tensors, bit for
        bit.  Per level i: a = conv (i,0)(P), P = R(cat[U(E(a)), f_{i-1}]), b = conv (i,1)(P), Q = R(E(b)); Q is
        the input of both conv (i-1,0) and head i (the reference pads E(b) once for each)."""
        from scsfm_hip import conv_wrw as CW, decoder as D

        def conv(k, x):
            m = self._conv(k)
            if CW.applies(x, m):  # (the weight gradient from libscsfm_wrw.so; the bias as ATen adds it)
                y = CW.conv3x3_valid(x, m.weight)
                return y if m.bias is None else y + m.bias.view(1, -1, 1, 1)
            return m(x)

        outputs = []
        x = D.pad(feats[-1])
        for i in range(4, -1, -1):
            a = conv(self._up[(i, 0)], x)
            x = D.up_cat_pad(a, feats[i - 1] if self.use_skips and i > 0 else None)
            b = conv(self._up[(i, 1)], x)
            if i == 0 and i not in self._head:
                break
            x = D.elu_pad(b)
            if i in self._head:
                outputs.append(self.alpha * self.sigmoid(conv(self._head[i], x)) + self.beta)
        return outputs[::-1]

    def forward_fused_bias(self, feats):
        """forward_fused with every convolution called without its bias, which the glue that follows adds in front of
        its ELU (scsfm_hip.decoder_bias.up_cat_pad / elu_pad) or of the head's sigmoid (disp_head), and whose gradient
        that glue's backward sums: ATen's broadcast add after each convolution and its grad_output.sum((0, 2, 3)) no
        longer run as passes of their own.  The low-channel convolutions that scsfm_hip.conv_wrw routes take their weight
        gradient from libscsfm_wrw.so (SCSFM_DECODER_WRW=0: MIOpen's, as every other layer).  Conv (0, 1) without a head at scale 0 has no glue behind it and keeps its
        module call.  At level 0 the padded tensor feeds the head alone: elu_pad, the head's convolution and disp_head
        are one autograd node there (scsfm_hip.decoder_dgrad.head_tail: the same three launches forward, one streaming
        kernel from libscsfm_dgrad.so backward; SCSFM_DECODER_DGRAD=0: the three nodes, as at the other levels)."""
        from scsfm_hip import conv_wrw as CW, decoder as D, decoder_bias as DB, decoder_dgrad as DG

        def conv(k, x):
            m = self._conv(k)
            if CW.applies(x, m):  # (the weight gradient from libscsfm_wrw.so)
                return CW.conv3x3_valid(x, m.weight), m.bias
            if CW.applies_without_wrw(x, m):  # (SCSFM_DECODER_WRW=0: the input gradient alone from libscsfm_dgrad.so)
                return CW.conv3x3_valid(x, m.weight, wrw=False), m.bias
            return F.conv2d(x, m.weight, None, m.stride, m.padding, m.dilation, m.groups), m.bias

        outputs = []
        x = D.pad(feats[-1])
        for i in range(4, -1, -1):
            a, bias = conv(self._up[(i, 0)], x)
            x = DB.up_cat_pad(a, bias, feats[i - 1] if self.use_skips and i > 0 else None)
            if i == 0 and i not in self._head:
                self._conv(self._up[(i, 1)])(x)
                break
            b, bias = conv(self._up[(i, 1)], x)
            if i == 0 and DG.applies(b, bias, self._conv(self._head[0])):
                head = self._conv(self._head[0])
                outputs.append(DG.head_tail(b, bias, head.weight, head.bias, self.alpha, self.beta))
                break
            x = DB.elu_pad(b, bias)
            if i in self._head:
                h, bias = conv(self._head[i], x)
                outputs.append(DB.disp_head(h, bias, self.alpha, self.beta))
        return outputs[::-1]


class DispResNet(nn.Module):
    def __init__(self, num_layers=18, pretrained=True):
        super().__init__()
        self.encoder = ResnetEncoder(num_layers=num_layers, pretrained=pretrained, num_input_images=1)
        self.decoder = DepthDecoder(self.encoder.num_ch_enc)

    def init_weights(self):
        pass

    def forward(self, x):
        outputs = self.decoder(self.encoder(x))
        return outputs if self.training else outputs[0]
