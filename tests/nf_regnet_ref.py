"""TEST INFRASTRUCTURE ONLY -- CPU fp32 restatement of the NF-RegNet image encoder (`--image_encoder nf_regnet`).

The reference builds it as ``timm.create_model('nf_regnet_b1', pretrained=True)`` (networks.py:671-672) and keeps
timm's classifier (no ``num_classes=0``), so its image features are the 1000 logits.  timm (0.6.7) is not installed
here, so this restates timm's ``NormFreeNet`` with ``_nfreg_cfg(depths=(2, 4, 7, 7))``: channels (48, 104, 208, 440)
times ``width_factor`` 0.75 (-> 40, 80, 160, 328), stem '3x3' (one ScaledStdConv2d 3->40, 3x3 / 2, no activation, so
EVERY stage strides), ``group_size`` 8, ``reg=True`` (the bottleneck width comes from the block's INPUT channels:
ratio 2.25, and 1.0 in the very first block), squeeze-excite on the mid channels between conv2 and conv3
(``attn``, ``rd_ratio`` 0.5, ``rd_divisor`` 8, ``round_limit`` 0), ``attn_gain`` 2.0, ``alpha`` 0.2, SiLU:

    a = silu(x) * beta ; shortcut = x or downsample(a) ; c1 = conv1(a) ; c2 = conv2(silu(c1)) ;
    u = 2 * c2 * sigmoid(fc2(relu(fc1(mean_hw c2)))) ; x' = alpha * conv3(silu(u)) + shortcut

then ``final_conv`` 328 -> make_divisible(0.75 * 1280) = 960, SiLU, global average pool, ``head.fc = Linear(960, 1000)``.

PARITY UNPINNED, as for the other restatements (oracle/nfnet_ref.py, tests/nf_resnet_ref.py): the reference holds no
test, golden vector or known answer at this boundary and timm is absent.  The only checks are structural anchors:
10,223,984 parameters (timm's published 10.22 M; ``rd_ratio`` 0.25 would give 8.03 M, ``stem_chs`` 16 would give
10,216,496), 66 weight-standardised convolutions (1 + 20 * 3 + 4 downsamples + 1), 20 squeeze-excite modules, 1000
features, timm's parameter registration order (stem.conv, then per block downsample.conv, conv1, conv2, attn.fc1,
attn.fc2, conv3, then final_conv, head.fc).

``ScaledStdConv2d``, ``SEModule``, ``DownsampleAvg`` and ``randomize_like_trained`` come from oracle/nfnet_ref.py
unchanged, ``ClassifierHead`` from tests/nf_resnet_ref.py.
"""
from collections import OrderedDict
from dataclasses import dataclass
from typing import Tuple

import torch.nn as nn
import torch.nn.functional as F

from oracle.nfnet_ref import (GAMMA_SILU, DownsampleAvg, ScaledStdConv2d, SEModule, make_divisible,  # noqa: F401
                              randomize_like_trained)
from nf_resnet_ref import ClassifierHead


@dataclass
class NfRegCfg:
    depths: Tuple[int, ...] = (2, 4, 7, 7)
    channels: Tuple[int, ...] = (48, 104, 208, 440)
    width_factor: float = 0.75
    group_size: int = 8
    bottle_ratio: float = 2.25
    first_ratio: float = 1.0       # timm: `1. if reg and stage_idx == 0 and block_idx == 0`... (first block only)
    num_features: int = 1280
    se_rd_ratio: float = 0.5
    se_rd_divisor: int = 8
    alpha: float = 0.2
    attn_gain: float = 2.0
    std_conv_eps: float = 1e-5
    gamma: float = GAMMA_SILU
    ch_div: int = 8
    num_classes: int = 1000


CONFIGS = {
    "nf_regnet_b1": NfRegCfg(),
    # build-defined miniature (the engine's "nf_regnet_tiny"): the ratio-1.0 first block, an identity-shortcut block,
    # a stage-0 stride-2 downsample 40 -> 40, group counts 5, 11, 11, 23, 27
    "nf_regnet_tiny": NfRegCfg(depths=(2, 1, 1, 1), channels=(48, 104, 128, 160), num_features=320, num_classes=24),
}


class NfRegBlock(nn.Module):
    def __init__(self, in_chs, out_chs, stride, alpha, beta, ratio, cfg, conv):
        super().__init__()
        mid = make_divisible(in_chs * ratio, cfg.ch_div)
        groups = mid // cfg.group_size
        mid = cfg.group_size * groups
        self.alpha, self.beta, self.attn_gain = alpha, beta, cfg.attn_gain
        self.downsample = (DownsampleAvg(in_chs, out_chs, stride, conv)
                           if in_chs != out_chs or stride != 1 else None)
        self.conv1 = conv(in_chs, mid, 1)
        self.conv2 = conv(mid, mid, 3, stride=stride, groups=groups)
        self.attn = SEModule(mid, cfg.se_rd_ratio, cfg.se_rd_divisor)
        self.conv3 = conv(mid, out_chs, 1, gain_init=0.)

    def mid_parts(self, x):
        """(c1, c2, gate, u, c3, x') of this block: what the engine stashes, for the layer-by-layer check."""
        a = F.silu(x) * self.beta
        shortcut = x if self.downsample is None else self.downsample(a)
        c1 = self.conv1(a)
        c2 = self.conv2(F.silu(c1))
        gate = self.attn.fc2(F.relu(self.attn.fc1(c2.mean((2, 3), keepdim=True)))).sigmoid()
        u = self.attn_gain * c2 * gate
        c3 = self.conv3(F.silu(u))
        return c1, c2, gate, u, c3, c3 * self.alpha + shortcut

    def forward(self, x):
        out = F.silu(x) * self.beta
        shortcut = x
        if self.downsample is not None:
            shortcut = self.downsample(out)
        out = self.conv1(out)
        out = self.conv2(F.silu(out))
        out = self.attn_gain * self.attn(out)
        out = self.conv3(F.silu(out))
        return out * self.alpha + shortcut


class NfRegNet(nn.Module):
    def __init__(self, cfg: NfRegCfg, in_chans=3):
        super().__init__()
        self.cfg = cfg

        def conv(i, o, k, stride=1, groups=1, gain_init=1.0):
            return ScaledStdConv2d(i, o, k, stride=stride, groups=groups, gamma=cfg.gamma,
                                   eps=cfg.std_conv_eps, gain_init=gain_init)

        stem_chs = make_divisible(cfg.channels[0] * cfg.width_factor, cfg.ch_div)
        self.stem = nn.Sequential(OrderedDict([("conv", conv(in_chans, stem_chs, 3, stride=2))]))
        prev, stages, expected_var = stem_chs, [], 1.0
        for si, depth in enumerate(cfg.depths):
            blocks = []
            for bi in range(depth):
                out_chs = make_divisible(cfg.channels[si] * cfg.width_factor, cfg.ch_div)
                ratio = cfg.first_ratio if si == 0 and bi == 0 else cfg.bottle_ratio
                # the '3x3' stem's stride is 2: every stage's first block strides
                blocks.append(NfRegBlock(prev, out_chs, 2 if bi == 0 else 1, cfg.alpha, 1. / expected_var ** 0.5,
                                         ratio, cfg, conv))
                if bi == 0:
                    expected_var = 1.
                expected_var += cfg.alpha ** 2
                prev = out_chs
            stages.append(nn.Sequential(*blocks))
        self.stages = nn.Sequential(*stages)
        feats = make_divisible(cfg.width_factor * cfg.num_features, cfg.ch_div)
        self.final_conv = conv(prev, feats, 1)
        self.num_features = feats
        self.head = ClassifierHead(feats, cfg.num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="linear")
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0., .01)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.stem(x)
        x = self.stages(x)
        return self.head(F.silu(self.final_conv(x)))


class ImageEncoder(nn.Module):
    """`.model` holds the network (parameter names gain the `model.` prefix, as in the reference's ImageEncoder);
    `.model.num_features` is the classifier's output width, the feature dimension the projection head sees."""

    def __init__(self, variant="nf_regnet_b1"):
        super().__init__()
        self.model = NfRegNet(CONFIGS[variant])
        self.model.num_features = self.model.cfg.num_classes

    def forward(self, x):
        return self.model(x)
