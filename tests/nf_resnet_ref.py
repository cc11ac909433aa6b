"""TEST INFRASTRUCTURE ONLY -- CPU fp32 restatement of the NF-ResNet image encoder (`--image_encoder nf_resnet50`).

The reference builds it as ``timm.create_model('nf_resnet50', pretrained=True)`` (networks.py:669-670) and keeps
timm's classifier (no ``num_classes=0``), so its image features are the 1000 logits (networks.py:818-819).  timm
(0.6.7) is not installed here, so this restates timm's ``NormFreeNet`` with
``_nfres_cfg(depths=(3, 4, 6, 3), channels=(256, 512, 1024, 2048), act_layer='relu', attn_layer=None)``:
stem '7x7_pool' (ScaledStdConv2d 3->64, 7x7 / 2, then MaxPool2d(3, 2, padding=1), no activation), bottleneck
blocks ``x' = alpha * conv3(relu(conv2(relu(conv1(a))))) + shortcut`` with ``a = relu(x) * beta`` and the
``DownsampleAvg`` shortcut on the first block of a stage, no squeeze-excite, no conv2b, no final conv,
``final_act = ReLU``, global average pool, ``head.fc = Linear(2048, 1000)``.

PARITY UNPINNED, as for the NFNet restatement (oracle/nfnet_ref.py): the reference holds no test, golden vector or
known answer at this boundary and timm is absent.  The only checks are structural anchors: 53 convolutions,
25,557,032 parameters (timm's published 25.56 M), 1000 features, timm's parameter registration order
(stem.conv, then per block downsample.conv (first block of a stage), conv1, conv2, conv3, then head.fc).

``ScaledStdConv2d``, ``DownsampleAvg`` and ``randomize_like_trained`` come from oracle/nfnet_ref.py unchanged.
"""
from collections import OrderedDict
from dataclasses import dataclass
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.nfnet_ref import DownsampleAvg, ScaledStdConv2d, make_divisible, randomize_like_trained  # noqa: F401

GAMMA_RELU = 1.7139588594436646  # timm _nonlin_gamma['relu']


@dataclass
class NfResCfg:
    depths: Tuple[int, ...] = (3, 4, 6, 3)
    channels: Tuple[int, ...] = (256, 512, 1024, 2048)
    stem_chs: int = 64
    bottle_ratio: float = 0.25
    alpha: float = 0.2
    std_conv_eps: float = 1e-5
    gamma: float = GAMMA_RELU
    ch_div: int = 8
    num_classes: int = 1000


CONFIGS = {
    "nf_resnet50": NfResCfg(),
    # build-defined miniature (the engine's "nf_resnet_tiny"): stage 0 is 256 wide, so its conv2 is 64 -> 64, and has two
    # blocks, the second with the identity shortcut
    "nf_resnet_tiny": NfResCfg(depths=(2, 1, 1, 1), channels=(256, 128, 192, 256), stem_chs=16, num_classes=24),
}


class NfResBlock(nn.Module):
    def __init__(self, in_chs, out_chs, stride, alpha, beta, cfg, conv):
        super().__init__()
        mid = make_divisible(out_chs * cfg.bottle_ratio, cfg.ch_div)
        self.alpha, self.beta = alpha, beta
        self.downsample = (DownsampleAvg(in_chs, out_chs, stride, conv)
                           if in_chs != out_chs or stride != 1 else None)
        self.conv1 = conv(in_chs, mid, 1)
        self.conv2 = conv(mid, mid, 3, stride=stride)
        self.conv3 = conv(mid, out_chs, 1, gain_init=0.)

    def forward(self, x):
        out = F.relu(x) * self.beta
        shortcut = x
        if self.downsample is not None:
            shortcut = self.downsample(out)
        out = self.conv1(out)
        out = self.conv2(F.relu(out))
        out = self.conv3(F.relu(out))
        return out * self.alpha + shortcut


class ClassifierHead(nn.Module):
    def __init__(self, chs, classes):
        super().__init__()
        self.fc = nn.Linear(chs, classes)

    def forward(self, x):
        return self.fc(x.mean((2, 3)))


class NfResNet(nn.Module):
    def __init__(self, cfg: NfResCfg, in_chans=3):
        super().__init__()
        self.cfg = cfg

        def conv(i, o, k, stride=1, groups=1, gain_init=1.0):
            return ScaledStdConv2d(i, o, k, stride=stride, groups=groups, gamma=cfg.gamma,
                                   eps=cfg.std_conv_eps, gain_init=gain_init)

        self.stem = nn.Sequential(OrderedDict([("conv", conv(in_chans, cfg.stem_chs, 7, stride=2)),
                                               ("pool", nn.MaxPool2d(3, stride=2, padding=1))]))
        prev, stages, expected_var = cfg.stem_chs, [], 1.0
        for si, depth in enumerate(cfg.depths):
            stride = 1 if si == 0 else 2   # the 7x7_pool stem's stride is 4
            blocks = []
            for bi in range(depth):
                out_chs = make_divisible(cfg.channels[si], cfg.ch_div)
                blocks.append(NfResBlock(prev, out_chs, stride if bi == 0 else 1, cfg.alpha,
                                         1. / expected_var ** 0.5, cfg, conv))
                if bi == 0:
                    expected_var = 1.
                expected_var += cfg.alpha ** 2
                prev = out_chs
            stages.append(nn.Sequential(*blocks))
        self.stages = nn.Sequential(*stages)
        self.num_features = prev
        self.head = ClassifierHead(prev, cfg.num_classes)
        for name, m in self.named_modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="linear")
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0., .01)
                nn.init.zeros_(m.bias)

    def stem_out(self, x):
        return self.stem.conv(x)

    def forward(self, x):
        x = self.stem(x)
        x = self.stages(x)
        return self.head(F.relu(x))


class ImageEncoder(nn.Module):
    """`.model` holds the network (parameter names gain the `model.` prefix, as in the reference's ImageEncoder);
    `.model.num_features` is the classifier's output width, the feature dimension the projection head sees."""

    def __init__(self, variant="nf_resnet50"):
        super().__init__()
        self.model = NfResNet(CONFIGS[variant])
        self.model.num_features = self.model.cfg.num_classes

    def forward(self, x):
        return self.model(x)
