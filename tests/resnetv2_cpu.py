"""CPU restatement of the deep-stem ResNet (`resnet50v2` / `resnet101v2`) and of PSPNet-POP on it, in plain torch.nn.

The deep stem is conv 3x3 s2 (3 -> 64), BN, ReLU, conv 3x3 (64 -> 64), BN, ReLU, conv 3x3 (64 -> 128), BN, ReLU, maxpool 3x3 s2 p1, and layer1 starts
from 128 channels.  Bottlenecks, pyramid, head and loss are the CPU oracle's (oracle/pop_oracle.py), by import.  tests/golden/make_golden_v2.py checks this
module bit for bit against the reference before it writes a golden record; the GPU tests use it as the same-machine comparison.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import pop_oracle as po


class DeepStemResNet(nn.Module):
    """Parameters under the names conv1/bn1/conv2/bn2/conv3/bn3/layer1..4; forward(img NCHW) -> x4 NCHW (or [x4, x3, x2, x1])."""

    def __init__(self, layers, dilated=True, os=8, multi_grid=False, relu_l3=True, relu_l4=True):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.conv2 = nn.Conv2d(64, 64, 3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(64)
        self.conv3 = nn.Conv2d(64, 128, 3, stride=1, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(128)
        inplanes = [128]

        def stage(planes, n, stride=1, dilation=1, grid=1, last_relu=True):
            mg = (lambda i: grid[i % len(grid)]) if isinstance(grid, tuple) else (lambda i: 1)
            blocks = [po.make_bottleneck(inplanes[0], planes, stride, dilation * mg(0), stride != 1 or inplanes[0] != planes * 4)]
            inplanes[0] = planes * 4
            for i in range(1, n):
                blocks.append(po.make_bottleneck(inplanes[0], planes, 1, dilation * mg(i), False, last_relu=True if i != n - 1 else last_relu))
            return nn.Sequential(*blocks)

        grid = (1, 2, 4) if multi_grid else (1, 1, 1)
        self.layer1 = stage(64, layers[0])
        self.layer2 = stage(128, layers[1], stride=2)
        if dilated and os == 8:
            self.layer3 = stage(256, layers[2], stride=1, dilation=2, last_relu=relu_l3)
            self.layer4 = stage(512, layers[3], stride=1, dilation=4, grid=grid, last_relu=relu_l4)
        elif dilated:
            self.layer3 = stage(256, layers[2], stride=2, last_relu=relu_l3)
            self.layer4 = stage(512, layers[3], stride=1, dilation=2, grid=grid, last_relu=relu_l4)
        else:
            self.layer3 = stage(256, layers[2], stride=2, last_relu=relu_l3)
            self.layer4 = stage(512, layers[3], stride=2, last_relu=relu_l4)

    def stem(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x = F.relu(self.bn3(self.conv3(x)))
        return F.max_pool2d(x, kernel_size=3, stride=2, padding=1)

    def forward(self, x, return_list=False):
        x = self.stem(x)
        outs = []
        for st in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in st:
                x = po.bottleneck_forward(blk, x)
            outs.append(x)
        return outs[::-1] if return_list else x


LAYERS = {'resnet50v2': (3, 4, 6, 3), 'resnet101v2': (3, 4, 23, 3)}


class PopV2(po.PopOracle):
    """PSPNet-POP on the deep-stem backbone: the oracle's parameter tree, pyramid, head and loss around DeepStemResNet."""

    def __init__(self, n_base, criterion=None, is_ft=False, n_novel=0, backbone='resnet50v2', **kw):
        bkw = {k: kw.pop(k) for k in ('dilated', 'os', 'multi_grid', 'relu_l3', 'relu_l4') if k in kw}
        super().__init__(n_base, criterion=criterion, is_ft=is_ft, n_novel=n_novel, _custom_backbone=DeepStemResNet(LAYERS[backbone], **bkw), **kw)

    def features(self, img):
        return po.ppm_forward(self.decoder, self.backbone(img))

    def forward(self, img, mask=None, img_b=None, mask_b=None):
        if not self.is_ft:
            preds = po.head_base(self, self.features(img))
            if self.criterion is not None and mask is not None:
                e = F.normalize(self.base_emb.unsqueeze(0), p=2, dim=-1).squeeze(0)
                return self.criterion(preds, mask, proto_sim=torch.matmul(e, e.t()))
            return preds
        if not self.training:
            return po.head_all(self, self.features(img))[0]
        full = torch.cat([img, img_b], dim=0)
        preds, preds2 = po.head_all(self, self.features(full))
        B = full.shape[0]
        mask_new = torch.stack([po.pseudo_label(preds2[B // 2 + b], mask_b[b], self.n_base) for b in range(B // 2)], dim=0)
        if self.criterion is not None and mask is not None:
            ne = F.normalize(self.novel_emb.float(), p=2, dim=-1)
            sim = torch.matmul(ne, torch.cat([ne, F.normalize(self.base_emb.float(), p=2, dim=-1)], dim=0).t())
            return self.criterion(preds.float(), torch.cat([mask, mask_new], dim=0), is_ft=True, proto_sim=sim)
        return preds
