"""VGG16 (torchvision topology) on the HIP kernels, plus its transfer-learning variant.

Reference parity: ``models.vgg16(pretrained=True)``
(another_neural_net.py:244; printout pytorch_training_inference_on_image.ipynb:1991-2041): 13
conv3x3(pad 1)+bias+ReLU in 5 stages (64,64 | 128,128 | 256x3 | 512x3 | 512x3) each followed by
MaxPool2d(2,2); AdaptiveAvgPool2d(7,7) (the identity at 224x224 input, asserted); classifier
Linear(25088,4096)-ReLU-Dropout(0.5)-Linear(4096,4096)-ReLU-Dropout(0.5)-Linear(4096,1000).
Transfer learning (another_neural_net.py:247-255): backbone frozen, ``classifier[6]`` replaced by
``Linear(4096,256)-ReLU-Dropout(0.4)-Linear(256,10)-LogSoftmax``.

NHWC note: the flatten before the classifier is in (H, W, C) order; ``load_torchvision`` permutes
the first classifier weight from torchvision's (C, H, W) order accordingly.
"""
from __future__ import annotations

import torch
from torch import nn

from ..ops import _lib
from ..ops.conv_blocks import MxAct, conv_bias_act_mx, mx_conv_chainable, mx_conv_mode
from ..ops.functions import linear_mxfp8, mxfp8_infer
from ..ops.kernels import K
from .layers import Conv2d, Dropout, Linear, MaxPool2d, MLPHead
from .resnet import STEM_CIN_PAD

CFG16 = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]


class VGG(nn.Module):
    def __init__(self, cfg=CFG16, num_classes=1000, compute_dtype=None):
        super().__init__()
        layers, cin, first = [], 3, True
        for v in cfg:
            if v == "M":
                layers.append(MaxPool2d(2, 2))
            else:
                layers.append(Conv2d(cin, v, 3, 1, 1, bias=True, relu=True, cin_pad=STEM_CIN_PAD if first else None))
                cin, first = v, False
        self.features = nn.Sequential(*layers)
        self.classifier = nn.Sequential(
            Linear(512 * 7 * 7, 4096, relu=True), Dropout(0.5),
            Linear(4096, 4096, relu=True), Dropout(0.5),
            Linear(4096, num_classes))
        self.compute_dtype = compute_dtype

    def _cdtype(self, device):
        if self.compute_dtype is not None:
            return self.compute_dtype
        return _lib.default_compute_dtype(device)

    def prepare_input(self, x):
        dt = self._cdtype(x.device)
        if dt == torch.bfloat16:
            scale = 1.0 / 255.0 if x.dtype == torch.uint8 else 1.0
            h = K.nchw_to_nhwc(x.contiguous(), STEM_CIN_PAD, scale, None, None)
        else:   # fp32: the reference precision
            scale = 1.0 / 255.0 if x.dtype == torch.uint8 else 1.0
            h = K.nchw_to_nhwc_f32(x.contiguous(), STEM_CIN_PAD, scale)
        return h.to(dt)

    def _features_mx(self, h):
        """The features in the mxfp8 inference conv mode (``ops.conv_blocks.mx_conv_mode``), walked here: a conv
        the block-scaled kernel takes runs ``conv_mxfp8_fwd`` on the pair its predecessor's epilogue emitted, with
        the ``MaxPool2d(2, 2)`` behind it fused into that epilogue; inner convs emit the pair only.  Any other
        layer (layer 0, with its channel-padded input) runs as it is on bf16, and the one quantiser of the chain
        follows it.  The last conv emits the pair when ``classifier[0]`` takes a block-scaled matmul path (its
        ``[B, 7, 7, 512]`` NHWC flatten, 16 scale bytes a pixel, is that Linear's operand as it stands), else bf16.
        Returns an :class:`MxAct`."""
        mods = list(self.features)
        fc = self.classifier[0]

        def mx_ok(i):
            return i < len(mods) and isinstance(mods[i], Conv2d) and mx_conv_chainable(mods[i])

        h, i = MxAct(h), 0
        while i < len(mods):
            m = mods[i]
            if not mx_ok(i):
                h, i = MxAct(m(h.y)), i + 1
                continue
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            pool = isinstance(nxt, MaxPool2d) and (nxt.k, nxt.s, nxt.pad) == (2, 2, 0)
            j = i + 2 if pool else i + 1
            if j < len(mods):
                mx = mx_ok(j)
            else:   # the classifier's operand: whole scale dwords per pixel, so the pixels' scale rows concatenate
                k0 = 49 * m.weight.shape[0]
                mx = (isinstance(fc, Linear) and m.weight.shape[0] % 128 == 0 and fc.in_features == k0
                      and mxfp8_infer(torch.empty((0, k0), dtype=torch.bfloat16), fc.weight))
            h, i = conv_bias_act_mx(h, m, pool, not mx, mx), j
        return h

    def features_flat(self, x):
        """``[B, 25088]`` features in (H, W, C) order.  In the mxfp8 conv mode next to a block-scaled matmul mode:
        their ``(q [B, 25088], e [B, 784])`` pair, views of what the last conv emitted, for :meth:`_head`."""
        h = self.prepare_input(x)
        h = self._features_mx(h) if mx_conv_mode(h) else self.features(h)
        assert h.shape[1] == 7 and h.shape[2] == 7, "AdaptiveAvgPool2d(7,7) implemented for 224x224 input only"
        if isinstance(h, MxAct):
            if h.y is None:
                return h.q.view(h.shape[0], -1), h.e.view(h.shape[0], -1)
            h = h.y
        return h.reshape(h.shape[0], -1)

    def _head(self, f):
        """(classifier input, the classifier's remaining modules): a pair from :meth:`features_flat` goes to
        ``classifier[0]``'s kernel as an already quantised operand."""
        head = list(self.classifier)
        if isinstance(f, tuple):
            fc = head.pop(0)
            f = linear_mxfp8(f, fc.weight, fc.bias, 1 if fc.relu else 0)[:, : fc.out_features]
        return f, head

    def forward_logits(self, x):
        f, head = self._head(self.features_flat(x))
        for mod in head[:-1]:
            f = mod(f)
        return head[-1].forward_logits(f) if hasattr(head[-1], "forward_logits") else head[-1](f)

    def forward(self, x):
        f, head = self._head(self.features_flat(x))
        for mod in head:
            f = mod(f)
        return f

    def freeze_backbone(self):
        """another_neural_net.py:247-248 (all params frozen before the head is replaced)."""
        for p in self.parameters():
            p.requires_grad_(False)
        return self

    def replace_head(self, head: nn.Module):
        self.classifier[-1] = head
        return self

    @torch.no_grad()
    def load_torchvision(self, sd: dict, load_head: bool | None = None):
        convs = [m for m in self.features if isinstance(m, Conv2d)]
        keys = sorted({k.rsplit(".", 1)[0] for k in sd if k.startswith("features.")}, key=lambda s: int(s.split(".")[1]))
        for conv, k in zip(convs, keys):
            w = sd[k + ".weight"]
            conv.weight.zero_()
            conv.weight[..., : w.shape[1]].copy_(w.permute(0, 2, 3, 1))
            conv.bias.copy_(sd[k + ".bias"])
        w0 = sd["classifier.0.weight"].view(4096, 512, 7, 7).permute(0, 2, 3, 1).reshape(4096, -1)
        self.classifier[0].load_torch(w0, sd["classifier.0.bias"])
        self.classifier[2].load_torch(sd["classifier.3.weight"], sd["classifier.3.bias"])
        w6 = sd.get("classifier.6.weight")
        head = self.classifier[-1]
        if load_head is not False and isinstance(head, Linear) and w6 is not None and \
                tuple(w6.shape) == (head.out_features, head.in_features):
            head.load_torch(w6, sd["classifier.6.bias"])
        elif load_head:
            raise ValueError("load_torchvision: head weights missing or of another shape")
        for p in self.parameters():   # bf16 compute shadows of a flat arena follow the new masters
            owner = getattr(p, "_flat_owner", None)
            if owner is not None:
                owner.refresh_shadows()
                break
        return self


def vgg16(num_classes=1000, **kw):
    return VGG(CFG16, num_classes, **kw)


def vgg16_transfer(num_classes=10, hidden=256, p=0.4, **kw):
    """The reference's VGG16 TL model (another_neural_net.py:244-255)."""
    m = vgg16(1000, **kw).freeze_backbone()
    return m.replace_head(MLPHead(4096, hidden, num_classes, p))
