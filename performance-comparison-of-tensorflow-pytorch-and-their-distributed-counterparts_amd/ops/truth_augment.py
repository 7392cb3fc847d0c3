"""fp64 truth of ``augment_batch`` (csrc/augment.hip) and the cases its tests share.

``gather`` is the sampling rule written out: a direct fp64 gather of the four bilinear taps, zero
outside the image, on the values the fp32 ``params`` hold.  ``grid_sample_form`` is the same rule as
``F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False)`` under the matching
affine grid; it is used only to cross-check ``gather``.  Neither shares code with ``ops/ref.py``.

The cases (tests/test_augment_cpu.py measures the floors of ``ops/ref.py`` over them,
tests/test_augment_gpu.py holds the kernel to the bounds): N = 5 random images of side 40 with a
garbage fourth byte, B = 7 samples ``IDX`` (repeats, any order), output sides 24 and 33, one
inverse affine map per case applied to every sample, and ``mixed`` with a different map per sample.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ..data.device_cache import compose_params
from ..data.imagefolder import IMAGENET_MEAN, IMAGENET_STD

N_IMAGES, SC, CPAD, SCALE = 5, 40, 8, 1.0 / 255.0
IDX = (4, 0, 4, 2, 1, 3, 0)
OUT_SIZES = (24, 33)

# maps whose taps all carry weight 0 or 1 on whole cache pixels: the result is a slice / flip /
# quarter turn of the cache (zero where it leaves the image), bit for bit
EXACT = {
    "crop": (1.0, 0.0, 8.0, 0.0, 1.0, 8.0),
    "flip": (-1.0, 0.0, 32.0, 0.0, 1.0, 8.0),
    "quarter_turn": (0.0, -1.0, 32.0, 1.0, 0.0, 8.0),
    "half_outside": (1.0, 0.0, -12.0, 0.0, 1.0, 5.0),
    "outside": (1.0, 0.0, 100.0, 0.0, 1.0, -90.0),
}


def _box(out_size, angle, flip, area=0.8, ratio=1.0, fx=0.5, fy=0.5):
    """The map of a crop box of ``area`` * SC^2 at offset fraction (fx, fy), rotated and flipped,
    through an intermediate frame four pixels wider than the output."""
    cw, ch = math.sqrt(area * ratio) * SC, math.sqrt(area / ratio) * SC
    row = compose_params([fx * (SC - cw)], [fy * (SC - ch)], [cw], [ch], [angle], [flip], out_size + 4, out_size)
    return tuple(float(v) for v in row[0])


def fractional(out_size):
    return {
        "rot_p15": _box(out_size, 15.0, False),                  # minimum-area box
        "rot_m15_flip": _box(out_size, -15.0, True, ratio=4 / 3, fx=0.25, fy=0.8),
        "rot_7p3_flip": _box(out_size, 7.3, True, area=0.93, ratio=0.8, fx=1.0, fy=0.0),
        "quarter_pixel": (1.0, 0.0, 8.25, 0.0, 1.0, 8.25),
    }


def cases(out_size):
    """{name: fp32 params [7, 6]}."""
    rows = dict(EXACT)
    rows.update(fractional(out_size))
    out = {k: torch.tensor([v] * len(IDX), dtype=torch.float32) for k, v in rows.items()}
    names = ["crop", "rot_p15", "flip", "rot_m15_flip", "half_outside", "rot_7p3_flip", "quarter_pixel"]
    out["mixed"] = torch.tensor([rows[k] for k in names], dtype=torch.float32)
    return out


def make_cache(seed=0, n=N_IMAGES, sc=SC):
    g = torch.Generator().manual_seed(1234 + seed)
    return torch.randint(0, 256, (n, sc, sc, 4), dtype=torch.uint8, generator=g)


def idx_tensor():
    return torch.tensor(IDX, dtype=torch.long)


def mean_std():
    return torch.tensor(IMAGENET_MEAN, dtype=torch.float32), torch.tensor(IMAGENET_STD, dtype=torch.float32)


# ------------------------------------------------------------------------------ truths
def _coords(params, out_size):
    q = params.double().view(-1, 6, 1, 1)
    px = (torch.arange(out_size, dtype=torch.float64) + 0.5).view(1, 1, -1)
    py = px.view(1, -1, 1)
    return q[:, 0] * px + q[:, 1] * py + q[:, 2], q[:, 3] * px + q[:, 4] * py + q[:, 5]


def gather(cache, idx, params, out_size):
    """Unrounded sample values, fp64 [B, O, O, 3]."""
    cache, idx, params = cache.cpu(), idx.cpu(), params.cpu()
    B, Sc, O = idx.numel(), cache.shape[1], int(out_size)
    u, v = _coords(params, O)
    x0, y0 = torch.floor(u - 0.5), torch.floor(v - 0.5)
    wx, wy = (u - 0.5) - x0, (v - 0.5) - y0
    img = cache[idx][..., :3].double()                       # [B, Sc, Sc, 3]
    bi = torch.arange(B).view(B, 1, 1).expand(B, O, O)
    out = torch.zeros(B, O, O, 3, dtype=torch.float64)
    for dy, dx, w in ((0, 0, (1 - wx) * (1 - wy)), (0, 1, wx * (1 - wy)), (1, 0, (1 - wx) * wy), (1, 1, wx * wy)):
        xi, yi = (x0 + dx), (y0 + dy)
        inside = (xi >= 0) & (xi < Sc) & (yi >= 0) & (yi < Sc)
        xs, ys = xi.clamp(0, Sc - 1).long(), yi.clamp(0, Sc - 1).long()
        out += torch.where(inside, w, torch.zeros_like(w)).unsqueeze(-1) * img[bi, ys, xs]
    return out


def grid_sample_form(cache, idx, params, out_size):
    """The same values through ``F.grid_sample`` in fp64 (cross-check of ``gather`` only)."""
    cache, idx, params = cache.cpu(), idx.cpu(), params.cpu()
    Sc = cache.shape[1]
    u, v = _coords(params, int(out_size))
    grid = torch.stack([2.0 * u / Sc - 1.0, 2.0 * v / Sc - 1.0], dim=-1)      # pixel i covers [i, i + 1)
    img = cache[idx][..., :3].double().permute(0, 3, 1, 2)
    y = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return y.permute(0, 2, 3, 1).contiguous()


def normalised(val, scale, mean=None, stdv=None, cpad=CPAD):
    """The truth of modes 1 / 2: fp64 [B, O, O, cpad] of (val*scale - mean) / std, pad channels 0."""
    a = val * float(scale)
    if mean is not None:
        a = (a - mean[:3].double().cpu()) / stdv[:3].double().cpu()
    return F.pad(a, (0, cpad - 3))


def exact_expected(cache, idx, row, out_size):
    """uint8 [B, 3, O, O] of an EXACT map by integer indexing of the zero-padded cache (no arithmetic
    on pixel values): source pixel (a*x + b*y + c', d*x + e*y + f') with c' = (a + b)/2 + c - 1/2."""
    a, b, c, d, e, f = row
    O, Sc, P = int(out_size), cache.shape[1], 128
    x = torch.arange(O).view(1, O)
    y = torch.arange(O).view(O, 1)
    xs = (a * x + b * y + ((a + b) / 2 + c - 0.5)).long().clamp(-P, Sc - 1 + P) + P
    ys = (d * x + e * y + ((d + e) / 2 + f - 0.5)).long().clamp(-P, Sc - 1 + P) + P
    padded = F.pad(cache.cpu()[..., :3].permute(0, 3, 1, 2), (P, P, P, P))      # [N, 3, Sc+2P, Sc+2P]
    return padded[idx.cpu()][:, :, ys, xs].contiguous()


def seg_pixels(x):
    """One segment per image and channel of an NHWC tensor: the spatial dimensions."""
    return x, (1, 2)
