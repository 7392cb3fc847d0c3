"""Device-resident decoded image set with fused on-device batch assembly (PARITY B5).

``ImageFolder`` decodes every file again in every epoch.  ``DeviceImageCache`` decodes each file
once -- the first time its index is asked for -- resizes it on the device with the Pillow-exact
``resize_image`` to a square of ``cache_size`` and keeps it there as RGBx uint8 ``[N, Sc, Sc, 4]``.
Every later batch is one ``augment_batch`` launch (csrc/augment.hip; ``ops/ref.py`` on a CPU
device): gather by index (the shuffle), one inverse affine map per sample (the augmentation),
normalisation and layout.  ``BatchLoader`` drives it like any dataset (``get_batch``, ``set_epoch``).

``affine_params`` is the reference's ``image_transforms['train']`` (another_neural_net.py:224-231:
RandomResizedCrop(256, scale=(0.8, 1.0)), RandomRotation(15), ColorJitter() -- the identity at its
default arguments --, RandomHorizontalFlip, CenterCrop(224), ToTensor, Normalize) folded into one
map from output pixel to cache coordinates; ``eval_params`` is the centre crop of
``image_transforms['valid']``.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from .imagefolder import IMAGENET_MEAN, IMAGENET_STD


@dataclasses.dataclass(frozen=True)
class AugmentSpec:
    scale: tuple = (0.8, 1.0)          # RandomResizedCrop area fraction
    ratio: tuple = (3 / 4, 4 / 3)      # RandomResizedCrop aspect ratio (log-uniform)
    degrees: float = 15.0              # RandomRotation
    flip: float = 0.5                  # RandomHorizontalFlip probability
    out_size: int = 224                # CenterCrop
    resize: int = 256                  # side of the intermediate frame (RandomResizedCrop's size)
    mean: tuple = IMAGENET_MEAN        # Normalize (applied by the bf16 / fp32 output modes)
    std: tuple = IMAGENET_STD


# ------------------------------------------------------------------------------ stateless draws
def _mix64(z):
    """splitmix64's finaliser on a uint64 array (wrap-around arithmetic)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash_uniform(seed, epoch, indices, draw):
    """U[0, 1) float64 per index: a stateless 64-bit hash of (seed, epoch, dataset index, draw
    number), 53 bits wide.  No state, so a sample's draws depend on nothing but these four."""
    idx = np.asarray(indices, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = _mix64(np.full(idx.shape, int(seed) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        h = _mix64(h ^ (np.full(idx.shape, int(epoch) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03)))
        h = _mix64(h ^ (idx * np.uint64(0x8CB92BA72F3D8DD7)))
        h = _mix64(h ^ (np.full(idx.shape, int(draw), dtype=np.uint64) * np.uint64(0xAEF17502108EF2D9) + np.uint64(1)))
    return (h >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


# draw numbers
_AREA, _RATIO, _LEFT, _TOP, _ANGLE, _FLIP = range(6)


def crop_boxes(spec, seed, epoch, indices, cache_size):
    """(l, t, cw, ch, angle in degrees, flip) float64 / bool arrays of the samples' draws."""
    Sc = float(cache_size)
    u = [hash_uniform(seed, epoch, indices, d) for d in range(6)]
    area = (spec.scale[0] + (spec.scale[1] - spec.scale[0]) * u[_AREA]) * Sc * Sc
    lo, hi = np.log(spec.ratio[0]), np.log(spec.ratio[1])
    r = np.exp(lo + (hi - lo) * u[_RATIO])
    cw, ch = np.sqrt(area * r), np.sqrt(area / r)
    # a side longer than the image is clamped to it and the other side keeps the drawn area
    # (area <= Sc^2, so at most one side is too long)
    wide, tall = cw > Sc, ch > Sc
    cw = np.where(wide, Sc, np.where(tall, area / Sc, cw))
    ch = np.where(tall, Sc, np.where(wide, area / Sc, ch))
    l, t = u[_LEFT] * (Sc - cw), u[_TOP] * (Sc - ch)
    angle = (2.0 * u[_ANGLE] - 1.0) * float(spec.degrees)
    return l, t, cw, ch, angle, u[_FLIP] < spec.flip


def compose_params(l, t, cw, ch, angle, flip, resize, out_size):
    """float32 [B, 6] inverse affine maps (a, b, c, d, e, f) of ``augment_batch``, composed in
    float64 from output pixel to cache coordinates:
      1. add (resize - out_size)/2: the centre crop, into the intermediate ``resize`` frame;
      2. undo the flip: x -> resize - x;
      3. rotate by the angle about resize/2 (counter-clockwise image rotation, as PIL's ``rotate``);
      4. scale by cw/resize, ch/resize and translate by (l, t): the crop box."""
    l, t, cw, ch, angle = (np.asarray(v, dtype=np.float64) for v in (l, t, cw, ch, angle))
    flip = np.asarray(flip, dtype=bool)
    R, o = float(resize), (float(resize) - float(out_size)) / 2.0
    h = R / 2.0
    th = np.deg2rad(angle)
    cs, sn = np.cos(th), np.sin(th)
    s = np.where(flip, -1.0, 1.0)
    x2 = s * o + np.where(flip, R, 0.0) - h          # steps 1-2 applied to the origin, about the centre
    y2 = o - h
    sx, sy = cw / R, ch / R
    out = np.stack([sx * cs * s, -sx * sn + 0.0, l + sx * (cs * x2 - sn * y2 + h),
                    sy * sn * s + 0.0, sy * cs, t + sy * (sn * x2 + cs * y2 + h)], axis=-1)
    return np.ascontiguousarray(out.reshape(-1, 6), dtype=np.float32)


def affine_params(spec, seed, epoch, indices, cache_size):
    """float32 [B, 6]: the training augmentation of every dataset index in ``indices`` for
    ``(seed, epoch)``.  Pure and vectorised; the draws are ``hash_uniform`` of (seed, epoch, index,
    draw number), so a sample's augmentation depends on neither the batch it lands in nor the number
    of ranks.  The crop box is a float box in cache coordinates: area U(scale) * Sc^2, log-uniform
    aspect ratio, uniform offset; then ``compose_params``.

    Deviations from torchvision:
      * a box that does not fit is clamped to the image (the long side to Sc, the other side keeping
        the drawn area), not drawn again -- ``train_augment`` clamps too;
      * the crop is taken in the squashed square cache image, not in the original file;
      * the pipeline is a single resampling pass, so output pixels that fall outside the
        intermediate ``resize`` frame (the corners a rotation brings in) show image content, not
        black; only pixels outside the cached image are black."""
    l, t, cw, ch, angle, flip = crop_boxes(spec, seed, epoch, indices, cache_size)
    return compose_params(l, t, cw, ch, angle, flip, spec.resize, spec.out_size)


def eval_params(n, cache_size, out_size):
    """float32 [n, 6]: the exact centre crop, a = e = 1, c = f = (Sc - out)/2."""
    o = (float(cache_size) - float(out_size)) / 2.0
    return np.tile(np.array([1.0, 0.0, o, 0.0, 1.0, o], dtype=np.float32), (int(n), 1))


# ------------------------------------------------------------------------------ the cache
_OUT_MODES = {"u8": 0, "bf16": 1, "f32": 2}


def default_spec(out_size):
    """The reference's train transform at ``out_size``: 224 -> an intermediate frame of 256 (8/7)."""
    return AugmentSpec(out_size=int(out_size), resize=max(int(out_size), int(round(out_size * 8 / 7))))


def cached(folder, device, augment=False, cache_gb=8.0, seed=0, train=True):
    """The ``--cache-device`` / ``--augment`` dataset of an entry point's loader: uint8 NCHW batches
    of ``folder.size`` (the models' input conversion scales them, as for the uncached loaders)."""
    return DeviceImageCache(folder, device if device is not None else "cpu",
                            augment=default_spec(folder.size) if augment else None,
                            seed=seed or 0, budget_gb=cache_gb, train=train)


def cache_stats(*loaders):
    """``data_cache`` of an entry point's JSON record: {images, bytes, decodes, augment} summed over
    the distinct caches behind ``loaders``; None when none of them is cached."""
    seen, tot = set(), None
    for ld in loaders:
        ds = getattr(ld, "ds", ld)
        if not isinstance(ds, DeviceImageCache) or id(ds._s) in seen:
            continue
        seen.add(id(ds._s))
        s = ds.stats()
        if tot is None:
            tot = s
        else:
            tot = {"images": tot["images"] + s["images"], "bytes": tot["bytes"] + s["bytes"],
                   "decodes": tot["decodes"] + s["decodes"], "augment": tot["augment"] or s["augment"]}
    return tot


class DeviceImageCache:
    """``folder``'s images, decoded once and resident on ``device`` (per process: under DDP each rank
    fills what its sampler hands it).

    Without ``augment`` the cache holds the images at ``cache_size`` (default: the folder's size) and
    a batch is uint8 NCHW, bitwise what ``ImageFolder.get_batch(idx, device, device_resize=True)``
    returns.  With ``augment`` (an :class:`AugmentSpec`) the cache side defaults to ``spec.resize``,
    training batches take ``affine_params`` and ``train=False`` the centre crop ``eval_params``, both
    ``spec.out_size`` wide.  ``out`` selects the kernel's output: ``"u8"`` uint8 NCHW (what the
    loaders yield and the models' input conversion takes), ``"bf16"`` / ``"f32"`` the normalised
    NHWC model input ``[B, O, O, cpad]`` with the spec's mean / std.

    The draws are those of ``(seed, epoch, index)``.  ``set_epoch`` names the epoch; a loader pass
    that nobody announced takes the next one (``begin_pass``), so every training loop sees a new
    augmentation per epoch whether or not it calls ``set_epoch``.

    ``view(train=False)`` shares the storage (one decode serves the train and the test loader)."""

    def __init__(self, folder, device, cache_size=None, augment=None, seed=0, budget_gb=8.0, train=True, out="u8",
                 cpad=8):
        self.folder, self.device = folder, torch.device(device)
        self.augment, self.seed, self.train, self.out, self.cpad = augment, int(seed), bool(train), out, int(cpad)
        if out not in _OUT_MODES:
            raise ValueError(f"out must be one of {sorted(_OUT_MODES)}")
        if cache_size is None:
            cache_size = augment.resize if augment is not None else folder.size
        self.cache_size = int(cache_size)
        self.out_size = int(augment.out_size) if augment is not None else self.cache_size
        if self.out_size > self.cache_size:
            raise ValueError(f"out_size {self.out_size} exceeds cache_size {self.cache_size}")
        n = len(folder)
        self.nbytes = n * self.cache_size * self.cache_size * 4
        if self.nbytes > float(budget_gb) * 1e9:
            raise ValueError(f"image cache needs {self.nbytes} bytes ({n} images of {self.cache_size}x"
                             f"{self.cache_size}x4), above the budget of {budget_gb} GB")
        self.epoch, self._epoch_given = 0, True        # the first pass is epoch 0 (see begin_pass)
        self.classes = folder.classes
        # shared between views: storage, fill state, counters
        self._s = {
            "cache": torch.empty((n, self.cache_size, self.cache_size, 4), dtype=torch.uint8, device=self.device),
            "labels": torch.tensor([y for _, y in folder.samples], dtype=torch.long).to(self.device),
            "filled": np.zeros(n, dtype=bool),
            "decodes": 0,
        }
        self._norm = None

    # ---- shared state ------------------------------------------------------------------------
    cache = property(lambda self: self._s["cache"])
    filled = property(lambda self: self._s["filled"])
    decodes = property(lambda self: self._s["decodes"])

    def view(self, train=None, out=None):
        """A second handle on the same storage with its own ``train`` / ``out`` / epoch."""
        import copy
        if out is not None and out not in _OUT_MODES:
            raise ValueError(f"out must be one of {sorted(_OUT_MODES)}")
        v = copy.copy(self)
        v.train = self.train if train is None else bool(train)
        v.out = self.out if out is None else out
        return v

    def __len__(self):
        return len(self.folder)

    def set_epoch(self, e):
        """The epoch of the next pass (and of direct ``get_batch`` calls)."""
        self.epoch = int(e)
        self._epoch_given = True

    def begin_pass(self):
        """Called by ``BatchLoader`` when it starts a pass over the data.  A pass that no
        ``set_epoch`` announced takes the epoch after the last one, so loops that never call
        ``set_epoch`` (``keras_fit``, ``--reference-compat``) still draw a new augmentation per epoch."""
        if not self._epoch_given:
            self.epoch += 1
        self._epoch_given = False

    def stats(self):
        return {"images": len(self), "bytes": int(self.nbytes), "decodes": int(self.decodes),
                "augment": self.augment is not None}

    # ---- fill --------------------------------------------------------------------------------
    def _fill(self, missing):
        from ..ops.kernels import K
        from .imagefolder import resize_on_device
        S, cuda = self.cache_size, self.device.type == "cuda"
        items = list(self.folder.pool.map(lambda i: self.folder.load_raw(i), [int(i) for i in missing]))
        if cuda:
            x = torch.cat([resize_on_device(t, S, self.device) for t, _ in items])
        else:
            x = torch.cat([K.resize_image(t.unsqueeze(0).contiguous(), S, S, 0, 8, 1.0, None, None) for t, _ in items])
        rgbx = torch.zeros((len(items), S, S, 4), dtype=torch.uint8, device=self.device)
        rgbx[..., :3] = x.permute(0, 2, 3, 1)
        self.cache.index_copy_(0, self._upload(torch.from_numpy(np.asarray(missing, dtype=np.int64))), rgbx)
        self.filled[missing] = True
        self._s["decodes"] += len(items)

    def _upload(self, t):
        if self.device.type != "cuda":
            return t
        return t.pin_memory().to(self.device, non_blocking=True)

    @staticmethod
    def _check_idx(idx, n):
        if isinstance(idx, torch.Tensor):
            idx = idx.detach().cpu().numpy()
        a = np.asarray(idx)
        if a.size == 0:
            a = a.astype(np.int64)
        if a.dtype.kind not in "iu" or a.ndim != 1:
            raise IndexError(f"image indices must be a 1-D sequence of integers, got dtype {a.dtype} shape {a.shape}")
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= n):
            raise IndexError(f"image index out of range [0, {n}): {int(a.min())}..{int(a.max())}")
        return a

    # ---- batches -----------------------------------------------------------------------------
    def get_batch(self, idx, device=None):
        from ..ops.kernels import K
        if device is not None and torch.device(device).type != self.device.type:
            raise ValueError(f"the cache lives on {self.device}, a batch was asked for on {device}")
        a = self._check_idx(idx, len(self))           # on the host, before anything is uploaded
        missing = np.unique(a[~self.filled[a]])
        if missing.size:
            self._fill(missing)
        if self.augment is not None and self.train:
            p = affine_params(self.augment, self.seed, self.epoch, a, self.cache_size)
        else:
            p = eval_params(a.size, self.cache_size, self.out_size)
        idx_d = self._upload(torch.from_numpy(a))
        p_d = self._upload(torch.from_numpy(p))
        mode = _OUT_MODES[self.out]
        mean = stdv = None
        if mode and self.augment is not None:
            if self._norm is None:
                self._norm = (torch.tensor(self.augment.mean, dtype=torch.float32, device=self.device),
                              torch.tensor(self.augment.std, dtype=torch.float32, device=self.device))
            mean, stdv = self._norm
        x = K.augment_batch(self.cache, idx_d, p_d, self.out_size, mode, self.cpad, 1.0 / 255.0 if mode else 1.0,
                            mean, stdv)
        return x, self._s["labels"].index_select(0, idx_d)
