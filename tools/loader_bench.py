"""Image-loader epochs with no model: what the input side alone delivers, in img/s.

Writes a folder of JPEGs with PIL into a temporary directory (2,048 files of 500x375, smooth content
plus noise, 10 classes) and times whole loader epochs at each batch size:
  (a) ``ImageFolder`` + ``BatchLoader``: decode every epoch, resize on the device;
  (b) ``DeviceImageCache`` epoch 1: the fill (decode once, resize, store);
  (c) ``DeviceImageCache`` epoch 2: one ``augment_batch`` launch per batch;
  (d) epoch 2 of an augmenting cache (256-pixel cache, B5 augmentation, 224 out).
One process; device events around each epoch, a synchronise at its end.  Also the device time of
one ``augment_batch`` launch of (d) at the largest batch size (events around 50 back-to-back
launches) with the bytes it moves, computed from the shapes.  One JSON line per measurement, on
stdout and in ``--out``.  Needs a GPU: there is no CPU fall-back.

Usage: python tools/loader_bench.py [--n 2048] [--batch-sizes 64,256] [--out profiles/loader_bench.jsonl]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pcmp  # noqa: E402,F401
from pcmp.data import device_cache as DC  # noqa: E402
from pcmp.data.imagefolder import ImageFolder  # noqa: E402
from pcmp.data.synthetic import BatchLoader  # noqa: E402


def write_jpegs(root, n, w=500, h=375, classes=10, seed=0):
    import concurrent.futures as cf

    from PIL import Image
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    for c in range(classes):
        os.makedirs(os.path.join(root, f"class_{c}"), exist_ok=True)

    def one(i):
        rng = np.random.RandomState(seed * 1000003 + i)
        fx, fy, ph = rng.uniform(0.01, 0.06), rng.uniform(0.01, 0.06), rng.uniform(0, 6.28, 3)
        img = np.stack([127 + 100 * np.sin(fx * xx + ph[0]) * np.cos(fy * yy), 127 + 100 * np.sin(fy * yy + ph[1]),
                        127 + 100 * np.cos(fx * xx + fy * yy + ph[2])], -1)
        img = np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, f"class_{i % classes}", f"img_{i:05d}.JPEG"), quality=90)

    with cf.ThreadPoolExecutor(16) as ex:
        list(ex.map(one, range(n)))


def epoch(loader, e):
    """(images, seconds by device events, seconds by the host clock) of one whole epoch."""
    loader.set_epoch(e)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    n = 0
    for x, y in loader:
        n += x.shape[0]
    end.record()
    torch.cuda.synchronize()
    return n, start.elapsed_time(end) * 1e-3, time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--batch-sizes", default="64,256")
    ap.add_argument("--dir", default=None, help="keep / reuse the JPEG folder here instead of a temporary one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "loader_bench needs a GPU"
    dev = torch.device("cuda", 0)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        root = args.dir or tmp
        if not os.path.isdir(os.path.join(root, "class_0")):
            t0 = time.perf_counter()
            write_jpegs(root, args.n)
            emit(step="write_jpegs", files=args.n, seconds=time.perf_counter() - t0)
        sizes = [int(b) for b in args.batch_sizes.split(",")]
        for B in sizes:
            folder = ImageFolder(root, size=224)

            def run(name, ds, e):
                n, dt, wall = epoch(BatchLoader(ds, B, device=dev, shuffle=True, seed=1), e)
                kw = {"decodes": ds.decodes} if hasattr(ds, "decodes") else {}     # decodes so far
                emit(step=name, batch=B, images=n, seconds=dt, host_seconds=wall, img_s=n / dt, **kw)

            run("a_imagefolder_epoch1", folder, 0)            # also warms the decode pool and resize_image
            run("a_imagefolder_epoch2", folder, 1)
            cache = DC.DeviceImageCache(folder, dev)
            run("b_cache_fill", cache, 0)
            run("c_cache_epoch2", cache, 1)
            run("c_cache_epoch3", cache, 2)
            aug = DC.DeviceImageCache(folder, dev, augment=DC.AugmentSpec(), seed=1)
            run("b_augment_cache_fill", aug, 0)
            run("d_augment_epoch2", aug, 1)
            run("d_augment_epoch3", aug, 2)
            if B == max(sizes):
                # the kernel alone: device time of one launch of (d), 50 back to back
                spec = aug.augment
                idx = np.arange(B) % len(aug)
                p = torch.from_numpy(DC.affine_params(spec, 1, 1, idx, aug.cache_size)).to(dev)
                i = torch.from_numpy(idx.astype(np.int64)).to(dev)
                op = torch.ops.pcmp.augment_batch
                mean, std = (torch.tensor(v, device=dev) for v in (spec.mean, spec.std))
                _, _, cw, ch, _, _ = DC.crop_boxes(spec, 1, 1, idx, aug.cache_size)
                for mode, name, osz in ((0, "u8", 3), (1, "bf16", 16)):
                    a = (aug.cache, i, p, spec.out_size, mode, 8, 1.0 / 255.0 if mode else 1.0) + ((mean, std) if mode else (None, None))
                    for _ in range(5):
                        op(*a)
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(50):
                        op(*a)
                    e.record()
                    torch.cuda.synchronize()
                    us = s.elapsed_time(e) * 1e3 / 50
                    # bytes the algorithm needs: every cache pixel under the (centre-cropped) box once,
                    # 4 bytes each, plus the output
                    frac = (spec.out_size / spec.resize) ** 2
                    rd = float((cw * ch).sum()) * frac * 4
                    wr = B * spec.out_size * spec.out_size * osz
                    emit(step="kernel_d", out=name, batch=B, us_per_launch=us, read_bytes=rd, write_bytes=wr,
                         gb_s=(rd + wr) / us * 1e-3, img_s=B / us * 1e6)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
