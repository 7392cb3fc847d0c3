"""``augment_batch`` on the CPU: the fp64 truth against ``F.grid_sample``, the distance of
``ops/ref.py:augment_batch`` (fp32) from it -- the *floor* --, the bounds tests/test_augment_gpu.py
holds the kernel to, ``affine_params``, ``DeviceImageCache`` on a CPU device and the entry point.

Floors, measured over every case of ``pcmp.ops.truth_augment`` (both output sides, with and without
mean / std), and the bounds that follow from them by the rule of tests/test_text_truth_cpu.py:
  * fp32 mode: ``seg_rel`` per image and channel; bound 1e-5, the floor is at most half of it;
  * bf16 mode: ``norm_err`` per image and channel with 2*floor <= k <= max(1, 4*floor);
  * uint8 mode: |out - unrounded truth| <= 0.5 + m for every element, m between 2x and 4x the fp32
    floor in LSB (the largest |val_fp32 - val_truth| on the 0..255 scale).
``test_reference_floors`` recomputes the floors and enforces the rule; no element is exempt.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pcmp  # noqa: F401
from pcmp.data import device_cache as DC
from pcmp.data.imagefolder import ImageFolder
from pcmp.ops import ref, truth as T, truth_augment as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# recorded floors of ops/ref.py and the bounds of the GPU test
FLOOR_LSB = 9.1e-4         # fp32: worst |val - truth| in LSB of the 0..255 scale (15 degrees, 40 -> 33)
FLOOR_F32 = 2.2e-6         # fp32 mode: worst seg_rel per image and channel (with mean / std; 8.3e-7 without)
FLOOR_BF16 = 0.252         # bf16 mode: worst norm_err
BOUND_F32 = 1e-5
K_BF16 = 1.0
M_U8 = 2.5e-3              # uint8 mode: |out - unrounded truth| <= 0.5 + M_U8


def all_cases():
    """(out_size, name, params) of every case."""
    for O in A.OUT_SIZES:
        for name, p in A.cases(O).items():
            yield O, name, p


def norm_variants():
    return ((None, None), A.mean_std())


def check_outputs(fn, cache, idx, O, params, truth_val, dev="cpu"):
    """Every mode of ``fn`` (ops/ref.py or torch.ops.pcmp) on one case against the truth, element by
    element; returns the worst (LSB error of mode 0 beyond 0.5, seg_rel of mode 2, norm_err of mode 1)."""
    worst = [0.0, 0.0, 0.0]
    u8 = fn(cache, idx, params, O, 0, A.CPAD, 1.0, None, None)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (idx.numel(), 3, O, O)
    e = (u8.cpu().double().permute(0, 2, 3, 1) - truth_val).abs()
    worst[0] = float(e.max()) - 0.5
    assert float(e.max()) <= 0.5 + M_U8, f"uint8: {int((e > 0.5 + M_U8).sum())} elements beyond 0.5 + {M_U8} (worst {float(e.max())})"
    for mean, stdv in norm_variants():
        t = A.normalised(truth_val, A.SCALE, mean, stdv)
        md, sd = (None, None) if mean is None else (mean.to(dev), stdv.to(dev))
        f32 = fn(cache, idx, params, O, 2, A.CPAD, A.SCALE, md, sd)
        bf = fn(cache, idx, params, O, 1, A.CPAD, A.SCALE, md, sd)
        assert f32.dtype == torch.float32 and bf.dtype == torch.bfloat16 and tuple(f32.shape) == tuple(bf.shape) == tuple(t.shape)
        for y in (f32, bf):
            assert bool((y[..., 3:] == 0).all()), "pad channels must be exact zeros"
        sr = float(T.seg_rel(f32.cpu()[..., :3], t[..., :3], A.seg_pixels(t)[1]).max())
        worst[1] = max(worst[1], sr)
        assert sr <= BOUND_F32, f"fp32 mode: seg_rel {sr} beyond {BOUND_F32}"
        worst[2] = max(worst[2], T.assert_elementwise(bf.cpu()[..., :3], t[..., :3], A.seg_pixels(t)[1], K_BF16, "bf16 mode"))
    return worst


def measure_floors():
    cache, idx = A.make_cache(), A.idx_tensor()
    lsb = f32 = bf = 0.0
    for O, name, p in all_cases():
        tv = A.gather(cache, idx, p, O)
        val = ref.augment_batch(cache, idx, p, O, 2, 3, 1.0, None, None)
        lsb = max(lsb, float((val.double() - tv).abs().max()))
        w = check_outputs(ref.augment_batch, cache, idx, O, p, tv)
        f32, bf = max(f32, w[1]), max(bf, w[2])
    return lsb, f32, bf


# ------------------------------------------------------------------------------ truth and floors
def test_truth_equals_grid_sample():
    cache, idx = A.make_cache(), A.idx_tensor()
    for O, name, p in all_cases():
        d = float((A.gather(cache, idx, p, O) - A.grid_sample_form(cache, idx, p, O)).abs().max())
        assert d <= 1e-9, (O, name, d)


def test_reference_floors():
    lsb, f32, bf = measure_floors()
    print("floors: lsb %.3g  seg_rel %.3g  bf16 norm_err %.3g" % (lsb, f32, bf))
    # the recorded floors are these measurements (within a factor of two for the fp32 ones)
    assert 0.5 * FLOOR_LSB <= lsb <= 2 * FLOOR_LSB and 0.5 * FLOOR_F32 <= f32 <= 2 * FLOOR_F32, (lsb, f32)
    assert abs(bf - FLOOR_BF16) <= 0.1 * FLOOR_BF16 + 0.02, bf
    assert 2 * f32 <= BOUND_F32 and 2 * FLOOR_F32 <= BOUND_F32
    assert 2 * bf <= K_BF16 <= max(1.0, 4 * bf) and 2 * FLOOR_BF16 <= K_BF16 <= max(1.0, 4 * FLOOR_BF16)
    assert 2 * lsb <= M_U8 <= 4 * lsb and 2 * FLOOR_LSB <= M_U8 <= 4 * FLOOR_LSB


def test_exact_cases_are_slices_of_the_cache():
    """ops/ref.py on the maps with whole-pixel taps: bitwise the indexed cache, in every mode."""
    cache, idx = A.make_cache(), A.idx_tensor()
    for O in A.OUT_SIZES:
        for name, row in A.EXACT.items():
            p = A.cases(O)[name]
            want = A.exact_expected(cache, idx, row, O)
            assert torch.equal(ref.augment_batch(cache, idx, p, O, 0, 8, 1.0, None, None), want), (O, name)
            assert torch.equal(ref.augment_batch(cache, idx, p, O, 1, 8, A.SCALE, *A.mean_std()),
                               ref.nchw_to_nhwc(want, 8, A.SCALE, *A.mean_std())), (O, name)
            assert torch.equal(ref.augment_batch(cache, idx, p, O, 2, 8, A.SCALE, None, None),
                               ref.nchw_to_nhwc_f32(want, 8, A.SCALE)), (O, name)
    assert int((A.exact_expected(cache, idx, A.EXACT["outside"], 24) != 0).sum()) == 0
    assert int((A.exact_expected(cache, idx, A.EXACT["crop"], 24) != 0).sum()) > 0


def test_comparator_rejects_a_shifted_sample():
    """A one-pixel shift of one sample and a dropped tap are beyond every bound."""
    cache, idx = A.make_cache(), A.idx_tensor()
    O = 24
    p = A.cases(O)["rot_p15"]
    tv = A.gather(cache, idx, p, O)
    q = p.clone()
    q[3, 2] += 1.0
    with pytest.raises(AssertionError):
        check_outputs(lambda c, i, pp, *a: ref.augment_batch(c, i, q, *a), cache, idx, O, p, tv)


# ------------------------------------------------------------------------------ affine_params
def test_identity_spec_is_the_centre_crop():
    spec = DC.AugmentSpec(scale=(1.0, 1.0), ratio=(1.0, 1.0), degrees=0.0, flip=0.0, out_size=224, resize=256)
    p = DC.affine_params(spec, 3, 5, np.arange(64), 256)
    assert p.dtype == np.float32 and p.shape == (64, 6)
    assert np.array_equal(p, np.tile(np.float32([1, 0, 16, 0, 1, 16]), (64, 1)))
    assert np.array_equal(p, DC.eval_params(64, 256, 224))


def test_params_depend_on_seed_epoch_index_only():
    spec = DC.AugmentSpec()
    a = DC.affine_params(spec, 1, 2, np.array([5, 9, 1000, 7]), 256)
    b = DC.affine_params(spec, 1, 2, np.array([7, 5]), 256)
    c = DC.affine_params(spec, 1, 2, np.array([9]), 256)
    assert np.array_equal(a[0], b[1]) and np.array_equal(a[3], b[0]) and np.array_equal(a[1], c[0])
    assert not np.array_equal(a, DC.affine_params(spec, 1, 3, np.array([5, 9, 1000, 7]), 256))
    assert not np.array_equal(a, DC.affine_params(spec, 2, 2, np.array([5, 9, 1000, 7]), 256))
    assert len({tuple(r) for r in DC.affine_params(spec, 1, 2, np.arange(512), 256)}) == 512


def test_draw_distributions():
    spec, Sc, n = DC.AugmentSpec(), 256, 4096
    l, t, cw, ch, angle, flip = DC.crop_boxes(spec, 0, 0, np.arange(n), Sc)
    eps = 1e-9
    assert bool((l >= 0).all() and (t >= 0).all() and (l + cw <= Sc + eps).all() and (t + ch <= Sc + eps).all())
    area = cw * ch / (Sc * Sc)
    assert bool((area >= spec.scale[0] - eps).all() and (area <= spec.scale[1] + eps).all())
    assert area.min() < 0.81 and area.max() > 0.99
    assert bool((np.abs(angle) <= spec.degrees).all()) and angle.min() < -14 and angle.max() > 14
    assert abs(float(flip.mean()) - 0.5) <= 0.05
    # the composed map sends the corners of the 256-frame onto the corners of the box when unrotated
    spec0 = DC.AugmentSpec(degrees=0.0, flip=0.0, out_size=256, resize=256)
    l, t, cw, ch, _, _ = DC.crop_boxes(spec0, 0, 0, np.arange(8), Sc)
    p = DC.affine_params(spec0, 0, 0, np.arange(8), Sc).astype(np.float64)
    assert np.allclose(p[:, 2], l, atol=1e-4) and np.allclose(p[:, 0] * 256 + p[:, 2], l + cw, atol=1e-4)
    assert np.allclose(p[:, 5], t, atol=1e-4) and np.allclose(p[:, 4] * 256 + p[:, 5], t + ch, atol=1e-4)


def test_flip_and_rotation_of_the_map():
    """Flip mirrors the map about the frame's centre column; a rotation keeps the frame's centre."""
    base = DC.compose_params([3.0], [5.0], [200.0], [180.0], [0.0], [False], 256, 224).astype(np.float64)[0]
    flp = DC.compose_params([3.0], [5.0], [200.0], [180.0], [0.0], [True], 256, 224).astype(np.float64)[0]
    # output column x under the flip reads what column 224 - x reads without it
    assert np.isclose(flp[0], -base[0]) and np.isclose(flp[2], base[0] * 224 + base[2], atol=1e-4)
    rot = DC.compose_params([3.0], [5.0], [200.0], [180.0], [15.0], [False], 256, 224).astype(np.float64)[0]
    ctr = lambda q: (q[0] * 112 + q[1] * 112 + q[2], q[3] * 112 + q[4] * 112 + q[5])
    assert np.allclose(ctr(rot), ctr(base), atol=1e-4) and np.allclose(ctr(base), (3 + 100, 5 + 90), atol=1e-4)


# ------------------------------------------------------------------------------ DeviceImageCache
SIZES = [(50, 37), (37, 50), (64, 64), (32, 32)]


def write_folder(root, n=12, classes=("a", "b", "c")):
    """n lossless PNGs (smooth content plus noise) in ``root/<class>/``; returns the root."""
    from PIL import Image
    rng = np.random.RandomState(7)
    for i in range(n):
        w, h = SIZES[i % len(SIZES)]
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(xx * 5 + i * 20) % 256, (yy * 7 + i * 11) % 256, ((xx + yy) * 3) % 256], -1)
        img = np.clip(img + rng.randint(-20, 21, img.shape), 0, 255).astype(np.uint8)
        d = os.path.join(str(root), classes[i % len(classes)])
        os.makedirs(d, exist_ok=True)
        Image.fromarray(img).save(os.path.join(d, f"img_{i:02d}.png"))
    return str(root)


def count_decodes(monkeypatch, folder):
    calls = []
    orig = folder.load_raw

    def load_raw(i):
        calls.append(i)
        return orig(i)

    monkeypatch.setattr(folder, "load_raw", load_raw)
    return calls


def test_cache_cpu_matches_imagefolder(tmp_path, monkeypatch):
    from pcmp.data.synthetic import BatchLoader
    root = write_folder(tmp_path)
    folder = ImageFolder(root, size=32)
    plain = ImageFolder(root, size=32)
    calls = count_decodes(monkeypatch, folder)
    cache = DC.DeviceImageCache(folder, "cpu", cache_size=32)
    assert len(cache) == 12 and cache.cache.shape == (12, 32, 32, 4) and not cache.filled.any()
    loader = BatchLoader(cache, 5, device="cpu", shuffle=True, seed=3)
    for epoch in range(2):
        loader.set_epoch(epoch)
        g = torch.Generator().manual_seed(3 + epoch)
        order = torch.randperm(12, generator=g).tolist()
        got = list(loader)
        assert len(got) == 3
        for b, (x, y) in enumerate(got):
            wx, wy = plain.get_batch(order[b * 5:(b + 1) * 5], "cpu")
            assert x.dtype == torch.uint8 and torch.equal(x, wx) and torch.equal(y, wy)
    assert cache.decodes == 12 and len(calls) == 12 and cache.filled.all()
    assert cache.stats() == {"images": 12, "bytes": 12 * 32 * 32 * 4, "decodes": 12, "augment": False}
    x, y = cache.get_batch([3, 3, 0], "cpu")          # repeats
    assert torch.equal(x[0], x[1]) and len(calls) == 12


def test_cache_index_and_budget_errors(tmp_path):
    folder = ImageFolder(write_folder(tmp_path), size=32)
    cache = DC.DeviceImageCache(folder, "cpu")
    for bad in ([12], [-1], [0, 99], [0.5], [True], [[0, 1]]):
        with pytest.raises(IndexError):
            cache.get_batch(bad, "cpu")
    assert cache.decodes == 0
    with pytest.raises(ValueError, match=str(12 * 32 * 32 * 4)):
        DC.DeviceImageCache(folder, "cpu", budget_gb=1e-5)


def test_cache_augmented_batches(tmp_path):
    folder = ImageFolder(write_folder(tmp_path), size=32)
    spec = DC.AugmentSpec(out_size=24, resize=28)
    cache = DC.DeviceImageCache(folder, "cpu", augment=spec, seed=11)
    assert cache.cache_size == 28 and cache.out_size == 24
    cache.set_epoch(1)
    x1, y1 = cache.get_batch([2, 7], "cpu")
    x2, _ = cache.get_batch([5, 2], "cpu")
    assert tuple(x1.shape) == (2, 3, 24, 24) and torch.equal(x1[0], x2[1])      # sample 2 in either batch
    assert torch.equal(x1, cache.get_batch([2, 7], "cpu")[0])                   # same (seed, epoch)
    cache.set_epoch(2)
    assert not torch.equal(x1, cache.get_batch([2, 7], "cpu")[0])
    assert cache.decodes == 3
    # the eval view shares the storage and takes the exact centre crop
    ev = cache.view(train=False)
    xe, ye = ev.get_batch([2], "cpu")
    assert torch.equal(xe[0], cache.cache[2, 2:26, 2:26, :3].permute(2, 0, 1)) and cache.decodes == 3
    # normalised NHWC output: the fp32 expression of the input conversion on the centre crop
    xn, _ = cache.view(train=False, out="f32").get_batch([2], "cpu")
    m, s = torch.tensor(spec.mean), torch.tensor(spec.std)
    assert tuple(xn.shape) == (1, 24, 24, 8) and bool((xn[..., 3:] == 0).all())
    assert torch.equal(xn[..., :3], (xe.permute(0, 2, 3, 1).float() * (1.0 / 255.0) - m) / s)


def test_every_pass_draws_a_new_augmentation(tmp_path):
    """``keras_fit`` (resnet.py) and ``--reference-compat`` iterate their loader without ``set_epoch``:
    each pass over an augmenting loader still takes the next epoch's draws; ``set_epoch`` names the
    epoch of the pass that follows it."""
    from pcmp.data.imagefolder import flow_from_directory, load_split_train_test

    def passes(loader, n, epochs=None):
        out = []
        for e in range(n):
            if epochs is not None:
                loader.set_epoch(epochs[e])
            out.append(torch.cat([x for x, _ in loader]))      # the loop of keras_fit: ``for x, y in train``
        return out

    root = write_folder(tmp_path)
    train = flow_from_directory(root, 32, 5, "cpu", augment=True, seed=4)
    a = passes(train, 3)
    assert train.ds.epoch == 2 and train.ds.decodes == 12
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2]) and not torch.equal(a[0], a[2])
    # the shuffle order is that of the loader's own epoch, which only set_epoch moves; named epochs
    # reproduce: the passes above were epochs 0, 1, 2 of this seed
    again = flow_from_directory(root, 32, 5, "cpu", augment=True, seed=4)
    for e in (2, 0, 1):
        again.ds.set_epoch(e)
        assert torch.equal(torch.cat([x for x, _ in again]), a[e]), e
    # a validation generator and an unaugmented cache are the same in every pass
    val = flow_from_directory(root, 32, 5, "cpu", augment=True, seed=4, train=False)
    v = passes(val, 2)
    assert torch.equal(v[0], v[1])
    # the split loaders: the train loader advances, the test loader (centre crop) does not
    tr, te = load_split_train_test(root, 0.25, 4, False, "cpu", seed=1, augment=True)
    tr.shuffle = te.shuffle = False
    t = passes(tr, 2)
    s = passes(te, 2)
    assert not torch.equal(t[0], t[1]) and torch.equal(s[0], s[1])
    with pytest.raises(ValueError):
        tr.ds.view(out="bf15")


# ------------------------------------------------------------------------------ entry point
def split_folders(tmp_path):
    write_folder(tmp_path / "train", 12)
    write_folder(tmp_path / "val", 8)
    return str(tmp_path)


@pytest.mark.parametrize("flag", ["--cache-device", "--augment"])
def test_resnet_entry_point_decodes_each_image_once(tmp_path, flag):
    data = split_folders(tmp_path)
    out = tmp_path / "record.json"
    cmd = [sys.executable, os.path.join(ROOT, "resnet.py"), "--device", "cpu", "--data-dir", data, "--image-size", "32",
           "--batch-size", "4", "--epochs", "2", flag, "--json", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads(out.read_text().splitlines()[-1])
    dc = rec["data_cache"]
    assert dc["images"] == 20 and dc["decodes"] == 20 and dc["augment"] == (flag == "--augment")
    side = 37 if flag == "--augment" else 32
    assert dc["bytes"] == 20 * side * side * 4


if __name__ == "__main__":
    print("floors: lsb %.3g  seg_rel %.3g  bf16 norm_err %.3g" % measure_floors())
