"""``torch.ops.pcmp.augment_batch`` (csrc/augment.hip) on the MI355X against the fp64 truth of
``pcmp.ops.truth_augment``, element by element and held to the bounds of tests/test_augment_cpu.py
(uint8: |out - unrounded truth| <= 0.5 + M_U8; fp32: seg_rel <= 1e-5 per image and channel; bf16:
norm_err <= 1), plus the bitwise properties: the whole-pixel maps equal the indexed cache and the
existing input conversion of it, the all-outside sample is (0 - mean)/std, pad channels are zero,
repeated indices repeat, two runs agree, slot offsets beyond 2^31 and 2^32 bytes are addressed
right; and ``DeviceImageCache`` on the device against ``ImageFolder``."""
import pytest
import torch

import pcmp  # noqa: F401
from pcmp.data import device_cache as DC
from pcmp.data.imagefolder import ImageFolder
from pcmp.ops import truth_augment as A

from test_augment_cpu import all_cases, check_outputs, count_decodes, write_folder

pytestmark = pytest.mark.gpu


def op():
    return torch.ops.pcmp.augment_batch


@pytest.fixture(scope="module")
def data(gpu):
    cache, idx = A.make_cache(), A.idx_tensor()
    truths = {(O, name): A.gather(cache, idx, p, O) for O, name, p in all_cases()}
    return cache.to(gpu), idx.to(gpu), truths


@pytest.mark.parametrize("O", A.OUT_SIZES)
def test_bounds_hold_for_every_element(gpu, data, O):
    cache, idx, truths = data
    worst = [0.0, 0.0, 0.0]
    for name, p in A.cases(O).items():
        w = check_outputs(op(), cache, idx, O, p.to(gpu), truths[(O, name)], gpu)
        print(f"O={O} {name}: u8 excess over 0.5 {w[0]:.3g}  fp32 seg_rel {w[1]:.3g}  bf16 norm_err {w[2]:.3g}")
        worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"O={O} worst: u8 excess {worst[0]:.3g}  fp32 seg_rel {worst[1]:.3g}  bf16 norm_err {worst[2]:.3g}")


@pytest.mark.parametrize("O", A.OUT_SIZES)
def test_exact_maps_are_the_indexed_cache(gpu, data, O):
    cache, idx, _ = data
    mean, stdv = (t.to(gpu) for t in A.mean_std())
    for name, row in A.EXACT.items():
        p = A.cases(O)[name].to(gpu)
        want = A.exact_expected(cache, idx, row, O).to(gpu)
        assert torch.equal(op()(cache, idx, p, O, 0, A.CPAD, 1.0, None, None), want), name
        for m, s in ((None, None), (mean, stdv)):
            assert torch.equal(op()(cache, idx, p, O, 1, A.CPAD, A.SCALE, m, s),
                               torch.ops.pcmp.nchw_to_nhwc(want, A.CPAD, A.SCALE, m, s)), (name, m is not None)
        assert torch.equal(op()(cache, idx, p, O, 2, A.CPAD, A.SCALE, None, None),
                           torch.ops.pcmp.nchw_to_nhwc_f32(want, A.CPAD, A.SCALE)), name


def test_outside_sample_pads_repeats_and_reruns(gpu, data):
    cache, idx, _ = data
    mean, stdv = (t.to(gpu) for t in A.mean_std())
    O = 33
    p = A.cases(O)["outside"].to(gpu)
    for mode, dt in ((1, torch.bfloat16), (2, torch.float32)):
        y = op()(cache, idx, p, O, mode, A.CPAD, A.SCALE, mean, stdv)
        want = ((0.0 - mean.cpu()) / stdv.cpu()).to(dt)           # IEEE fp32 on the host
        assert torch.equal(y[..., :3].cpu(), want.expand(len(A.IDX), O, O, 3))
        assert bool((y[..., 3:] == 0).all())
        assert int(op()(cache, idx, p, O, mode, A.CPAD, A.SCALE, None, None).ne(0).sum()) == 0
    assert int(op()(cache, idx, p, O, 0, A.CPAD, 1.0, None, None).ne(0).sum()) == 0
    for name in ("rot_p15", "rot_7p3_flip", "half_outside"):
        p = A.cases(O)[name].to(gpu)
        for mode in (0, 1, 2):
            args = (cache, idx, p, O, mode, A.CPAD, A.SCALE if mode else 1.0) + ((mean, stdv) if mode else (None, None))
            y = op()(*args)
            assert torch.equal(y[0], y[2]) and torch.equal(y[1], y[6]), "repeated idx entries"      # IDX 4,0,4,...,0
            assert not torch.equal(y[0], y[1])
            assert torch.equal(y, op()(*args)), "run-to-run bitwise equality"
    # an index outside the cache reads nothing: the all-outside sample
    bad = torch.tensor([0, A.N_IMAGES, -1], device=gpu)
    y = op()(cache, bad, A.cases(24)["crop"][:3].to(gpu), 24, 0, A.CPAD, 1.0, None, None)
    assert int(y[0].ne(0).sum()) > 0 and int(y[1:].ne(0).sum()) == 0


def test_slot_offsets_beyond_32_bits(gpu):
    """16,400 slots of 256x256x4: slot 8,199 starts beyond 2^31 bytes, slot 16,399 beyond 2^32.  The
    4.3 GB are never filled; three slots are written and gathered."""
    n, Sc, O = 16400, 256, 16
    cache = torch.empty((n, Sc, Sc, 4), dtype=torch.uint8, device=gpu)
    slots = [0, 8199, 16399]
    assert slots[1] * Sc * Sc * 4 > 2 ** 31 and slots[2] * Sc * Sc * 4 > 2 ** 32
    g = torch.Generator().manual_seed(5)
    imgs = torch.randint(0, 256, (3, Sc, Sc, 4), dtype=torch.uint8, generator=g).to(gpu)
    for s, im in zip(slots, imgs):
        cache[s].copy_(im)
    idx = torch.tensor([16399, 0, 8199, 16399], device=gpu)
    p = torch.tensor([[1.0, 0.0, 200.0, 0.0, 1.0, 100.0]] * 4, device=gpu)
    y = op()(cache, idx, p, O, 0, A.CPAD, 1.0, None, None)
    want = imgs[[2, 0, 1, 2]][:, 100:116, 200:216, :3].permute(0, 3, 1, 2)
    assert torch.equal(y, want)
    del cache
    torch.cuda.empty_cache()


def test_argument_checks(gpu, data):
    cache, idx, _ = data
    p = A.cases(24)["crop"].to(gpu)
    ok = (cache, idx, p, 24, 1, A.CPAD, A.SCALE, None, None)
    op()(*ok)

    def bad(**kw):
        names = ("cache", "idx", "params", "out_size", "mode", "cpad", "scale", "mean", "stdv")
        args = [kw.get(n, v) for n, v in zip(names, ok)]
        with pytest.raises(RuntimeError):
            op()(*args)

    bad(cache=cache.float())
    bad(idx=idx.int())
    bad(params=p.double())
    bad(params=p[:, :5].contiguous())
    bad(params=p[:3])
    bad(cache=cache[:, :, ::2])                       # non-contiguous
    bad(cache=cache[..., :3].contiguous())            # three bytes per pixel
    bad(out_size=0)
    bad(cpad=2)
    bad(mode=3)
    bad(mean=torch.zeros(3, device=gpu))              # mean without std
    bad(cache=cache.cpu())
    # a contiguous view at a storage offset of one byte: the dword loads would be misaligned
    buf = torch.zeros(cache.numel() + 4, dtype=torch.uint8, device=gpu)
    bad(cache=buf[1:1 + cache.numel()].view(cache.shape))
    op()(buf[4:].view(cache.shape), *ok[1:])


# ------------------------------------------------------------------------------ DeviceImageCache
def test_cache_gpu_matches_imagefolder(gpu, tmp_path, monkeypatch):
    root = write_folder(tmp_path)
    folder, plain = ImageFolder(root, size=32), ImageFolder(root, size=32)
    calls = count_decodes(monkeypatch, folder)
    cache = DC.DeviceImageCache(folder, gpu)
    assert cache.cache_size == 32 and cache.cache.is_cuda
    for epoch in range(2):
        cache.set_epoch(epoch)
        order = torch.randperm(12, generator=torch.Generator().manual_seed(epoch)).tolist()
        for i in range(0, 12, 5):
            x, y = cache.get_batch(order[i:i + 5], gpu)
            wx, wy = plain.get_batch(order[i:i + 5], gpu, device_resize=True)
            assert x.dtype == torch.uint8 and x.is_cuda and torch.equal(x, wx) and torch.equal(y, wy)
    assert cache.decodes == 12 and len(calls) == 12
    with pytest.raises(IndexError):
        cache.get_batch([12], gpu)


def test_cache_gpu_augmented_batches(gpu, tmp_path):
    folder = ImageFolder(write_folder(tmp_path), size=32)
    spec = DC.AugmentSpec(out_size=24, resize=28)
    cache = DC.DeviceImageCache(folder, gpu, augment=spec, seed=11)
    cache.set_epoch(1)
    x1, _ = cache.get_batch([2, 7], gpu)
    x2, _ = cache.get_batch([5, 2], gpu)
    assert tuple(x1.shape) == (2, 3, 24, 24) and x1.dtype == torch.uint8
    assert torch.equal(x1[0], x2[1]), "sample i is the same in batch [i, j] and in batch [k, i]"
    assert torch.equal(x1, cache.get_batch([2, 7], gpu)[0]), "same (seed, epoch), same batch"
    cache.set_epoch(2)
    assert not torch.equal(x1, cache.get_batch([2, 7], gpu)[0])
    assert cache.decodes == 3
    # the CPU path resamples the same cached bytes with the same maps: the two differ only where the
    # unrounded value lies within the fp32 floor (1e-3 LSB on either side) of a rounding boundary --
    # about 0.4 % of the elements, and by one step
    cpu = DC.DeviceImageCache(ImageFolder(folder.root, size=32), "cpu", augment=spec, seed=11)
    cpu.set_epoch(2)
    d = (cache.get_batch([2, 7], gpu)[0].cpu().int() - cpu.get_batch([2, 7], "cpu")[0].int()).abs()
    assert int(d.max()) <= 1 and float((d > 0).float().mean()) < 0.01
    # the normalised bf16 model input of the eval view: the input conversion of the centre crop
    ev = cache.view(train=False)
    xe, _ = ev.get_batch([2, 7], gpu)
    xn, _ = cache.view(train=False, out="bf16").get_batch([2, 7], gpu)
    m = torch.tensor(spec.mean, device=gpu)
    s = torch.tensor(spec.std, device=gpu)
    assert torch.equal(xn, torch.ops.pcmp.nchw_to_nhwc(xe, 8, 1.0 / 255.0, m, s))
