"""GPU tests of the fused augmentation kernel (csrc/augment_batch.hip) and the loaders on it (rovit_hip/augment.py, data/dataset.py).

Oracles: ``augment_reference`` in fp64 on the rows the kernel itself reports (the image and the draw are tested separately; the reference
is pinned against torch's own resampling in tests/test_augment_cpu.py) and ``draw_params_reference`` (numpy Philox).  Inputs are
uniform-noise uint8 images: a wrong tap, channel, flip or matrix entry shows as an error of order 1.

Tolerance of the image test, on the normalised output, no pixel excluded: max-abs <= 1.7e-4 when the source sides are <= 64, <= 6e-4
otherwise.  Basis: an fp32 evaluation of the same formulas deviates from fp64 by 3.6e-5 (37 x 53 -> 32 x 32), 6.8e-5 (64 x 64 -> 224 x 224),
2.2e-4 (224 x 224 -> 224 x 224) and 3.8e-4 (256 x 300 -> 224 x 224) with these ranges; the error grows with the source side through the
fp32 source coordinate (one ulp of a coordinate near 256 is 3e-5 of a pixel, times a slope of up to 1/0.224 per pixel on noise, times
the contrast and brightness gains of up to 1.4 each).  Bounds of about 5x that noise (4e-4 and 2e-3) came first; the kernel, which builds
the coordinate from the exact offset to the output centre, measured 1.8e-5, 4.1e-5, 4.3e-5 (B = 1) / 1.5e-4 (B = 3) and 6.8e-5 on the
five cases below, far under them, so the bounds now stand at 4x the largest measured value of each class."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_cpu  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
SEVERITY = {n: i for i, n in enumerate(CLASS_NAMES)}


def dev():
    return torch.device('cuda:0')


def full_config():
    from rovit_hip.augment import AugmentConfig
    return AugmentConfig(hflip=0.5, vflip=0.5, scale=(0.25, 1.0), ratio=(3 / 4, 4 / 3), rotate_deg=30.0, brightness=0.4, contrast=0.4,
                         saturation=0.4, hue=0.1)


def make_store(n, h, w, seed):
    from rovit_hip.augment import DeviceImageStore
    lab = torch.arange(n) % 4
    return DeviceImageStore.synthetic(lab, lab, dev(), size=(h, w), seed=seed)


CASES = [  # store shape, output size, store indices of the batch
    ((5, 37, 53), (32, 32), [4, 0, 2, 2, 1, 4, 3]),
    ((4, 64, 64), (224, 224), [3, 0, 2]),
    ((3, 224, 224), (224, 224), [1]),
    ((3, 224, 224), (224, 224), [2, 0, 1]),
    ((2, 256, 300), (224, 224), [1, 0]),
]


@pytest.mark.parametrize('shape,out_size,idx', CASES, ids=['37x53_to_32', '64_to_224', '224_b1', '224_b3', '256x300_to_224'])
def test_kernel_matches_the_fp64_reference_on_its_own_rows(shape, out_size, idx):
    from rovit_hip.augment import augment_reference, draw_params_reference
    n, h, w = shape
    store = make_store(n, h, w, seed=h + w)
    cfg, seed, epoch = full_config(), 0xC0FFEE12345, 3
    out, rows = store.batch(idx, cfg, seed, epoch, return_params=True, out_size=out_size)
    assert out.shape == (len(idx), 3) + out_size and out.dtype == torch.float32 and rows.shape == (len(idx), 12)
    want = augment_reference(store.images, idx, rows, out_size)                     # fp64 on the device, the kernel's own rows
    err = float((out.double() - want).abs().max())
    bound = 1.7e-4 if max(h, w) <= 64 else 6e-4
    print(f'augment_batch {h}x{w} -> {out_size[0]}x{out_size[1]} B={len(idx)}: max-abs error {err:.3e} (bound {bound:.0e})')
    assert err <= bound, (err, bound)
    # explicit rows: bit for bit the drawn run that reported them
    again = store.batch(idx, cfg, seed + 1, epoch + 1, params=rows, out_size=out_size)
    assert torch.equal(again, out)
    # the drawn rows: flips exact, every other entry one or two fp32 roundings from the exact-u evaluation
    ref = draw_params_reference(idx, cfg, seed, epoch)
    got = rows.cpu().numpy()
    assert np.array_equal(got[:, :2], ref[:, :2]) and np.array_equal(got[:, 11], np.zeros(len(idx), np.float32))
    assert (np.abs(got[:, 2:11].astype(np.float64) - ref[:, 2:11]) <= 1e-6 * np.maximum(1.0, np.abs(ref[:, 2:11]))).all()
    # repeated store indices carry the same row and the same image
    for a in range(len(idx)):
        for b in range(a + 1, len(idx)):
            if idx[a] == idx[b]:
                assert torch.equal(rows[a], rows[b]) and torch.equal(out[a], out[b])


def test_drawn_rows_match_the_numpy_restatement_over_many_indices():
    from rovit_hip.augment import draw_params_reference
    store = make_store(4096, 4, 4, seed=1)
    idx = torch.randperm(4096, generator=torch.Generator().manual_seed(0))
    cfg, seed, epoch = full_config(), (7 << 32) + 11, (1 << 32) + 5                 # both halves of seed and epoch in use
    _, rows = store.batch(idx, cfg, seed, epoch, return_params=True, out_size=(4, 4))
    ref, got = draw_params_reference(idx, cfg, seed, epoch), rows.cpu().numpy()
    assert np.array_equal(got[:, :2], ref[:, :2]) and 0.4 < got[:, 0].mean() < 0.6 and 0.4 < got[:, 1].mean() < 0.6
    assert (np.abs(got[:, 2:11].astype(np.float64) - ref[:, 2:11]) <= 1e-6 * np.maximum(1.0, np.abs(ref[:, 2:11]))).all()


def test_identity_fast_path_and_forced_flip():
    from rovit_hip.augment import IMAGENET_MEAN, IMAGENET_STD, AugmentConfig
    store = make_store(3, 224, 224, seed=9)
    idx = [2, 0, 1, 0]
    out, rows = store.batch(idx, AugmentConfig.identity(), 4, 1, return_params=True)
    assert torch.equal(rows[:, [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]].cpu(), torch.tensor([0, 0, 1, 0, 0, 1, 1, 1, 0, 0.]).expand(4, 10))    # all but ux, uy
    mean, std = torch.tensor(IMAGENET_MEAN, device=dev()).view(1, 3, 1, 1), torch.tensor(IMAGENET_STD, device=dev()).view(1, 3, 1, 1)
    src = store.images[idx]
    want32 = (src.float() / 255 - mean) / std
    want64 = (src.double() / 255 - mean.double()) / std.double()
    e32, e64 = float((out - want32).abs().max()), float((out.double() - want64).abs().max())
    print(f'identity path: max-abs error {e32:.3e} against the fp32 recipe, {e64:.3e} against fp64')
    assert e32 <= 1e-6 and e64 <= 1e-6
    forced = rows.clone()
    forced[:, 0] = 1.0
    assert torch.equal(store.batch(idx, params=forced), out.flip(-1))
    forced[:, 1] = 1.0
    assert torch.equal(store.batch(idx, params=forced), out.flip(-1).flip(-2))
    # the default config is flip + normalise: every sample is the plain image or its mirror image, bit for bit, as its row says
    out_d, rows_d = store.batch(idx, AugmentConfig(), 4, 1, return_params=True)
    for k in range(4):
        assert torch.equal(out_d[k], out[k].flip(-1) if float(rows_d[k, 0]) else out[k])
    # the general path at identity rows (a store of another size cannot take the fast path) agrees with the reference as well
    small = make_store(2, 112, 112, seed=10)
    from rovit_hip.augment import augment_reference
    o, r = small.batch([1, 0], AugmentConfig.identity(), 4, 1, return_params=True)
    assert float((o.double() - augment_reference(small.images, [1, 0], r, (224, 224))).abs().max()) <= 6e-4


def test_split_invariance_epochs_and_determinism():
    store = make_store(16, 48, 56, seed=21)
    idx = [9, 3, 15, 0, 3, 7, 12, 1]
    cfg = full_config()
    one, rows = store.batch(idx, cfg, 77, 5, return_params=True, out_size=(40, 44))
    two = torch.cat([store.batch(idx[:4], cfg, 77, 5, out_size=(40, 44)), store.batch(idx[4:], cfg, 77, 5, out_size=(40, 44))])
    eight = torch.cat([store.batch([i], cfg, 77, 5, out_size=(40, 44)) for i in idx])
    assert torch.equal(one, two) and torch.equal(one, eight)
    assert torch.equal(store.batch(idx, cfg, 77, 5, out_size=(40, 44)), one)                          # run to run
    assert torch.equal(store.batch(torch.tensor(idx, device=dev()), cfg, 77, 5, out_size=(40, 44)), one)    # device index tensor
    other, rows_o = store.batch(idx, cfg, 77, 6, return_params=True, out_size=(40, 44))
    for k in range(8):
        assert not torch.equal(other[k], one[k]) and not torch.equal(rows_o[k], rows[k])
    assert not torch.equal(store.batch(idx, cfg, 78, 5, out_size=(40, 44)), one)
    # the same holds on the fast path (224 x 224 store, default config)
    big = make_store(8, 224, 224, seed=22)
    order = [5, 1, 7, 0, 2, 6, 3, 4]
    a = big.batch(order, None, 3, 2)
    b = torch.cat([big.batch(order[:4], None, 3, 2), big.batch(order[4:], None, 3, 2)])
    assert torch.equal(a, b) and torch.equal(a[[1]], big.batch([1], None, 3, 2))


def test_device_cache_loaders_follow_the_store():
    from data.dataset import DeviceAugmentLoader, create_dataloaders
    from rovit_hip.augment import IMAGENET_MEAN, IMAGENET_STD
    kw = dict(class_names=CLASS_NAMES, severity_map=SEVERITY, batch_size=8, seed=5, synthetic=45, device=dev(), device_cache=True)
    tr, va, te = create_dataloaders('data/Augmented Image', 'data/Original Image', **kw)
    assert all(isinstance(l, DeviceAugmentLoader) for l in (tr, va, te)) and (len(tr), len(va), len(te)) == (5, 2, 2)
    assert tr.store.images.is_cuda and tr.store.images.dtype == torch.uint8 and tr.store.nbytes == 45 * 3 * 224 * 224 + 2 * 45 * 8
    assert tr.dataset.dataset.get_class_weights().shape == (4,)
    mean, std = torch.tensor(IMAGENET_MEAN, device=dev()).view(1, 3, 1, 1), torch.tensor(IMAGENET_STD, device=dev()).view(1, 3, 1, 1)
    for ld, n in ((tr, 36), (va, 9), (te, 11)):
        epoch = ld.epoch
        order, seen = ld.epoch_order(epoch), 0
        for b, (x, c, s) in enumerate(ld):
            sel = order[b * 8:(b + 1) * 8]
            assert x.is_cuda and x.dtype == torch.float32 and x.shape == (len(sel), 3, 224, 224) and not c.is_cuda and not s.is_cuda
            assert torch.equal(c, ld.store.labels.cpu()[sel]) and torch.equal(s, ld.store.severities.cpu()[sel]) and c.dtype == torch.long
            plain = (ld.store.images[sel.to(dev())].float() / 255 - mean) / std
            if ld is tr:            # flip + normalise: each image or its mirror image
                d = torch.minimum((x - plain).abs().amax((1, 2, 3)), (x - plain.flip(-1)).abs().amax((1, 2, 3)))
            else:                   # identity
                d = (x - plain).abs().amax((1, 2, 3))
            assert float(d.max()) <= 1e-6
            seen += len(sel)
        assert seen == n and ld.epoch == epoch + 1                      # the last batches are short: 36 = 4*8 + 4, 9 = 8 + 1, 11 = 8 + 3
    assert sorted(tr.epoch_order(0).tolist()) == sorted(tr.dataset.indices) and not torch.equal(tr.epoch_order(0), tr.epoch_order(1))
    # device labels, a batch of one, drop_last
    one = DeviceAugmentLoader(tr.store, [7, 3, 11], 1, False, labels_on_device=True)
    got = list(one)
    assert len(got) == 3 and all(x.shape == (1, 3, 224, 224) and c.is_cuda and s.is_cuda for x, c, s in got)
    assert [int(c) for _, c, _ in got] == tr.store.labels[[7, 3, 11]].tolist()
    assert [x.shape[0] for x, _, _ in DeviceAugmentLoader(tr.store, list(range(10)), 4, True, drop_last=True)] == [4, 4]
    # set_epoch replays an epoch bit for bit
    tr.set_epoch(0)
    first = [x for x, _, _ in tr]
    tr.set_epoch(0)
    assert all(torch.equal(a, b) for a, b in zip(first, [x for x, _, _ in tr]))


def test_ten_training_steps_on_the_store_loader():
    from data.dataset import create_dataloaders
    from data.transforms import cutmix_or_mixup
    from models.rovit_kan import RoViTKAN
    from rovit_hip.losses import JointLoss
    from rovit_hip.optim import RoViTAdamW
    tr, _, _ = create_dataloaders(None, None, CLASS_NAMES, SEVERITY, batch_size=8, seed=1, synthetic=50, device=dev(), device_cache=True,
                                  device_augment=full_config(), store_size=(96, 128))
    torch.manual_seed(3)
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=2))
    m = m.to(dev()).train()
    m.curriculum_stage = 4
    opt = RoViTAdamW(m, lr=1e-3)
    loss_fn = JointLoss(1.0, 0.5, 0.5, 2.0)
    rng = np.random.RandomState(0)
    losses = []
    while len(losses) < 10:
        for x, c, s in tr:
            x, c, s = x.to(dev()), c.to(dev()), s.to(dev())
            assert x.shape[1:] == (3, 224, 224)
            x, la, lb, lam = cutmix_or_mixup(x, c, True, True, 1.0, 0.2, rng=rng)
            opt.zero_grad()
            out = m(x)
            loss = lam * loss_fn(out, la, s, 4)['total_loss'] + (1 - lam) * loss_fn(out, lb, s, 4)['total_loss']
            loss.backward()
            opt.step()
            losses.append(loss.detach())
            if len(losses) == 10:
                break
    assert tr.epoch == 2 and bool(torch.isfinite(torch.stack(losses)).all())


def test_image_folder_is_decoded_once_into_the_store(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from data.dataset import RoseLeafDataset, create_dataloaders
    from rovit_hip.augment import AugmentConfig, DeviceImageStore
    rs = np.random.RandomState(4)
    for k in range(12):
        d = tmp_path / CLASS_NAMES[k % 3]
        d.mkdir(exist_ok=True)
        Image.fromarray(rs.randint(0, 256, (20 + k, 33 - k, 3), dtype=np.uint8)).save(d / f'leaf_{k:02d}.png')
    ds = RoseLeafDataset(tmp_path, CLASS_NAMES, SEVERITY, None, 'original')
    store = DeviceImageStore.from_dataset(ds, dev(), size=(24, 32))
    assert len(store) == 12 and store.images.is_cuda and store.images.shape == (12, 3, 24, 32) and store.dataset is ds
    assert torch.equal(store.labels.cpu(), ds.labels) and torch.equal(store.severities.cpu(), ds.severities)
    for k, (path, _) in enumerate(ds.samples):
        with Image.open(path) as im:
            want = torch.from_numpy(np.asarray(im.convert('RGB').resize((32, 24))).copy()).permute(2, 0, 1)
        assert torch.equal(store.images[k].cpu(), want), path
    x = store.batch(list(range(12)), AugmentConfig.identity(), out_size=(24, 32))
    assert x.shape == (12, 3, 24, 32) and bool(torch.isfinite(x).all())
    tr, va, te = create_dataloaders(tmp_path, tmp_path, CLASS_NAMES, SEVERITY, batch_size=5, seed=2, device=dev(), device_cache=True,
                                    store_size=(24, 32))
    assert sum(x.shape[0] for x, _, _ in tr) + sum(x.shape[0] for x, _, _ in va) == 12 and sum(x.shape[0] for x, _, _ in te) == 12
    assert next(iter(te))[0].shape == (5, 3, 224, 224)


def test_errors_are_loud_before_any_launch():
    from rovit_hip import RovitHipError
    from rovit_hip.augment import AugmentConfig, DeviceImageStore
    store = make_store(4, 32, 32, seed=2)
    cpu = DeviceImageStore(store.images.cpu(), store.labels.cpu(), store.severities.cpu())
    with pytest.raises(RovitHipError):
        cpu.batch([0, 1])
    with pytest.raises(RovitHipError):
        store.batch([0, 1], out_size=(32, 30))
    with pytest.raises(RovitHipError):
        store.batch([0, 1], AugmentConfig(scale=(0.5, 0.2)))
    with pytest.raises(RovitHipError):
        store.batch([0, 1], AugmentConfig(hflip=1.5))
    with pytest.raises(RovitHipError):
        store.batch([0, 4])                                                  # a host index list is range-checked on the host
    with pytest.raises(RovitHipError):
        store.batch([0, 1], params=torch.zeros(3, 12))
    # the C entry refuses what the Python layer cannot see: out overlapping src, a bad range, an unaligned out, a width of 30
    from rovit_hip import native
    buf = torch.zeros(2 * 3 * 32 * 32, dtype=torch.float32, device=dev())
    alias = DeviceImageStore(buf.view(torch.uint8)[:4 * 3 * 32 * 32].view(4, 3, 32, 32), store.labels, store.severities)
    with pytest.raises(RovitHipError, match='alias'):
        alias.batch([0, 1], out_size=(32, 32), out=buf.view(2, 3, 32, 32))
    idx = torch.tensor([0, 1], device=dev())
    out = torch.empty(2 * 3 * 32 * 32 + 4, dtype=torch.float32, device=dev())
    lib, good = native.load(), AugmentConfig().to_c()
    import ctypes

    def rc(cfg=good, o=out, wo=32, n=4):
        return lib.rovit_augment_batch(store.images.data_ptr(), n, 32, 32, idx.data_ptr(), 2, None, None, ctypes.addressof(cfg), 0, 0,
                                       o.data_ptr(), 32, wo, native.stream_ptr())
    assert rc() == 0
    assert rc(cfg=AugmentConfig(scale=(0.5, 0.2)).to_c()) == -1
    assert rc(cfg=AugmentConfig(vflip=-0.5).to_c()) == -1 and rc(wo=30) == -1 and rc(n=0) == -1
    assert rc(o=out[1:]) == -2 and b'aligned' in lib.rovit_last_error_string()
    assert lib.rovit_augment_batch(None, 4, 32, 32, idx.data_ptr(), 2, None, None, ctypes.addressof(good), 0, 0, out.data_ptr(), 32, 32,
                                   native.stream_ptr()) == -3
    torch.cuda.synchronize()
