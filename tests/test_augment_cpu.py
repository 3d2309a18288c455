"""CPU tests of the augmentation feature's references and host logic (rovit_hip/augment.py, data/dataset.py), independent of any kernel:
``augment_reference`` against torch's own resampling and hand-made known answers, ``draw_params_reference`` against the properties the
draws promise, ``DeviceAugmentLoader``'s bookkeeping, and ``create_dataloaders`` unchanged when the new arguments keep their defaults."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rovit_hip.augment import (IMAGENET_MEAN, IMAGENET_STD, ROW, AugmentConfig, DeviceImageStore, augment_reference, colour_matrix,
                               draw_params_reference, sample_grid)

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
SEVERITY = {n: i for i, n in enumerate(CLASS_NAMES)}
FULL = AugmentConfig(hflip=0.5, vflip=0.5, scale=(0.25, 1.0), ratio=(3 / 4, 4 / 3), rotate_deg=30.0, brightness=0.4, contrast=0.4,
                     saturation=0.4, hue=0.1)
MEAN = torch.tensor(IMAGENET_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
STD = torch.tensor(IMAGENET_STD, dtype=torch.float64).view(1, 3, 1, 1)


def noise(n, h, w, seed=0):
    return torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def rows(n, **kw):
    """n identity rows with the named columns overridden."""
    p = torch.zeros(n, ROW, dtype=torch.float64)
    p[:, 2] = 1.0            # area
    p[:, 4:6] = 0.5          # ux, uy
    p[:, 7:10] = 1.0         # brightness, contrast, saturation
    names = ('flip_h', 'flip_v', 'area', 'log_ratio', 'ux', 'uy', 'theta', 'brightness', 'contrast', 'saturation', 'hue')
    for k, v in kw.items():
        p[:, names.index(k)] = torch.as_tensor(v, dtype=torch.float64)
    return p


def plain(u8):
    return (u8.double() / 255 - MEAN) / STD


def test_geometry_equals_grid_sample_border_on_random_rows():
    src = noise(6, 37, 53, seed=1)
    idx = [5, 0, 3, 3, 1, 4, 2, 0]
    p = torch.from_numpy(draw_params_reference(idx, FULL, seed=11, epoch=2)).double()
    p[:, 7:10], p[:, 10] = 1.0, 0.0                                   # geometry only
    Ho, Wo = 32, 40
    got = augment_reference(src, idx, p, (Ho, Wo))
    sx, sy = sample_grid(p, (37, 53), (Ho, Wo))
    grid = torch.stack([(2 * sx + 1) / 53 - 1, (2 * sy + 1) / 37 - 1], dim=-1)     # align_corners=False: pixel centre k <-> (2k + 1)/size - 1
    want = F.grid_sample(src[idx].double() / 255, grid, mode='bilinear', padding_mode='border', align_corners=False)
    assert float((got - (want - MEAN) / STD).abs().max()) < 1e-10
    assert float(p[:, 6].abs().max()) > 0.1 and float(p[:, 2].min()) < 0.6     # the rows do rotate and crop


def test_identity_and_flips_are_known_answers():
    src = noise(3, 20, 28, seed=2)
    idx = [2, 0, 1]
    ident = augment_reference(src, idx, rows(3), (20, 28))
    assert float((ident - plain(src[idx])).abs().max()) < 1e-12
    assert float((augment_reference(src, idx, rows(3, flip_h=1.0), (20, 28)) - ident.flip(-1)).abs().max()) < 1e-12
    assert float((augment_reference(src, idx, rows(3, flip_v=1.0), (20, 28)) - ident.flip(-2)).abs().max()) < 1e-12
    # ux, uy do not matter when nothing is cropped
    assert float((augment_reference(src, idx, rows(3, ux=0.1, uy=0.9), (20, 28)) - ident).abs().max()) < 1e-12


def test_quarter_turn_is_rot90_counter_clockwise():
    src = noise(2, 24, 24, seed=3)
    got = augment_reference(src, [0, 1], rows(2, theta=math.pi / 2), (24, 24))
    assert float((got - torch.rot90(plain(src), 1, (-2, -1))).abs().max()) < 1e-10
    back = augment_reference(src, [0, 1], rows(2, theta=-math.pi / 2), (24, 24))
    assert float((back - torch.rot90(plain(src), -1, (-2, -1))).abs().max()) < 1e-10


def test_upscaling_by_two_is_bilinear_interpolate():
    src = noise(2, 16, 20, seed=4)
    got = augment_reference(src, [1, 0], rows(2), (32, 40))
    want = F.interpolate(src[[1, 0]].double() / 255, size=(32, 40), mode='bilinear', align_corners=False)
    assert float((got - (want - MEAN) / STD).abs().max()) < 1e-12


def test_crop_window_follows_area_ratio_and_offsets():
    """area = 1/4 at ratio 1 with ux = uy = 0 is the top-left quarter: the corners of the sampling grid sit half an output pixel inside it."""
    p = rows(1, area=0.25, ux=0.0, uy=0.0)
    sx, sy = sample_grid(p, (40, 60), (10, 10))
    assert abs(float(sx[0, 0, 0]) - (0.5 * 30 / 10 - 0.5)) < 1e-12 and abs(float(sx[0, 0, -1]) - (30 - 0.5 * 30 / 10 - 0.5)) < 1e-12
    assert abs(float(sy[0, 0, 0]) - (0.5 * 20 / 10 - 0.5)) < 1e-12 and abs(float(sy[0, -1, 0]) - (20 - 0.5 * 20 / 10 - 0.5)) < 1e-12
    # a ratio that would leave the image is clipped to it (no retry loop): w = min(Ws, ...)
    sx, _ = sample_grid(rows(1, area=1.0, log_ratio=math.log(4 / 3)), (40, 60), (10, 10))
    assert abs(float(sx[0, 0, -1] - sx[0, 0, 0]) - 60 * 9 / 10) < 1e-12


def test_colour_matrix_known_answers():
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    assert float((colour_matrix(one, zero)[0] - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12
    s, h = torch.tensor([0.7], dtype=torch.float64), torch.tensor([0.13], dtype=torch.float64)
    assert float((colour_matrix(s, h + 1.0) - colour_matrix(s, h)).abs().max()) < 1e-12          # hue = 1 is a full turn
    grey = colour_matrix(zero, torch.tensor([0.3], dtype=torch.float64))[0]
    luma = torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64)
    assert float((grey - luma.expand(3, 3)).abs().max()) < 1e-12                                  # s = 0: every channel is the luma
    # a hue turn keeps the luma and is not the identity
    turned = colour_matrix(one, torch.tensor([0.25], dtype=torch.float64))[0]
    assert float((luma @ turned - luma).abs().max()) < 1e-12 and float((turned - torch.eye(3, dtype=torch.float64)).abs().max()) > 0.3


def test_saturation_zero_gives_three_equal_luma_channels():
    src = noise(1, 8, 12, seed=5)
    got = augment_reference(src, [0], rows(1, saturation=0.0), (8, 12)) * STD + MEAN
    luma = (src.double() / 255 * torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64).view(1, 3, 1, 1)).sum(1, keepdim=True)
    assert float((got - luma.expand(-1, 3, -1, -1)).abs().max()) < 1e-12


def test_brightness_and_contrast_on_hand_made_pixels():
    src = torch.tensor([0, 51, 102, 204, 255, 128, 64, 32], dtype=torch.uint8).view(1, 1, 2, 4).expand(1, 3, 2, 4).contiguous()
    v = src.double() / 255
    for b, c in ((1.3, 1.0), (1.0, 0.6), (0.8, 1.4), (1.4, 1.4)):
        got = augment_reference(src, [0], rows(1, brightness=b, contrast=c), (2, 4)) * STD + MEAN
        want = (b * (0.5 + c * (v - 0.5))).clamp(0, 1)                      # pivot 0.5, contrast first, ONE clamp at the end
        assert float((got - want).abs().max()) < 1e-12
    # 255 at brightness 1.4 saturates, 0 at contrast 1.4 clamps at 0: the clamp is exercised
    got = augment_reference(src, [0], rows(1, brightness=1.4, contrast=1.4), (2, 4)) * STD + MEAN
    assert float(got.max()) == 1.0 and float(got.min()) == 0.0


def test_reference_in_fp32_stays_close_to_fp64():
    src = noise(2, 64, 64, seed=6)
    p = torch.from_numpy(draw_params_reference([0, 1], FULL, 3, 0))
    d = augment_reference(src, [0, 1], p, (64, 64), dtype=torch.float32).double() - augment_reference(src, [0, 1], p, (64, 64))
    assert float(d.abs().max()) < 4e-4


def test_draws_lie_in_their_ranges_and_flips_follow_u():
    from oracle.philox import philox4x32_10
    idx = np.arange(5000)
    p = draw_params_reference(idx, FULL, seed=0x1234567890AB, epoch=(1 << 32) + 7)
    assert p.dtype == np.float32 and p.shape == (5000, ROW)
    lo = [0, 0, 0.25, math.log(3 / 4), 0, 0, -math.radians(30), 0.6, 0.6, 0.6, -0.1, 0]
    hi = [1, 1, 1.0, math.log(4 / 3), 1, 1, math.radians(30), 1.4, 1.4, 1.4, 0.1, 0]
    for k in range(ROW):
        assert p[:, k].min() >= np.float32(lo[k]) - 1e-6 and p[:, k].max() <= np.float32(hi[k]) + 1e-6, k
        if k not in (0, 1, 11):
            assert p[:, k].max() - p[:, k].min() > 0.9 * (hi[k] - lo[k]), k           # and fill them
    assert set(np.unique(p[:, 0])) == {0.0, 1.0} and 0.45 < p[:, 0].mean() < 0.55 and 0.45 < p[:, 1].mean() < 0.55
    # flips are exactly u < p for the fp32 u of word x / y of round 0
    n = idx.size
    seed, epoch = 0x1234567890AB, (1 << 32) + 7
    w = philox4x32_10([idx, np.zeros(n), np.full(n, epoch & 0xFFFFFFFF), np.full(n, epoch >> 32)], [seed & 0xFFFFFFFF, seed >> 32])
    for col, prob in ((0, 0.3), (1, 0.8)):
        q = draw_params_reference(idx, AugmentConfig(hflip=0.3, vflip=0.8), seed, epoch)
        u = (w[col] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        assert np.array_equal(q[:, col], (u < np.float32(prob)).astype(np.float32))
    # the default config draws nothing but the horizontal flip; identity draws nothing at all
    d = draw_params_reference(idx, AugmentConfig(), 5, 1)
    assert np.array_equal(d[:, 1:4], np.tile(np.float32([0, 1, 0]), (n, 1))) and np.array_equal(d[:, 6:11], np.tile(np.float32([0, 1, 1, 1, 0]), (n, 1)))
    assert not draw_params_reference(idx, AugmentConfig.identity(), 5, 1)[:, :2].any()


def test_draws_depend_on_store_index_seed_and_epoch_only():
    idx = np.array([7, 3, 3, 100000, 0, 2 ** 31 + 5, 12])
    p = draw_params_reference(idx, FULL, 9, 4)
    perm = np.array([4, 0, 6, 2, 1, 5, 3])
    assert np.array_equal(draw_params_reference(idx[perm], FULL, 9, 4), p[perm])
    assert np.array_equal(np.concatenate([draw_params_reference(idx[:3], FULL, 9, 4), draw_params_reference(idx[3:], FULL, 9, 4)]), p)
    assert np.array_equal(p[1], p[2]) and not np.array_equal(p[0], p[1])
    assert np.array_equal(draw_params_reference(torch.as_tensor(idx), FULL, 9, 4), p)
    for other in (draw_params_reference(idx, FULL, 9, 5), draw_params_reference(idx, FULL, 10, 4), draw_params_reference(idx, FULL, 9, 4 + (1 << 32)),
                  draw_params_reference(idx, FULL, 9 + (1 << 32), 4)):
        assert not np.isclose(other[:, 2:11], p[:, 2:11]).all(axis=1).any()


def test_config_validation_is_loud():
    from rovit_hip import RovitHipError
    for bad in (dict(scale=(0.5, 0.2)), dict(scale=(0.0, 1.0)), dict(scale=(0.5, 1.5)), dict(hflip=1.5), dict(vflip=-0.1), dict(ratio=(2.0, 1.0)),
                dict(hue=-0.1), dict(rotate_deg=float('nan'))):
        with pytest.raises(RovitHipError):
            AugmentConfig(**bad).validate()
    AugmentConfig().validate(), FULL.validate(), AugmentConfig.identity().validate()
    from data.transforms import device_augmentation
    assert device_augmentation(hue=0.1, scale=(0.5, 1.0)) == AugmentConfig(hue=0.1, scale=(0.5, 1.0))
    c = FULL.to_c()
    assert abs(c.theta_max - math.radians(30)) < 1e-7 and abs(c.log_ratio_lo - math.log(0.75)) < 1e-7 and c.hue == np.float32(0.1)


def _cpu_store(n=23, seed=3):
    from data.dataset import RoseLeafDataset
    ds = RoseLeafDataset(None, CLASS_NAMES, SEVERITY, None, 'augmented', synthetic=n, seed=seed, device=torch.device('cpu'), materialize=False)
    return DeviceImageStore.synthetic(ds.labels, ds.severities, 'cpu', size=(8, 8), seed=seed, dataset=ds), ds


def test_store_on_the_cpu_holds_bytes_but_has_no_cpu_path():
    from rovit_hip import RovitHipError
    store, ds = _cpu_store()
    assert len(store) == 23 and store.images.dtype == torch.uint8 and store.nbytes == 23 * 3 * 64 + 2 * 23 * 8
    assert store.dataset is ds and ds.images is None and torch.equal(store.severities, store.labels)
    assert torch.equal(DeviceImageStore.synthetic(ds.labels, ds.severities, 'cpu', (8, 8), seed=3).images, store.images)     # seeded
    assert 100 < float(store.images.float().mean()) < 155 and int(store.images.max()) > 250 and int(store.images.min()) < 5
    with pytest.raises(RovitHipError):
        store.batch([0, 1])
    with pytest.raises(RovitHipError):
        DeviceImageStore(torch.zeros(2, 3, 4, 4), ds.labels[:2], ds.severities[:2])             # not uint8
    with pytest.raises(RovitHipError):
        store.upload_indices([0, 23])
    with pytest.raises(RuntimeError):
        ds[0]
    # the labels-only dataset draws the labels the fp32 synthetic dataset draws
    from data.dataset import RoseLeafDataset
    assert torch.equal(RoseLeafDataset(None, CLASS_NAMES, SEVERITY, synthetic=23, seed=3).labels, ds.labels)


def test_loader_bookkeeping_on_a_cpu_built_index_list():
    from torch.utils.data import Subset
    from data.dataset import DeviceAugmentLoader, RoseLeafDataset
    store, ds = _cpu_store()
    idx = [22, 0, 5, 7, 9, 11, 13, 2, 4, 6]
    ld = DeviceAugmentLoader(store, idx, 4, True, FULL, seed=5)
    assert len(ld) == 3 and len(DeviceAugmentLoader(store, idx, 4, True, FULL, 5, drop_last=True)) == 2
    assert len(DeviceAugmentLoader(store, idx, 1, False)) == 10 and len(DeviceAugmentLoader(store, idx, 64, False)) == 1
    assert isinstance(ld.dataset, Subset) and isinstance(ld.dataset.dataset, RoseLeafDataset) and ld.dataset.indices == idx
    assert ld.dataset.dataset.get_class_weights().shape == (4,)
    assert DeviceAugmentLoader(store, idx, 4, False).config == AugmentConfig()
    # the order is a function of (seed, epoch); unshuffled loaders keep the list
    o0, o1 = ld.epoch_order(0), ld.epoch_order(1)
    assert sorted(o0.tolist()) == sorted(idx) and not torch.equal(o0, o1) and torch.equal(ld.epoch_order(0), o0)
    assert torch.equal(DeviceAugmentLoader(store, idx, 4, True, FULL, seed=5).epoch_order(1), o1)
    assert not torch.equal(DeviceAugmentLoader(store, idx, 4, True, FULL, seed=6).epoch_order(0), o0)
    assert DeviceAugmentLoader(store, idx, 4, False).epoch_order(3).tolist() == idx
    # every __iter__ is a new epoch (the generator body needs the device: it raises at the first batch here, after the counter moved)
    from rovit_hip import RovitHipError
    assert ld.epoch == 0
    for want in (1, 2):
        with pytest.raises(RovitHipError):
            next(iter(ld))
        assert ld.epoch == want
    ld.set_epoch(7)
    with pytest.raises(RovitHipError):
        next(iter(ld))
    assert ld.epoch == 8
    with pytest.raises(IndexError):
        DeviceAugmentLoader(store, [0, 23], 4, False)
    with pytest.raises(RovitHipError):
        DeviceAugmentLoader(store, idx, 4, False, AugmentConfig(scale=(0.5, 0.2)))


def test_create_dataloaders_defaults_are_the_old_behaviour():
    from data.dataset import DeviceAugmentLoader, DeviceBatchLoader, create_dataloaders
    from data.transforms import augmented_transforms, original_transforms
    kw = dict(augmented_root='nope/a', original_root='nope/o', class_names=CLASS_NAMES, severity_map=SEVERITY, batch_size=8, seed=3, synthetic=40,
              device=torch.device('cpu'))
    old = create_dataloaders(augmented_transform=original_transforms(), original_transform=original_transforms(), **kw)
    new = create_dataloaders(augmented_transform=original_transforms(), original_transform=original_transforms(), device_cache=False,
                             device_augment=None, store_size=None, **kw)
    for a, b in zip(old, new):
        assert type(a) is DeviceBatchLoader and type(b) is DeviceBatchLoader and len(a) == len(b)
        (xa, ca, sa), (xb, cb, sb) = next(iter(a)), next(iter(b))
        assert torch.equal(xa, xb) and torch.equal(ca, cb) and torch.equal(sa, sb) and xa.dtype == torch.float32
    # the first training batch is what the parent's formula gives: normalised randn images of the seeded split, in the seeded order
    base = old[0].dataset.dataset
    order = torch.as_tensor(old[0].dataset.indices)[torch.randperm(len(old[0].dataset), generator=torch.Generator().manual_seed(3))]
    x, c, _ = next(iter(create_dataloaders(augmented_transform=original_transforms(), **kw)[0]))
    assert torch.equal(x, original_transforms()(base.images[order[:8]])) and torch.equal(c, base.labels[order[:8]])
    assert type(create_dataloaders(augmented_transform=augmented_transforms(), **kw)[0]) is DeviceBatchLoader
    # device_cache=True builds the three store loaders (on the CPU: bookkeeping only)
    tr, va, te = create_dataloaders(device_cache=True, store_size=(16, 20), **kw)
    assert all(type(l) is DeviceAugmentLoader for l in (tr, va, te)) and (len(tr), len(va), len(te)) == (4, 1, 2)
    assert tr.store is va.store and tr.store.images.shape == (40, 3, 16, 20) and te.store.images.shape == (10, 3, 16, 20)
    assert tr.config == AugmentConfig() and va.config == te.config == AugmentConfig.identity() and tr.shuffle and not va.shuffle
    assert tr.dataset.indices == old[0].dataset.indices and torch.equal(tr.dataset.dataset.labels, base.labels)
    custom = create_dataloaders(device_cache=True, device_augment=FULL, store_size=(8, 8), **kw)[0]
    assert custom.config == FULL
