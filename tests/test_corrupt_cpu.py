"""CPU tests of the corruption reference (rovit_hip/corrupt.py: ``corrupt_reference``, the oracle of tests/test_gpu_corrupt.py), of the
CPU path of ``corrupt`` and of ``DeviceCorruptLoader`` on a CPU store.

The integer JPEG rule is pinned to PIL's encoder (``quality=q, subsampling=0``): the mean absolute difference must be at most 1.5
levels and at most a fifth of the codec's own distortion, mean |PIL - source|.  Measured with these two images: 0.10 to 0.32 levels on
the smooth one (distortion 6.0 to 15.9) and 0.75 to 1.45 on the noise one (distortion 12.2 to 61.0)."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corrupt_cases as cc  # noqa: E402
from rovit_hip import corrupt as K  # noqa: E402
from rovit_hip.augment import IMAGENET_MEAN, IMAGENET_STD, DeviceImageStore  # noqa: E402
from rovit_hip.native import RovitHipError  # noqa: E402

BLURS = ('gaussian_blur', 'defocus_blur', 'motion_blur')


def plain(images_u8, idx):
    mean, std = (np.array(t, dtype=np.float64).reshape(1, 3, 1, 1) for t in (IMAGENET_MEAN, IMAGENET_STD))
    return (np.asarray(images_u8)[list(idx)].astype(np.float64) / 255.0 - mean) / std


def pin_images():
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:64, 0:64]
    smooth = np.stack([128 + 90 * np.sin(xx / 9.0) * np.cos(yy / 13.0), 128 + 80 * np.cos(xx / 7.0 + yy / 11.0), 100 + 60 * np.sin(yy / 5.0)])
    smooth = np.clip(smooth + rng.normal(0.0, 8.0, (3, 64, 64)), 0, 255).astype(np.uint8)
    return {'smooth': smooth, 'noise': rng.integers(0, 256, (3, 64, 64), dtype=np.uint8)}


@pytest.mark.parametrize('which', ['smooth', 'noise'])
@pytest.mark.parametrize('quality', [80, 30, 18, 12, 8, 5])
def test_jpeg_rule_is_pinned_to_pil(which, quality):
    from PIL import Image
    img = pin_images()[which]
    buf = io.BytesIO()
    Image.fromarray(img.transpose(1, 2, 0)).save(buf, 'JPEG', quality=quality, subsampling=0)
    pil = np.asarray(Image.open(buf).convert('RGB')).transpose(2, 0, 1).astype(np.int64)
    mine = K.jpeg_levels(img[None], quality)[0].astype(np.int64)
    diff, distortion = float(np.abs(mine - pil).mean()), float(np.abs(pil - img.astype(np.int64)).mean())
    print(f'jpeg {which} q={quality}: mean |rule - PIL| {diff:.3f} levels, mean |PIL - source| {distortion:.2f}')
    assert diff <= 1.5 and diff <= distortion / 5.0, (diff, distortion)


@pytest.mark.parametrize('name,param', [('brightness', 0.0), ('contrast', 1.0), ('saturate', 1.0), ('pixelate', 1.0), ('gaussian_noise', 0.0)])
def test_identity_parameters_give_the_plain_normalisation(name, param):
    images, idx = cc.store_images(cc.SHAPES[0]), cc.INDICES[cc.SHAPES[0]]
    out = K.corrupt_reference(images, idx, name, seed=cc.SEED, param=param)
    assert out.dtype == np.float64 and np.array_equal(out, plain(images, idx))


@pytest.mark.parametrize('name', BLURS)
@pytest.mark.parametrize('severity', [1, 5])
def test_blur_of_a_constant_image_is_that_constant(name, severity):
    images = np.empty((2, 3, 24, 40), np.uint8)
    images[:, 0], images[:, 1], images[:, 2] = 255, 0, 102          # 102 / 255 = 0.4 is no binary fraction
    out = K.corrupt_reference(images, [1, 0], name, severity, seed=3)
    assert np.array_equal(out, plain(images, [1, 0]))


def test_jpeg_of_a_blockwise_constant_image_at_quality_100():
    rng = np.random.default_rng(5)
    coarse = rng.integers(0, 256, (2, 3, 4, 5), dtype=np.uint8)
    images = np.repeat(np.repeat(coarse, 8, axis=2), 8, axis=3)
    levels = K.jpeg_levels(images, 100)
    assert levels.shape == images.shape and levels.dtype == np.uint8
    assert int(np.abs(levels.astype(np.int64) - images.astype(np.int64)).max()) <= 1


def test_jpeg_pads_and_crops_sides_that_are_no_multiple_of_8():
    images, idx = cc.store_images(cc.SHAPES[0]), cc.INDICES[cc.SHAPES[0]]          # 37 x 53
    out, u8 = K.corrupt_reference(images, idx, 'jpeg', 1, return_u8=True)
    assert out.shape == (len(idx), 3, 37, 53) and u8.shape == out.shape and u8.dtype == np.uint8
    # the padded image's own round trip, cropped: the rule of the docstring
    padded = np.pad(images, ((0, 0), (0, 0), (0, 3), (0, 3)), mode='edge')
    assert np.array_equal(u8, K.jpeg_levels(padded, 25)[list(idx)][:, :, :37, :53])
    assert float(np.abs(u8.astype(np.float64) - images[list(idx)]).mean()) > 5.0          # quality 25 on noise does distort


def test_jpeg_intermediates_fit_int32():
    """The kernel computes in int32: the rule evaluated in int32 numpy (which wraps silently) must equal the int64 evaluation on the
    harshest input, saturated binary noise, at the mildest and the harshest quantisation."""
    rng = np.random.default_rng(11)
    images = (rng.integers(0, 2, (2, 3, 64, 64)) * 255).astype(np.uint8)
    for quality in (100, 5):
        assert np.array_equal(K.jpeg_levels(images, quality, dtype=np.int32), K.jpeg_levels(images, quality))


def test_impulse_share_is_binomial():
    images = cc.store_images(cc.SHAPES[1])
    for severity in (1, 5):
        p = K.corruption_param('impulse_noise', severity)
        u8 = K.corrupt_reference(np.full_like(images, 128), [1], 'impulse_noise', severity, seed=9, return_u8=True)[1]
        n = u8.size
        hit = int((u8 != 128).sum())
        assert abs(hit - n * p) <= 5.0 * np.sqrt(n * p * (1 - p)), (hit, n * p)
        assert abs(int((u8 == 0).sum()) - n * p / 2) <= 5.0 * np.sqrt(n * p / 2), 'pepper share'
        assert set(np.unique(u8)) <= {0, 128, 255}


def test_normals_have_zero_mean_and_unit_variance():
    images = np.full((2, 3, 64, 64), 128, np.uint8)
    sigma = 0.1
    out = K.corrupt_reference(images, [1], 'gaussian_noise', seed=21, param=sigma)
    std = np.array(IMAGENET_STD).reshape(1, 3, 1, 1)
    n = (out - plain(images, [1])) * std / float(np.float32(sigma))          # 128/255 +- 5 sigma stays inside [0, 1]: nothing is clamped
    count = n[0, 0].size
    for c in range(3):
        assert abs(float(n[0, c].mean())) <= 5.0 / np.sqrt(count), c
        assert abs(float(n[0, c].var()) - 1.0) <= 5.0 * np.sqrt(2.0 / count), c
    assert abs(float(np.corrcoef(n[0, 0].ravel(), n[0, 1].ravel())[0, 1])) <= 5.0 / np.sqrt(count)          # the cos and sin branches


@pytest.mark.parametrize('name', K.CORRUPTIONS)
def test_an_image_depends_on_the_store_index_alone(name):
    shape = cc.SHAPES[0]
    images = cc.store_images(shape)
    whole, _ = cc.reference(shape, name, 3)
    idx = cc.INDICES[shape]
    perm = [3, 1, 4, 0, 2]
    parts = [K.corrupt_reference(images, perm[:2], name, 3, seed=cc.SEED), K.corrupt_reference(images, perm[2:], name, 3, seed=cc.SEED)]
    by_index = dict(zip(perm, np.concatenate(parts)))
    for row, i in enumerate(idx):
        assert np.array_equal(whole[row], by_index[i]), (name, i)


def test_another_seed_gives_other_noise_and_theta_differs_between_images():
    shape = cc.SHAPES[0]
    images = cc.store_images(shape)
    for name in ('gaussian_noise', 'shot_noise', 'impulse_noise', 'motion_blur'):
        a = K.corrupt_reference(images, [0, 1], name, 3, seed=1)
        b = K.corrupt_reference(images, [0, 1], name, 3, seed=2)
        assert not np.array_equal(a, b), name
    theta = K.motion_theta([0, 1, 2, 3], seed=1)
    assert len(set(theta.tolist())) == 4 and float(theta.min()) >= 0.0 and float(theta.max()) < 2.0 * np.pi


def test_unknown_names_severities_and_parameters_raise():
    images = cc.store_images(cc.SHAPES[0])
    with pytest.raises(RovitHipError):
        K.corrupt_reference(images, [0], 'fog')
    for severity in (0, 6, 2.5, True):
        with pytest.raises(RovitHipError):
            K.corruption_param('jpeg', severity)
    for name, param in (('gaussian_blur', 7.0), ('motion_blur', 2.5), ('pixelate', 0.0), ('jpeg', 0.0), ('shot_noise', 0.0), ('impulse_noise', 1.5),
                        ('defocus_blur', 19.0), ('brightness', float('nan'))):
        with pytest.raises(RovitHipError):
            K.corrupt_reference(images, [0], name, param=param)
    with pytest.raises(RovitHipError):
        K.corrupt_reference(images, [5], 'brightness')
    assert K.CORRUPTIONS.index('jpeg') == 10 and [K.corruption_param('jpeg', s) for s in (1, 5)] == [25.0, 7.0]
    assert all(len(K.SEVERITY_TABLE[n]) == 5 for n in K.CORRUPTIONS) and set(K.SEVERITY_TABLE) == set(K.CORRUPTIONS)


def cpu_store(shape):
    images = torch.from_numpy(cc.store_images(shape).copy())
    labels = torch.arange(shape[0]) % 4
    return DeviceImageStore(images, labels, (labels + 1) % 4)


def test_a_cpu_store_runs_the_reference_through_the_same_entry_point():
    shape = cc.SHAPES[0]
    store = cpu_store(shape)
    out, u8 = store.corrupt(list(cc.INDICES[shape]), 'contrast', 3, seed=cc.SEED, return_u8=True)
    want, want_u8 = cc.reference(shape, 'contrast', 3)
    assert out.dtype == torch.float32 and torch.equal(out, torch.from_numpy(want.copy()).float()) and np.array_equal(u8.numpy(), want_u8)
    with pytest.raises(RovitHipError):
        store.corrupt([shape[0]], 'contrast')


def test_corrupt_loader_on_a_cpu_store():
    from data.dataset import DeviceCorruptLoader
    shape = cc.SHAPES[0]
    store = cpu_store(shape)
    order = [4, 0, 2, 1, 3]
    loader = DeviceCorruptLoader(store, order, 2, 'pixelate', 3, seed=cc.SEED)
    assert len(loader) == 3 and loader.store is store and list(loader.dataset.indices) == order
    batches = list(loader)
    assert [b[0].shape[0] for b in batches] == [2, 2, 1]
    assert torch.cat([b[1] for b in batches]).tolist() == store.labels[order].tolist()          # no shuffle, labels aligned
    assert torch.cat([b[2] for b in batches]).tolist() == store.severities[order].tolist()
    want = K.corrupt_reference(store.images, order, 'pixelate', 3, seed=cc.SEED)
    assert torch.equal(torch.cat([b[0] for b in batches]), torch.from_numpy(want).float())
    assert torch.equal(torch.cat([b[0] for b in loader]), torch.cat([b[0] for b in batches]))          # every pass: the same bits
    with pytest.raises(RovitHipError):
        DeviceCorruptLoader(store, order, 2, 'fog', 3)
    with pytest.raises(RovitHipError):
        DeviceCorruptLoader(store, order, 2, 'jpeg', 6)
    with pytest.raises(IndexError):
        DeviceCorruptLoader(store, [5], 2, 'jpeg', 1)


def test_evaluate_corruptions_needs_a_store():
    from evaluation.evaluator import Evaluator
    ev = Evaluator.__new__(Evaluator)
    ev.test_loader = [(torch.zeros(1, 3, 224, 224), torch.zeros(1), torch.zeros(1))]
    with pytest.raises(RovitHipError, match='device_cache=True'):
        ev.evaluate_corruptions()
