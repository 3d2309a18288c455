"""GPU tests of the corruption kernels (csrc/corrupt.hip), of ``rovit_hip.corrupt.corrupt`` on them and of
``Evaluator.evaluate_corruptions``.

Oracle: ``corrupt_reference`` (numpy: fp64, int64 for ``jpeg`` and the integer sums; pinned on the CPU in tests/test_corrupt_cpu.py).
Stores, index lists and the bounds with their derivation are in tests/corrupt_cases.py: per family, 4x the largest deviation of an
fp32 numpy evaluation of the same formulas from fp64 (noise 1.44e-5, photometric 3.44e-6, stencil 6.0e-5, cell 1.8e-6), max-abs on
the normalised output with no pixel excluded; ``jpeg`` bit for bit on the uint8 output and within 1e-6 on the fp32 one;
``impulse_noise`` with the exact set of replaced pixels.  The kernels' measured distances are in DESIGN.md section 2."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import corrupt_cases as cc  # noqa: E402
from oracle import ref_cpu  # noqa: E402  (checker only)
from rovit_hip.corrupt import CORRUPTIONS, corrupt_reference  # noqa: E402

pytestmark = pytest.mark.gpu

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]


def dev():
    return torch.device('cuda:0')


def make_store(shape):
    from rovit_hip.augment import DeviceImageStore
    labels = torch.arange(shape[0]) % 4
    return DeviceImageStore(torch.from_numpy(cc.store_images(shape).copy()).to(dev()), labels, (labels + 1) % 4)


@pytest.mark.parametrize('name', CORRUPTIONS)
@pytest.mark.parametrize('shape', cc.SHAPES, ids=cc.shape_id)
def test_kernel_matches_the_reference(shape, name):
    store, idx = make_store(shape), list(cc.INDICES[shape])
    for severity in cc.SEVERITIES:
        out, u8 = store.corrupt(idx, name, severity, seed=cc.SEED, return_u8=True)
        assert out.shape == (len(idx), 3) + shape[1:] and out.dtype == torch.float32 and u8.dtype == torch.uint8 and u8.shape == out.shape
        want, want_u8 = cc.reference(shape, name, severity)
        err = float(np.abs(out.double().cpu().numpy() - want).max())
        bound = cc.JPEG_FP32_BOUND if name == 'jpeg' else cc.BOUND[cc.FAMILY[name]]
        print(f'corrupt {name} severity {severity} {cc.shape_id(shape)}: max-abs error {err:.3e} (bound {bound:.2e})')
        assert err <= bound, (name, severity, err, bound)
        if name in ('jpeg', 'impulse_noise'):          # integer codec; exact mask on exactly representable levels
            assert np.array_equal(u8.cpu().numpy(), want_u8), (name, severity)
        else:                                          # a level may flip where 255 z + 0.5 sits on an integer; nothing else may differ
            assert int(np.abs(u8.cpu().numpy().astype(np.int64) - want_u8).max()) <= 1
        plain = store.corrupt(idx, name, severity, seed=cc.SEED)          # without out_u8: the same fp32 bits
        assert torch.equal(plain, out)


@pytest.mark.parametrize('name', CORRUPTIONS)
def test_an_image_has_the_same_bits_in_every_batch(name):
    shape = cc.SHAPES[0]
    store = make_store(shape)
    order = [3, 1, 4, 0, 2]
    whole = store.corrupt(order, name, 3, seed=cc.SEED)
    parts = torch.cat([store.corrupt(order[:1], name, 3, seed=cc.SEED), store.corrupt(order[1:3], name, 3, seed=cc.SEED),
                       store.corrupt(order[3:], name, 3, seed=cc.SEED)])
    back = store.corrupt(order[::-1], name, 3, seed=cc.SEED)
    for row, i in enumerate(order):
        assert torch.equal(whole[row], parts[row]) and torch.equal(whole[row], back[len(order) - 1 - row]), (name, i)
    assert not torch.equal(whole[0], whole[1])


def test_contrast_is_bit_identical_from_run_to_run():
    shape = cc.SHAPES[2]
    store, idx = make_store(shape), list(cc.INDICES[shape])
    first = store.corrupt(idx, 'contrast', 5, seed=cc.SEED)
    for _ in range(3):
        assert torch.equal(store.corrupt(idx, 'contrast', 5, seed=cc.SEED), first)


def test_plane_sums_are_the_integer_sums():
    from rovit_hip import native
    for shape in cc.SHAPES:
        store = make_store(shape)
        idx = torch.tensor(list(cc.INDICES[shape]) + [shape[0]], device=dev())          # the last index is outside the store
        sums = torch.full((idx.numel(), 3), -1, dtype=torch.int64, device=dev())
        native.call('rovit_corrupt_stats', native.ptr(store.images), shape[0], shape[1], shape[2], native.ptr(idx), idx.numel(),
                    native.ptr(sums), native.stream_ptr())
        want = cc.store_images(shape).astype(np.int64).sum(axis=(2, 3))[list(cc.INDICES[shape])]
        assert np.array_equal(sums.cpu().numpy()[:-1], want) and sums[-1].tolist() == [0, 0, 0]


@pytest.mark.parametrize('name', ['gaussian_noise', 'contrast', 'defocus_blur', 'pixelate', 'jpeg'])
def test_an_index_outside_the_store_gives_a_nan_image(name):
    shape = cc.SHAPES[0]
    store = make_store(shape)
    good = store.corrupt([1, 0, 2], name, 3, seed=cc.SEED)
    for bad in (shape[0], -1, 2 ** 40):
        idx = torch.tensor([1, bad, 0, 2], dtype=torch.long, device=dev())
        out, u8 = store.corrupt(idx, name, 3, seed=cc.SEED, return_u8=True)
        assert bool(torch.isnan(out[1]).all()) and int(u8[1].max()) == 0
        assert torch.equal(out[[0, 2, 3]], good)


def test_arguments_are_checked_before_any_launch():
    from rovit_hip.native import RovitHipError
    store = make_store(cc.SHAPES[0])
    for name, kw in (('fog', {}), ('jpeg', {'severity': 6}), ('gaussian_blur', {'param': 7.0}), ('pixelate', {'param': 2.5})):
        with pytest.raises(RovitHipError):
            store.corrupt([0], name, **kw)
    with pytest.raises(RovitHipError):
        store.corrupt([cc.SHAPES[0][0]], 'jpeg')                      # a host index list is range-checked on the host
    with pytest.raises(RovitHipError):
        store.corrupt([0], 'jpeg', out=torch.empty(1, 3, 8, 8, device=dev()))


def test_corrupt_loader_yields_the_kernel_batches():
    from data.dataset import DeviceCorruptLoader
    shape = cc.SHAPES[0]
    store = make_store(shape)
    order = [4, 0, 2, 1, 3]
    loader = DeviceCorruptLoader(store, order, 2, 'motion_blur', 3, seed=cc.SEED, labels_on_device=True)
    batches = list(loader)
    assert len(loader) == 3 and [b[0].shape[0] for b in batches] == [2, 2, 1] and batches[0][1].is_cuda
    assert torch.equal(torch.cat([b[0] for b in batches]), store.corrupt(order, 'motion_blur', 3, seed=cc.SEED))
    assert torch.cat([b[1] for b in batches]).tolist() == store.labels[order].tolist()


def test_evaluate_corruptions_matches_a_hand_written_loop(tmp_path):
    from evaluation.evaluator import Evaluator
    from models.rovit_kan import RoViTKAN
    from rovit_hip.augment import DeviceImageStore
    from rovit_hip.evaluation import EvalAccumulator
    model = RoViTKAN(pretrained=False)
    model.load_state_dict(ref_cpu.init_rovit_state(seed=23), strict=True)          # seeded random weights
    model = model.to(dev()).eval()
    labels = torch.arange(16) % 4
    store = DeviceImageStore.synthetic(labels, labels, dev(), size=(224, 224), seed=5)
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=CLASS_NAMES, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    ev = Evaluator(model, None, cfg, dev())
    names, severities, seed = ['gaussian_noise', 'brightness'], (2, 5), 11
    result = ev.evaluate_corruptions(store, corruptions=names, severities=severities, seed=seed, params={'brightness': {2: 0.0}})

    def by_hand(name, severity, param):
        acc, preds, conf = EvalAccumulator(4), [], []
        with torch.no_grad():
            for lo in range(0, 16, 64):
                sel = list(range(16))[lo:lo + 64]
                out = model(store.corrupt(sel, name, severity, seed=seed, param=param))
                acc.update(out, store.labels[sel], store.severities[sel])
                preds.append(out['cls_logits'].argmax(dim=1))
                conf.append(torch.softmax(out['cls_logits'].float(), dim=1).max(dim=1).values)
        return acc.compute(), torch.cat(preds), torch.cat(conf)

    clean_m, clean_pred, _ = by_hand('brightness', 1, 0.0)
    assert result['clean']['n'] == 16 and result['clean']['correct'] == clean_m['correct'] and result['clean']['flip_rate'] == 0.0
    for name in names:
        for s in severities:
            param = 0.0 if (name, s) == ('brightness', 2) else None
            m, pred, conf = by_hand(name, s, param)
            card = result['cells'][name][s]
            for k in ('accuracy', 'macro_f1', 'mae', 'brier_score', 'ece', 'n', 'correct'):
                assert card[k] == m[k], (name, s, k, card[k], m[k])
            assert card['flip_rate'] == float((pred != clean_pred).sum()) / 16.0
            assert card['mean_confidence'] == pytest.approx(float(conf.double().mean()), abs=1e-6)
            assert ('mean_sigma' in card) == ('mean_sigma' in result['clean'])
    same = result['cells']['brightness'][2]                            # c = 0: the clean pass again
    assert all(same[k] == result['clean'][k] for k in ('n', 'correct', 'accuracy', 'macro_f1')) and same['flip_rate'] == 0.0
    for name in names:
        errors = [100.0 - result['cells'][name][s]['accuracy'] for s in severities]
        assert result['error'][name] == pytest.approx(sum(errors) / 2)
        assert result['relative_error'][name] == pytest.approx(result['error'][name] - (100.0 - result['clean']['accuracy']))
    assert result['mean_corruption_error'] == pytest.approx(sum(result['error'].values()) / 2)
    again = ev.evaluate_corruptions(store, corruptions=names, severities=severities, seed=seed, params={'brightness': {2: 0.0}}, baseline=result)
    for name in names:
        if sum(100.0 - result['cells'][name][s]['accuracy'] for s in severities) > 0:
            assert again['ce'][name] == 1.0
        else:
            assert again['ce'][name] is None
    assert (tmp_path / 'corruption_results.txt').read_text().count('gaussian_noise') == 1 and (tmp_path / 'corruption_results.json').exists()
