"""CPU tests of the Grad-CAM++ surface: the C entry points reject bad arguments before anything is launched, the workspace size
query, the Python entry point's argument checks and the drop-in class's non-GPU contract."""
import ctypes

import pytest
import torch


@pytest.fixture(scope='module')
def native():
    from rovit_hip import native as n
    import os
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    n.load()
    return n


def _params(native, depth=12):
    # dummy non-null addresses: every call here is refused by the argument checks, so nothing is ever dereferenced
    n = native.load().rovit_vit_num_params(depth)
    return (ctypes.c_void_p * n)(*([16] * n))


def _gradcam(native, params=True, prep=256, ws=256, feats=8, w1=8, b1=8, w2=8, b2=8, hidden=128, classes=4, logits=8, cam=8,
             batch=2, depth=12):
    native.call('rovit_vit_gradcam', _params(native) if params else None, prep, ws, feats, w1, b1, w2, b2, hidden, classes, None, logits,
                None, cam, None, None, batch, depth, None)


def test_forward_gradcam_rejects_bad_arguments(native):
    for kw, match in (({'images': None}, 'null'), ({'feats': None}, 'null'), ({'prep': None}, 'null'), ({'batch': 0}, 'batch'),
                      ({'depth': 0}, 'depth'), ({'depth': 65}, 'depth')):
        a = {'images': 8, 'prep': 256, 'ws': 256, 'feats': 8, 'batch': 2, 'depth': 12}
        a.update(kw)
        with pytest.raises(native.RovitHipError, match=match):
            native.call('rovit_vit_forward_gradcam', a['images'], _params(native), a['prep'], a['ws'], a['feats'], a['batch'], a['depth'],
                        None)


@pytest.mark.parametrize('kw', [{'params': False}, {'prep': None}, {'ws': None}, {'feats': None}, {'w1': None}, {'b1': None},
                                {'w2': None}, {'b2': None}, {'logits': None}, {'cam': None}])
def test_gradcam_rejects_null_pointers(native, kw):
    with pytest.raises(native.RovitHipError, match='null'):
        _gradcam(native, **kw)


@pytest.mark.parametrize('kw,match', [({'batch': 0}, 'batch'), ({'batch': -3}, 'batch'), ({'depth': 0}, 'depth'), ({'depth': 65}, 'depth'),
                                      ({'hidden': 0}, 'hidden'), ({'hidden': 4096}, 'hidden'), ({'classes': 0}, 'classes'),
                                      ({'classes': 100000}, 'classes')])
def test_gradcam_rejects_bad_shapes(native, kw, match):
    with pytest.raises(native.RovitHipError, match=match):
        _gradcam(native, **kw)


def test_gradcam_map_rejects_bad_arguments(native):
    with pytest.raises(native.RovitHipError, match='null'):
        native.call('rovit_gradcam_map', None, 8, 1, None)
    with pytest.raises(native.RovitHipError, match='null'):
        native.call('rovit_gradcam_map', 8, None, 1, None)
    with pytest.raises(native.RovitHipError, match='batch'):
        native.call('rovit_gradcam_map', 8, 8, 0, None)


def test_gradcam_workspace_size(native):
    lib = native.load()
    g = lib.rovit_vit_gradcam_workspace_bytes(256, 12)
    assert lib.rovit_vit_workspace_bytes(256, 12, 0) <= g < lib.rovit_vit_workspace_bytes(256, 12, 1) / 2
    for b in (1, 7, 64):
        assert lib.rovit_vit_gradcam_workspace_bytes(b, 12) >= lib.rovit_vit_workspace_bytes(b, 12, 0)
    assert lib.rovit_vit_gradcam_workspace_bytes(0, 12) == 0 and lib.rovit_vit_gradcam_workspace_bytes(4, 0) == 0


def test_python_entry_rejects_bad_arguments_before_touching_the_model():
    from rovit_hip import RovitHipError
    from rovit_hip.gradcam import grad_cam_pp
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False)
    x = torch.zeros(2, 3, 224, 224)
    for bad in (-1, 4, 1.5, True, torch.tensor([0, 4]), torch.tensor([0, 1, 2]), torch.tensor([0.0, 1.0]), 'cat'):
        with pytest.raises(RovitHipError, match='class_idx'):
            grad_cam_pp(m, x, class_idx=bad)
    with pytest.raises(RovitHipError, match='GPU'):
        grad_cam_pp(m, x)
    with pytest.raises(RovitHipError, match='GPU'):
        grad_cam_pp(m, x, class_idx=torch.tensor([3, 0]))
    with pytest.raises(RovitHipError, match='224'):
        grad_cam_pp(m, torch.zeros(2, 3, 32, 32))
    assert all(p.grad is None for p in m.parameters())
    assert m.backbone.model._engine is None          # nothing was prepared


def test_drop_in_class_contract_without_a_gpu():
    from explainability import GradCAMPlusPlus
    from models.rovit_kan import RoViTKAN
    from rovit_hip import RovitHipError
    m = RoViTKAN(pretrained=False)
    c = GradCAMPlusPlus(m, device='cpu')
    assert c.model is m and c.device == 'cpu'
    with pytest.raises(NotImplementedError, match='cv2'):
        c.visualize(torch.zeros(1, 3, 224, 224), None)
    with pytest.raises(NotImplementedError, match='cv2'):
        c.overlay_on_image(None, None)
    m.train()
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(RovitHipError):           # no CPU fallback
        c.compute(x)
    assert not m.training and not x.requires_grad   # eval() as the reference; the caller's tensor untouched
