"""CPU tests of the attention-rollout surface: the C entry points reject bad arguments before anything is launched, the
bindings match the header, and the drop-in class keeps the reference's non-GPU contract."""
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


def _forward_rollout(native, head_fusion=0, rollout=8, batch=2, images=8):
    # dummy non-null addresses: every call here is refused by the argument checks, so nothing is ever dereferenced
    params = (ctypes.c_void_p * native.load().rovit_vit_num_params(12))(*([16] * native.load().rovit_vit_num_params(12)))
    native.call('rovit_vit_forward_rollout', images, params, 256, 256, 8, rollout, head_fusion, batch, 12, None)


@pytest.mark.parametrize('head_fusion', [-1, 3, 7])
def test_forward_rollout_rejects_bad_head_fusion(native, head_fusion):
    with pytest.raises(native.RovitHipError, match='head_fusion'):
        _forward_rollout(native, head_fusion=head_fusion)


def test_forward_rollout_rejects_null_pointers(native):
    with pytest.raises(native.RovitHipError, match='null'):
        _forward_rollout(native, rollout=None)
    with pytest.raises(native.RovitHipError, match='null'):
        _forward_rollout(native, images=None)


def test_forward_rollout_rejects_empty_batch(native):
    with pytest.raises(native.RovitHipError, match='batch'):
        _forward_rollout(native, batch=0)


def test_rollout_map_rejects_bad_arguments(native):
    with pytest.raises(native.RovitHipError, match='null'):
        native.call('rovit_rollout_map', None, 8, 1, None)
    with pytest.raises(native.RovitHipError, match='null'):
        native.call('rovit_rollout_map', 8, None, 1, None)
    with pytest.raises(native.RovitHipError, match='batch'):
        native.call('rovit_rollout_map', 8, 8, 0, None)


def test_python_rollout_rejects_unknown_fusion_before_touching_the_model():
    from rovit_hip import RovitHipError
    from rovit_hip.rollout import attention_rollout
    with pytest.raises(RovitHipError, match='head_fusion'):
        attention_rollout(None, torch.zeros(1, 3, 224, 224), head_fusion='bogus')


def test_drop_in_class_contract_without_a_gpu():
    from explainability import ViTAttentionRollout
    from models.rovit_kan import RoViTKAN
    r = ViTAttentionRollout(RoViTKAN(pretrained=False), device='cpu', discard_ratio=0.5)
    assert r.discard_ratio == 0.5 and r.device == 'cpu'
    with pytest.raises(NotImplementedError, match='cv2'):
        r.visualize(torch.zeros(1, 3, 224, 224), None)
    with pytest.raises(NotImplementedError, match='cv2'):
        r.overlay_on_image(None, None)
    # no CPU fallback: the product path refuses host tensors
    from rovit_hip import RovitHipError
    with pytest.raises(RovitHipError):
        r.generate(torch.zeros(1, 3, 224, 224))
