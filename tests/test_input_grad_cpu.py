"""CPU tests of the image gradients (rovit_hip/input_grad.py): input_gradients refuses every bad argument before it touches the model or
launches anything, the fp64 integrated-gradients oracle the GPU tests use agrees with a closed form, and the C entries reject bad
arguments before anything is launched."""
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


def _refused(m, x, match, **kw):
    from rovit_hip import RovitHipError
    with pytest.raises(RovitHipError, match=match):
        m.input_gradients(x, **kw)


def test_input_gradients_refuses_bad_arguments_before_touching_the_model():
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False)
    x = torch.zeros(2, 3, 224, 224, requires_grad=True)
    flags = [p.requires_grad for p in m.parameters()]
    _refused(m, x, 'GPU')                                               # the valid call: the CPU tensor is what is refused
    _refused(m, x, 'GPU', target='kan_severity', steps=4, baseline=torch.ones(3, 1, 1), chunk=3)
    _refused(m, torch.zeros(2, 3, 224, 225), 'expects')
    _refused(m, torch.zeros(0, 3, 224, 224), 'empty')
    _refused(m, torch.zeros(2, 3, 224, 224, dtype=torch.int32), 'floating point')
    _refused(m, [x], 'expects')
    for bad in (-1, 1.5, True, '2', None):
        _refused(m, x, 'steps', steps=bad)
    for bad in (0, -3, 2.0, False):
        _refused(m, x, 'chunk', chunk=bad)
    _refused(m, x, 'baseline', baseline=torch.zeros(2, 3, 224, 224))    # steps == 0: no baseline
    _refused(m, x, 'broadcast', steps=2, baseline=torch.zeros(3, 3, 224, 224))
    _refused(m, x, 'broadcast', steps=2, baseline=torch.zeros(2, 3, 224))
    _refused(m, x, 'broadcast', steps=2, baseline=torch.zeros(1, 3, 224, 224, 1))
    _refused(m, x, 'floating-point', steps=2, baseline=torch.zeros(2, 3, 224, 224, dtype=torch.long))
    for bad in ('severity', 'CLASS', 3):
        _refused(m, x, 'unknown target|target must be', target=bad)
    _refused(m, x, 'one target per call', target=['mu', 'log_var'])
    _refused(m, x, 'class_idx', target='mu', class_idx=1)
    _refused(m, x, 'class_idx', class_idx=4)
    _refused(m, x, 'class_idx', class_idx=torch.tensor([0, 1, 2]))
    _refused(m, x, 'class_idx', class_idx=torch.tensor([0.0, 1.0]))
    for stage, bad in ((1, 'ordinal_severity'), (2, 'mu'), (2, 'log_var'), (3, 'kan_severity')):
        m.curriculum_stage = stage
        _refused(m, x, 'curriculum stage', target=bad)
    m.curriculum_stage = 4
    assert all(p.grad is None for p in m.parameters()) and x.grad is None
    assert [p.requires_grad for p in m.parameters()] == flags
    assert m.backbone.model._engine is None          # nothing was prepared


def test_input_gradients_refuses_heads_outside_the_fused_head_phase():
    from models.rovit_kan import RoViTKAN
    x = torch.zeros(1, 3, 224, 224)
    _refused(RoViTKAN(pretrained=False, hidden_dim=130), x, 'head phase')
    _refused(RoViTKAN(pretrained=False, num_classes=9), x, 'head phase')
    wide = RoViTKAN(pretrained=False, kan_layers=[192, 128, 1])
    _refused(wide, x, 'hook recipe', target='kan_severity')
    _refused(wide, x, 'head phase', target='mu')                   # stage 4 runs the KAN stack in the head phase too
    wide.curriculum_stage = 3
    _refused(wide, x, 'GPU', target='mu')


def test_fp32_precision_refuses_images_that_require_grad():
    from models.backbone import DeiTTiny
    from rovit_hip import RovitHipError
    vit = DeiTTiny(depth=1)
    vit.precision = 'fp32'
    for p in vit.parameters():
        p.requires_grad_(False)
    with pytest.raises(RovitHipError, match='no gradient with respect to the images'):
        vit(torch.zeros(1, 3, 224, 224, requires_grad=True))


@pytest.mark.parametrize('steps', [1, 3, 8, 32])
def test_ig_reference_against_closed_form(steps):
    """f(x) = sum a x^2 + b x per sample: the right Riemann sum of the straight-line path from x' has a closed form."""
    from rovit_hip.input_grad import ig_reference
    g = torch.Generator().manual_seed(steps)
    a = torch.randn(5, 7, dtype=torch.float64, generator=g)
    b = torch.randn(5, 7, dtype=torch.float64, generator=g)
    x = torch.randn(4, 5, 7, dtype=torch.float64, generator=g)
    xb = torch.randn(1, 5, 7, dtype=torch.float64, generator=g)
    f = lambda t: (a * t * t + b * t).flatten(1).sum(1)
    got = ig_reference(f, x, xb.expand_as(x), steps)
    d = x - xb
    # grad at xb + (s/m) d is 2a(xb + (s/m) d) + b; the mean over s = 1..m of s/m is (m + 1) / (2m)
    want = d * (2 * a * xb + b + 2 * a * d * (steps + 1) / (2 * steps))
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    if steps == 32:         # completeness gap of the right rule on a quadratic: sum a d^2 / m
        gap = (got.flatten(1).sum(1) - (f(x) - f(xb.expand_as(x))))
        assert torch.allclose(gap, (a * d * d).flatten(1).sum(1) / steps, rtol=1e-10, atol=1e-10)


def test_c_entries_reject_bad_arguments(native):
    lib = native.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    dg = lib.rovit_patch_embed_dgrad
    assert dg(None, 192, p, p, 1, 1, 1.0, 0, None) != 0
    assert dg(p, 192, p, p, 0, 1, 1.0, 0, None) != 0
    assert dg(p, 192, p, p, 1, 0, 1.0, 0, None) != 0
    assert dg(p, 100, p, p, 1, 1, 1.0, 0, None) != 0
    assert dg(ctypes.c_void_p(p.value + 2), 192, p, p, 1, 1, 1.0, 0, None) != 0
    assert b'patch_embed_dgrad' in lib.rovit_last_error_string()
    bi = lib.rovit_vit_backward_input
    n = lib.rovit_vit_num_params(2)
    params = (ctypes.c_void_p * n)(*([p.value] * n))
    # bad ranges and shapes are refused before any launch
    assert bi(p, p, params, p, p, None, 4, 2, 1, 1, 0, None, p, 1, 1.0, 0) != 0          # d_images with a range that ends above block 0
    assert b'block 0' in lib.rovit_last_error_string()
    assert bi(p, p, params, p, p, None, 4, 2, 1, 0, 0, None, p, 3, 1.0, 0) != 0          # batch 4 is not a multiple of 3 copies
    assert b'multiple' in lib.rovit_last_error_string()
    assert bi(p, p, params, p, p, None, 4, 2, 1, 0, 0, None, ctypes.c_void_p(p.value + 4), 1, 1.0, 0) != 0
    assert bi(p, p, params, p, p, None, 4, 2, 2, 0, 0, None, None, 1, 1.0, 0) != 0       # bad range
    assert lib.rovit_vit_backward(p, p, params, p, p, None, 4, 2, 1, 0, 0, None) != 0    # the old entry still needs grads
    assert b'null grads' in lib.rovit_last_error_string()
