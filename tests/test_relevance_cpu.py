"""CPU tests of the attention relevance (rovit_hip/relevance.py): attention_relevance refuses every bad argument before it touches the
model or launches anything, and the two C entries (rovit_attention_relevance_step, rovit_vit_backward_relevance) reject bad arguments
with an error code before anything is launched."""
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
        m.attention_relevance(x, **kw)


def test_attention_relevance_refuses_bad_arguments_before_touching_the_model():
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False)
    x = torch.zeros(2, 3, 224, 224, requires_grad=True)
    flags = [p.requires_grad for p in m.parameters()]
    _refused(m, x, 'attention_relevance: the images must be on the GPU')      # the valid call: the CPU tensor is what is refused
    _refused(m, x, 'GPU', target='kan_severity', chunk=1, upsample=False, return_values=True)
    _refused(m, torch.zeros(2, 3, 224, 225), 'expects')
    _refused(m, torch.zeros(2, 224, 224), 'expects')
    _refused(m, torch.zeros(0, 3, 224, 224), 'empty')
    _refused(m, torch.zeros(2, 3, 224, 224, dtype=torch.int32), 'floating point')
    _refused(m, [x], 'expects')
    for bad in (0, -3, 2.0, False, None):
        _refused(m, x, 'chunk', chunk=bad)
    for bad in ('severity', 'CLASS', 3):
        _refused(m, x, 'unknown target|target must be', target=bad)
    _refused(m, x, 'one target per call', target=['mu', 'log_var'])
    _refused(m, x, 'one target per call', target=('class',))
    _refused(m, x, 'class_idx', target='mu', class_idx=1)
    for bad in (4, -1, 1.0, True):
        _refused(m, x, 'class_idx', class_idx=bad)
    _refused(m, x, 'class_idx', class_idx=torch.tensor([0, 1, 2]))
    _refused(m, x, 'class_idx', class_idx=torch.tensor([0.0, 1.0]))
    _refused(m, x, 'class_idx', class_idx=torch.tensor([0, 4]))
    for stage, bad in ((1, 'ordinal_severity'), (2, 'mu'), (2, 'log_var'), (3, 'kan_severity')):
        m.curriculum_stage = stage
        _refused(m, x, 'curriculum stage', target=bad)
    m.curriculum_stage = 4
    assert all(p.grad is None for p in m.parameters()) and x.grad is None
    assert [p.requires_grad for p in m.parameters()] == flags
    assert m.backbone.model._engine is None          # nothing was prepared


def test_attention_relevance_refuses_heads_outside_the_fused_head_phase():
    from models.rovit_kan import RoViTKAN
    x = torch.zeros(1, 3, 224, 224)
    _refused(RoViTKAN(pretrained=False, hidden_dim=130), x, 'attention_relevance: the heads / KAN stack are outside')
    _refused(RoViTKAN(pretrained=False, num_classes=9), x, 'head phase')
    wide = RoViTKAN(pretrained=False, kan_layers=[192, 128, 1])
    _refused(wide, x, 'hook recipe', target='kan_severity')
    _refused(wide, x, 'head phase', target='mu')                   # stage 4 runs the KAN stack in the head phase too
    wide.curriculum_stage = 3
    _refused(wide, x, 'GPU', target='mu')


def test_c_entries_reject_bad_arguments(native):
    lib = native.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    st = lib.rovit_attention_relevance_step
    for k in range(5):                                   # qkv, lse2, dout, u, scratch
        args = [p] * 5
        args[k] = None
        assert st(*args, 2, 0, None) != 0
        assert b'null pointer' in lib.rovit_last_error_string()
    for bad in (0, -1):
        assert st(p, p, p, p, p, bad, 0, None) != 0
        assert st(p, p, p, p, p, bad, 1, None) != 0
    assert b'attention_relevance_step' in lib.rovit_last_error_string()
    assert st(ctypes.c_void_p(p.value + 2), p, p, p, p, 1, 0, None) != 0     # qkv / dout 16-byte aligned
    assert st(p, p, ctypes.c_void_p(p.value + 4), p, p, 1, 0, None) != 0
    br = lib.rovit_vit_backward_relevance
    n = lib.rovit_vit_num_params(2)
    params = (ctypes.c_void_p * n)(*([p.value] * n))
    good = [p, params, p, p, 4, 2, 0, p, p, None]          # d_features, params, prep, workspace, batch, depth, mlp_path, rel, scratch
    for k in (0, 1, 2, 3, 7, 8):
        args = list(good)
        args[k] = None
        assert br(*args) != 0
    assert b'null' in lib.rovit_last_error_string()
    for k, bad in ((4, 0), (4, -3), (5, 0), (5, 65), (6, 7)):
        args = list(good)
        args[k] = bad
        assert br(*args) != 0
    assert br(p, params, ctypes.c_void_p(p.value + 8), p, 4, 2, 0, p, p, None) != 0     # prep 16-byte aligned
