"""CPU tests of the deletion / insertion curves (rovit_hip/perturbation.py): patch scores, ranking, step counts and the source rows of
rovit_vit_forward_tokens against hand-written expectations; perturbation_reference against an analytic function whose curves and areas
are known in closed form; every refusal of perturbation_curves before it touches the model or launches anything; the C entries' own
argument checks."""
import ctypes

import numpy as np
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


# ---- scores, ranking, steps ------------------------------------------------------------------------------------------------------

def _np_scores(s):
    """numpy restatement: patch p = 14 i + j covers rows 16 i .. 16 i + 15 and columns 16 j .. 16 j + 15 of every channel."""
    s = np.asarray(s, dtype=np.float64)
    B = s.shape[0]
    if s.shape[1:] == (14, 14) or s.shape[1:] == (196,):
        return s.reshape(B, 196)
    if s.ndim == 3:
        s = s[:, None]
    out = np.zeros((B, 196))
    for i in range(14):
        for j in range(14):
            out[:, 14 * i + j] = s[:, :, 16 * i:16 * i + 16, 16 * j:16 * j + 16].sum(axis=(1, 2, 3))
    return out


@pytest.mark.parametrize('shape', [(3, 14, 14), (3, 196), (3, 224, 224), (3, 3, 224, 224)])
def test_patch_scores_of_every_shape(shape):
    from rovit_hip.perturbation import patch_scores
    s = torch.randn(*shape, generator=torch.Generator().manual_seed(len(shape)))
    got = patch_scores(s)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, 196)
    np.testing.assert_allclose(got.numpy(), _np_scores(s.numpy()), rtol=1e-12, atol=1e-10)
    # a map that is one patch's indicator ranks that patch first
    from rovit_hip.perturbation import patch_order
    one = torch.zeros(1, 224, 224)
    one[0, 16 * 5 + 3, 16 * 7 + 9] = 1.0                  # inside patch 14 * 5 + 7
    assert int(patch_order(one)[0, 0]) == 77


def test_ties_go_to_the_lower_index_and_nan_is_minus_infinity():
    from rovit_hip.perturbation import patch_order
    s = torch.zeros(2, 196)
    s[0, [10, 3, 50]] = 2.0                                   # three-way tie on top
    s[0, 7] = float('nan')
    s[0, 8] = float('-inf')
    s[1] = -1.0
    s[1, 100] = float('nan')
    s[1, 0] = float('inf')
    o = patch_order(s)
    assert o[0, :3].tolist() == [3, 10, 50]
    zeros = [p for p in range(196) if p not in (3, 10, 50, 7, 8)]
    assert o[0, 3:194].tolist() == zeros                      # the remaining zeros in index order
    assert o[0, 194:].tolist() == [7, 8]                      # NaN ties with -inf and goes first by index
    assert o[1, 0] == 0 and o[1, 195] == 100
    assert o[1, 1:195].tolist() == [p for p in range(1, 196) if p != 100]
    # the same rule for a (B,3,224,224) map whose NaN sits in one pixel of one channel
    g = torch.ones(1, 3, 224, 224)
    g[0, 1, 20, 20] = float('nan')                            # patch 14 + 1
    assert int(patch_order(g)[0, 195]) == 15


@pytest.mark.parametrize('steps', [1, 3, 7, 28, 50, 196])
def test_step_counts(steps):
    from fractions import Fraction
    from rovit_hip.perturbation import step_counts
    ks = step_counts(steps)
    assert len(ks) == steps + 1 and ks[0] == 0 and ks[-1] == 196
    assert ks == [int(Fraction(196 * s, steps)) for s in range(steps + 1)]
    assert all(a <= b for a, b in zip(ks, ks[1:]))
    if steps == 28:
        assert ks == list(range(0, 197, 7))
    if steps == 3:
        assert ks == [0, 65, 130, 196]
    if steps == 196:
        assert ks == list(range(197))


# ---- source rows -----------------------------------------------------------------------------------------------------------------

def _rank_of(order):
    from rovit_hip.perturbation import _ranks
    return _ranks(torch.tensor([order]))


def test_source_rows_replace_and_drop_by_hand():
    from rovit_hip.perturbation import perturbed_mask, source_rows
    order = [5, 0, 195, 2] + [p for p in range(196) if p not in (5, 0, 195, 2)]
    rank = _rank_of(order)
    # deletion of 3: patches 5, 0, 195 from the baseline
    m = perturbed_mask(rank, True, 3)
    assert m.sum() == 3 and bool(m[0, 5] & m[0, 0] & m[0, 195])
    src = source_rows(m, 'replace')
    want = [0] + [1 + p for p in range(196)]
    for p in (5, 0, 195):
        want[1 + p] = -2 - p
    assert src.dtype == torch.int32 and src[0].tolist() == want
    assert src[0, 1] == -2 and src[0, 6] == -7 and src[0, 196] == -197
    drop = source_rows(m, 'drop', 197 - 3)
    assert drop[0].tolist() == [0] + [1 + p for p in range(196) if p not in (5, 0, 195)]
    # insertion of 2: everything but 5 and 0 perturbed
    m = perturbed_mask(rank, False, 2)
    assert m.sum() == 194 and not m[0, 5] and not m[0, 0]
    assert source_rows(m, 'drop', 1 + 2)[0].tolist() == [0, 1, 6]
    src = source_rows(m, 'replace')[0].tolist()
    assert src[:3] == [0, 1, -3] and src[6] == 6 and src[196] == -197
    # the endpoints: nothing perturbed is the identity, everything perturbed is the baseline (the class token stays the image's)
    assert source_rows(perturbed_mask(rank, True, 0), 'replace')[0].tolist() == list(range(197))
    assert source_rows(perturbed_mask(rank, True, 196), 'replace')[0].tolist() == [0] + [-1 - r for r in range(1, 197)]
    assert source_rows(perturbed_mask(rank, True, 196), 'drop', 1)[0].tolist() == [0]
    assert source_rows(perturbed_mask(rank, False, 196), 'drop', 197)[0].tolist() == list(range(197))


def test_per_row_masks():
    from rovit_hip.perturbation import _ranks, patch_order, perturbed_mask
    s = torch.randn(4, 196, generator=torch.Generator().manual_seed(3))
    rank = _ranks(patch_order(s))
    order = patch_order(s)
    d = torch.tensor([True, False, True, False])
    k = torch.tensor([0, 5, 100, 196])
    m = perturbed_mask(rank, d, k)
    for i in range(4):
        want = torch.zeros(196, dtype=torch.bool)
        sel = order[i, :int(k[i])] if d[i] else order[i, int(k[i]):]
        want[sel] = True
        assert torch.equal(m[i], want)


# ---- the pixel recipe ------------------------------------------------------------------------------------------------------------

def test_perturbation_reference_on_an_analytic_function():
    """f(x) = sum_p w_p * mean of patch p over x, x = 1, baseline 0: deletion of the k highest-ranked patches leaves the sum of the
    other weights, insertion keeps the k highest; the trapezoid areas follow from the cumulative sums."""
    from rovit_hip.perturbation import NP, perturbation_reference, step_counts, trapezoid_auc
    g = torch.Generator().manual_seed(11)
    B, steps = 3, 7
    w = torch.rand(B, 196, generator=g, dtype=torch.float64)
    x = torch.ones(B, 3, 224, 224, dtype=torch.float64)
    x[1] *= 2.0

    def f(imgs):
        pm = imgs.view(imgs.shape[0], 3, 14, 16, 14, 16).mean(dim=(1, 3, 5)).reshape(imgs.shape[0], 196)
        return (pm * w).sum(1)

    sal = w.view(B, 14, 14)
    fr = torch.tensor([k / NP for k in step_counts(steps)], dtype=torch.float64)
    ks = step_counts(steps)
    top = torch.sort(w, dim=1, descending=True).values
    cum = torch.cat([torch.zeros(B, 1, dtype=torch.float64), top.cumsum(1)], dim=1)        # cum[:, k] = sum of the k highest
    scale = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64).view(B, 1)
    want_del = scale * (cum[:, -1:] - cum[:, ks])
    want_ins = scale * cum[:, ks]
    for base in (torch.zeros(1, 3, 224, 224, dtype=torch.float64), torch.zeros(B, 3, 224, 224, dtype=torch.float64)):
        d = perturbation_reference(f, x, sal, 'deletion', steps, base)
        i = perturbation_reference(f, x, sal, 'insertion', steps, base)
        torch.testing.assert_close(d, want_del, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(i, want_ins, rtol=1e-12, atol=1e-12)
        # closed-form areas: trapezoids over the fractions of the cumulative sums
        a_del = sum((want_del[:, s] + want_del[:, s + 1]) * (fr[s + 1] - fr[s]) / 2 for s in range(steps))
        torch.testing.assert_close(trapezoid_auc(d, fr), a_del, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(trapezoid_auc(d, fr) + trapezoid_auc(i, fr), scale[:, 0] * cum[:, -1], rtol=1e-12, atol=1e-12)
    # a uniform map: deletion in patch-index order (the tie rule), f of a patch indicator weight
    w.fill_(0.0)
    w[:, 0] = 1.0
    d = perturbation_reference(f, x, torch.ones(B, 196, dtype=torch.float64), 'deletion', 196, torch.zeros_like(x))
    assert torch.equal(d[:, 0], scale[:, 0]) and bool((d[:, 1:] == 0).all())


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def _refused(m, x, sal, match, **kw):
    from rovit_hip import RovitHipError
    with pytest.raises(RovitHipError, match=match):
        m.perturbation_curves(x, sal, **kw)


def test_perturbation_curves_refuses_bad_arguments_before_touching_the_model():
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False)
    x = torch.zeros(2, 3, 224, 224, requires_grad=True)
    sal = torch.rand(2, 14, 14)
    flags = [p.requires_grad for p in m.parameters()]
    _refused(m, x, sal, 'perturbation_curves: the images must be on the GPU')       # the valid call: the CPU images are refused
    _refused(m, x, {'a': sal, 'b': torch.rand(2, 224, 224)}, 'GPU', target='mu', perturbation='drop', steps=196)
    _refused(m, x, sal, 'GPU', baseline=torch.zeros(3, 224, 224))
    for bad in (0, 197, -1, 2.0, True, None):
        _refused(m, x, sal, 'steps must be an int in \\[1, 196\\]', steps=bad)
    for bad in ('del', ('deletion', 'deletion'), (), ['insertion', 'erase'], 3):
        _refused(m, x, sal, 'modes', modes=bad)
    for bad in ('blur', None, 'Replace'):
        _refused(m, x, sal, 'perturbation must be one of', perturbation=bad)
    _refused(m, x, sal, "'drop' removes patches .* no baseline", perturbation='drop', baseline=torch.zeros(1, 3, 224, 224))
    _refused(m, x, {'a': sal, 'b': torch.rand(3, 14, 14)}, "saliency 'b' holds 3 maps for 2 images")
    _refused(m, x, torch.rand(1, 196), 'holds 1 maps for 2 images')
    _refused(m, x, {}, 'non-empty')
    _refused(m, x, {1: sal}, 'str keys')
    for bad in (torch.rand(2, 15, 15), torch.rand(2, 195), torch.rand(2, 1, 224, 224), torch.rand(2), [sal]):
        _refused(m, x, bad, 'saliency')
    _refused(m, x, torch.ones(2, 196, dtype=torch.int64), 'floating-point')
    _refused(m, torch.zeros(2, 3, 224, 225), sal, 'expects')
    _refused(m, torch.zeros(2, 224, 224), sal, 'expects')
    _refused(m, torch.zeros(2, 3, 224, 224, dtype=torch.int32), sal, 'floating point')
    for bad in (0, -3, 2.0, False, None):
        _refused(m, x, sal, 'chunk', chunk=bad)
    _refused(m, x, sal, 'unknown target', target='severity')
    _refused(m, x, sal, 'one target per call', target=['mu', 'log_var'])
    _refused(m, x, sal, 'class_idx', target='mu', class_idx=1)
    _refused(m, x, sal, 'class_idx', class_idx=4)
    _refused(m, x, sal, 'class_idx', class_idx=torch.tensor([0, 1, 2]))
    _refused(m, x, sal, 'baseline of shape', baseline=torch.zeros(2, 3, 16, 16))
    _refused(m, x, sal, 'baseline must be a floating-point tensor', baseline=0.0)
    m.curriculum_stage = 3
    _refused(m, x, sal, 'curriculum stage', target='kan_severity')
    m.curriculum_stage = 4
    assert all(p.grad is None for p in m.parameters()) and x.grad is None
    assert [p.requires_grad for p in m.parameters()] == flags
    assert m.backbone.model._engine is None          # nothing was prepared


def test_c_entries_reject_bad_arguments(native):
    lib = native.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    n = lib.rovit_vit_num_params(2)
    params = (ctypes.c_void_p * n)(*([p.value] * n))
    em = lib.rovit_vit_embed
    good = [p, params, p, p, 4, 2, None]                # images, params, prep, tokens, n, depth
    for k in range(4):
        args = list(good)
        args[k] = None
        assert em(*args) != 0
        assert b'vit_embed: null' in lib.rovit_last_error_string()
    for k, bad in ((4, 0), (4, -1), (5, 0), (5, 65)):
        args = list(good)
        args[k] = bad
        assert em(*args) != 0
    assert em(p, params, p, ctypes.c_void_p(p.value + 4), 4, 2, None) != 0          # tokens 16-byte aligned
    ft = lib.rovit_vit_forward_tokens
    # img_tokens, base_tokens, n_img, base_shared, seq_img, src, tokens, params, prep, workspace, features, n_seq, depth, mlp_path
    good = [p, p, 2, 0, p, p, 197, params, p, p, p, 4, 2, 0, None]
    for k in (0, 1, 4, 5, 7, 8, 9, 10):
        args = list(good)
        args[k] = None
        assert ft(*args) != 0
        assert b'null' in lib.rovit_last_error_string()
    for k, bad in ((6, 0), (6, 198), (6, -1), (2, 0), (11, 0), (12, 0), (12, 65), (13, 3)):
        args = list(good)
        args[k] = bad
        assert ft(*args) != 0
    args = list(good)
    args[6] = 198
    ft(*args)
    assert b'tokens must be in [1, 197]' in lib.rovit_last_error_string()
    for k in (0, 1, 8, 9):                               # the tables, prep and workspace 16-byte aligned
        args = list(good)
        args[k] = ctypes.c_void_p(p.value + 4)
        assert ft(*args) != 0
