"""CPU tests of the per-head attention statistics' host code (rovit_hip/head_stats.py): the fp64 oracle on matrices with known
statistics, the finalise restatement, and the refusals that need no GPU."""
import numpy as np
import pytest
import torch

import head_stats_cases as cases
from rovit_hip import head_stats as hs
from rovit_hip.native import RovitHipError


def test_stat_names_and_scales():
    assert len(hs.STAT_NAMES) == 8 and len(hs.TOKEN_STAT_NAMES) == 4
    assert hs.STAT_NAMES[0] == 'entropy' and hs.STAT_NAMES[1] == 'distance' and hs.STAT_NAMES[7] == 'locality'
    assert abs(hs.DISTANCE_SCALE - 294.2) < 0.05 and hs.ENTROPY_SCALE == cases.LN197


def test_uniform_probabilities_give_the_analytic_values():
    ref = hs.head_stats_reference([cases.uniform_probs(2)])
    exp = cases.uniform_expected()
    assert ref['summary'].shape == (2, 1, 3, 8) and ref['cls_attention'].shape == (2, 1, 3, 196) and ref['per_token'].shape == (2, 1, 3, 197, 4)
    tok = ref['per_token']
    assert np.abs(tok[..., 0] - cases.LN197).max() < 1e-12                       # every entropy is ln 197
    assert np.abs(tok[..., 2] - 1 / 197).max() < 1e-15 and np.abs(tok[..., 3] - 1 / 197).max() < 1e-15
    assert np.all(tok[..., 0, 1] == 0) and np.abs(tok[..., 1:, 1] - exp['distance_per_query']).max() < 1e-10
    assert abs(exp['distance_per_query'].min() - 86.02) < 0.01 and abs(exp['distance_per_query'].max() - 161.03) < 0.01
    assert abs(exp['distance'] - 116.4922) < 1e-4
    assert exp['neighbours'].min() == 4 and exp['neighbours'].max() == 9 and abs(exp['neighbours'].mean() - 8.1633) < 1e-4
    s = ref['summary']
    assert np.abs(s - exp['summary']).max() < 1e-10
    assert abs(s[0, 0, 0, 1] - 116.4922) < 1e-4
    assert abs(s[0, 0, 0, 7] - 8.1633 / 197) < 1e-6 and abs(s[0, 0, 0, 7] - 8.1633 / 196) > 1e-4   # not renormalised over the patches
    assert np.abs(ref['cls_attention'] - 1 / 197).max() < 1e-15


def test_identity_probabilities():
    ref = hs.head_stats_reference([cases.identity_probs()])
    assert np.isfinite(ref['summary']).all() and np.isfinite(ref['per_token']).all()
    assert np.all(ref['per_token'][..., 0] == 0) and np.all(ref['per_token'][..., 1] == 0)      # entropies 0, distances 0
    s = ref['summary'][0, 0, 0]
    assert s[0] == 0 and s[1] == 0 and s[2] == 0 and s[3] == 1 and s[4] == 0 and s[5] == 1 and s[6] == 1 and s[7] == 1
    assert np.all(ref['cls_attention'] == 0)


def test_right_neighbour_probabilities():
    ref = hs.head_stats_reference([cases.right_neighbour_probs()])
    D = ref['per_token'][0, 0, 0, :, 1]
    col = (np.arange(1, 197) - 1) % 14
    assert np.all(D[1:][col < 13] == 16.0) and np.all(D[1:][col == 13] == 0.0) and D[0] == 0
    s = ref['summary'][0, 0, 0]
    assert abs(s[1] - 16.0 * 13 / 14) < 1e-12 and s[7] == 1 and s[0] == 0 and abs(s[3] - 15 / 197) < 1e-15


def test_rows_without_patch_mass_have_distance_zero():
    P = np.zeros((1, 3, 197, 197))
    P[..., 0] = 1.0                                    # every query puts everything on the class token
    ref = hs.head_stats_reference([P])
    assert np.isfinite(ref['summary']).all() and np.all(ref['per_token'][..., 1] == 0) and np.all(ref['summary'][..., 2] == 1)


def test_reference_takes_tensors_and_several_blocks():
    rng = np.random.default_rng(0)
    P = rng.random((2, 3, 197, 197))
    P /= P.sum(-1, keepdims=True)
    a = hs.head_stats_reference([P, P[::-1].copy()])
    b = hs.head_stats_reference([torch.from_numpy(P), torch.from_numpy(P[::-1].copy())])
    assert a['summary'].shape == (2, 2, 3, 8) and np.array_equal(a['summary'], b['summary'])
    assert np.array_equal(a['summary'][:, 0], a['summary'][::-1, 1])
    with pytest.raises(RovitHipError):
        hs.head_stats_reference([P[:, :, :100]])


@pytest.mark.parametrize('n', cases.FINALIZE_N)
def test_finalize_reference_is_split_invariant_and_handles_empty_groups(n):
    C = cases.FINALIZE_CLASSES
    summary, cls, labels = cases.finalize_rows(n)
    blk = hs.finalize_reference((summary, cls), labels, C)
    assert np.isfinite(blk).all()
    # however the rows are cut and put together again, the block is the same bits
    for split in cases.finalize_splits(n):
        at, parts = 0, []
        for k in split:
            parts.append((summary[at:at + k], cls[at:at + k], labels[at:at + k]))
            at += k
        again = hs.finalize_reference((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])),
                                      np.concatenate([p[2] for p in parts]), C)
        assert np.array_equal(blk, again)
    res = hs.result_from_block(blk, 2, 3, C)
    assert res['groups'] == ['all', 0, 1, 2, 3] and res['count'][0] == n and res['count'][1:].sum() == n
    e = 1 + cases.FINALIZE_EMPTY_CLASS
    assert res['count'][e] == 0 and not res['mean'][e].any() and not res['var'][e].any() and not res['cls_attention_mean'][e].any()
    x = summary.astype(np.float64)
    assert np.allclose(res['mean'][0], x.mean(0), rtol=1e-13, atol=0)
    assert np.allclose(res['cls_attention_mean'][0], cls.astype(np.float64).mean(0), rtol=1e-13, atol=0)
    if n == 1:
        assert not res['var'].any()                     # one row: variance 0, not NaN
        assert np.array_equal(res['mean'][0], x[0])
    else:
        assert np.allclose(res['var'][0], x.var(0, ddof=1), rtol=1e-11, atol=0)
    for c in range(C):
        sel = labels == c
        assert res['count'][1 + c] == sel.sum()
        if sel.sum() > 1:
            assert np.allclose(res['var'][1 + c], x[sel].var(0, ddof=1), rtol=1e-11, atol=0)


def test_finalize_reference_without_classes():
    summary, cls, _ = cases.finalize_rows(5)
    blk = hs.finalize_reference((summary, cls), None, None)
    assert blk.shape == (1 + 2 * 48 + 2 * 3 * 196,) and blk[0] == 5
    with pytest.raises(RovitHipError):
        hs.finalize_reference((summary, cls), None, 3)


def test_stated_order_mean_is_a_mean():
    rng = np.random.default_rng(1)
    v = rng.random((2, 3, 197)).astype(np.float32)
    assert np.abs(cases.stated_order_mean(v, False) - v.astype(np.float64).mean(-1)).max() < 197 * 2.0 ** -24
    assert np.abs(cases.stated_order_mean(v, True) - v[..., 1:].astype(np.float64).mean(-1)).max() < 197 * 2.0 ** -24


def test_cpu_tensors_and_bad_arguments_are_refused():
    from models.backbone import DeiTTinyBackbone
    from models.rovit_kan import RoViTKAN
    from explainability import AttentionHeadAnalysis
    x = torch.zeros(1, 3, 224, 224)
    m = RoViTKAN(pretrained=False)
    with pytest.raises(RovitHipError):
        m.attention_head_stats(x)
    with pytest.raises(RovitHipError):
        m.backbone.attention_head_stats(x, per_token=True)
    with pytest.raises(RovitHipError):
        hs.attention_head_stats(m.backbone.model, x)
    with pytest.raises(RovitHipError):
        m.attention_head_stats([(x, torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long))], per_token=True)
    with pytest.raises(RovitHipError):
        AttentionHeadAnalysis(m, 'cpu').compute(x)
    acc = hs.AttentionHeadStats(12, num_classes=4)
    with pytest.raises(RovitHipError):
        acc.update(m, x, torch.zeros(1))
    with pytest.raises(RovitHipError):
        acc.update_rows(torch.zeros(1, 12, 3, 8), torch.zeros(1, 12, 3, 196), torch.zeros(1))
    with pytest.raises(RovitHipError):
        acc.compute()
    with pytest.raises(RovitHipError):
        hs.AttentionHeadStats(12, heads=4)
    with pytest.raises(RovitHipError):
        hs.AttentionHeadStats(0)
    assert isinstance(m.backbone, DeiTTinyBackbone)


def test_block_words_match_the_layout():
    from rovit_hip import native
    lib = native.load()
    for depth, classes in ((2, 0), (2, 4), (12, 4)):
        R, Q, stride, G = hs.block_layout(depth, 3, classes)
        assert lib.rovit_head_stats_block_words(depth, 3, classes) == G * stride == (classes + 1) * (1 + 2 * R + Q)
    assert lib.rovit_head_stats_block_words(0, 3, 4) == 0
