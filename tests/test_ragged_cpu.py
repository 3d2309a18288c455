"""CPU tests of the ragged-batch forward: the C entries refuse bad arguments before any launch and name the argument; ragged_layout
against hand-written expectations; the ``ragged`` keyword of perturbation_curves, patch_shap and PatchSHAP."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ragged_cases import L, L_SHUFFLED, cycle_lengths, layout_reference, offsets_of


@pytest.fixture(scope='module')
def native():
    from rovit_hip import native as n
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return n


def _host(values):
    return (ctypes.c_int * len(values))(*values)


def _err(lib):
    return lib.rovit_last_error_string().decode()


# ---- the C entries ---------------------------------------------------------------------------------------------------------------

BAD_OFFSETS = [
    ([1, 5, 9, 12, 20], r'seq_offsets_host[0] must be 0'),
    ([0, 5, 5, 12, 20], 'sequence 1 has 0 rows'),
    ([0, 5, 4, 12, 20], 'sequence 1 has -1 rows'),
    ([0, 5, 203, 210, 220], 'sequence 1 has 198 rows'),
    ([0, 197, 394, 591, 789], 'sequence 3 has 198 rows'),
]


def test_forward_ragged_rejects_bad_arguments(native):
    lib = native.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    n = lib.rovit_vit_num_params(2)
    params = (ctypes.c_void_p * n)(*([p.value] * n))
    off = _host([0, 5, 9, 12, 20])
    fr = lib.rovit_vit_forward_ragged
    # img_tokens, base_tokens, n_img, base_shared, seq_img, src, offsets_dev, offsets_host, params, prep, workspace, features, n_seq, depth,
    # mlp_path, stream
    good = [p, p, 2, 0, p, p, p, off, params, p, p, p, 4, 2, 1, None]
    names = {0: 'img_tokens', 1: 'base_tokens', 4: 'seq_img', 5: 'src', 6: 'seq_offsets_dev', 7: 'seq_offsets_host', 8: 'params', 9: 'prep',
             10: 'workspace', 11: 'features'}
    for k, name in names.items():
        args = list(good)
        args[k] = None
        assert fr(*args) != 0
        assert _err(lib) == f'vit_forward_ragged: null {name}'
    for k, bad, word in ((2, 0, 'n_img'), (12, 0, 'n_seq'), (12, -1, 'n_seq'), (13, 0, 'depth'), (13, 65, 'depth'), (14, 3, 'mlp_path'),
                         (14, -1, 'mlp_path')):
        args = list(good)
        args[k] = bad
        assert fr(*args) != 0
        assert _err(lib).startswith('vit_forward_ragged: ') and word in _err(lib)
    for k, word in ((9, 'prep'), (10, 'workspace')):
        args = list(good)
        args[k] = ctypes.c_void_p(p.value + 4)
        assert fr(*args) != 0
        assert _err(lib) == f'vit_forward_ragged: {word} must be 16-byte aligned'
    for values, msg in BAD_OFFSETS:
        args = list(good)
        args[7] = _host(values)
        assert fr(*args) != 0
        assert _err(lib).startswith('vit_forward_ragged: ') and msg in _err(lib), _err(lib)
    for k in (0, 1):                                     # the token tables 16-byte aligned: refused by the first launch's own check
        args = list(good)
        args[k] = ctypes.c_void_p(p.value + 4)
        assert fr(*args) != 0
        assert 'aligned' in _err(lib)


def test_attention_ragged_entries_reject_bad_arguments(native):
    lib = native.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    off = _host([0, 5, 9, 12, 20])
    # qkv, out, lse2, offsets_dev, offsets_host, n_seq, heads, head_dim, scale, stream
    full = ('attention_fwd_ragged', lib.rovit_attention_fwd_ragged, [p, p, None, p, off, 4, 3, 64, 0.125, None],
            {0: 'qkv', 1: 'out', 3: 'seq_offsets_dev', 4: 'seq_offsets_host'}, 4, 5, 7)
    # qkv, out, lse2, x_rows, x_cls, offsets_dev, offsets_host, n_seq, heads, head_dim, scale, stream
    cls = ('attention_cls_fwd_ragged', lib.rovit_attention_cls_fwd_ragged, [p, p, None, None, None, p, off, 4, 3, 64, 0.125, None],
           {0: 'qkv', 1: 'out', 5: 'seq_offsets_dev', 6: 'seq_offsets_host'}, 6, 7, 9)
    for what, fn, good, names, k_off, k_n, k_hd in (full, cls):
        for k, name in names.items():
            args = list(good)
            args[k] = None
            assert fn(*args) != 0
            assert _err(lib) == f'{what}: null {name}'
        for k, bad, word in ((k_n, 0, 'n_seq'), (k_n, -2, 'n_seq'), (k_hd, 32, 'head_dim'), (k_hd - 1, 0, 'heads')):
            args = list(good)
            args[k] = bad
            assert fn(*args) != 0
            assert _err(lib).startswith(what + ': ') and word in _err(lib)
        for values, msg in BAD_OFFSETS:
            args = list(good)
            args[k_off] = _host(values)
            assert fn(*args) != 0
            assert _err(lib).startswith(what + ': ') and msg in _err(lib), _err(lib)
        for k in (0, 1):
            args = list(good)
            args[k] = ctypes.c_void_p(p.value + 4)
            assert fn(*args) != 0
            assert _err(lib) == f'{what}: qkv and out must be 16-byte aligned'
    # x_rows and x_cls go together
    for k in (3, 4):
        args = list(cls[2])
        args[k] = p
        assert cls[1](*args) != 0
        assert 'x_rows and x_cls go together' in _err(lib)


def test_ragged_workspace_bytes(native):
    lib = native.load()
    # the inference plan of max_rows rows: what 256 sequences of 197 tokens need holds 50 432 rows in any split into sequences
    rows = 256 * 197
    w = lib.rovit_vit_ragged_workspace_bytes(rows, 12)
    assert w >= lib.rovit_vit_workspace_bytes(256, 12, 0)
    assert w > rows * 192 * 4
    assert lib.rovit_vit_ragged_workspace_bytes(197, 2) < lib.rovit_vit_ragged_workspace_bytes(198, 2) <= w
    for bad in ((0, 2), (-1, 2), (197, 0), (197, 65)):
        assert lib.rovit_vit_ragged_workspace_bytes(*bad) == 0
    assert lib.rovit_version() == 440


# ---- ragged_layout ---------------------------------------------------------------------------------------------------------------

def test_layout_packs_longest_first_and_restores_the_order():
    from rovit_hip.ragged import ragged_layout
    calls, perm = ragged_layout(np.array([3, 197, 1, 50, 197, 2]), 400)
    # longest first, ties in the caller's order: 197 (1), 197 (4) | 50 (3), 3 (0), 2 (5), 1 (2); 394 + 50 would pass 400
    assert [c[0].tolist() for c in calls] == [[1, 4], [3, 0, 5, 2]]
    assert calls[0][1].tolist() == [0, 197, 394] and calls[0][1].dtype == np.int32
    assert calls[1][1].tolist() == [0, 50, 53, 55, 56]
    assert perm.tolist() == [3, 0, 5, 2, 1, 4]
    packed = np.concatenate([c[0] for c in calls])
    assert packed[perm].tolist() == list(range(6))


def test_layout_edge_cases():
    from rovit_hip.ragged import ragged_layout
    calls, perm = ragged_layout([1], 197)                                  # a single class-token sequence
    assert len(calls) == 1 and calls[0][0].tolist() == [0] and calls[0][1].tolist() == [0, 1] and perm.tolist() == [0]
    calls, _ = ragged_layout([197, 100, 97, 197], 394)                      # lengths that exactly fill max_rows, twice
    assert [c[0].tolist() for c in calls] == [[0, 3], [1, 2]]
    assert [c[1].tolist() for c in calls] == [[0, 197, 394], [0, 100, 197]]
    calls, _ = ragged_layout([197, 197, 1], 393)                            # one row short: the second sequence opens a new call
    assert [c[0].tolist() for c in calls] == [[0], [1, 2]]
    calls, _ = ragged_layout(torch.tensor(L_SHUFFLED), 197 * 256)
    assert len(calls) == 1 and [L_SHUFFLED[i] for i in calls[0][0]] == sorted(L, reverse=True)


@pytest.mark.parametrize('max_rows', [197, 200, 394, 1000, 197 * 256])
def test_layout_against_the_plain_loop(max_rows):
    from rovit_hip.ragged import ragged_layout
    lengths = cycle_lengths(37) + [197] * 5 + [1] * 9
    calls, perm = ragged_layout(lengths, max_rows)
    assert [c[0].tolist() for c in calls] == layout_reference(lengths, max_rows)
    for seq, off in calls:
        assert off.tolist() == offsets_of([lengths[i] for i in seq]).tolist()
        assert off[-1] <= max_rows
    assert np.concatenate([c[0] for c in calls])[perm].tolist() == list(range(len(lengths)))


def test_layout_refuses_bad_arguments():
    from rovit_hip import RovitHipError
    from rovit_hip.ragged import ragged_layout
    for bad in ([], [0], [198], [[1, 2]], [1.5], np.array([5, -1])):
        with pytest.raises(RovitHipError, match='ragged_layout: '):
            ragged_layout(bad, 197)
    for bad in (196, 0, True, 2.5, None):
        with pytest.raises(RovitHipError, match='max_rows'):
            ragged_layout([1, 2], bad)


# ---- the keyword -----------------------------------------------------------------------------------------------------------------

def test_curves_and_shap_take_the_ragged_keyword():
    from rovit_hip import RovitHipError
    from explainability.shap import PatchSHAP
    from models.rovit_kan import RoViTKAN
    m = RoViTKAN(pretrained=False)
    x = torch.zeros(2, 3, 224, 224)
    sal = torch.rand(2, 14, 14)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(RovitHipError, match='perturbation_curves: ragged must be a bool'):
            m.perturbation_curves(x, sal, perturbation='drop', ragged=bad)
        with pytest.raises(RovitHipError, match='patch_shap: ragged must be a bool'):
            m.patch_shap(x, players=2, ragged=bad)
        with pytest.raises(RovitHipError, match='patch_shap: ragged must be a bool'):
            PatchSHAP(m, device='cpu').explain_batch(x, players=2, ragged=bad)
    # CPU tensors: the flag changes nothing -- the same refusal either way, for both perturbations
    for ragged in (False, True):
        for pert in ('drop', 'replace'):
            with pytest.raises(RovitHipError, match='perturbation_curves: the images must be on the GPU'):
                m.perturbation_curves(x, sal, perturbation=pert, ragged=ragged)
            with pytest.raises(RovitHipError, match='patch_shap: the images must be on the GPU'):
                m.patch_shap(x, players=2, perturbation=pert, ragged=ragged)
    assert m.backbone.model._engine is None          # nothing was prepared
