"""CPU tests of PatchDropout (rovit_hip.patch_dropout): the numpy statement of the draw, the module's argument checks and k rounding,
the refusals that are decided before anything touches a device, and the Trainer's reading of ``config.train.patch_keep``."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_training_cpu import StubModel, _config, _loader


def _pd():
    from rovit_hip import patch_dropout
    return patch_dropout


@pytest.mark.parametrize('k', [1, 15, 98, 196])
def test_draw_reference_rows_are_sorted_unique_and_in_range(k):
    keep = _pd().draw_reference(3, 5, 17, k)
    assert keep.shape == (17, k) and keep.dtype == np.int32
    assert keep.min() >= 0 and keep.max() < 196
    assert (np.diff(keep, axis=1) > 0).all()              # strictly ascending: sorted and unique
    if k == 196:
        assert (keep == np.arange(196)).all()


def test_draw_reference_depends_on_sample_step_and_seed_and_on_nothing_else():
    pd = _pd()
    a = pd.draw_reference(11, 4, 3, 98)
    assert not (a[0] == a[1]).all() and not (a[1] == a[2]).all()          # different b
    assert not (a == pd.draw_reference(11, 5, 3, 98)).all(axis=1).any()    # different step
    assert not (a == pd.draw_reference(12, 4, 3, 98)).all(axis=1).any()    # different seed
    assert not (a == pd.draw_reference(11, 4 + (1 << 32), 3, 98)).all(axis=1).any()     # the step's high word counts
    assert not (a == pd.draw_reference(11 + (1 << 32), 4, 3, 98)).all(axis=1).any()     # the seed's high word counts
    assert (a == pd.draw_reference(11, 4, 3, 98)).all()                    # the same triple
    assert (a[:2] == pd.draw_reference(11, 4, 2, 98)).all()                # a sample's row does not depend on the batch size
    # a smaller k keeps a subset of a larger k's patches (the same ranks, another threshold)
    small = pd.draw_reference(11, 4, 3, 15)
    assert all(set(small[b]) <= set(a[b]) for b in range(3))


def test_draw_reference_breaks_equal_keys_by_patch_index(monkeypatch):
    """All 196 keys equal: the pair (key, patch) still ranks them 0..195, so the first k patches are kept."""
    from oracle import philox
    monkeypatch.setattr(philox, 'philox4x32_10', lambda counter, key: [np.full(np.asarray(counter[0]).shape, 7, np.uint64)] * 4)
    assert (_pd().draw_reference(0, 0, 2, 5) == np.arange(5)).all()


def test_draw_reference_is_uniform_over_the_patches():
    """4 096 draws at k = 98 (64 steps of 64 samples, seed 2023): every patch is kept 2 048 times +- 6 binomial standard deviations
    (sqrt(4096 / 4) = 32; 6 x 32 = 192)."""
    pd = _pd()
    counts = np.zeros(196, np.int64)
    for step in range(64):
        counts += np.bincount(pd.draw_reference(2023, step, 64, 98).ravel(), minlength=196)
    assert counts.sum() == 4096 * 98
    assert np.abs(counts - 2048).max() <= 192, (counts.min(), counts.max())


def test_maps_reference_is_the_gather_convention_and_its_inverse():
    pd = _pd()
    keep = pd.draw_reference(1, 2, 4, 31)
    src, inv = pd.maps_reference(keep)
    assert src.shape == (4, 32) and inv.shape == (4, 197) and src.dtype == inv.dtype == np.int32
    assert (src[:, 0] == 0).all() and (src[:, 1:] == keep + 1).all()
    for b in range(4):
        assert (inv[b, src[b]] == np.arange(32)).all()
        assert (inv[b] >= 0).sum() == 32 and (inv[b][inv[b] < 0] == -1).all()


@pytest.mark.parametrize('bad', [dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(step=-1), dict(step=1 << 64), dict(B=0), dict(k=0),
                                 dict(k=197)])
def test_draw_reference_argument_checks(bad):
    args = dict(seed=0, step=0, B=2, k=5)
    args.update(bad)
    with pytest.raises(ValueError):
        _pd().draw_reference(**args)


def test_k_rounding():
    pd = _pd()
    assert [pd.kept_patches(v) for v in (1.0, 0.75, 0.5, 0.25, 0.1, 0.01, 0.004, 0.001, 0.0025)] == [196, 147, 98, 49, 20, 2, 1, 1, 1]
    assert pd.kept_patches(97.5 / 196) == 98 and pd.kept_patches(97.4 / 196) == 97          # halves go up


def test_set_patch_dropout_argument_checks_and_state():
    from models.backbone import DeiTTinyBackbone
    from models.rovit_kan import RoViTKAN
    bb = DeiTTinyBackbone(pretrained=False)
    assert bb.model.patch_keep == 1.0 and bb.patch_dropout_step == 0 and bb.last_patch_keep is None
    for keep in (0.0, -0.5, 1.5, float('nan'), '0.5', None, True):
        with pytest.raises(ValueError):
            bb.set_patch_dropout(keep=keep)
    for seed in (-1, 1 << 64, 0.5, None, True):
        with pytest.raises(ValueError):
            bb.set_patch_dropout(keep=0.5, seed=seed)
    assert bb.model.patch_keep == 1.0                                   # a refused call changes nothing
    bb.patch_dropout_step = 41
    assert bb.set_patch_dropout(keep=0.5, seed=9) is bb
    assert (bb.model.patch_keep, bb.model.patch_dropout_seed, bb.patch_dropout_step) == (0.5, 9, 0)      # the counter restarts
    bb.patch_dropout_step = 7
    assert bb.model.patch_dropout_step == 7
    for step in (-1, 1 << 64, 1.0, True):
        with pytest.raises(ValueError):
            bb.patch_dropout_step = step
    keys = set(bb.state_dict())
    assert not [k for k in keys if 'patch_dropout' in k or 'extra_state' in k]          # the reference's key set is unchanged
    m = RoViTKAN(pretrained=False)
    assert m.set_patch_dropout(0.25, seed=3) is m
    assert (m.backbone.model.patch_keep, m.backbone.model.patch_dropout_seed) == (0.25, 3)
    m.set_patch_dropout()
    assert m.backbone.model.patch_keep == 1.0


def test_refusals_come_before_any_device_work():
    """Hooks, images that require grad and the data-parallel wrapper are refused with patch dropout on -- on CPU tensors, so the message is
    the refusal's own and not the missing device's.  With patch dropout off, or in eval() mode, the same calls take the existing paths."""
    from models.backbone import DeiTTinyBackbone
    from rovit_hip import RovitHipError
    bb = DeiTTinyBackbone(pretrained=False).set_patch_dropout(0.5)
    bb.train()
    x = torch.zeros(1, 3, 224, 224)
    h = bb.model.blocks[0].norm1.register_forward_hook(lambda *a: None)
    with pytest.raises(RovitHipError, match='hook'):
        bb(x)
    h.remove()
    h = bb.model.blocks[1].attn.register_forward_hook(lambda *a: None)
    with pytest.raises(RovitHipError, match='hook'):
        bb(x)
    h.remove()
    with pytest.raises(RovitHipError, match='images require grad'):
        bb(x.clone().requires_grad_())
    eng = bb.model.engine
    eng.range_hook = lambda *a: None                 # what rovit_hip.parallel.GradSync installs
    with pytest.raises(RovitHipError, match='data-parallel'):
        bb(x)
    eng.range_hook = None
    eng.backward_ranges = [(11, 6), (5, 0)]
    with pytest.raises(RovitHipError, match='data-parallel'):
        bb(x)
    eng.backward_ranges = None
    assert bb.patch_dropout_step == 0                # a refused forward draws nothing
    # nothing refused any more: the call now gets as far as the device and fails THERE on a CPU tensor
    with pytest.raises(RovitHipError, match='CPU tensor'):
        bb(x)
    # eval() mode is the dense path, with its own message for the same CPU tensor, and draws nothing
    step = bb.patch_dropout_step
    bb.eval()
    with pytest.raises(RovitHipError, match='CPU tensor'):
        bb(x)
    assert bb.patch_dropout_step == step


def test_forward_kept_checks_its_indices_and_refuses_like_the_module():
    from models.backbone import DeiTTinyBackbone
    from rovit_hip import RovitHipError
    pd = _pd()
    bb = DeiTTinyBackbone(pretrained=False)
    x = torch.zeros(2, 3, 224, 224)
    for keep in ([[0, 1]], [[0, 1], [1, 1]], [[1, 0], [0, 1]], [[0, 196], [0, 1]], [[-1, 0], [0, 1]], [[0.0, 1.0], [0.0, 1.0]], [0, 1],
                 np.zeros((2, 0), np.int64)):
        with pytest.raises(ValueError):
            pd.forward_kept(bb, x, keep)
    with pytest.raises(RovitHipError, match='images require grad'):
        pd.forward_kept(bb, x.clone().requires_grad_(), [[0, 1], [2, 3]])
    h = bb.model.blocks[0].norm1.register_full_backward_hook(lambda *a: None)
    with pytest.raises(RovitHipError, match='hook'):
        pd.forward_kept(bb, x, [[0, 1], [2, 3]])
    h.remove()


def test_trainer_reads_patch_keep_and_ignores_a_config_without_it(tmp_path):
    from models.rovit_kan import RoViTKAN
    from training import JointLoss, Trainer

    def trainer(model, **train_fields):
        cfg = _config(tmp_path)
        for k, v in train_fields.items():
            setattr(cfg.train, k, v)
        opt = torch.optim.SGD(model.parameters(), lr=1e-2)
        return Trainer(model, _loader((3,), 1), _loader((3,), 2), opt, torch.optim.lr_scheduler.StepLR(opt, 1), JointLoss(), cfg,
                       torch.device('cpu'))
    # no field: a model without set_patch_dropout (the stub has none) is accepted and nothing is called
    t = trainer(StubModel())
    assert t.patch_keep == 1.0 and not hasattr(t.model, 'set_patch_dropout')
    t.save_checkpoint(tmp_path / 'a.pth', 1, {})
    assert 'patch_dropout_step' not in torch.load(tmp_path / 'a.pth', weights_only=False)
    m = RoViTKAN(pretrained=False)
    assert trainer(m).model.backbone.model.patch_keep == 1.0
    assert trainer(m, patch_keep=1.0).model.backbone.model.patch_keep == 1.0
    t = trainer(m, patch_keep=0.5, patch_seed=17)
    assert (m.backbone.model.patch_keep, m.backbone.model.patch_dropout_seed) == (0.5, 17)
    m.backbone.patch_dropout_step = 12
    t.save_checkpoint(tmp_path / 'b.pth', 1, {})
    m.backbone.patch_dropout_step = 0
    t.load_checkpoint(tmp_path / 'b.pth')
    assert m.backbone.patch_dropout_step == 12
    with pytest.raises(ValueError):
        trainer(RoViTKAN(pretrained=False), patch_keep=0.0)
