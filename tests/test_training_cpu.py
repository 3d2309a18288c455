"""CPU tests of the training epoch's host logic: ``JointLoss.mixed`` on CPU tensors against an fp64 restatement of the reference's
``lam * L(a) + (1 - lam) * L(b)``, ``TrainRecord``'s host path against the trainer's own sums, and the drop-in ``training.Trainer`` on a stub
model (stage per epoch, unfreeze epoch, history, early stopping, checkpoint keys and round trip, the mixed-labels quirk)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from training_fp64 import HEADS, LOSSES, WEIGHTS, check_against_fp64, make_batch, mixed_fp64


# ---- 1. JointLoss.mixed on CPU tensors ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_alpha', [False, True])
@pytest.mark.parametrize('B', [1, 7, 300])
def test_mixed_on_cpu_tensors_matches_the_fp64_restatement(B, with_alpha):
    from rovit_hip.losses import JointLoss
    out, ta, tb, sev, alpha = make_batch(B, seed=B)
    alpha = alpha if with_alpha else None
    lf = JointLoss(*WEIGHTS, focal_alpha=alpha)
    for stage in (1, 2, 3, 4):
        for lam in (0.0, 0.3, 1.0):
            o = {k: v.clone().requires_grad_(True) for k, v in out.items()}
            got = lf.mixed(o, ta, tb, lam, sev, stage)
            assert set(got) == set(LOSSES)
            got['total_loss'].backward()
            ref_l, ref_g = mixed_fp64(out, ta, tb, lam, sev, stage, WEIGHTS, alpha)
            check_against_fp64(got, {k: o[k].grad for k in HEADS}, ref_l, ref_g, tag=(B, stage, lam))


@pytest.mark.parametrize('stage', [1, 2, 3, 4])
def test_mixed_without_a_second_label_column_is_forward(stage):
    from rovit_hip.losses import JointLoss
    out, ta, tb, sev, alpha = make_batch(7, seed=3)
    lf = JointLoss(*WEIGHTS, focal_alpha=alpha)
    want = lf(out, ta, sev, stage)
    for got in (lf.mixed(out, ta, None, 0.4, sev, stage), lf.mixed(out, ta, tb, 1.0, sev, stage)):
        for k in LOSSES:
            assert torch.equal(got[k], want[k]), k
    with pytest.raises(RuntimeError):
        lf.mixed(out, ta, tb, 1.5, sev, stage)


# ---- 2. TrainRecord, host path --------------------------------------------------------------------------------------------------------

def _record_batches(sizes, nan_batch=None):
    from rovit_hip.training import TrainRecord
    g = torch.Generator().manual_seed(11)
    rec = TrainRecord(capacity=2)
    sums, correct, total = [0.0] * 5, 0, 0
    for i, B in enumerate(sizes):
        logits = torch.randn(B, 4, generator=g)
        labels = torch.randint(0, 4, (B,), generator=g)
        losses = {k: torch.rand((), generator=g) * 3 for k in LOSSES}
        if i == nan_batch:
            losses['total_loss'] = torch.tensor(float('nan'))
        rec.update(losses, logits, labels)
        # the trainer's sums (training/trainer.py:144-153)
        for j, k in enumerate(LOSSES):
            sums[j] += losses[k].item()
        _, predicted = logits.max(1)
        total += labels.size(0)
        correct += predicted.eq(labels).sum().item()
    return rec, sums, correct, total


def test_train_record_host_path_reproduces_the_trainers_sums():
    sizes = (7, 7, 7, 3)
    rec, sums, correct, total = _record_batches(sizes)
    assert rec.n == 24 == total and rec.n_batches == 4
    m = rec.compute()
    assert set(m) == {'loss', 'cls_loss', 'ord_loss', 'unc_loss', 'kan_loss', 'accuracy'}
    for j, k in enumerate(LOSSES):
        want = sums[j] / len(sizes)                          # means over batches, not samples
        assert abs(m['loss' if k == 'total_loss' else k] - want) <= 1e-12 * abs(want), k
    assert m['accuracy'] == 100. * correct / total
    assert rec.nonfinite_batches == 0
    rows = rec.rows()
    assert rows.shape == (4, 8) and rows[:, 6].tolist() == list(sizes)
    rec.reset()
    assert rec.n == 0 and rec.n_batches == 0
    with pytest.raises(RuntimeError):
        rec.compute()


def test_train_record_counts_a_nan_batch_and_reports_a_nan_mean():
    rec, sums, correct, total = _record_batches((7, 7, 7, 3), nan_batch=2)
    m = rec.compute()
    assert rec.nonfinite_batches == 1
    assert math.isnan(m['loss']) and math.isnan(sums[4] / 4)          # as the reference would print
    assert m['cls_loss'] == pytest.approx(sums[0] / 4, rel=1e-12) and m['accuracy'] == 100. * correct / total


# ---- 3. training.Trainer on a stub model --------------------------------------------------------------------------------------------------

class StubModel(nn.Module):
    """The six-key output dict from linear layers, plus the three members the Trainer touches."""

    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.backbone = nn.Linear(3 * 4 * 4, 16)
        self.cls, self.ord, self.unc, self.kan = nn.Linear(16, 4), nn.Linear(16, 3), nn.Linear(16, 2), nn.Linear(16, 1)
        self.events = []
        self._stage = 4

    @property
    def curriculum_stage(self):
        return self._stage

    @curriculum_stage.setter
    def curriculum_stage(self, v):
        self._stage = v
        self.events.append(('stage', v))

    def freeze_backbone(self):
        self.events.append(('freeze',))

    def unfreeze_backbone(self):
        self.events.append(('unfreeze',))

    def forward(self, x):
        f = torch.tanh(self.backbone(x.flatten(1)))
        u = self.unc(f)
        return {'cls_logits': self.cls(f), 'ordinal_logits': self.ord(f), 'mu': u[:, :1], 'log_var': u[:, 1:],
                'kan_severity': 3 * torch.sigmoid(self.kan(f)), 'features': f}


def _loader(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    batches = []
    for B in sizes:
        y = torch.randint(0, 4, (B,), generator=g)
        batches.append((torch.randn(B, 3, 4, 4, generator=g), y, y.clone()))
    return batches


def _stage_for_epoch(epoch):          # module level: the config is pickled into the checkpoint
    return min(4, epoch)


def _config(tmp_path, epochs=4, patience=10, freeze=1, mixed_precision=False, mix=False):
    return SimpleNamespace(
        flags=SimpleNamespace(use_cutmix=mix, use_mixup=mix, cutmix_alpha=1.0, mixup_alpha=0.2, mixed_precision=mixed_precision,
                              gradient_clip=1.0, freeze_backbone_epochs=freeze, curriculum=True),
        train=SimpleNamespace(epochs=epochs, early_stop_patience=patience, learning_rate=1e-2, weight_decay=0.0),
        paths=SimpleNamespace(checkpoints_dir=tmp_path),
        get_stage_for_epoch=_stage_for_epoch)


def _trainer(tmp_path, lr=1e-2, seed=0, **cfg):
    from training import JointLoss, Trainer
    model = StubModel(seed)
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    config = _config(tmp_path, **cfg)
    return Trainer(model, _loader((7, 7, 7, 3), 1), _loader((5, 4), 2), opt, sched, JointLoss(), config, torch.device('cpu'))


def test_training_package_keeps_the_reference_import_paths():
    import rovit_hip.losses
    import rovit_hip.optim
    from training.losses import JointLoss
    from training.optimizer import build_optimizer, build_scheduler, get_lr
    from training.trainer import Trainer
    assert JointLoss is rovit_hip.losses.JointLoss and build_optimizer is rovit_hip.optim.build_optimizer
    assert build_scheduler is rovit_hip.optim.build_scheduler and get_lr is rovit_hip.optim.get_lr
    for name in ('train_epoch', 'val_epoch', 'fit', 'save_checkpoint', 'load_checkpoint'):
        assert callable(getattr(Trainer, name))


def test_trainer_fit_stages_unfreeze_history_and_checkpoint(tmp_path, capsys):
    t = _trainer(tmp_path, epochs=4, freeze=1)
    assert t.best_val_loss == float('inf') and t.patience_counter == 0 and t.best_epoch == 0
    history = t.fit()
    assert set(history) == {'train_loss', 'val_loss', 'train_acc', 'val_acc'} and all(len(v) == 4 for v in history.values())
    assert all(np.isfinite(v).all() for v in history.values())
    ev = [e for i, e in enumerate(t.model.events) if i == 0 or e != t.model.events[i - 1]]        # consecutive repeats folded
    assert ev[0] == ('freeze',)
    stages = [e[1] for e in ev if e[0] == 'stage']
    assert [v for i, v in enumerate(stages) if i == 0 or v != stages[i - 1]] == [1, 2, 3, 4]       # config.get_stage_for_epoch(epoch)
    assert ev.count(('unfreeze',)) == 1 and ev[ev.index(('unfreeze',)) - 1] == ('stage', 2)        # epoch == freeze_backbone_epochs + 1
    assert t.optimizer.param_groups[0]['lr'] == pytest.approx(1e-2 * 0.5 ** 4)                     # scheduler.step() once per epoch
    assert t.last_train_record.n == 24 and t.last_train_record.n_batches == 4 and t.last_train_record.nonfinite_batches == 0
    assert t.best_epoch >= 1 and t.best_val_loss == min(history['val_loss'][:t.best_epoch])
    out = capsys.readouterr().out
    assert 'Epoch 1/4 (Stage 1): 20%..50%..70%..100% Loss: ' in out                                # 4 batches: marks at 20, 50, 70, 100
    ck = torch.load(tmp_path / 'best_model.pth', weights_only=False)
    assert set(ck) == {'epoch', 'model_state_dict', 'optimizer_state_dict', 'scheduler_state_dict', 'best_val_loss', 'metrics', 'config'}
    assert ck['epoch'] == t.best_epoch and ck['best_val_loss'] == t.best_val_loss and ck['metrics']['loss'] == t.best_val_loss


def test_trainer_stops_early_after_patience_epochs_without_improvement(tmp_path):
    t = _trainer(tmp_path, lr=0.0, epochs=10, patience=2, freeze=0)          # lr 0: the validation loss never changes
    history = t.fit()
    assert len(history['val_loss']) == 3 and t.best_epoch == 1 and t.patience_counter == 2
    assert ('freeze',) not in t.model.events


def test_trainer_checkpoint_round_trip_ignores_a_scaler_state(tmp_path):
    t = _trainer(tmp_path, epochs=2, freeze=0, mixed_precision=True)
    t.fit()
    path = tmp_path / 'best_model.pth'
    ck = torch.load(path, weights_only=False)
    assert 'scaler_state_dict' not in ck                                     # mixed_precision accepted, no scaler
    ck['scaler_state_dict'] = {'scale': 65536.0}                             # as a reference checkpoint would carry
    torch.save(ck, path)
    fresh = _trainer(tmp_path, seed=5, epochs=2, freeze=0)
    x = torch.randn(3, 3, 4, 4)
    assert not torch.equal(fresh.model(x)['cls_logits'], StubModel(0)(x)['cls_logits'])
    fresh.load_checkpoint(path)
    assert fresh.best_val_loss == ck['best_val_loss']
    want = StubModel(0)
    want.load_state_dict(ck['model_state_dict'])
    for k, v in fresh.model(x).items():
        assert torch.equal(v, want(x)[k]), k
    assert fresh.scheduler.state_dict()['last_epoch'] == ck['scheduler_state_dict']['last_epoch']


@pytest.mark.parametrize('mixed_precision', [False, True])
def test_trainer_mixes_the_labels_only_on_the_mixed_precision_branch(tmp_path, monkeypatch, mixed_precision):
    """The reference's quirk (training/trainer.py:104-111 against :131-133), kept: mix_loss = config.flags.mixed_precision."""
    import data.transforms as transforms

    def mix_on_the_host(images, perm, mode, lam=1.0, box=(0, 0, 0, 0)):
        out = images.clone()
        if mode == 'mixup':
            return lam * images + (1 - lam) * images[perm]
        y0, y1, x0, x1 = box
        out[:, :, y0:y1, x0:x1] = images[perm][:, :, y0:y1, x0:x1]
        return out
    monkeypatch.setattr(transforms, 'mix_images', mix_on_the_host)
    np.random.seed(0)
    t = _trainer(tmp_path, epochs=1, freeze=0, mixed_precision=mixed_precision, mix=True)
    assert t.mix_loss is mixed_precision
    calls = []
    real = t.loss_fn.mixed
    monkeypatch.setattr(t.loss_fn, 'mixed', lambda o, la, lb, lam, *a, **k: (calls.append((lb is not None, lam)), real(o, la, lb, lam, *a, **k))[1])
    m = t.train_epoch(1)
    assert len(calls) == 4 and np.isfinite(m['loss'])
    if mixed_precision:
        assert all(has_b for has_b, _ in calls) and any(lam < 1.0 for _, lam in calls)
    else:
        assert all(not has_b and lam == 1.0 for has_b, lam in calls)
