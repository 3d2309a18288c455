"""``training.trainer.Trainer`` of the reference (training/trainer.py) on the HIP path, one device synchronisation per epoch each way.

Same constructor, methods (``train_epoch(epoch)``, ``val_epoch()``, ``fit()``, ``save_checkpoint``, ``load_checkpoint``) and attributes
(``best_val_loss``, ``patience_counter``, ``best_epoch``) as the reference's class, so ``scripts/train.py`` and ``experiments/ablation.py``
run on it unchanged.  The config stays duck-typed: ``config.flags`` (use_cutmix, use_mixup, cutmix_alpha, mixup_alpha, mixed_precision,
gradient_clip, freeze_backbone_epochs, curriculum), ``config.train`` (epochs, early_stop_patience), ``config.paths.checkpoints_dir`` and
``config.get_stage_for_epoch(epoch)``.

* ``train_epoch`` is ``rovit_hip.training.train_epoch``: the CutMix / MixUp loss is one launch and nothing is read back before the epoch's
  single copy of a 9-word result block.  ``val_epoch`` is ``rovit_hip.evaluation.validate``.
* A quirk of the reference, kept: its labels enter the loss mixed only on the ``mixed_precision and cuda`` branch (trainer.py:99-111); the
  other branch (trainer.py:131-133) takes the loss against ``class_labels`` alone, on mixed images.  So ``mix_loss = flags.mixed_precision``.
  The ``cuda`` half of that condition is not carried over: this trainer has no scaler for a device to switch off, so with
  ``mixed_precision=True`` it mixes the labels on a CPU device too, where the reference would not.
* No ``GradScaler``.  The backbone computes in bf16, which has fp32's exponent range, so there is no loss scale to maintain: the
  ``mixed_precision`` flag is accepted (and selects the branch above), no ``scaler_state_dict`` is written, one found at load is ignored.  What
  a scaler's skipped steps would have told the user is ``trainer.last_train_record.nonfinite_batches``, the batches of the last epoch whose
  total loss was not finite.
* With an optimizer that keeps a weight average (``RoViTAdamW(ema_decay=...)``; the reference has none) ``val_epoch`` validates the
  averaged weights (``optimizer.swap_ema()``), so early stopping and ``best_model.pth`` follow them; the checkpoint gains
  ``'ema_state_dict'`` while ``'model_state_dict'`` stays the raw weights training resumes from.  Without one nothing changes.
* ``config.train.patch_keep`` < 1 (read with ``getattr``; the reference's ``Config`` has no such field) switches PatchDropout on
  (``model.set_patch_dropout``; ``config.train.patch_seed``, default 0): training steps run on the kept tokens, validation on all.  The
  checkpoint then gains ``'patch_dropout_step'``.  Without the field nothing changes.
"""
from pathlib import Path
from typing import Dict, List, Optional

import torch

from rovit_hip.evaluation import validate
from rovit_hip.training import TrainRecord, train_epoch

RULE = '=' * 60


class Trainer:
    def __init__(self, model: torch.nn.Module, train_loader, val_loader, optimizer, scheduler, loss_fn, config, device: torch.device,
                 logger=None):
        self.model = model.to(device)
        self.train_loader, self.val_loader = train_loader, val_loader
        self.optimizer, self.scheduler, self.loss_fn = optimizer, scheduler, loss_fn
        self.config, self.device, self.logger = config, device, logger
        self.scaler = None                                  # kept as an attribute; never a GradScaler (module docstring)
        self.mix_loss = bool(config.flags.mixed_precision)
        # PatchDropout (not in the reference, whose Config has no such field): config.train.patch_keep < 1 trains on kept tokens
        self.patch_keep = float(getattr(config.train, 'patch_keep', 1.0))
        if self.patch_keep != 1.0:
            self.model.set_patch_dropout(keep=self.patch_keep, seed=int(getattr(config.train, 'patch_seed', 0)))
        self.last_train_record: Optional[TrainRecord] = None
        self.best_val_loss = float('inf')
        self.patience_counter = 0
        self.best_epoch = 0

    def train_epoch(self, epoch: int) -> Dict[str, float]:
        flags = self.config.flags
        stage = self.config.get_stage_for_epoch(epoch)
        self.model.curriculum_stage = stage                  # before unfreeze_backbone(), as in the reference; train_epoch sets it again
        if epoch == flags.freeze_backbone_epochs + 1:
            self.model.unfreeze_backbone()
        print(f'Epoch {epoch}/{self.config.train.epochs} (Stage {stage}): ', end='', flush=True)
        num_batches = len(self.train_loader)

        def progress(batch_idx: int) -> None:
            # a mark at every tenth of the epoch; host arithmetic only
            done = int((batch_idx + 1) / num_batches * 100) // 10
            before = (int(batch_idx / num_batches * 100) if batch_idx > 0 else 0) // 10
            if done > before:
                print('100%' if done == 10 else f'{done * 10}%..', end='', flush=True)

        record = TrainRecord()
        metrics = train_epoch(self.model, self.train_loader, self.optimizer, self.loss_fn, stage, use_cutmix=flags.use_cutmix,
                              use_mixup=flags.use_mixup, cutmix_alpha=flags.cutmix_alpha, mixup_alpha=flags.mixup_alpha,
                              mix_loss=self.mix_loss, gradient_clip=flags.gradient_clip, record=record, progress=progress)
        self.last_train_record = record
        print(f" Loss: {metrics['loss']:.4f}, Acc: {metrics['accuracy']:.2f}%")          # after the epoch's one synchronisation
        if record.nonfinite_batches:
            print(f'  {record.nonfinite_batches} of {record.n_batches} batches had a non-finite loss')
        return metrics

    def _has_ema(self) -> bool:
        return getattr(self.optimizer, 'ema_decay', None) is not None

    def val_epoch(self) -> Dict[str, float]:
        if self._has_ema():
            with self.optimizer.swap_ema():
                return validate(self.model, self.val_loader, self.loss_fn)
        return validate(self.model, self.val_loader, self.loss_fn)

    def fit(self) -> Dict[str, List[float]]:
        cfg, flags = self.config, self.config.flags
        print(f'\n{RULE}\nStarting Training\n{RULE}')
        print(f'Device: {self.device}\nTotal Epochs: {cfg.train.epochs}\nCurriculum: {getattr(flags, "curriculum", None)}')
        print(f'Mixed Precision: {flags.mixed_precision} (bf16 backbone, no loss scaling)\n{RULE}\n')
        if flags.freeze_backbone_epochs > 0:
            self.model.freeze_backbone()
            print(f'Backbone frozen for first {flags.freeze_backbone_epochs} epochs\n')
        history = {'train_loss': [], 'val_loss': [], 'train_acc': [], 'val_acc': []}
        for epoch in range(1, cfg.train.epochs + 1):
            train_metrics = self.train_epoch(epoch)
            val_metrics = self.val_epoch()
            self.scheduler.step()
            if self.logger:
                self.logger.log_epoch(epoch, cfg.get_stage_for_epoch(epoch), train_metrics, val_metrics)
            print(f'\nEpoch {epoch}/{cfg.train.epochs}')
            print(f"  Train Loss: {train_metrics['loss']:.4f} | Acc: {train_metrics['accuracy']:.2f}%")
            print(f"  Val Loss: {val_metrics['loss']:.4f} | Acc: {val_metrics['accuracy']:.2f}%")
            history['train_loss'].append(train_metrics['loss'])
            history['val_loss'].append(val_metrics['loss'])
            history['train_acc'].append(train_metrics['accuracy'])
            history['val_acc'].append(val_metrics['accuracy'])
            if val_metrics['loss'] < self.best_val_loss:
                self.best_val_loss, self.best_epoch, self.patience_counter = val_metrics['loss'], epoch, 0
                self.save_checkpoint(Path(cfg.paths.checkpoints_dir) / 'best_model.pth', epoch, val_metrics)
                print(f"  [BEST] New best model saved (Val Loss: {val_metrics['loss']:.4f})")
            else:
                self.patience_counter += 1
                print(f'  No improvement ({self.patience_counter}/{cfg.train.early_stop_patience})')
            if self.patience_counter >= cfg.train.early_stop_patience:
                print(f'\n{RULE}\nEarly stopping triggered at epoch {epoch}')
                print(f'Best epoch: {self.best_epoch} (Val Loss: {self.best_val_loss:.4f})\n{RULE}\n')
                break
        print(f'\n{RULE}\nTraining Complete\nBest Epoch: {self.best_epoch}\nBest Val Loss: {self.best_val_loss:.4f}\n{RULE}\n')
        return history

    def save_checkpoint(self, path, epoch: int, metrics: Dict) -> None:
        """The reference's keys, minus ``scaler_state_dict`` (there is no scaler); plus ``ema_state_dict`` with an averaging optimizer."""
        ck = {'epoch': epoch, 'model_state_dict': self.model.state_dict(), 'optimizer_state_dict': self.optimizer.state_dict(),
              'scheduler_state_dict': self.scheduler.state_dict(), 'best_val_loss': self.best_val_loss, 'metrics': metrics,
              'config': self.config}
        if self._has_ema():
            ck['ema_state_dict'] = self.optimizer.ema_state_dict()
        if self.patch_keep != 1.0:
            ck['patch_dropout_step'] = self.model.backbone.patch_dropout_step
        torch.save(ck, path)

    def load_checkpoint(self, path) -> None:
        """Restores model, optimiser, scheduler and ``best_val_loss``; a ``scaler_state_dict`` (a reference checkpoint) is ignored.  The
        checkpoint holds the pickled config object, so it is read with ``weights_only=False``: load only files you wrote."""
        checkpoint = torch.load(path, map_location=self.device, weights_only=False)
        self.model.load_state_dict(checkpoint['model_state_dict'])
        self.optimizer.load_state_dict(checkpoint['optimizer_state_dict'])
        if self._has_ema() and 'ema_state_dict' in checkpoint:
            self.optimizer.load_ema_state_dict(checkpoint['ema_state_dict'])
        if self.patch_keep != 1.0 and 'patch_dropout_step' in checkpoint:
            self.model.backbone.patch_dropout_step = checkpoint['patch_dropout_step']
        self.scheduler.load_state_dict(checkpoint['scheduler_state_dict'])
        self.best_val_loss = checkpoint['best_val_loss']
        print(f"Checkpoint loaded from {path}\nEpoch: {checkpoint['epoch']}\nVal Loss: {checkpoint['best_val_loss']:.4f}")
