"""A training epoch with one device synchronisation.

Replaces the body of the reference's ``Trainer.train_epoch`` (training/trainer.py:79-160).  With CutMix / MixUp on, that loop calls the
loss twice on the same head outputs, mixes the five dict entries with 15 element-wise launches on 0-dim tensors, back-propagates
through that arithmetic, and reads six values per step with ``.item()``, each of which drains the queue.

``train_epoch`` calls ``JointLoss.mixed`` instead: ONE launch (``rovit_joint_loss_mixed``) computes the mixed loss, its gradient, and
writes the batch's row of a ``TrainRecord`` -- the five losses, the number of rows whose argmax equals the first label column, the batch
size and a non-finite flag -- at a row index the host already knows.  ``TrainRecord.compute`` launches ``rovit_train_finalize`` and copies
its 9-word result block to the host: the epoch's only synchronisation.

On CPU tensors ``TrainRecord`` keeps the rows on the host and reduces them with numpy in fp64, as ``EvalAccumulator`` does, so the host
logic (and ``training.Trainer``) is testable without a GPU.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import native
from .native import RovitHipError

LOSS_KEYS = ('cls_loss', 'ord_loss', 'unc_loss', 'kan_loss', 'total_loss')        # order of rovit_joint_loss_mixed's losses_out


def result_block_from_rows(rows: np.ndarray) -> np.ndarray:
    """The result block of ``rovit_train_finalize`` (include/rovit_hip.h) from epoch-table rows (n, 8) of 4-byte words, on the host:
    int64 words with the fp64 section stored bit for bit."""
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, native.TRAIN_ROW_WORDS)
    blk = np.zeros(native.TRAIN_RESULT_WORDS, dtype=np.int64)
    blk[native.TRAIN_N_ROWS] = rows.shape[0]
    blk[native.TRAIN_SAMPLES] = rows[:, native.TRAIN_ROW_BATCH].astype(np.int64).sum()
    blk[native.TRAIN_CORRECT] = rows[:, native.TRAIN_ROW_CORRECT].astype(np.int64).sum()
    blk[native.TRAIN_NONFINITE] = rows[:, native.TRAIN_ROW_NONFINITE].astype(np.int64).sum()
    losses = rows[:, native.TRAIN_ROW_LOSS:native.TRAIN_ROW_LOSS + 5].copy().view(np.float32).astype(np.float64)
    blk.view(np.float64)[native.TRAIN_LOSS:native.TRAIN_LOSS + 5] = losses.sum(axis=0)
    return blk


class TrainRecord:
    """Score card of one training epoch; see the module docstring.  Nothing but ``compute`` / ``result_block`` synchronises.

    ``n`` (samples) and ``n_batches`` are counted on the host; ``nonfinite_batches`` -- the batches whose total loss was not finite, what a
    ``GradScaler``'s skipped steps would have told the user -- comes from the result block, so reading it is ``compute``'s synchronisation."""

    def __init__(self, capacity: int = 256):
        if not (isinstance(capacity, int) and 1 <= capacity <= native.TRAIN_MAX_ROWS):
            raise RovitHipError(f'TrainRecord: capacity must be in 1..{native.TRAIN_MAX_ROWS}, got {capacity!r}')
        self._capacity0 = capacity
        self._table: Optional[torch.Tensor] = None          # device: (capacity, 8) int32 words; kept across reset()
        self.reset()

    def reset(self) -> None:
        self.n = 0
        self.n_batches = 0
        self.device: Optional[torch.device] = None
        self._cpu: List[np.ndarray] = []                    # CPU path: one row of 8 words per batch
        self._block: Optional[np.ndarray] = None

    # -- device table: rows are written by rovit_joint_loss_mixed (JointLoss.mixed(record=...)) --
    def _bind(self, device: torch.device) -> None:
        if self.device is None:
            self.device = device
        elif device != self.device:
            raise RovitHipError(f'TrainRecord: batch on {device}, earlier batches on {self.device}; reset() first')

    def _next_row(self, device: torch.device):
        """(table, row, capacity) for the next launch; grows the table by doubling with a stream-ordered device copy."""
        self._bind(device)
        if self._table is not None and self._table.device != device:
            self._table = None                           # left from an epoch on another device
        cap = self._table.shape[0] if self._table is not None else 0
        if self.n_batches + 1 > cap:
            if self.n_batches + 1 > native.TRAIN_MAX_ROWS:
                raise RovitHipError(f'TrainRecord: more than {native.TRAIN_MAX_ROWS} batches in one epoch')
            new = torch.empty((min(native.TRAIN_MAX_ROWS, max(2 * cap, self._capacity0)), native.TRAIN_ROW_WORDS), dtype=torch.int32, device=device)
            if self._table is not None:
                new[:self.n_batches].copy_(self._table[:self.n_batches])          # device-to-device: no synchronisation
            self._table = new
        return self._table, self.n_batches, self._table.shape[0]

    def _commit(self, batch: int) -> None:
        self._block = None
        self.n += batch
        self.n_batches += 1

    # -- host path --
    def update(self, losses, cls_logits: torch.Tensor, class_labels: torch.Tensor) -> None:
        """Record one batch from CPU tensors: the loss dict (or a 5-vector [cls, ord, unc, kan, total]), the class logits and the labels
        the accuracy is counted against (training/trainer.py:144-153).  Device batches are recorded by the loss launch itself:
        ``JointLoss.mixed(..., record=self)``."""
        logits = cls_logits.detach()
        if logits.is_cuda:
            raise RovitHipError('TrainRecord.update is the host path; on the device the row is written by JointLoss.mixed(..., record=)')
        self._bind(logits.device)
        if isinstance(losses, torch.Tensor):
            vec = losses.detach().reshape(-1).float()
        else:
            vec = torch.stack([losses[k].detach().float().reshape(()) for k in LOSS_KEYS])
        if vec.numel() != 5:
            raise RovitHipError(f'TrainRecord.update: a loss tensor must hold 5 values [cls, ord, unc, kan, total], got {vec.numel()}')
        labels = class_labels.detach().reshape(-1).long()
        if logits.dim() != 2 or labels.numel() != logits.shape[0]:
            raise RovitHipError(f'TrainRecord.update: logits {tuple(logits.shape)} against {labels.numel()} labels')
        row = np.zeros(native.TRAIN_ROW_WORDS, dtype=np.int32)
        row[native.TRAIN_ROW_LOSS:native.TRAIN_ROW_LOSS + 5] = vec.numpy().astype(np.float32).view(np.int32)
        row[native.TRAIN_ROW_CORRECT] = int(logits.max(1)[1].eq(labels).sum())
        row[native.TRAIN_ROW_BATCH] = logits.shape[0]
        row[native.TRAIN_ROW_NONFINITE] = 0 if np.isfinite(float(vec[4])) else 1
        self._cpu.append(row)
        self._commit(int(logits.shape[0]))

    # -- results --
    def rows(self) -> np.ndarray:
        """The recorded rows (n_batches, 8) as int32 words on the host (a device-to-host copy of the table on the device path)."""
        if self.n_batches < 1:
            raise RovitHipError('TrainRecord: nothing recorded yet')
        if self.device.type == 'cuda':
            return self._table[:self.n_batches].cpu().numpy()
        return np.stack(self._cpu)

    def result_block(self) -> np.ndarray:
        """The finalise's result block as 9 int64 words on the host (fp64 section bit for bit).  On the device this is the epoch's one
        synchronising call; the block is kept until the next batch or ``reset``."""
        if self._block is not None:
            return self._block
        if self.n_batches < 1:
            raise RovitHipError('TrainRecord: nothing recorded yet')
        if self.device.type != 'cuda':
            self._block = result_block_from_rows(np.stack(self._cpu))
            return self._block
        result = torch.empty(native.TRAIN_RESULT_WORDS, dtype=torch.int64, device=self.device)
        d = native.TrainFinal()
        d.n_rows, d.capacity = self.n_batches, self._table.shape[0]
        d.table, d.result = native.ptr(self._table), native.ptr(result)
        native.call('rovit_train_finalize', ctypes.byref(d), native.stream_ptr())
        self._block = result.cpu().numpy()               # the single device-to-host copy of the epoch
        return self._block

    @property
    def nonfinite_batches(self) -> int:
        return int(self.result_block()[native.TRAIN_NONFINITE])

    def compute(self) -> Dict[str, float]:
        """loss, cls_loss, ord_loss, unc_loss, kan_loss as means over BATCHES (the reference divides by ``len(loader)``,
        training/trainer.py:172-178) and accuracy in percent over samples."""
        blk = self.result_block()
        sums = blk.view(np.float64)[native.TRAIN_LOSS:native.TRAIN_LOSS + 5]
        nb = int(blk[native.TRAIN_N_ROWS])
        correct, total = int(blk[native.TRAIN_CORRECT]), int(blk[native.TRAIN_SAMPLES])
        if nb != self.n_batches or total != self.n:
            raise RovitHipError(f'TrainRecord: the device counted {nb} batches / {total} samples, the host {self.n_batches} / {self.n}')
        m = {('loss' if k == 'total_loss' else k): float(sums[i]) / nb for i, k in enumerate(LOSS_KEYS)}
        m['accuracy'] = 100. * correct / total            # the trainer's own expression (trainer.py:178)
        return {k: m[k] for k in ('loss', 'cls_loss', 'ord_loss', 'unc_loss', 'kan_loss', 'accuracy')}


def train_epoch(model: torch.nn.Module, loader, optimizer, loss_fn, stage: int, *, use_cutmix: bool, use_mixup: bool,
                cutmix_alpha: float = 1.0, mixup_alpha: float = 0.2, mix_loss: bool = True, gradient_clip: Optional[float] = None,
                rng=None, record: Optional[TrainRecord] = None, progress: Optional[Callable[[int], None]] = None) -> Dict[str, float]:
    """The body of the reference's ``Trainer.train_epoch`` (training/trainer.py:54-181) with one synchronisation, at the end.

    Per batch: ``data.transforms.cutmix_or_mixup`` when either flag is set (``rng``: its numpy generator), the forward, ``loss_fn.mixed``
    (one launch: loss, gradient and the batch's row of the record), ``zero_grad``, ``backward``, the gradient clip and the step.  A
    ``RoViTAdamW`` clips inside ``step()``; for any other optimiser ``clip_grad_norm_(model.parameters(), gradient_clip)`` is called as the
    reference does.  ``mix_loss=False`` is the reference's branch without a scaler (trainer.py:131-133): the images are mixed, the loss is
    taken against the unmixed labels.  ``record``: a ``TrainRecord`` to fill (reset first); ``progress(batch_index)`` is called after every
    step and receives no device value.  Returns the reference's six metrics."""
    from data.transforms import cutmix_or_mixup
    from .optim import RoViTAdamW
    if not hasattr(loss_fn, 'mixed'):
        raise RovitHipError('train_epoch needs a loss with a .mixed() method (rovit_hip.losses.JointLoss)')
    model.train()
    model.curriculum_stage = stage
    dev = next(model.parameters()).device
    rec = record if record is not None else TrainRecord()
    rec.reset()
    own_clip = gradient_clip is not None and not isinstance(optimizer, RoViTAdamW)
    for batch_idx, (images, class_labels, severity_labels) in enumerate(loader):
        images = images.to(dev, non_blocking=True)
        class_labels = class_labels.to(dev, non_blocking=True)
        severity_labels = severity_labels.to(dev, non_blocking=True)
        labels_b, lam = None, 1.0
        if use_cutmix or use_mixup:
            images, _, labels_b, lam = cutmix_or_mixup(images, class_labels, use_cutmix=use_cutmix, use_mixup=use_mixup,
                                                       cutmix_alpha=cutmix_alpha, mixup_alpha=mixup_alpha, rng=rng)
            if not mix_loss:
                labels_b, lam = None, 1.0
        outputs = model(images)
        losses = loss_fn.mixed(outputs, class_labels, labels_b, lam, severity_labels, stage, record=rec)
        optimizer.zero_grad()
        losses['total_loss'].backward()
        if own_clip:
            torch.nn.utils.clip_grad_norm_(model.parameters(), gradient_clip)
        optimizer.step()
        if progress is not None:
            progress(batch_idx)
    if rec.n_batches < 1:
        raise RovitHipError('train_epoch: the loader yielded no batch')
    return rec.compute()
