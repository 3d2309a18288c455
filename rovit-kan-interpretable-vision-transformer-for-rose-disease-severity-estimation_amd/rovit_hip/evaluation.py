"""Test-set evaluation and validation with one device synchronisation per epoch.

Replaces the collection loop of the reference's ``Evaluator.evaluate`` (evaluation/evaluator.py:37-67: softmax, argmax, squeeze,
exp and five device-to-host copies per batch), the six ``.item()`` per batch of ``Trainer.val_epoch`` (training/trainer.py:183-231)
and the sklearn / scipy calls of evaluation/metrics.py.

``EvalAccumulator.update`` is ONE launch per batch (``rovit_eval_accumulate``): it records probabilities, predicted class, label,
predicted and true severity, exp(0.5 log_var) and, optionally, the five loss values ``JointLoss`` left on the device, at a row offset
the host already knows.  ``compute`` launches ``rovit_eval_finalize`` and copies its 272-word result block to the host: the epoch's only
synchronisation.  Everything reported is derived from that block on the host in fp64.

``EvalAccumulator.bootstrap`` and ``paired_bootstrap`` put percentile intervals and a paired test on those numbers
(``rovit_eval_bootstrap``: every resample's score card on the device, one copy for the whole call); ``bootstrap_reference`` is their
numpy restatement.

``EvalAccumulator.selective`` scores the uncertainty estimates (``rovit_eval_selective``): risk-coverage curves, AURC, E-AURC and the
accept thresholds of every (score, risk) pair, one copy for the whole call; ``selective_reference`` states the definitions in numpy fp64.

``EvalAccumulator.calibrate`` acts on the score card (``rovit_eval_calibrate``): one temperature for the classifier, one scale for the
Gaussian head's sigma and the observed coverage of its central intervals, fitted on the recorded rows (normally the validation split)
with a fixed number of launches and one copy; ``Calibration.apply`` (``rovit_eval_recalibrate``) gives the calibrated record as a new
accumulator, ``Calibration.transform`` rescales a model's output dict for deployment; ``calibration_reference`` is the numpy statement.

``EvalAccumulator.conformal`` turns the recorded rows (normally the validation split) into distribution-free guarantees
(``rovit_eval_conformal``): split-conformal thresholds of label-set scores (LAC, APS, RAPS) and severity residuals, each ONE order
statistic found by an O(n) radix select, one copy for the whole call; ``Conformal.evaluate`` scores test rows against them
(``rovit_eval_conformal_apply``), ``Conformal.predict`` gives label sets and severity intervals for deployment;
``conformal_reference`` is the numpy statement.

``EvalAccumulator.rank_method`` (``'auto'``, ``'count'`` or ``'sort'``) chooses how the finalise and ``selective`` rank their columns: the
O(n^2) counting rank, or the device radix sort of ``rovit_hip.rank`` from ``native.RANK_SORT_ROWS`` rows on; the result blocks are
byte-identical either way.

On CPU tensors the same class runs the plain torch / numpy fp64 restatement below (``result_block_from_arrays``), as
``JointLoss._forward_tensor_ops`` does: the host logic is testable without a GPU, and ``evaluation.metrics`` is built on it.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import native
from .native import RovitHipError

LOSS_KEYS = ('cls_loss', 'ord_loss', 'unc_loss', 'kan_loss', 'total_loss')        # order of rovit_joint_loss's losses_out


# ---- host restatement (fp64 / exact integers) -----------------------------------------------------------------------------------

def doubled_ranks(x: np.ndarray) -> np.ndarray:
    """R_i = 2 #{x_j < x_i} + #{x_j == x_i} + 1: twice the tie-averaged rank, an exact integer (mean exactly n + 1)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    s = np.sort(x)
    lo = np.searchsorted(s, x, side='left').astype(np.int64)
    hi = np.searchsorted(s, x, side='right').astype(np.int64)
    return 2 * lo + (hi - lo) + 1


def rank_sums(a: np.ndarray, b: np.ndarray):
    """(sum da db, sum da^2, sum db^2, non-finite in a, non-finite in b) with d = R - n - 1, as Python integers."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    n = a.shape[0]
    bad_a, bad_b = int((~np.isfinite(a)).sum()), int((~np.isfinite(b)).sum())
    if bad_a or bad_b:
        return 0, 0, 0, bad_a, bad_b
    da = (doubled_ranks(a) - (n + 1)).astype(object)          # Python integers: exact beyond int64 too
    db = (doubled_ranks(b) - (n + 1)).astype(object)
    return int((da * db).sum()), int((da * da).sum()), int((db * db).sum()), 0, 0


def rho_from_rank_sums(sab: int, saa: int, sbb: int, bad_a: int = 0, bad_b: int = 0) -> float:
    """Spearman's rho = Pearson correlation of the tie-averaged ranks; NaN for a constant column or any non-finite value."""
    if bad_a or bad_b or saa <= 0 or sbb <= 0:
        return float('nan')
    return float(sab) / (math.sqrt(float(saa)) * math.sqrt(float(sbb)))


def bin_edges(n_bins: int) -> np.ndarray:
    return np.linspace(0, 1, n_bins + 1)


def result_block_from_arrays(y_true, y_pred, y_probs, severity_true, severity_pred, num_classes: int, n_bins: int = 10,
                             loss_rows: Optional[np.ndarray] = None) -> np.ndarray:
    """The result block of ``rovit_eval_finalize`` (include/rovit_hip.h) from recorded arrays, on the host: int64 words with the fp64
    section stored bit for bit.  Sums are over the whole arrays, so the block cannot depend on how the rows arrived."""
    C = int(num_classes)
    y_true = np.asarray(y_true).astype(np.int64).reshape(-1)
    y_pred = np.asarray(y_pred).astype(np.int64).reshape(-1)
    p = np.asarray(y_probs, dtype=np.float64).reshape(len(y_true), C)
    st = np.asarray(severity_true, dtype=np.float64).reshape(-1)
    sp = np.asarray(severity_pred, dtype=np.float64).reshape(-1)
    n = len(y_true)
    blk = np.zeros(native.EVAL_RESULT_WORDS, dtype=np.int64)
    f = blk.view(np.float64)
    ok = (y_true >= 0) & (y_true < C)
    pred = np.clip(y_pred, 0, C - 1)
    blk[native.EVAL_CONFUSION:native.EVAL_CONFUSION + C * C] = np.bincount(y_true[ok] * C + pred[ok], minlength=C * C)
    conf = p[np.arange(n), pred]
    edges = bin_edges(n_bins)
    correct = pred == y_true
    for k in range(n_bins):
        m = (conf > edges[k]) & (conf <= edges[k + 1])
        blk[native.EVAL_BIN_COUNT + k] = int(m.sum())
        blk[native.EVAL_BIN_CORRECT + k] = int((m & correct).sum())
        f[native.EVAL_BIN_CONF + k] = conf[m].sum()
    onehot = np.zeros_like(p)
    onehot[np.arange(n)[ok], y_true[ok]] = 1.0
    f[native.EVAL_BRIER] = ((p - onehot) ** 2).sum(axis=1).sum()
    f[native.EVAL_ABS_ERR] = np.abs(st - sp).sum()
    sab, saa, sbb, bad_a, bad_b = rank_sums(st, sp)
    blk[native.EVAL_RANK:native.EVAL_RANK + 3] = [sab, saa, sbb]
    blk[native.EVAL_NONFINITE:native.EVAL_NONFINITE + 2] = [bad_a, bad_b]
    blk[native.EVAL_BAD_LABELS] = int((~ok).sum())
    blk[native.EVAL_N] = n
    if loss_rows is not None and len(loss_rows):
        f[native.EVAL_LOSS:native.EVAL_LOSS + 5] = np.asarray(loss_rows, dtype=np.float64).reshape(-1, 5).sum(axis=0)
    return blk


def prf_from_confusion(cm: np.ndarray):
    """precision, recall, F1 (fractions) and support per class with sklearn's ``zero_division=0``."""
    cm = np.asarray(cm, dtype=np.float64)
    tp = np.diag(cm)
    pred_n, true_n = cm.sum(axis=0), cm.sum(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        prec = np.where(pred_n > 0, tp / pred_n, 0.0)
        rec = np.where(true_n > 0, tp / true_n, 0.0)
        f1 = np.where(pred_n + true_n > 0, 2.0 * tp / (pred_n + true_n), 0.0)
    return prec, rec, f1, true_n.astype(np.int64)


def f1_averages(cm: np.ndarray):
    """(macro, weighted) F1 as fractions.  Macro averages over the classes that occur in the labels or the predictions, which is what
    ``f1_score(average='macro')`` without ``labels=`` does; weighted weighs by support."""
    _, _, f1, support = prf_from_confusion(cm)
    cm = np.asarray(cm)
    present = (cm.sum(axis=0) + cm.sum(axis=1)) > 0
    macro = float(f1[present].mean()) if present.any() else 0.0
    weighted = float((f1 * support).sum() / support.sum()) if support.sum() > 0 else 0.0
    return macro, weighted


def metrics_from_block(blk: np.ndarray, num_classes: int, n_bins: int, n_loss_rows: int = 0) -> Dict:
    """Every reported metric from one result block (reference units: percent where evaluation/metrics.py returns percent)."""
    C = int(num_classes)
    blk = np.asarray(blk, dtype=np.int64)
    f = blk.view(np.float64)
    n = int(blk[native.EVAL_N])
    if n < 1:
        raise RovitHipError('evaluation: no samples recorded')
    if int(blk[native.EVAL_BAD_LABELS]):
        raise RovitHipError(f'evaluation: {int(blk[native.EVAL_BAD_LABELS])} class labels outside [0, {C})')
    cm = blk[native.EVAL_CONFUSION:native.EVAL_CONFUSION + C * C].reshape(C, C).copy()
    prec, rec, f1, support = prf_from_confusion(cm)
    macro, weighted = f1_averages(cm)
    ece = 0.0
    for k in range(n_bins):
        cnt = int(blk[native.EVAL_BIN_COUNT + k])
        if cnt > 0:
            ece += abs(f[native.EVAL_BIN_CONF + k] / cnt - int(blk[native.EVAL_BIN_CORRECT + k]) / cnt) * (cnt / n)
    rho = rho_from_rank_sums(*(int(v) for v in blk[native.EVAL_RANK:native.EVAL_RANK + 5]))
    m = {'n': n, 'correct': int(np.trace(cm)), 'accuracy': float(np.trace(cm)) / n * 100.0, 'macro_f1': macro * 100.0, 'weighted_f1': weighted * 100.0,
         'mae': float(f[native.EVAL_ABS_ERR]) / n, 'spearman_rho': rho, 'spearman': rho, 'brier_score': float(f[native.EVAL_BRIER]) / n,
         'ece': float(ece), 'confusion_matrix': cm,
         'per_class': [{'precision': float(prec[c]) * 100.0, 'recall': float(rec[c]) * 100.0, 'f1': float(f1[c]) * 100.0,
                        'support': int(support[c])} for c in range(C)]}
    if n_loss_rows > 0:
        sums = f[native.EVAL_LOSS:native.EVAL_LOSS + 5]
        for k, name in enumerate(LOSS_KEYS):
            m['loss' if name == 'total_loss' else name] = float(sums[k]) / n_loss_rows          # means over BATCHES (trainer.py:221-228)
    return m


# ---- the accumulator ---------------------------------------------------------------------------------------------------------

def _loss_vector(losses) -> torch.Tensor:
    """The five loss values as one contiguous fp32 vector [cls, ord, unc, kan, total], without a launch when they already are one
    (``JointLoss`` on the device returns views of the kernel's five-float output)."""
    if isinstance(losses, torch.Tensor):
        v = losses.detach().reshape(-1)
        if v.numel() != 5:
            raise RovitHipError(f'evaluation: a loss tensor must hold 5 values [cls, ord, unc, kan, total], got {v.numel()}')
        return v.float().contiguous()
    ts = [losses[k].detach() for k in LOSS_KEYS]
    base = ts[0]
    if all(t.dtype == torch.float32 and t.numel() == 1 and t.device == base.device
           and t.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
           and t.storage_offset() == base.storage_offset() + i for i, t in enumerate(ts)):
        return base.as_strided((5,), (1,), base.storage_offset())
    return torch.stack([t.float().reshape(()) for t in ts])


class EvalAccumulator:
    """Streaming score card of one pass over a data set; see the module docstring.  ``update`` never synchronises."""

    def __init__(self, num_classes: int, n_bins: int = 10, capacity: int = 4096):
        if not (isinstance(num_classes, int) and 2 <= num_classes <= native.EVAL_MAX_CLASSES):
            raise RovitHipError(f'EvalAccumulator: num_classes must be in 2..{native.EVAL_MAX_CLASSES}, got {num_classes!r}')
        if not (isinstance(n_bins, int) and 1 <= n_bins <= native.EVAL_MAX_BINS):
            raise RovitHipError(f'EvalAccumulator: n_bins must be in 1..{native.EVAL_MAX_BINS}, got {n_bins!r}')
        if not (isinstance(capacity, int) and 1 <= capacity <= native.EVAL_MAX_ROWS):
            raise RovitHipError(f'EvalAccumulator: capacity must be in 1..{native.EVAL_MAX_ROWS}, got {capacity!r}')
        self.num_classes, self.n_bins, self._capacity0 = num_classes, n_bins, capacity
        self.rank_method = 'auto'                                  # 'count' | 'sort' | 'auto': how _finalize and selective rank; no result depends on it
        self.reset()

    def reset(self) -> None:
        self.n = 0
        self.n_loss_rows = 0
        self.device: Optional[torch.device] = None
        self._has_uncertainty = False
        self._rec: Dict[str, torch.Tensor] = {}
        self._loss_table: Optional[torch.Tensor] = None
        self._edges: Optional[torch.Tensor] = None
        self._cpu: List[Dict[str, torch.Tensor]] = []          # CPU path: the batches as they came
        self._cpu_losses: List[torch.Tensor] = []
        self._block: Optional[np.ndarray] = None
        self._block_dev: Optional[torch.Tensor] = None         # the finalise's block and rank counts on the device: bootstrap() reads them
        self._rank_counts: Optional[torch.Tensor] = None
        self._extra_names: Optional[tuple] = None              # fixed by the first update that passes ``extra``
        self._extra: Dict[str, torch.Tensor] = {}              # device path: growable fp32 columns beside the record

    # -- device record arrays --
    _FIELDS = (('probs', torch.float32), ('pred', torch.int32), ('label', torch.int32), ('sev_pred', torch.float32),
               ('sev_true', torch.float32), ('uncertainty', torch.float32))

    def _alloc(self, cap: int) -> Dict[str, torch.Tensor]:
        return {k: torch.empty((cap, self.num_classes) if k == 'probs' else (cap,), dtype=dt, device=self.device) for k, dt in self._FIELDS}

    def _reserve(self, rows: int) -> None:
        cap = self._rec['pred'].shape[0] if self._rec else 0
        if rows <= cap:
            return
        if rows > native.EVAL_MAX_ROWS:
            raise RovitHipError(f'EvalAccumulator: {rows} samples exceed the limit of {native.EVAL_MAX_ROWS} (the rank sums are exact in '
                                'int64 up to there)')
        new_cap = min(native.EVAL_MAX_ROWS, max(rows, 2 * cap, self._capacity0))
        new = self._alloc(new_cap)
        for k, t in self._rec.items():
            new[k][:self.n].copy_(t[:self.n])             # device-to-device, stream-ordered: no synchronisation
        self._rec = new
        for k, t in self._extra.items():
            self._extra[k] = torch.empty(new_cap, dtype=torch.float32, device=self.device)
            self._extra[k][:self.n].copy_(t[:self.n])

    def _reserve_losses(self, rows: int) -> None:
        cap = self._loss_table.shape[0] if self._loss_table is not None else 0
        if rows <= cap:
            return
        new = torch.empty((max(rows, 2 * cap, 256), 5), dtype=torch.float32, device=self.device)
        if self._loss_table is not None:
            new[:self.n_loss_rows].copy_(self._loss_table[:self.n_loss_rows])
        self._loss_table = new

    def update(self, outputs: Dict[str, Optional[torch.Tensor]], class_labels: torch.Tensor, severity_labels: torch.Tensor,
               losses=None, extra: Optional[Dict[str, torch.Tensor]] = None) -> None:
        """Record one batch: the model's output dict, the class labels and the severity labels (host or device tensors), and
        optionally the dict ``JointLoss`` returned (or a 5-vector [cls, ord, unc, kan, total]).  ``extra``: named per-row (B,) or (B, 1)
        tensors (``{'mu': outputs['mu'], 'mutual_information': mc['mutual_information']}``) kept as fp32 columns beside the record for
        ``selective``; the first ``update`` that passes one fixes the set of names, and it must be the accumulator's first batch."""
        logits = outputs['cls_logits'].detach()
        if logits.dim() != 2 or logits.shape[1] != self.num_classes or logits.shape[0] < 1:
            raise RovitHipError(f'EvalAccumulator.update: cls_logits must be (B >= 1, {self.num_classes}), got {tuple(logits.shape)}')
        B = logits.shape[0]
        kan, lv = outputs.get('kan_severity'), outputs.get('log_var')
        if outputs.get('mu') is None:
            lv = None                                     # evaluator.py:64: uncertainty needs both mu and log_var
        for name, t in (('kan_severity', kan), ('log_var', lv), ('class_labels', class_labels), ('severity_labels', severity_labels)):
            if t is not None and t.numel() != B:
                raise RovitHipError(f'EvalAccumulator.update: {name} has {t.numel()} values for a batch of {B}')
        if extra is not None:
            extra = self._check_extra(extra, B)
        elif self._extra_names is not None:
            raise RovitHipError(f'EvalAccumulator.update: earlier batches carried the extra columns {sorted(self._extra_names)}, this one none')
        if self.device is None:
            self.device = logits.device
        elif logits.device != self.device:
            raise RovitHipError(f'EvalAccumulator.update: batch on {logits.device}, earlier batches on {self.device}; reset() first')
        self._block = self._block_dev = self._rank_counts = None
        if lv is not None:
            self._has_uncertainty = True
        if not logits.is_cuda:
            self._cpu.append({'logits': logits.float(), 'kan': None if kan is None else kan.detach().float().reshape(-1),
                              'lv': None if lv is None else lv.detach().float().reshape(-1),
                              'label': class_labels.detach().long().reshape(-1).cpu(), 'sev': severity_labels.detach().reshape(-1).cpu(),
                              'extra': {} if extra is None else {k: t.detach().float().reshape(-1).cpu() for k, t in extra.items()}})
            if extra is not None:
                self._extra_names = tuple(extra)
            if losses is not None:
                self._cpu_losses.append(_loss_vector(losses).cpu())
                self.n_loss_rows += 1
            self.n += B
            return
        dev = self.device
        f = lambda t: None if t is None else t.detach().float().reshape(-1).contiguous()
        logits, kan, lv = logits.float().contiguous(), f(kan), f(lv)
        # host labels: an asynchronous copy on the current stream, not .numpy()
        labels = class_labels.detach().reshape(-1).to(dev, non_blocking=True).long().contiguous()
        sev = severity_labels.detach().reshape(-1).to(dev, non_blocking=True)
        sev_i64 = sev.dtype == torch.int64
        sev = (sev if sev_i64 else sev.float()).contiguous()
        self._reserve(self.n + B)
        lvec = None
        if losses is not None:
            lvec = _loss_vector(losses).to(dev, non_blocking=True)
            self._reserve_losses(self.n_loss_rows + 1)
        d = native.EvalBatch()
        d.batch, d.num_classes, d.offset, d.capacity, d.severity_is_int64 = B, self.num_classes, self.n, self._rec['pred'].shape[0], int(sev_i64)
        d.loss_row, d.loss_capacity = self.n_loss_rows, 0 if self._loss_table is None else self._loss_table.shape[0]
        d.cls_logits, d.kan_severity, d.log_var = native.ptr(logits), native.ptr(kan), native.ptr(lv)
        d.class_labels, d.severity_labels, d.losses = native.ptr(labels), native.ptr(sev), native.ptr(lvec)
        for k, _ in self._FIELDS:
            setattr(d, k, native.ptr(self._rec[k]))
        d.loss_table = native.ptr(self._loss_table)
        native.call('rovit_eval_accumulate', ctypes.byref(d), native.stream_ptr())
        if extra is not None:
            self._extra_names = tuple(extra)
            for k, t in extra.items():
                if k not in self._extra:
                    self._extra[k] = torch.empty(self._rec['pred'].shape[0], dtype=torch.float32, device=dev)
                self._extra[k][self.n:self.n + B].copy_(t.detach().reshape(-1), non_blocking=True)          # stream-ordered, converts to fp32
        self.n += B
        if lvec is not None:
            self.n_loss_rows += 1

    def _check_extra(self, extra, B: int) -> Dict[str, torch.Tensor]:
        if not isinstance(extra, dict) or not extra:
            raise RovitHipError('EvalAccumulator.update: extra must be a non-empty dict of per-row tensors')
        for k, t in extra.items():
            if not isinstance(k, str) or k in SELECTIVE_BUILTIN:
                raise RovitHipError(f'EvalAccumulator.update: {k!r} cannot name an extra column (a string other than {sorted(SELECTIVE_BUILTIN)})')
            if not isinstance(t, torch.Tensor) or t.numel() != B or t.dim() > 2:
                raise RovitHipError(f'EvalAccumulator.update: extra column {k!r} must be a (B,) or (B, 1) tensor for a batch of {B}')
        if self._extra_names is None and self.n > 0:
            raise RovitHipError(f'EvalAccumulator.update: {self.n} rows were recorded without extra columns; pass them from the first batch on')
        if self._extra_names is not None and set(extra) != set(self._extra_names):
            raise RovitHipError(f'EvalAccumulator.update: extra columns {sorted(extra)} differ from the {sorted(self._extra_names)} of the '
                                'first batch')
        return extra

    # -- results --
    def _cpu_arrays(self):
        cat = lambda k: torch.cat([b[k] for b in self._cpu])
        logits = cat('logits')
        probs = torch.softmax(logits, dim=1)
        sev_true = torch.cat([b['sev'].float() for b in self._cpu])
        sev_pred = torch.cat([b['sev'].float() if b['kan'] is None else b['kan'] for b in self._cpu])
        unc = torch.cat([torch.full((len(b['label']),), float('nan')) if b['lv'] is None else torch.exp(0.5 * b['lv']) for b in self._cpu])
        label = cat('label')
        label = torch.where((label >= 0) & (label < self.num_classes), label, torch.full_like(label, -1))
        return {'probs': probs.numpy(), 'pred': torch.argmax(probs, dim=1).numpy().astype(np.int32), 'label': label.numpy().astype(np.int32),
                'sev_pred': sev_pred.numpy(), 'sev_true': sev_true.numpy(), 'uncertainty': unc.numpy()}

    def result_block(self) -> np.ndarray:
        """The finalise's result block as 272 int64 words on the host (fp64 section bit for bit).  On the device this is the epoch's
        one synchronising call; the block is kept until the next ``update`` or ``reset``."""
        if self._block is not None:
            return self._block
        if self.n < 1:
            raise RovitHipError('EvalAccumulator: nothing recorded yet')
        if not self.device.type == 'cuda':
            a = self._cpu_arrays()
            rows = torch.stack(self._cpu_losses).numpy() if self._cpu_losses else None
            self._block = result_block_from_arrays(a['label'], a['pred'], a['probs'], a['sev_true'], a['sev_pred'], self.num_classes,
                                                   self.n_bins, rows)
            return self._block
        self._block = self._finalize().cpu().numpy()     # the single device-to-host copy of the epoch
        return self._block

    def _finalize(self) -> torch.Tensor:
        """Launch ``rovit_eval_finalize`` (once per set of rows) and return its result block on the device.  The block and the rank
        counts stay alive until the next ``update`` or ``reset``: they are the bootstrap kernel's inputs."""
        if self._block_dev is not None:
            return self._block_dev
        dev = self.device
        if self._edges is None:
            self._edges = torch.from_numpy(bin_edges(self.n_bins)).to(dev, non_blocking=True)
        counts = torch.empty(4 * self.n, dtype=torch.int32, device=dev)
        partials = torch.empty(native.load().rovit_eval_partials_doubles(self.n), dtype=torch.float64, device=dev)
        result = torch.empty(native.EVAL_RESULT_WORDS, dtype=torch.int64, device=dev)
        d = native.EvalFinal()
        d.n, d.num_classes, d.n_bins, d.n_loss_rows = self.n, self.num_classes, self.n_bins, self.n_loss_rows
        for k in ('probs', 'pred', 'label', 'sev_pred', 'sev_true'):
            setattr(d, k, native.ptr(self._rec[k]))
        d.loss_table = native.ptr(self._loss_table)
        d.bin_edges, d.rank_counts, d.partials, d.result = (native.ptr(t) for t in (self._edges, counts, partials, result))
        method = native.rank_method(self.rank_method, self.n, 'EvalAccumulator.rank_method')
        rank_bytes = native.load().rovit_eval_finalize_rank_workspace_bytes(self.n) if method == native.RANK_SORT else 0
        rank_ws = torch.empty(rank_bytes, dtype=torch.uint8, device=dev) if rank_bytes else None
        native.call('rovit_eval_finalize_ex', ctypes.byref(d), method, native.ptr(rank_ws), rank_bytes, native.stream_ptr())
        self._block_dev, self._rank_counts = result, counts
        return result

    def compute(self) -> Dict:
        return metrics_from_block(self.result_block(), self.num_classes, self.n_bins, self.n_loss_rows)

    def arrays(self) -> Dict[str, Optional[np.ndarray]]:
        """``y_true, y_pred, y_probs, severity_true, severity_pred, uncertainty`` as numpy (what the reference's plots need);
        ``uncertainty`` is None when no batch carried mu and log_var."""
        if self.n < 1:
            raise RovitHipError('EvalAccumulator: nothing recorded yet')
        if self.device.type == 'cuda':
            a = {k: t[:self.n].cpu().numpy() for k, t in self._rec.items()}
        else:
            a = self._cpu_arrays()
        return {'y_true': a['label'].astype(np.int64), 'y_pred': a['pred'].astype(np.int64), 'y_probs': a['probs'],
                'severity_true': a['sev_true'], 'severity_pred': a['sev_pred'],
                'uncertainty': a['uncertainty'] if self._has_uncertainty else None}

    # -- selective prediction --
    def _selective_names(self, scores, risks, coverages):
        extras = self._extra_names or ()
        if scores is None:
            scores = ['confidence', 'entropy'] + (['sigma'] if self._has_uncertainty else [])
        if risks is None:
            risks = ['error', 'abs_err']
        if isinstance(scores, str) or isinstance(risks, str):
            raise RovitHipError('selective: scores and risks are sequences of names')
        scores, risks = list(scores), list(risks)
        if not (isinstance(coverages, int) and not isinstance(coverages, bool) and 1 <= coverages <= native.EVAL_SEL_MAX_COVERAGES):
            raise RovitHipError(f'selective: coverages must be an int in 1..{native.EVAL_SEL_MAX_COVERAGES}, got {coverages!r}')
        for what, names, limit, builtin in (('score', scores, native.EVAL_SEL_MAX_SCORES, SELECTIVE_SCORES),
                                            ('risk', risks, native.EVAL_SEL_MAX_RISKS, tuple(SELECTIVE_RISKS) + ('mu_abs_err',))):
            if not 1 <= len(names) <= limit or len(set(names)) != len(names):
                raise RovitHipError(f'selective: 1..{limit} distinct {what} names are needed, got {names!r}')
            for name in names:
                if name not in builtin and name not in extras:
                    raise RovitHipError(f'selective: unknown {what} {name!r} (known: {sorted(builtin)} and the extra columns {sorted(extras)})')
        if 'sigma' in scores and not self._has_uncertainty:
            raise RovitHipError("selective: the score 'sigma' needs batches that carried mu and log_var (no uncertainty head was recorded)")
        if 'mu_abs_err' in risks and 'mu' not in extras:
            raise RovitHipError("selective: the risk 'mu_abs_err' needs the extra column 'mu' (update(..., extra={'mu': outputs['mu']}))")
        return scores, risks

    def selective(self, scores: Optional[Sequence[str]] = None, risks: Optional[Sequence[str]] = None, coverages: int = 20,
                  return_keys: bool = False, _max_workgroups: int = 0) -> Dict:
        """Selective-prediction score card: does each uncertainty score know which rows the model gets wrong?

        ``scores`` (higher = less certain): ``'confidence'`` 1 - max p, ``'entropy'`` of the recorded probabilities, ``'sigma'`` the
        recorded exp(0.5 log_var), or the name of an ``extra`` column; default confidence and entropy, plus sigma when a batch carried mu
        and log_var.  ``risks`` (>= 0): ``'error'`` 1 where the prediction is wrong, ``'abs_err'`` |sev_true - sev_pred|, ``'mu_abs_err'``
        |sev_true - mu| (needs the extra column ``'mu'``), or an extra column; default error and abs_err.  The definitions are those
        of ``selective_reference``.  Returns ``{'n', 'coverages' (the actual k_p / n), 'risks': {risk: {'mean', 'oracle_aurc',
        'oracle_curve'}}, 'scores': {score: {'thresholds', risk: {'aurc', 'e_aurc', 'normalized', 'curve'}}}}``; ``thresholds[p]`` is the
        score value up to which rows are accepted to keep the fraction ``coverages[p]``.  ``return_keys`` adds ``'keys'`` (S, n) and
        ``'risk_values'`` (K, n), the fp32 columns that were ranked, and ``'block'``, the result block as int64 words.  On the device the call makes ONE device-to-host copy, and non-finite
        scores, non-finite or negative risks and class labels outside [0, C) raise after it."""
        if self.n < 1:
            raise RovitHipError('EvalAccumulator: nothing recorded yet')
        scores, risks = self._selective_names(scores, risks, coverages)
        S, K, P, n = len(scores), len(risks), coverages, self.n
        if self.device.type != 'cuda':
            extras = {k: torch.cat([b['extra'][k] for b in self._cpu]).numpy() for k in (self._extra_names or ())}
            keys, values = selective_columns(self._cpu_arrays(), extras, scores, risks)
            block = selective_block(keys, values, P, bad_labels=int((self._cpu_arrays()['label'] < 0).sum()))
        else:
            off = native.eval_selective_offsets(S, K, P)
            W = off['words']
            out = torch.empty(W + ((S + K) * n + 1) // 2 * int(bool(return_keys)), dtype=torch.int64, device=self.device)
            ws_bytes = native.load().rovit_eval_selective_workspace_bytes(n, S, K)
            workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            d = native.EvalSel()
            d.n, d.num_classes, d.num_scores, d.num_risks, d.num_coverages, d.max_workgroups = n, self.num_classes, S, K, P, _max_workgroups
            keep = []                                            # columns made for this call stay alive until it is enqueued
            for i, name in enumerate(scores):
                d.score_kind[i] = SELECTIVE_SCORES.get(name, native.EVAL_SEL_SCORE_COLUMN)
                if name not in SELECTIVE_SCORES:
                    d.score_column[i] = native.ptr(self._extra[name])
            for i, name in enumerate(risks):
                d.risk_kind[i] = SELECTIVE_RISKS.get(name, native.EVAL_SEL_RISK_COLUMN)
                if name == 'mu_abs_err':
                    keep.append((self._rec['sev_true'][:n] - self._extra['mu'][:n]).abs())
                    d.risk_column[i] = native.ptr(keep[-1])
                elif name not in SELECTIVE_RISKS:
                    d.risk_column[i] = native.ptr(self._extra[name])
            for k, _ in self._FIELDS:
                setattr(d, k, native.ptr(self._rec[k]))
            d.workspace, d.workspace_bytes, d.result = native.ptr(workspace), ws_bytes, native.ptr(out)
            if return_keys:
                f = out[W:].view(torch.float32)
                d.keys_out, d.risks_out = native.ptr(f), native.ptr(f[S * n:])
            method = native.rank_method(self.rank_method, n, 'EvalAccumulator.rank_method')
            rank_bytes = native.load().rovit_eval_selective_rank_workspace_bytes(n, S, K) if method == native.RANK_SORT else 0
            rank_ws = torch.empty(rank_bytes, dtype=torch.uint8, device=self.device) if rank_bytes else None
            native.call('rovit_eval_selective_ex', ctypes.byref(d), method, native.ptr(rank_ws), rank_bytes, native.stream_ptr())
            host = out.cpu().numpy()                             # the call's single device-to-host copy
            block = host[:W]
            if return_keys:
                f = host[W:].view(np.float32)
                keys, values = f[:S * n].reshape(S, n), f[S * n:(S + K) * n].reshape(K, n)
        res = selective_from_block(block, scores, risks, P, self.num_classes)
        if return_keys:
            res['keys'], res['risk_values'], res['block'] = keys, values, block
        return res

    # -- post-hoc calibration --
    def _extra_column(self, name: str) -> np.ndarray:
        if self.device.type == 'cuda':
            return self._extra[name][:self.n].cpu().numpy()
        return torch.cat([b['extra'][name] for b in self._cpu]).numpy()

    def calibrate(self, levels: int = 9, return_block: bool = False, _max_workgroups: int = 0) -> 'Calibration':
        """Fit a post-hoc calibration on the recorded rows (normally those of the validation split): the temperature T that minimises
        the NLL of softmax(log p / T) over T in [1/32, 32], and, when the batches carried mu and log_var and the extra column ``'mu'``
        was recorded, the scale s = sqrt(mean z^2) of sigma with z = (sev_true - mu) / sigma, plus the observed coverage of the
        central Gaussian intervals at the ``levels`` nominal levels k / (levels + 1).  The definitions are those of
        ``calibration_reference``.  Rows whose class label is outside [0, C) are left out of the temperature and counted
        (``bad_labels``); rows with a non-finite or non-positive sigma or a non-finite mu or sev_true are left out of the regression
        part and counted (``bad_sigma``).  ``return_block`` keeps the raw result block (int64 words) on the result.  On the device the
        call makes ONE device-to-host copy, and it raises after it when no row has a valid label."""
        if not (isinstance(levels, int) and not isinstance(levels, bool) and 1 <= levels <= native.EVAL_CAL_MAX_LEVELS):
            raise RovitHipError(f'calibrate: levels must be an int in 1..{native.EVAL_CAL_MAX_LEVELS}, got {levels!r}')
        if self.n < 1:
            raise RovitHipError('EvalAccumulator: nothing recorded yet')
        has_reg = self._has_uncertainty and 'mu' in (self._extra_names or ())
        n, L = self.n, levels
        if self.device.type != 'cuda':
            block = calibration_block(self._cpu_arrays(), {'mu': self._extra_column('mu')} if has_reg else {}, self.num_classes, L)
        else:
            ws_bytes = native.load().rovit_eval_calibrate_workspace_bytes(n, self.num_classes)
            workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            out = torch.empty(native.EVAL_CAL_COVERAGE + L, dtype=torch.int64, device=self.device)
            widths = torch.tensor(coverage_half_widths(L), dtype=torch.float64).to(self.device, non_blocking=True) if has_reg else None
            d = native.EvalCal()
            d.n, d.num_classes, d.num_levels, d.max_workgroups = n, self.num_classes, L, _max_workgroups
            d.probs, d.label, d.sev_true = (native.ptr(self._rec[k]) for k in ('probs', 'label', 'sev_true'))
            if has_reg:
                d.uncertainty, d.mu, d.half_widths = native.ptr(self._rec['uncertainty']), native.ptr(self._extra['mu']), native.ptr(widths)
            d.workspace, d.workspace_bytes, d.result = native.ptr(workspace), ws_bytes, native.ptr(out)
            native.call('rovit_eval_calibrate', ctypes.byref(d), native.stream_ptr())
            block = out.cpu().numpy()                            # the call's single device-to-host copy
        return calibration_from_block(block, L, has_reg, self.num_classes, keep_block=return_block)

    # -- split conformal prediction --
    def _conformal_names(self, scores) -> List[str]:
        extras = self._extra_names or ()
        if scores is None:
            scores = ['lac', 'aps', 'raps', 'kan_abs'] + (['mu_abs'] if 'mu' in extras else []) + \
                (['mu_scaled'] if 'mu' in extras and self._has_uncertainty else [])
        if isinstance(scores, str):
            raise RovitHipError('conformal: scores is a sequence of names')
        scores = list(scores)
        if not 1 <= len(scores) <= native.EVAL_CONF_MAX_SCORES or len(set(scores)) != len(scores):
            raise RovitHipError(f'conformal: 1..{native.EVAL_CONF_MAX_SCORES} distinct score names are needed, got {scores!r}')
        for name in scores:
            if name not in CONFORMAL_KINDS and name not in extras:
                raise RovitHipError(f'conformal: unknown score {name!r} (known: {sorted(CONFORMAL_KINDS)} and the extra columns {sorted(extras)})')
            if name in ('mu_abs', 'mu_scaled') and 'mu' not in extras:
                raise RovitHipError(f"conformal: the score {name!r} needs the extra column 'mu' (update(..., extra={{'mu': outputs['mu']}}))")
            if name == 'mu_scaled' and not self._has_uncertainty:
                raise RovitHipError("conformal: the score 'mu_scaled' needs batches that carried mu and log_var (no uncertainty head was recorded)")
        return scores

    def _conformal_descriptor(self, scores: Sequence[str], num_levels: int, p: Dict) -> 'native.EvalConf':
        """The part of ``rovit_eval_conf`` the fit and the application share, for this accumulator's device record."""
        d = native.EvalConf()
        d.n, d.num_classes, d.num_scores, d.num_levels = self.n, self.num_classes, len(scores), num_levels
        d.class_conditional, d.randomized, d.raps_k, d.raps_lambda = int(p['class_conditional']), int(p['randomized']), p['raps_k'], p['raps_lambda']
        d.seed, d.row_offset = p['seed'], 0
        for i, name in enumerate(scores):
            d.score_kind[i] = CONFORMAL_KINDS.get(name, native.EVAL_CONF_COLUMN)
            if name not in CONFORMAL_KINDS:
                d.score_column[i] = native.ptr(self._extra[name])
        for k in ('probs', 'label', 'sev_pred', 'sev_true', 'uncertainty'):
            setattr(d, k, native.ptr(self._rec[k]))
        if 'mu' in self._extra:
            d.mu = native.ptr(self._extra['mu'])
        return d

    def _host_columns(self):
        """(arrays, extras) of a CPU accumulator, as the numpy statements read them."""
        return self._cpu_arrays(), {k: self._extra_column(k) for k in (self._extra_names or ())}

    def conformal(self, alphas: Sequence[float] = (0.1,), scores: Optional[Sequence[str]] = None, class_conditional: bool = False,
                  randomized: bool = True, seed: int = 0, raps_lambda: float = 0.01, raps_k: int = 1, return_scores: bool = False,
                  _max_workgroups: int = 0) -> 'Conformal':
        """Fit split-conformal thresholds on the recorded rows (normally those of the validation split; the record
        ``Calibration.apply`` returns works too).  ``scores`` names 1..8 nonconformity scores: ``'lac'`` 1 - p_y, ``'aps'``
        cum(y) - u p_y, ``'raps'`` aps + lambda max(0, r(y) - raps_k), ``'kan_abs'`` |sev_true - sev_pred|, ``'mu_abs'`` |sev_true - mu|,
        ``'mu_scaled'`` |sev_true - mu| / sigma, or the name of an ``extra`` column (taken as it is); default the first four, plus the mu
        scores the record allows.  For every score, level alpha and group (all labelled rows; with ``class_conditional`` also the
        rows of each true class) the threshold is the k-th smallest valid score, k = n_g + 1 - floor((n_g + 1) alpha), +inf
        ('trivial') when k > n_g.  The definitions are those of ``conformal_reference``.  Rows with a class label outside [0, C) are
        left out and counted (``bad_labels``), rows whose score is non-finite (or whose sigma is not positive and finite, for
        ``'mu_scaled'``) are left out of that score and counted (``bad_rows``).  ``return_scores`` keeps the (M, n) fp32 score columns,
        the drawn ``u`` and the raw result block on the result.  On the device the call makes ONE device-to-host copy, and it raises
        after it when a score has no valid row."""
        if self.n < 1:
            raise RovitHipError('EvalAccumulator: nothing recorded yet')
        scores = self._conformal_names(scores)
        alphas, fractions = _check_conformal_args(alphas, seed, raps_lambda, raps_k, self.num_classes)
        p = {'class_conditional': bool(class_conditional), 'randomized': bool(randomized), 'seed': seed, 'raps_lambda': float(raps_lambda),
             'raps_k': raps_k}
        M, A, G, n = len(scores), len(alphas), 1 + self.num_classes * int(bool(class_conditional)), self.n
        columns = u = None
        if self.device.type != 'cuda':
            arrays, extras = self._host_columns()
            ref = conformal_reference(arrays, extras, self.num_classes, alphas, scores, **p)
            block, columns, u = ref['block'], ref['columns'], ref['u']
        else:
            W = native.eval_conformal_words(M, G, A)
            out = torch.empty(W + ((M + 1) * n + 1) // 2 * int(bool(return_scores)), dtype=torch.int64, device=self.device)
            ws_bytes = native.load().rovit_eval_conformal_workspace_bytes(n, M, G, A)
            workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            d = self._conformal_descriptor(scores, A, p)
            d.max_workgroups = _max_workgroups
            for i, fr in enumerate(fractions):
                d.alpha_num[i], d.alpha_den[i] = fr.numerator, fr.denominator
            d.workspace, d.workspace_bytes, d.result = native.ptr(workspace), ws_bytes, native.ptr(out)
            if return_scores:
                f = out[W:].view(torch.float32)
                d.scores_out, d.u_out = native.ptr(f), native.ptr(f[M * n:])
            native.call('rovit_eval_conformal', ctypes.byref(d), native.stream_ptr())
            host = out.cpu().numpy()                             # the call's single device-to-host copy
            block = host[:W]
            if return_scores:
                f = host[W:].view(np.float32)
                columns, u = f[:M * n].reshape(M, n), f[M * n:(M + 1) * n]
        res = conformal_from_block(block, alphas, scores, self.num_classes, **p)
        if return_scores:
            res.score_columns, res.u, res.block = columns, u, np.array(block)
        return res

    # -- bootstrap --
    def _bootstrap_launch(self, num_resamples: int, seed: int, stratified: bool, table: torch.Tensor, blocks: Optional[torch.Tensor],
                          max_workgroups: int = 0) -> torch.Tensor:
        """Device path: the finalise if it has not run on these rows, then ``rovit_eval_bootstrap`` into the caller's int64 views
        (``table``: R * EVAL_BOOT_COLS words, ``blocks``: R * EVAL_RESULT_WORDS words or None).  Returns the point block on the
        device.  Nothing here synchronises."""
        block = self._finalize()
        dev, n, C = self.device, self.n, self.num_classes
        perm = starts = workspace = None
        if stratified:
            label = self._rec['label'][:n].long()
            key = torch.where(label < 0, torch.full_like(label, C), label)           # bad labels: a last segment of their own
            perm = torch.sort(key, stable=True)[1].int()
            # the class counts by index_add_, not torch.bincount: bincount reads its output size back from the device
            counts = torch.zeros(C + 1, dtype=torch.int64, device=dev).index_add_(0, key, torch.ones_like(key))
            starts = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).int()
        ws_bytes = native.load().rovit_eval_bootstrap_workspace_bytes(n, num_resamples)
        if ws_bytes:
            workspace = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
        d = native.EvalBoot()
        d.n, d.num_classes, d.n_bins, d.num_resamples, d.max_workgroups, d.seed = n, C, self.n_bins, num_resamples, max_workgroups, seed
        for k in ('probs', 'pred', 'label', 'sev_pred', 'sev_true'):
            setattr(d, k, native.ptr(self._rec[k]))
        d.bin_edges, d.rank_counts, d.perm, d.starts = (native.ptr(t) for t in (self._edges, self._rank_counts, perm, starts))
        d.workspace, d.workspace_bytes = native.ptr(workspace), ws_bytes
        d.table, d.blocks = native.ptr(table), native.ptr(blocks)
        native.call('rovit_eval_bootstrap', ctypes.byref(d), native.stream_ptr())
        return block

    def bootstrap(self, num_resamples: int = 1000, seed: int = 0, confidence: float = 0.95, stratified: bool = False,
                  return_table: bool = False, return_blocks: bool = False, _max_workgroups: int = 0) -> Dict:
        """Percentile bootstrap of the score card: per metric ``{'value', 'mean', 'se', 'lo', 'hi'}`` -- the point estimate of
        ``compute()``, the mean and the standard deviation (ddof = 1) over the replicates, and the ``confidence`` percentile interval
        (``np.nanquantile``, linear); the per-class precision / recall / F1 under ``'per_class'``; the number of replicates whose rho
        is NaN beside rho (``'n_nan'``).  ``stratified`` resamples inside each true class, so every replicate keeps the supports.
        ``return_table`` adds the (R, EVAL_BOOT_COLS) metric table, ``return_blocks`` every replicate's result block (R, 272).
        On the device the call makes ONE device-to-host copy; it brings the point block along when ``compute()`` has not run yet.
        Class labels outside [0, C) raise, as in ``compute()``."""
        R = _check_bootstrap_args(num_resamples, seed, confidence)
        if self.n < 1:
            raise RovitHipError('EvalAccumulator: nothing recorded yet')
        W, COLS = native.EVAL_RESULT_WORDS, native.EVAL_BOOT_COLS
        if self.device.type != 'cuda':
            point = self.compute()
            table, blocks = bootstrap_reference(self.arrays(), self.num_classes, self.n_bins, R, seed, stratified)
        else:
            out = torch.empty(W + R * COLS + (R * W if return_blocks else 0), dtype=torch.int64, device=self.device)
            block = self._bootstrap_launch(R, seed, stratified, out[W:W + R * COLS], out[W + R * COLS:] if return_blocks else None,
                                           _max_workgroups)
            out[:W].copy_(block)
            host = out.cpu().numpy()                         # the call's single device-to-host copy
            if self._block is None:
                self._block = host[:W].copy()
            point = self.compute()
            table = host[W:W + R * COLS].view(np.float64).reshape(R, COLS)
            blocks = host[W + R * COLS:].reshape(R, W) if return_blocks else None
        res = {name: _interval(table[:, col], point[name], confidence) for name, col in BOOT_METRICS}
        res['spearman_rho']['n_nan'] = int(np.isnan(table[:, native.EVAL_BOOT_RHO]).sum())
        res['per_class'] = [{k: _interval(table[:, col + c], point['per_class'][c][k], confidence) for k, col in BOOT_CLASS_METRICS}
                            for c in range(self.num_classes)]
        res.update(num_resamples=R, seed=seed, confidence=confidence, stratified=bool(stratified))
        if return_table:
            res['table'] = table
        if return_blocks:
            res['blocks'] = blocks
        return res

# ---- post-hoc calibration: restatement, result and application -------------------------------------------------------------------

CALIBRATION_STATUS = {native.EVAL_CAL_INTERIOR: 'interior', native.EVAL_CAL_AT_MIN: 'at_min', native.EVAL_CAL_AT_MAX: 'at_max'}


def coverage_levels(levels: int) -> List[float]:
    """The nominal levels a_k = k / (L + 1), k = 1..L."""
    return [k / (levels + 1) for k in range(1, levels + 1)]


def coverage_half_widths(levels: int) -> List[float]:
    """q_k = Phi^-1(1/2 + a_k / 2): the central interval of level a_k is mu +- q_k sigma."""
    from statistics import NormalDist
    return [NormalDist().inv_cdf(0.5 + a / 2.0) for a in coverage_levels(levels)]


def calibration_log_probs(probs) -> np.ndarray:
    """l = max(log p, ln 2^-100) with the fp32 probabilities promoted to fp64; the clamp is part of the definition."""
    p = np.asarray(probs, dtype=np.float32).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.fmax(np.log(p), native.EVAL_CAL_LOG_FLOOR)


def calibration_g(l: np.ndarray, y: np.ndarray, u: float) -> float:
    """g(u) = sum_i (sum_c w[i,c] l[i,c] - l[i,y_i]) with w = softmax(beta l[i,:]), beta = exp(u): the NLL's derivative in beta."""
    if not len(y):
        return 0.0
    e = np.exp(math.exp(u) * (l - l.max(axis=1, keepdims=True)))
    return float(((e * l).sum(axis=1) / e.sum(axis=1) - l[np.arange(len(y)), y]).sum())


def calibration_nll_sum(l: np.ndarray, y: np.ndarray, u: float) -> float:
    """sum_i (logsumexp_c(beta l[i,c]) - beta l[i,y_i]) with beta = exp(u)."""
    if not len(y):
        return 0.0
    beta, m = math.exp(u), l.max(axis=1)
    return float((beta * m + np.log(np.exp(beta * (l - m[:, None])).sum(axis=1)) - beta * l[np.arange(len(y)), y]).sum())


def calibration_candidates(lo: float, hi: float) -> List[float]:
    """u_j = lo + (hi - lo) (j / 63) for j < 63 and u_63 = hi exactly."""
    M = native.EVAL_CAL_CANDIDATES
    return [lo + (hi - lo) * (j / (M - 1)) for j in range(M - 1)] + [hi]


def _record_columns(arrays: Dict, extras: Optional[Dict]):
    """probs, label (-1 or outside [0, C): bad), sev_true, sigma and mu from either naming: ``_cpu_arrays`` / ``selective_columns``
    (probs, label, sev_true, uncertainty) or ``arrays()`` (y_probs, y_true, severity_true, uncertainty)."""
    pick = lambda *keys: next((arrays[k] for k in keys if k in arrays), None)
    mu = (extras or {}).get('mu')
    return pick('probs', 'y_probs'), pick('label', 'y_true'), pick('sev_true', 'severity_true'), arrays.get('uncertainty'), mu


def calibration_reference(arrays: Dict, extras: Optional[Dict], num_classes: int, levels: int = 9) -> Dict:
    """The definitions of the post-hoc calibration in numpy fp64: ``arrays`` as ``EvalAccumulator.arrays()`` returns them (or with the
    keys ``selective_columns`` reads), ``extras`` the extra columns (``{'mu': ...}``; without it, or with ``uncertainty`` None, there is
    no regression part).

    Temperature: a root search on g (``calibration_g``), which is non-decreasing in u = -ln T because the NLL is convex in beta = 1/T:
    4 rounds of 64 candidates (``calibration_candidates``); round 0 spans [-ln 32, ln 32], where g(u_0) >= 0 ends the search at T = 32
    ('at_max') and no g(u_j) >= 0 at T = 1/32 ('at_min'); otherwise j* is the first j >= 1 with g(u_j) >= 0 (63 if none), the next
    bracket is [u_{j*-1}, u_{j*}], and u* is the secant point of the last one (lo when both g are equal).
    Sigma scale: over the rows with a finite sigma > 0 and finite mu and sev_true, z = (sev_true - mu) / sigma, sum z^2 and sum ln sigma.
    Coverage: count[k] = #{|sev_true - mu| <= q_k sigma} with ``coverage_half_widths``.
    Returns the words of the result block by name; the oracle of the kernel, and what ``calibrate()`` runs for CPU tensors."""
    C, L = int(num_classes), int(levels)
    probs, label, st, sigma, mu = _record_columns(arrays, extras)
    label = np.asarray(label).astype(np.int64).reshape(-1)
    n = len(label)
    ok = (label >= 0) & (label < C)
    l, y = calibration_log_probs(np.asarray(probs).reshape(n, C))[ok], label[ok]
    lo, hi, status = -native.EVAL_CAL_U_MAX, native.EVAL_CAL_U_MAX, native.EVAL_CAL_INTERIOR
    for r in range(native.EVAL_CAL_ROUNDS):
        us = calibration_candidates(lo, hi)
        g = [calibration_g(l, y, u) for u in us]
        first = next((j for j in range(1, len(us)) if g[j] >= 0.0), None)
        if r == 0 and g[0] >= 0.0:
            status, lo, hi, g_lo, g_hi = native.EVAL_CAL_AT_MAX, us[0], us[0], g[0], g[0]
            break
        if r == 0 and first is None:
            status, lo, hi, g_lo, g_hi = native.EVAL_CAL_AT_MIN, us[-1], us[-1], g[-1], g[-1]
            break
        j = len(us) - 1 if first is None else first
        lo, hi, g_lo, g_hi = us[j - 1], us[j], g[j - 1], g[j]
    u = lo if g_hi == g_lo else lo - (hi - lo) * (g_lo / (g_hi - g_lo))          # the ratio lies in [-1, 0]: no overflow
    out = {'n': n, 'n_valid': int(ok.sum()), 'bad_labels': int((~ok).sum()), 'status': status, 'u': u, 'u_lo': lo, 'u_hi': hi, 'g_lo': g_lo,
           'g_hi': g_hi, 'nll_sum': calibration_nll_sum(l, y, 0.0), 'nll_calibrated_sum': calibration_nll_sum(l, y, u),
           'n_reg': 0, 'bad_sigma': 0, 'sum_z2': 0.0, 'sum_log_sigma': 0.0, 'coverage_counts': np.zeros(L, dtype=np.int64),
           'has_regression': sigma is not None and mu is not None}
    if out['has_regression']:
        sg = np.asarray(sigma, dtype=np.float32).astype(np.float64).reshape(-1)
        m = np.asarray(mu, dtype=np.float32).astype(np.float64).reshape(-1)
        t = np.asarray(st, dtype=np.float32).astype(np.float64).reshape(-1)
        with np.errstate(invalid='ignore'):
            good = np.isfinite(sg) & (sg > 0) & np.isfinite(m) & np.isfinite(t)
        sg, d = sg[good], (t - m)[good]
        z = d / sg
        out.update(n_reg=int(good.sum()), bad_sigma=int((~good).sum()), sum_z2=float((z * z).sum()), sum_log_sigma=float(np.log(sg).sum()),
                   coverage_counts=np.array([int((np.abs(d) <= q * sg).sum()) for q in coverage_half_widths(L)], dtype=np.int64))
    return out


def calibration_block(arrays: Dict, extras: Optional[Dict], num_classes: int, levels: int = 9) -> np.ndarray:
    """The result block of ``rovit_eval_calibrate`` (include/rovit_hip.h) from recorded arrays, on the host, through
    ``calibration_reference``: int64 words with the fp64 values stored bit for bit."""
    ref = calibration_reference(arrays, extras, num_classes, levels)
    blk = np.zeros(native.EVAL_CAL_COVERAGE + int(levels), dtype=np.int64)
    f = blk.view(np.float64)
    for word, key in ((native.EVAL_CAL_N_VALID, 'n_valid'), (native.EVAL_CAL_BAD_LABELS, 'bad_labels'), (native.EVAL_CAL_N_REG, 'n_reg'),
                      (native.EVAL_CAL_BAD_SIGMA, 'bad_sigma'), (native.EVAL_CAL_STATUS, 'status'), (native.EVAL_CAL_N, 'n')):
        blk[word] = ref[key]
    for word, key in ((native.EVAL_CAL_U, 'u'), (native.EVAL_CAL_NLL, 'nll_sum'), (native.EVAL_CAL_NLL_CAL, 'nll_calibrated_sum'),
                      (native.EVAL_CAL_G_LO, 'g_lo'), (native.EVAL_CAL_G_HI, 'g_hi'), (native.EVAL_CAL_U_LO, 'u_lo'), (native.EVAL_CAL_U_HI, 'u_hi'),
                      (native.EVAL_CAL_SUM_Z2, 'sum_z2'), (native.EVAL_CAL_SUM_LOG_SIGMA, 'sum_log_sigma')):
        f[word] = ref[key]
    blk[native.EVAL_CAL_COVERAGE:] = ref['coverage_counts']
    return blk


class Calibration:
    """A fitted post-hoc calibration: ``temperature`` T (probabilities become softmax(log p / T)), ``status`` ('interior', or 'at_min' /
    'at_max' when the fit stopped at T = 1/32 / 32), ``sigma_scale`` s (sigma becomes s sigma; None without a regression part), the row
    counts ``n``, ``bad_labels``, ``bad_sigma`` and ``diagnostics``: ``nll`` and ``nll_calibrated`` (mean NLL of the fitted rows at T = 1
    and at T), ``gaussian_nll`` and ``gaussian_nll_calibrated`` (mean of ln sigma + z^2 / 2 before and after; None without the regression
    part), ``levels`` (nominal) and ``coverage`` (the observed fractions of the rows it was fitted on, before scaling)."""

    def __init__(self, temperature: float, status: str = 'interior', sigma_scale: Optional[float] = None, n: int = 0, bad_labels: int = 0,
                 bad_sigma: int = 0, diagnostics: Optional[Dict] = None, block: Optional[np.ndarray] = None):
        if not (isinstance(temperature, float) and 0.0 < temperature < math.inf):
            raise RovitHipError(f'Calibration: the temperature must be a positive finite float, got {temperature!r}')
        if sigma_scale is not None and not (isinstance(sigma_scale, float) and 0.0 < sigma_scale < math.inf):
            raise RovitHipError(f'Calibration: sigma_scale must be None or a positive finite float, got {sigma_scale!r}')
        if status not in CALIBRATION_STATUS.values():
            raise RovitHipError(f'Calibration: unknown status {status!r}')
        self.temperature, self.status, self.sigma_scale = temperature, status, sigma_scale
        self.n, self.bad_labels, self.bad_sigma = int(n), int(bad_labels), int(bad_sigma)
        self.diagnostics = dict(diagnostics or {})
        self.block = block

    def __repr__(self) -> str:
        return f'Calibration(temperature={self.temperature!r}, status={self.status!r}, sigma_scale={self.sigma_scale!r}, n={self.n})'

    def to_dict(self) -> Dict:
        """Plain floats, ints, strings and lists of them: ``json.dumps`` takes it, ``from_dict`` restores it."""
        plain = lambda v: [float(x) for x in v] if isinstance(v, (list, tuple, np.ndarray)) else (None if v is None else float(v))
        return {'temperature': self.temperature, 'status': self.status, 'sigma_scale': self.sigma_scale, 'n': self.n,
                'bad_labels': self.bad_labels, 'bad_sigma': self.bad_sigma, 'diagnostics': {k: plain(v) for k, v in self.diagnostics.items()}}

    @classmethod
    def from_dict(cls, d: Dict) -> 'Calibration':
        scale = d.get('sigma_scale')
        return cls(float(d['temperature']), d.get('status', 'interior'), None if scale is None else float(scale), d.get('n', 0),
                   d.get('bad_labels', 0), d.get('bad_sigma', 0), d.get('diagnostics'))

    def transform(self, outputs: Dict) -> Dict:
        """A model's output dict for deployment: ``cls_logits / T`` and, with a sigma scale, ``log_var + 2 ln s`` (so exp(0.5 log_var)
        becomes s sigma), in torch; every other key holds the same tensor."""
        out = dict(outputs)
        out['cls_logits'] = outputs['cls_logits'] / self.temperature
        if self.sigma_scale is not None and outputs.get('log_var') is not None:
            out['log_var'] = outputs['log_var'] + 2.0 * math.log(self.sigma_scale)
        return out

    def apply(self, acc: 'EvalAccumulator') -> 'EvalAccumulator':
        """The calibrated record as a NEW accumulator on the same device (``acc`` is left untouched): p' = softmax(log p / T) and
        sigma' = s sigma in fp32 (``rovit_eval_recalibrate``, one launch); the predicted class is carried over (the argmax does not
        change for T > 0), and the labels, the severities, the loss rows and every extra column are copied.  ``compute``, ``selective``,
        ``bootstrap`` and ``calibrate`` work on the result.  On CPU tensors the stored logits are divided by T and ``log_var`` gets
        + 2 ln s, as ``transform`` does."""
        if not isinstance(acc, EvalAccumulator) or acc.n < 1:
            raise RovitHipError('Calibration.apply: an EvalAccumulator with recorded rows is needed')
        new = EvalAccumulator(acc.num_classes, acc.n_bins, acc._capacity0)
        new.rank_method = acc.rank_method
        new.n, new.n_loss_rows, new.device, new._has_uncertainty, new._extra_names = acc.n, acc.n_loss_rows, acc.device, acc._has_uncertainty, acc._extra_names
        shift = None if self.sigma_scale is None else 2.0 * math.log(self.sigma_scale)
        if acc.device.type != 'cuda':
            for b in acc._cpu:
                c = dict(b)
                c['logits'] = b['logits'] / self.temperature
                if shift is not None and b['lv'] is not None:
                    c['lv'] = b['lv'] + shift
                new._cpu.append(c)
            new._cpu_losses = list(acc._cpu_losses)
            return new
        n = acc.n
        new._rec = new._alloc(n)
        for k in ('pred', 'label', 'sev_pred', 'sev_true') + (() if shift is not None else ('uncertainty',)):
            new._rec[k].copy_(acc._rec[k][:n])                   # device-to-device, stream-ordered
        new._extra = {k: t[:n].clone() for k, t in acc._extra.items()}
        if acc._loss_table is not None:
            new._loss_table = acc._loss_table[:max(acc.n_loss_rows, 1)].clone()
        d = native.EvalRecal()
        d.n, d.num_classes, d.beta, d.sigma_scale = n, acc.num_classes, 1.0 / self.temperature, 1.0 if shift is None else self.sigma_scale
        d.probs, d.probs_out = native.ptr(acc._rec['probs']), native.ptr(new._rec['probs'])
        if shift is not None:
            d.uncertainty, d.uncertainty_out = native.ptr(acc._rec['uncertainty']), native.ptr(new._rec['uncertainty'])
        native.call('rovit_eval_recalibrate', ctypes.byref(d), native.stream_ptr())
        return new


def calibration_from_block(blk: np.ndarray, levels: int, has_regression: bool, num_classes: int, keep_block: bool = False) -> Calibration:
    """The ``Calibration`` that ``EvalAccumulator.calibrate`` returns from one result block; T, s and the Gaussian NLLs are derived here
    in fp64.  Raises when no row has a valid label."""
    blk = np.asarray(blk, dtype=np.int64)
    f = blk.view(np.float64)
    n, n_valid, n_reg = (int(blk[w]) for w in (native.EVAL_CAL_N, native.EVAL_CAL_N_VALID, native.EVAL_CAL_N_REG))
    if n_valid < 1:
        raise RovitHipError(f'calibrate: none of the {n} recorded rows has a class label in [0, {num_classes})')
    status = CALIBRATION_STATUS[int(blk[native.EVAL_CAL_STATUS])]
    temperature = {'at_min': 1.0 / 32.0, 'at_max': 32.0}.get(status, math.exp(-float(f[native.EVAL_CAL_U])))
    diag = {'nll': float(f[native.EVAL_CAL_NLL]) / n_valid, 'nll_calibrated': float(f[native.EVAL_CAL_NLL_CAL]) / n_valid, 'gaussian_nll': None,
            'gaussian_nll_calibrated': None, 'levels': coverage_levels(levels), 'coverage': None}
    scale = None
    if has_regression and n_reg >= 1:
        z2, ls = float(f[native.EVAL_CAL_SUM_Z2]), float(f[native.EVAL_CAL_SUM_LOG_SIGMA])
        diag['coverage'] = [int(c) / n_reg for c in blk[native.EVAL_CAL_COVERAGE:native.EVAL_CAL_COVERAGE + levels]]
        diag['gaussian_nll'] = (ls + 0.5 * z2) / n_reg
        if 0.0 < z2 < math.inf:
            scale = math.sqrt(z2 / n_reg)
            diag['gaussian_nll_calibrated'] = (ls + n_reg * math.log(scale) + 0.5 * z2 / (scale * scale)) / n_reg
    return Calibration(temperature, status, scale, n, int(blk[native.EVAL_CAL_BAD_LABELS]), int(blk[native.EVAL_CAL_BAD_SIGMA]) if has_regression else 0,
                       diag, blk.copy() if keep_block else None)


# ---- split conformal prediction: restatement, result and application ----------------------------------------------------------------

CONFORMAL_KINDS = {'lac': native.EVAL_CONF_LAC, 'aps': native.EVAL_CONF_APS, 'raps': native.EVAL_CONF_RAPS, 'kan_abs': native.EVAL_CONF_KAN_ABS,
                   'mu_abs': native.EVAL_CONF_MU_ABS, 'mu_scaled': native.EVAL_CONF_MU_SCALED}
CONFORMAL_CLASS_SCORES = ('lac', 'aps', 'raps')


def conformal_fraction(alpha):
    """alpha as the rational num / den the device computes k with: ``Fraction(str(alpha)).limit_denominator(2^20)``, 0 < alpha < 1."""
    from fractions import Fraction
    try:
        fr = Fraction(str(alpha)).limit_denominator(native.EVAL_CONF_MAX_DEN)
    except (ValueError, ZeroDivisionError):
        raise RovitHipError(f'conformal: the level {alpha!r} is not a number') from None
    if not 0 < fr < 1:
        raise RovitHipError(f'conformal: a level must lie in (0, 1), got {alpha!r}')
    return fr


def conformal_rank(n_g: int, fraction) -> int:
    """k = n_g + 1 - floor((n_g + 1) alpha) in integers; k > n_g means the threshold is +inf ('trivial')."""
    return n_g + 1 - ((n_g + 1) * fraction.numerator) // fraction.denominator


def _check_conformal_args(alphas, seed, raps_lambda, raps_k, num_classes):
    if isinstance(alphas, (int, float)):
        alphas = (alphas,)
    alphas = [float(a) for a in alphas]
    if not 1 <= len(alphas) <= native.EVAL_CONF_MAX_LEVELS or len(set(alphas)) != len(alphas):
        raise RovitHipError(f'conformal: 1..{native.EVAL_CONF_MAX_LEVELS} distinct levels are needed, got {alphas!r}')
    fractions = [conformal_fraction(a) for a in alphas]
    if not (isinstance(seed, int) and 0 <= seed < 1 << 64):
        raise RovitHipError(f'conformal: seed must be an integer in [0, 2^64), got {seed!r}')
    if not (isinstance(raps_k, int) and not isinstance(raps_k, bool) and 0 <= raps_k <= native.EVAL_MAX_CLASSES):
        raise RovitHipError(f'conformal: raps_k must be an int in 0..{native.EVAL_MAX_CLASSES}, got {raps_k!r}')
    if not (isinstance(raps_lambda, (int, float)) and 0.0 <= raps_lambda < math.inf):
        raise RovitHipError(f'conformal: raps_lambda must be finite and >= 0, got {raps_lambda!r}')
    return alphas, fractions


def conformal_uniforms(n: int, seed: int, row_offset: int = 0) -> np.ndarray:
    """u of rows row_offset .. row_offset + n - 1 as the kernels draw it: w = word 0 of Philox4x32-10 with key ``seed`` and counter
    (row, 0, EVAL_CONF_STREAM, 0); u = (fp32(w >> 8) + 0.5) * 2^-24 in fp32 (the addition rounds to even once w >> 8 >= 2^23)."""
    from oracle.philox import philox4x32_10 as philox          # checker only, like the bootstrap's draws
    row = np.arange(n, dtype=np.uint64) + np.uint64(row_offset)
    w = philox([row, np.zeros(n, np.uint64), np.full(n, native.EVAL_CONF_STREAM, np.uint64), np.zeros(n, np.uint64)],
               [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])[0]
    return ((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def conformal_class_scores(probs, name: str, u=None, raps_lambda: float = 0.01, raps_k: int = 1):
    """s(c) of every row and candidate class c for 'lac', 'aps' or 'raps': ``(fp32, exact)``, both (n, C).  The classes are ordered by
    p descending, ties by lower index first; r(c) is the 1-based rank and cum(c) the float32 running sum in rank order up to and
    including c.  ``exact`` is the fp64 statement 1 - p, cum - u p, cum - u p + lambda max(0, r - raps_k) on those fp32 inputs; ``fp32``
    rounds it the way the kernel does (one rounding for 1 - p and for the fused cum - u p, a second one for the fused RAPS term).  A
    NaN probability makes the row's aps and raps NaN."""
    p = np.asarray(probs, dtype=np.float32)
    n, C = p.shape
    if name == 'lac':
        s = (np.float32(1.0) - p) + np.float32(0.0)
        return s, s.astype(np.float64)
    with np.errstate(invalid='ignore'):
        order = np.argsort(-p, axis=1, kind='stable')
        cum_sorted = np.cumsum(np.take_along_axis(p, order, axis=1), axis=1, dtype=np.float32)
    rank = np.argsort(order, axis=1, kind='stable')                      # 0-based rank of class c
    cum = np.take_along_axis(cum_sorted, rank, axis=1).astype(np.float64)
    uu = np.zeros(n) if u is None else np.asarray(u, dtype=np.float32).astype(np.float64)
    exact = cum - uu[:, None] * p.astype(np.float64)
    s = exact.astype(np.float32)
    if name == 'raps':
        pen = float(np.float32(raps_lambda)) * np.maximum(0, rank + 1 - int(raps_k)).astype(np.float64)
        exact = exact + pen
        s = (s.astype(np.float64) + pen).astype(np.float32)
    bad = np.isnan(p).any(axis=1)
    s, exact = s + np.float32(0.0), exact + 0.0
    s[bad], exact[bad] = np.nan, np.nan
    return s, exact


def conformal_scores(arrays: Dict, extras: Optional[Dict], num_classes: int, scores: Sequence[str], randomized: bool = True, seed: int = 0,
                     raps_lambda: float = 0.01, raps_k: int = 1, row_offset: int = 0) -> Dict:
    """The score columns of recorded arrays (either naming, see ``_record_columns``; ``label`` None: no labels, class scores only):
    ``columns`` (M, n) fp32 as the kernel rounds them, ``exact`` (M, n) the fp64 statements on the fp32 inputs, ``valid`` (M, n),
    ``u`` (n) fp32 (zeros unless ``randomized``), ``label_ok`` (n), ``class_scores`` {name: (n, C) fp32} for the class scores and
    ``sigma``.  A class score of a row without a valid label is NaN."""
    C = int(num_classes)
    probs, label, st, sigma, mu = _record_columns(arrays, extras)
    sp = next((arrays[k] for k in ('sev_pred', 'severity_pred') if k in arrays), None)
    probs = np.asarray(probs, dtype=np.float32).reshape(-1, C)
    n = probs.shape[0]
    f32 = lambda v: None if v is None else np.asarray(v, dtype=np.float32).reshape(-1)
    st, sp, sigma, mu = f32(st), f32(sp), f32(sigma), f32(mu)
    if label is None:
        label_ok, y = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    else:
        label = np.asarray(label).astype(np.int64).reshape(-1)
        label_ok = (label >= 0) & (label < C)
        y = np.where(label_ok, label, 0)
    u = conformal_uniforms(n, seed, row_offset) if randomized else np.zeros(n, dtype=np.float32)
    columns, exact, valid, per_class = [], [], [], {}
    for name in scores:
        ok = label_ok.copy()
        with np.errstate(divide='ignore', invalid='ignore'):
            if name in CONFORMAL_CLASS_SCORES:
                s, e = conformal_class_scores(probs, name, u, raps_lambda, raps_k)
                per_class[name] = s
                col = np.where(label_ok, s[np.arange(n), y], np.float32(np.nan))
                ex = np.where(label_ok, e[np.arange(n), y], np.nan)
            elif name in ('kan_abs', 'mu_abs'):
                col = np.abs(st - (sp if name == 'kan_abs' else mu)) + np.float32(0.0)
                ex = col.astype(np.float64)
            elif name == 'mu_scaled':
                ex = np.abs(st - mu).astype(np.float64) / sigma.astype(np.float64) + 0.0
                col = ex.astype(np.float32)
                ok &= np.isfinite(sigma) & (sigma > 0)
            else:
                col = f32(extras[name]) + np.float32(0.0)
                ex = col.astype(np.float64)
        columns.append(col.astype(np.float32))
        exact.append(ex)
        valid.append(ok & np.isfinite(col))
    return {'columns': np.stack(columns), 'exact': np.stack(exact), 'valid': np.stack(valid), 'u': u, 'label_ok': label_ok,
            'class_scores': per_class, 'sigma': sigma}


def conformal_valid(columns, scores: Sequence[str], label, sigma, num_classes: int) -> np.ndarray:
    """(M, n): the rows the fit uses of given score columns: a label in [0, C), a finite score and, for 'mu_scaled', a finite sigma > 0."""
    label = np.asarray(label).astype(np.int64).reshape(-1)
    ok = (label >= 0) & (label < num_classes)
    valid = np.isfinite(np.asarray(columns, dtype=np.float32)) & ok[None, :]
    for m, name in enumerate(scores):
        if name == 'mu_scaled':
            sg = np.asarray(sigma, dtype=np.float32).reshape(-1)
            with np.errstate(invalid='ignore'):
                valid[m] &= np.isfinite(sg) & (sg > 0)
    return valid


def conformal_block(columns, valid, label, num_classes: int, fractions, class_conditional: bool = False) -> np.ndarray:
    """The result block of ``rovit_eval_conformal`` (include/rovit_hip.h) from (M, n) fp32 score columns and their validity, on the
    host: per entry (score, group, level) n_g, k (``conformal_rank``), the threshold ``np.sort(valid scores)[k - 1]`` as fp32 bits,
    less = #{< threshold}, equal = #{== threshold}; k > n_g: less = n_g, equal = 0, +inf, trivial."""
    columns = np.atleast_2d(np.asarray(columns, dtype=np.float32))
    valid = np.atleast_2d(np.asarray(valid, dtype=bool))
    label = np.asarray(label).astype(np.int64).reshape(-1)
    C, (M, n), A = int(num_classes), columns.shape, len(fractions)
    G = 1 + C if class_conditional else 1
    ok = (label >= 0) & (label < C)
    blk = np.zeros(native.eval_conformal_words(M, G, A), dtype=np.int64)
    blk[native.EVAL_CONF_N], blk[native.EVAL_CONF_BAD_LABELS], blk[native.EVAL_CONF_N_LABELLED] = n, int((~ok).sum()), int(ok.sum())
    for m in range(M):
        blk[native.EVAL_CONF_BAD_ROWS + m] = int((ok & ~valid[m]).sum())
        for g in range(G):
            rows = valid[m] & ok if g == 0 else valid[m] & (label == g - 1)
            v = np.sort(columns[m][rows])
            for a, fr in enumerate(fractions):
                at = native.EVAL_CONF_ENTRIES + native.EVAL_CONF_ENTRY_WORDS * ((m * G + g) * A + a)
                n_g = int(v.shape[0])
                k = conformal_rank(n_g, fr)
                if k > n_g:
                    blk[at:at + 6] = [n_g, k, n_g, 0, 0x7F800000, 1]
                else:
                    q = v[k - 1]
                    blk[at:at + 6] = [n_g, k, int((v < q).sum()), int((v == q).sum()), int(q.view(np.uint32)), 0]
    return blk


def conformal_reference(arrays: Dict, extras: Optional[Dict], num_classes: int, alphas: Sequence[float] = (0.1,),
                        scores: Sequence[str] = ('lac', 'aps', 'raps', 'kan_abs'), class_conditional: bool = False, randomized: bool = True,
                        seed: int = 0, raps_lambda: float = 0.01, raps_k: int = 1) -> Dict:
    """The definitions of split conformal prediction in numpy: ``arrays`` as ``EvalAccumulator.arrays()`` returns them (or with the keys
    ``selective_columns`` reads), ``extras`` the extra columns.  Scores: ``conformal_scores``.  Groups: 0 = every row with a label in
    [0, C); with ``class_conditional`` 1 + c = the rows of true class c.  Threshold of (score, group, level): the k-th smallest valid
    score, k = n_g + 1 - floor((n_g + 1) alpha) with alpha as ``conformal_fraction`` (``conformal_block``).  Returns the score dict of
    ``conformal_scores`` plus ``block``, the result block: the oracle of the kernel, and what ``conformal()`` runs for CPU tensors."""
    _, label, _, _, _ = _record_columns(arrays, extras)
    out = conformal_scores(arrays, extras, num_classes, scores, randomized, seed, raps_lambda, raps_k)
    out['block'] = conformal_block(out['columns'], out['valid'], label, num_classes, [conformal_fraction(a) for a in alphas], class_conditional)
    return out


def conformal_membership(class_scores: np.ndarray, thresholds: np.ndarray, class_conditional: bool) -> np.ndarray:
    """(n, C) bool: class c is in the set iff s(c) <= threshold of group 1 + c (``class_conditional``) or of group 0; ``thresholds``
    holds one score's and one level's G values.  NaN scores are in no set."""
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    q = thr[1:][None, :] if class_conditional else thr[0]
    with np.errstate(invalid='ignore'):
        return np.asarray(class_scores, dtype=np.float32) <= q


def conformal_apply_block(arrays: Dict, extras: Optional[Dict], num_classes: int, scores: Sequence[str], thresholds, class_conditional: bool = False,
                          randomized: bool = True, seed: int = 0, raps_lambda: float = 0.01, raps_k: int = 1, row_offset: int = 0):
    """The result block of ``rovit_eval_conformal_apply`` (include/rovit_hip.h) from recorded arrays and (M, G, A) fp32 thresholds, on
    the host, and the (n, M_cls, A) membership bytes (bit c: class c is in the set).  The sum of sigma is in fp64."""
    C, M = int(num_classes), len(scores)
    thr = np.asarray(thresholds, dtype=np.float32).reshape(M, 1 + C if class_conditional else 1, -1)
    A = thr.shape[2]
    sc = conformal_scores(arrays, extras, C, scores, randomized, seed, raps_lambda, raps_k, row_offset)
    _, label, _, _, _ = _record_columns(arrays, extras)
    label = np.asarray(label).astype(np.int64).reshape(-1)
    n, ok = len(label), sc['label_ok']
    per = 16 + 32 * A
    blk = np.zeros(native.eval_conformal_apply_words(M, A), dtype=np.int64)
    blk[native.EVAL_CONF_N], blk[native.EVAL_CONF_BAD_LABELS], blk[native.EVAL_CONF_N_LABELLED] = n, int((~ok).sum()), int(ok.sum())
    member = np.zeros((n, sum(s in CONFORMAL_CLASS_SCORES for s in scores), A), dtype=np.uint8)
    mc = 0
    for m, name in enumerate(scores):
        base = native.EVAL_CONF_APPLY_SCORES + m * per
        valid = sc['valid'][m]
        blk[base], blk[base + 1] = int(valid.sum()), int((ok & ~valid).sum())
        y = label[valid]
        if name in CONFORMAL_CLASS_SCORES:
            blk[base + 8:base + 8 + C] = np.bincount(y, minlength=C)
        if name == 'mu_scaled':
            blk[base + 2:base + 3].view(np.float64)[0] = sc['sigma'][valid].astype(np.float64).sum()
        for a in range(A):
            at = base + 16 + 32 * a
            if name in CONFORMAL_CLASS_SCORES:
                inside = conformal_membership(sc['class_scores'][name], thr[m, :, a], class_conditional)
                member[:, mc, a] = (inside.astype(np.uint8) << np.arange(C, dtype=np.uint8)[None, :]).sum(axis=1)
                size, hit = inside.sum(axis=1)[valid], inside[valid][np.arange(len(y)), y]
                blk[at:at + C + 1] = np.bincount(size, minlength=C + 1)
                blk[at + 9:at + 9 + C + 1] = np.bincount(size[hit], minlength=C + 1)
                blk[at + 18:at + 18 + C] = np.bincount(y[hit], minlength=C)
                blk[at + 26] = int(hit.sum())
            else:
                blk[at + 26] = int((sc['columns'][m][valid] <= thr[m, 0, a]).sum())
        mc += name in CONFORMAL_CLASS_SCORES
    return blk, member


class Conformal:
    """Fitted split-conformal thresholds: ``alphas``, ``scores``, ``thresholds[score][alpha]`` (a float; with ``class_conditional`` an
    array of 1 + C: group 0 = all rows, 1 + c = true class c), ``status[score][alpha]`` ('ok' or 'trivial': k > n_g, the threshold is
    +inf; an array of strings with ``class_conditional``), ``n[score]`` (the valid rows n_g), ``k[score][alpha]``, ``less`` and ``equal``
    (the fitted rows below and at the threshold), ``bad_labels``, ``bad_rows[score]`` and the parameters the scores depend on
    (``num_classes``, ``class_conditional``, ``randomized``, ``seed``, ``raps_lambda``, ``raps_k``) and ``rows``, the number of rows it
    was fitted on: their u took the Philox counters 0 .. rows - 1, so ``evaluate`` draws the test rows' u from ``rows`` on.  A new row's label set
    {c : s(c) <= threshold} contains its true class with probability >= 1 - alpha when the row is exchangeable with the fitted ones
    (per class with ``class_conditional``); the interval centre +- threshold (times sigma for ``'mu_scaled'``) contains its severity."""

    def __init__(self, alphas, scores, num_classes: int, thresholds: Dict, status: Dict, n: Dict, k: Dict, less: Optional[Dict] = None,
                 equal: Optional[Dict] = None, bad_labels: int = 0, bad_rows: Optional[Dict] = None, class_conditional: bool = False,
                 randomized: bool = True, seed: int = 0, raps_lambda: float = 0.01, raps_k: int = 1, rows: int = 0):
        self.alphas, self.scores, self.num_classes = [float(a) for a in alphas], list(scores), int(num_classes)
        self.rows = int(rows)
        self.thresholds, self.status, self.n, self.k, self.less, self.equal = thresholds, status, n, k, less or {}, equal or {}
        self.bad_labels, self.bad_rows = int(bad_labels), dict(bad_rows or {})
        self.class_conditional, self.randomized, self.seed = bool(class_conditional), bool(randomized), int(seed)
        self.raps_lambda, self.raps_k = float(raps_lambda), int(raps_k)
        self.score_columns = self.u = self.block = None          # conformal(return_scores=True)

    def __repr__(self) -> str:
        return (f'Conformal(scores={self.scores!r}, alphas={self.alphas!r}, class_conditional={self.class_conditional}, '
                f'randomized={self.randomized}, n={self.n.get(self.scores[0])!r})')

    @property
    def params(self) -> Dict:
        return {'class_conditional': self.class_conditional, 'randomized': self.randomized, 'seed': self.seed, 'raps_lambda': self.raps_lambda,
                'raps_k': self.raps_k}

    def to_dict(self) -> Dict:
        """Plain floats, ints, strings and lists of them (levels in the order of ``alphas``; +inf as the string 'inf'): ``json.dumps``
        takes it, ``from_dict`` restores it."""
        def plain(v):
            if isinstance(v, (list, tuple, np.ndarray)):
                return [plain(x) for x in v]
            if isinstance(v, (str, np.str_)):
                return str(v)
            if isinstance(v, (float, np.floating)):
                return 'inf' if v == math.inf else float(v)
            return int(v)
        per_level = lambda d: {s: [plain(d[s][a]) for a in self.alphas] for s in self.scores}
        out = {'alphas': list(self.alphas), 'scores': list(self.scores), 'num_classes': self.num_classes, 'thresholds': per_level(self.thresholds),
               'status': per_level(self.status), 'n': {s: plain(self.n[s]) for s in self.scores}, 'k': per_level(self.k),
               'less': per_level(self.less) if self.less else {}, 'equal': per_level(self.equal) if self.equal else {},
               'bad_labels': self.bad_labels, 'bad_rows': {s: int(self.bad_rows.get(s, 0)) for s in self.scores}, 'rows': self.rows}
        out.update(self.params)
        return out

    @classmethod
    def from_dict(cls, d: Dict) -> 'Conformal':
        alphas, scores = [float(a) for a in d['alphas']], list(d['scores'])
        cc = bool(d.get('class_conditional', False))
        number = lambda v, kind: (np.array([kind(x) for x in v]) if isinstance(v, list) else kind(v))
        per_level = lambda key, kind: {s: {a: number(d[key][s][i], kind) for i, a in enumerate(alphas)} for s in scores} if d.get(key) else {}
        return cls(alphas, scores, d['num_classes'], per_level('thresholds', float), per_level('status', str),
                   {s: number(d['n'][s], int) for s in scores}, per_level('k', int), per_level('less', int), per_level('equal', int),
                   d.get('bad_labels', 0), d.get('bad_rows'), cc, d.get('randomized', True), d.get('seed', 0), d.get('raps_lambda', 0.01),
                   d.get('raps_k', 1), d.get('rows', 0))

    def threshold_array(self, scores: Optional[Sequence[str]] = None, alphas: Optional[Sequence[float]] = None) -> np.ndarray:
        """(M, G, A) fp32: the thresholds as ``rovit_eval_conformal_apply`` reads them."""
        scores, alphas = list(scores or self.scores), list(alphas or self.alphas)
        G = 1 + self.num_classes if self.class_conditional else 1
        out = np.zeros((len(scores), G, len(alphas)), dtype=np.float32)
        for m, s in enumerate(scores):
            for a, alpha in enumerate(alphas):
                out[m, :, a] = np.asarray(self.thresholds[s][alpha], dtype=np.float32).reshape(-1)
        return out

    def _check_record(self, acc: 'EvalAccumulator', what: str) -> None:
        if not isinstance(acc, EvalAccumulator) or acc.n < 1:
            raise RovitHipError(f'{what}: an EvalAccumulator with recorded rows is needed')
        if acc.num_classes != self.num_classes:
            raise RovitHipError(f'{what}: fitted on {self.num_classes} classes, the accumulator holds {acc.num_classes}')
        if list(acc._conformal_names(self.scores)) != self.scores:          # raises when a column the scores need is missing
            raise RovitHipError(f'{what}: the accumulator cannot provide the scores {self.scores!r}')

    def evaluate(self, acc: 'EvalAccumulator', _max_workgroups: int = 0) -> Dict:
        """Score the test rows of another accumulator against the fitted thresholds: ``{'n', 'bad_labels', 'scores': {score: {'n',
        'bad_rows', 'levels': {alpha: {...}}}}}``.  Per class score and level: ``coverage``, ``mean_set_size``, ``size_histogram`` (sizes
        0..C), ``coverage_by_class``, ``coverage_by_size``, ``empty_rate``, ``singleton_rate`` and ``singleton_accuracy`` (NaN where a
        denominator is 0).  Per regression score and level: ``coverage``, ``mean_width`` (2 q for the absolute scores, 2 q mean sigma for
        ``'mu_scaled'``) and ``infinite``.  An extra-column score: ``coverage``.  Rows are left out and counted as in the fit.  With
        ``class_conditional`` class c is in the set iff s(c) <= the threshold of group 1 + c; the other scores use group 0.  u is drawn
        for the counter ``rows`` + the row's index in ``acc``, past the fitted rows' draws.  On the device the call makes ONE device-to-host copy (``'block'`` holds it)."""
        self._check_record(acc, 'Conformal.evaluate')
        M, A, C = len(self.scores), len(self.alphas), self.num_classes
        thr = self.threshold_array()
        if acc.device.type != 'cuda':
            arrays, extras = acc._host_columns()
            block, _ = conformal_apply_block(arrays, extras, C, self.scores, thr, row_offset=self.rows, **self.params)
        else:
            n = acc.n
            out = torch.empty(native.eval_conformal_apply_words(M, A), dtype=torch.int64, device=acc.device)
            ws_bytes = native.load().rovit_eval_conformal_apply_workspace_bytes(n, M)
            workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=acc.device)
            thr_dev = torch.from_numpy(thr.reshape(-1)).to(acc.device, non_blocking=True)
            d = acc._conformal_descriptor(self.scores, A, self.params)
            d.max_workgroups, d.row_offset = _max_workgroups, self.rows
            d.thresholds, d.workspace, d.workspace_bytes, d.result = native.ptr(thr_dev), native.ptr(workspace), ws_bytes, native.ptr(out)
            native.call('rovit_eval_conformal_apply', ctypes.byref(d), native.stream_ptr())
            block = out.cpu().numpy()                            # the call's single device-to-host copy
        res = conformal_metrics_from_block(block, self.scores, self.alphas, thr, C)
        res['block'] = np.array(block)
        return res

    def _level(self, alpha) -> float:
        if alpha is None:
            return self.alphas[0]
        if float(alpha) not in self.alphas:
            raise RovitHipError(f'Conformal: the level {alpha!r} was not fitted (fitted: {self.alphas!r})')
        return float(alpha)

    def predict(self, outputs: Dict, score: str = 'aps', alpha: Optional[float] = None, row_offset: int = 0) -> Dict:
        """Label sets and severity intervals of a model's output dict, for deployment: ``'sets'`` (B, C) bool from the class score
        ``score`` at level ``alpha`` (None: the first fitted level), ``'set_size'`` (B,), and, when their score was fitted,
        ``'kan_interval'`` = kan_severity +- q ('kan_abs') and ``'mu_interval'`` = mu +- q sigma ('mu_scaled', sigma = exp(0.5 log_var))
        or mu +- q ('mu_abs', used when 'mu_scaled' was not fitted), both (B, 2).  The softmax is torch's; on the device the membership
        comes from ``rovit_eval_conformal_apply``'s score function in one launch, with u drawn for the rows ``row_offset + i``, and
        nothing is copied to the host.  Offsets from ``rows`` on keep the draws apart from those of the fitted rows."""
        if score not in CONFORMAL_CLASS_SCORES or score not in self.scores:
            raise RovitHipError(f'Conformal.predict: {score!r} is not a fitted class score (fitted: {[s for s in self.scores if s in CONFORMAL_CLASS_SCORES]!r})')
        alpha = self._level(alpha)
        if not (isinstance(row_offset, int) and 0 <= row_offset < 1 << 32):
            raise RovitHipError(f'Conformal.predict: row_offset must be an integer in [0, 2^32), got {row_offset!r}')
        logits = outputs['cls_logits'].detach()
        C = self.num_classes
        if logits.dim() != 2 or logits.shape[1] != C or logits.shape[0] < 1:
            raise RovitHipError(f'Conformal.predict: cls_logits must be (B >= 1, {C}), got {tuple(logits.shape)}')
        B = logits.shape[0]
        probs = torch.softmax(logits.float(), dim=1).contiguous()
        thr = self.threshold_array([score], [alpha])
        bits = torch.arange(C, device=logits.device)
        if not logits.is_cuda:
            s, _ = conformal_class_scores(probs.numpy(), score, conformal_uniforms(B, self.seed, row_offset) if self.randomized else None,
                                          self.raps_lambda, self.raps_k)
            sets = torch.from_numpy(conformal_membership(s, thr[0, :, 0], self.class_conditional))
        else:
            member = torch.empty(B, dtype=torch.uint8, device=logits.device)
            thr_dev = torch.from_numpy(thr.reshape(-1)).to(logits.device, non_blocking=True)
            d = native.EvalConf()
            d.n, d.num_classes, d.num_scores, d.num_levels, d.class_conditional, d.randomized = B, C, 1, 1, int(self.class_conditional), int(self.randomized)
            d.raps_k, d.raps_lambda, d.seed, d.row_offset = self.raps_k, self.raps_lambda, self.seed, row_offset
            d.score_kind[0] = CONFORMAL_KINDS[score]
            d.probs, d.thresholds, d.member_out = native.ptr(probs), native.ptr(thr_dev), native.ptr(member)
            native.call('rovit_eval_conformal_apply', ctypes.byref(d), native.stream_ptr())
            sets = ((member.long()[:, None] >> bits[None, :]) & 1).bool()
        out = {'sets': sets, 'set_size': sets.sum(dim=1)}
        flat = lambda t: t.detach().float().reshape(-1)
        band = lambda centre, half: torch.stack([centre - half, centre + half], dim=1)
        if 'kan_abs' in self.scores and outputs.get('kan_severity') is not None:
            out['kan_interval'] = band(flat(outputs['kan_severity']), float(self.threshold_array(['kan_abs'], [alpha])[0, 0, 0]))
        if outputs.get('mu') is not None:
            if 'mu_scaled' in self.scores and outputs.get('log_var') is not None:
                q = float(self.threshold_array(['mu_scaled'], [alpha])[0, 0, 0])
                out['mu_interval'] = band(flat(outputs['mu']), q * torch.exp(0.5 * flat(outputs['log_var'])))
            elif 'mu_abs' in self.scores:
                out['mu_interval'] = band(flat(outputs['mu']), float(self.threshold_array(['mu_abs'], [alpha])[0, 0, 0]))
        return out


def conformal_from_block(blk: np.ndarray, alphas: Sequence[float], scores: Sequence[str], num_classes: int, class_conditional: bool = False,
                         randomized: bool = True, seed: int = 0, raps_lambda: float = 0.01, raps_k: int = 1) -> Conformal:
    """The ``Conformal`` that ``EvalAccumulator.conformal`` returns from one result block.  Raises when a score has no valid row."""
    blk = np.asarray(blk, dtype=np.int64)
    C, M, A = int(num_classes), len(scores), len(alphas)
    G = 1 + C if class_conditional else 1
    n = int(blk[native.EVAL_CONF_N])
    if int(blk[native.EVAL_CONF_N_LABELLED]) < 1:
        raise RovitHipError(f'conformal: none of the {n} recorded rows has a class label in [0, {C})')
    e = blk[native.EVAL_CONF_ENTRIES:native.EVAL_CONF_ENTRIES + native.EVAL_CONF_ENTRY_WORDS * M * G * A].reshape(M, G, A, native.EVAL_CONF_ENTRY_WORDS)
    q = e[..., 4].astype(np.uint32).view(np.float32)
    pick = (lambda v: v.copy()) if class_conditional else (lambda v: v[0].item())
    fields = {'thresholds': {}, 'status': {}, 'k': {}, 'less': {}, 'equal': {}}
    n_valid = {}
    for m, s in enumerate(scores):
        if int(e[m, 0, 0, 0]) < 1:
            raise RovitHipError(f'conformal: the score {s!r} has no valid row among the {n} recorded ones')
        n_valid[s] = pick(e[m, :, 0, 0])
        for key, values in (('thresholds', q[m].astype(np.float64)), ('k', e[m, :, :, 1]), ('less', e[m, :, :, 2]), ('equal', e[m, :, :, 3]),
                            ('status', np.where(e[m, :, :, 5] != 0, 'trivial', 'ok'))):
            fields[key][s] = {alpha: pick(values[:, a]) for a, alpha in enumerate(alphas)}
    return Conformal(alphas, scores, C, fields['thresholds'], fields['status'], n_valid, fields['k'], fields['less'], fields['equal'],
                     int(blk[native.EVAL_CONF_BAD_LABELS]), {s: int(blk[native.EVAL_CONF_BAD_ROWS + m]) for m, s in enumerate(scores)},
                     class_conditional, randomized, seed, raps_lambda, raps_k, n)


def conformal_metrics_from_block(blk: np.ndarray, scores: Sequence[str], alphas: Sequence[float], thresholds: np.ndarray, num_classes: int) -> Dict:
    """The dict ``Conformal.evaluate`` returns from one result block of ``rovit_eval_conformal_apply``; every ratio is taken in fp64."""
    blk = np.asarray(blk, dtype=np.int64)
    f = blk.view(np.float64)
    C, A = int(num_classes), len(alphas)
    per = 16 + 32 * A
    ratio = lambda a, b: float(a) / float(b) if b else float('nan')
    res = {'n': int(blk[native.EVAL_CONF_N]), 'bad_labels': int(blk[native.EVAL_CONF_BAD_LABELS]), 'scores': {}}
    for m, name in enumerate(scores):
        base = native.EVAL_CONF_APPLY_SCORES + m * per
        nv = int(blk[base])
        entry = {'n': nv, 'bad_rows': int(blk[base + 1]), 'levels': {}}
        for a, alpha in enumerate(alphas):
            at = base + 16 + 32 * a
            q = float(thresholds[m, 0, a])
            lv = {'coverage': ratio(blk[at + 26], nv)}
            if name in CONFORMAL_CLASS_SCORES:
                hist, by_size, by_class = blk[at:at + C + 1], blk[at + 9:at + 9 + C + 1], blk[at + 18:at + 18 + C]
                lv.update(mean_set_size=ratio(int((np.arange(C + 1) * hist).sum()), nv), size_histogram=[int(v) for v in hist],
                          coverage_by_class=[ratio(by_class[c], blk[base + 8 + c]) for c in range(C)],
                          coverage_by_size=[ratio(by_size[k], hist[k]) for k in range(C + 1)], empty_rate=ratio(hist[0], nv),
                          singleton_rate=ratio(hist[1], nv), singleton_accuracy=ratio(by_size[1], hist[1]))
            elif name in ('kan_abs', 'mu_abs'):
                lv.update(mean_width=2.0 * q, infinite=math.isinf(q))
            elif name == 'mu_scaled':
                lv.update(mean_width=2.0 * q * ratio(f[base + 2], nv), infinite=math.isinf(q))
            entry['levels'][alpha] = lv
        res['scores'][name] = entry
    return res


# ---- selective prediction: restatement and summaries ---------------------------------------------------------------------------

SELECTIVE_SCORES = {'confidence': native.EVAL_SEL_CONFIDENCE, 'entropy': native.EVAL_SEL_ENTROPY, 'sigma': native.EVAL_SEL_SIGMA}
SELECTIVE_RISKS = {'error': native.EVAL_SEL_ERROR, 'abs_err': native.EVAL_SEL_ABS_ERR}
SELECTIVE_BUILTIN = frozenset(SELECTIVE_SCORES) | frozenset(SELECTIVE_RISKS) | {'mu_abs_err'}


def coverage_counts(n: int, coverages: int) -> np.ndarray:
    """k_p = ceil(p n / P) for p = 1..P, in integers: the rows kept at curve point p."""
    p = np.arange(1, coverages + 1, dtype=np.int64)
    return (p * n + coverages - 1) // coverages


def selective_risks(u, l) -> np.ndarray:
    """r_1..r_n of one score column ``u`` (fp32) and one risk column ``l``: the rows by ascending u (stable, so ties keep the row order),
    Pref the fp64 running sum of the sorted risks, and for a tie group in slots [g, g + m) and g < k <= g + m
    r_k = (Pref[g] + (k - g) (Pref[g + m] - Pref[g]) / m) / k: every row of a group counts with the group's mean risk."""
    u = np.asarray(u, dtype=np.float32).reshape(-1)
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    n = u.shape[0]
    order = np.argsort(u, kind='stable')
    us = u[order]
    pref = np.concatenate([[0.0], np.cumsum(l[order])])
    g = np.searchsorted(us, us, side='left')
    m = np.searchsorted(us, us, side='right') - g
    k = np.arange(1, n + 1)
    return (pref[g] + (k - g) * (pref[g + m] - pref[g]) / m) / k


def selective_reference(keys, risks, coverages: int = 20) -> Dict[str, np.ndarray]:
    """The definitions of the selective-prediction score card in numpy fp64: ``keys`` (S, n) fp32 score columns (higher = less
    certain), ``risks`` (K, n) fp32 risk columns >= 0.  Returns ``n``, ``k`` (k_p), ``coverages`` (k_p / n), per risk ``mean`` (K,) = r_n,
    ``oracle_aurc`` (K,) and ``oracle_curve`` (K, P) (the risk ordered by itself), per pair ``aurc`` (S, K) = (1/n) sum_k r_k and
    ``curve`` (S, K, P) = r_{k_p}, and per score ``thresholds`` (S, P): the score in sorted slot k_p - 1, widened.  The oracle of the
    kernel, and what ``selective()`` runs for CPU tensors."""
    keys = np.atleast_2d(np.asarray(keys, dtype=np.float32))
    risks = np.atleast_2d(np.asarray(risks, dtype=np.float32))
    (S, n), K, P = keys.shape, risks.shape[0], int(coverages)
    if risks.shape[1] != n or n < 1 or P < 1:
        raise RovitHipError(f'selective_reference: keys {keys.shape} and risks {risks.shape} must share n >= 1 rows, coverages >= 1')
    kp = coverage_counts(n, P)
    out = {'n': n, 'k': kp, 'coverages': kp / n, 'mean': np.zeros(K), 'oracle_aurc': np.zeros(K), 'oracle_curve': np.zeros((K, P)),
           'aurc': np.zeros((S, K)), 'curve': np.zeros((S, K, P)), 'thresholds': np.zeros((S, P))}
    for k in range(K):
        r = selective_risks(risks[k], risks[k])
        out['mean'][k], out['oracle_aurc'][k], out['oracle_curve'][k] = r[n - 1], r.sum() / n, r[kp - 1]
        for s in range(S):
            r = selective_risks(keys[s], risks[k])
            out['aurc'][s, k], out['curve'][s, k] = r.sum() / n, r[kp - 1]
    for s in range(S):
        out['thresholds'][s] = np.sort(keys[s], kind='stable')[kp - 1].astype(np.float64)
    return out


def selective_block(keys, risks, coverages: int = 20, bad_labels: int = 0) -> np.ndarray:
    """The result block of ``rovit_eval_selective`` (include/rovit_hip.h) from the ranked columns, on the host: int64 words with the
    fp64 section stored bit for bit, through ``selective_reference`` (skipped when a counter makes the order meaningless)."""
    keys = np.atleast_2d(np.asarray(keys, dtype=np.float32))
    risks = np.atleast_2d(np.asarray(risks, dtype=np.float32))
    (S, n), K, P = keys.shape, risks.shape[0], int(coverages)
    off = native.eval_selective_offsets(S, K, P)
    blk = np.zeros(off['words'], dtype=np.int64)
    f = blk.view(np.float64)
    blk[native.EVAL_SEL_NONFINITE_KEYS] = int((~np.isfinite(keys)).sum())
    blk[native.EVAL_SEL_NONFINITE_RISKS] = int((~np.isfinite(risks)).sum())
    blk[native.EVAL_SEL_NEGATIVE_RISKS] = int((risks < 0).sum())
    blk[native.EVAL_SEL_BAD_LABELS] = bad_labels
    blk[native.EVAL_SEL_N] = n
    if blk[:native.EVAL_SEL_NEGATIVE_RISKS + 1].any():
        return blk
    ref = selective_reference(keys, risks, P)
    for k in range(K):
        at = off['risks'] + k * (2 + P)
        f[at], f[at + 1], f[at + 2:at + 2 + P] = ref['mean'][k], ref['oracle_aurc'][k], ref['oracle_curve'][k]
        for s in range(S):
            at = off['pairs'] + (s * K + k) * (1 + P)
            f[at], f[at + 1:at + 1 + P] = ref['aurc'][s, k], ref['curve'][s, k]
    for s in range(S):
        f[off['thresholds'] + s * P:off['thresholds'] + (s + 1) * P] = ref['thresholds'][s]
    return blk


def selective_columns(arrays: Dict[str, np.ndarray], extras: Dict[str, np.ndarray], scores: Sequence[str], risks: Sequence[str]):
    """The (S, n) score and (K, n) risk columns in fp32 from recorded arrays (keys probs, pred, label, sev_pred, sev_true, uncertainty)
    and extra columns, as the kernel's prepare stage builds them: numpy float32 for confidence and abs_err, fp64 rounded to fp32 for
    entropy."""
    probs = np.asarray(arrays['probs'], dtype=np.float32)
    st, sp = np.asarray(arrays['sev_true'], dtype=np.float32), np.asarray(arrays['sev_pred'], dtype=np.float32)

    def entropy():
        p = probs.astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            return (-np.where(p == 0, 0.0, p * np.log(p)).sum(axis=1)).astype(np.float32)
    make = {'confidence': lambda: np.float32(1.0) - probs.max(axis=1), 'entropy': entropy,
            'sigma': lambda: np.asarray(arrays['uncertainty'], dtype=np.float32),
            'error': lambda: (np.asarray(arrays['pred']) != np.asarray(arrays['label'])).astype(np.float32),
            'abs_err': lambda: np.abs(st - sp), 'mu_abs_err': lambda: np.abs(st - np.asarray(extras['mu'], dtype=np.float32))}
    column = lambda name, kinds: make[name]() if name in kinds else np.asarray(extras[name], dtype=np.float32)
    return (np.stack([column(s, ('confidence', 'entropy', 'sigma')) for s in scores]),
            np.stack([column(r, ('error', 'abs_err', 'mu_abs_err')) for r in risks]))


def selective_from_block(blk: np.ndarray, scores: Sequence[str], risks: Sequence[str], coverages: int, num_classes: int) -> Dict:
    """The dict ``EvalAccumulator.selective`` returns from one result block; raises on its counters."""
    S, K, P = len(scores), len(risks), int(coverages)
    off = native.eval_selective_offsets(S, K, P)
    blk = np.asarray(blk, dtype=np.int64)
    f = blk.view(np.float64)
    n = int(blk[native.EVAL_SEL_N])
    for word, text in ((native.EVAL_SEL_BAD_LABELS, f'class labels outside [0, {num_classes})'),
                       (native.EVAL_SEL_NONFINITE_KEYS, 'non-finite score values'), (native.EVAL_SEL_NONFINITE_RISKS, 'non-finite risk values'),
                       (native.EVAL_SEL_NEGATIVE_RISKS, 'negative risk values')):
        if int(blk[word]):
            raise RovitHipError(f'selective: {int(blk[word])} {text}')
    res = {'n': n, 'coverages': coverage_counts(n, P) / n, 'risks': {}, 'scores': {}}
    for k, risk in enumerate(risks):
        at = off['risks'] + k * (2 + P)
        res['risks'][risk] = {'mean': float(f[at]), 'oracle_aurc': float(f[at + 1]), 'oracle_curve': f[at + 2:at + 2 + P].copy()}
    for s, score in enumerate(scores):
        entry = {'thresholds': f[off['thresholds'] + s * P:off['thresholds'] + (s + 1) * P].copy()}
        for k, risk in enumerate(risks):
            at = off['pairs'] + (s * K + k) * (1 + P)
            aurc, mean, oracle = float(f[at]), res['risks'][risk]['mean'], res['risks'][risk]['oracle_aurc']
            e_aurc = aurc - oracle
            entry[risk] = {'aurc': aurc, 'e_aurc': e_aurc, 'normalized': e_aurc / (mean - oracle) if mean != oracle else float('nan'),
                           'curve': f[at + 1:at + 1 + P].copy()}
        res['scores'][score] = entry
    return res


# ---- bootstrap: restatement and summaries ---------------------------------------------------------------------------------------

BOOT_METRICS = (('accuracy', native.EVAL_BOOT_ACCURACY), ('macro_f1', native.EVAL_BOOT_MACRO_F1), ('weighted_f1', native.EVAL_BOOT_WEIGHTED_F1),
                ('mae', native.EVAL_BOOT_MAE), ('spearman_rho', native.EVAL_BOOT_RHO), ('brier_score', native.EVAL_BOOT_BRIER),
                ('ece', native.EVAL_BOOT_ECE))
BOOT_CLASS_METRICS = (('precision', native.EVAL_BOOT_PRECISION), ('recall', native.EVAL_BOOT_RECALL), ('f1', native.EVAL_BOOT_F1))


def _check_bootstrap_args(num_resamples, seed, confidence) -> int:
    if not (isinstance(num_resamples, int) and 1 <= num_resamples <= native.EVAL_BOOT_MAX_RESAMPLES):
        raise RovitHipError(f'bootstrap: num_resamples must be in 1..{native.EVAL_BOOT_MAX_RESAMPLES}, got {num_resamples!r}')
    if not (isinstance(seed, int) and 0 <= seed < 1 << 64):
        raise RovitHipError(f'bootstrap: seed must be an integer in [0, 2^64), got {seed!r}')
    if not 0.0 < confidence < 1.0:
        raise RovitHipError(f'bootstrap: confidence must lie in (0, 1), got {confidence!r}')
    return num_resamples


def stratification(y_true, num_classes: int):
    """(perm, starts) of a stratified bootstrap: the rows in a stable order by true class with the bad labels last, and the C + 2
    segment starts."""
    y = np.asarray(y_true).astype(np.int64).reshape(-1)
    key = np.where((y < 0) | (y >= num_classes), num_classes, y)
    perm = np.argsort(key, kind='stable').astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=num_classes + 1))]).astype(np.int64)
    return perm, starts


def bootstrap_indices(n: int, r: int, seed: int, starts=None, perm=None) -> np.ndarray:
    """The n rows replicate ``r`` draws, as ``rovit_eval_bootstrap`` draws them: Philox4x32-10 with key ``seed`` and counter
    (j // 4, r, EVAL_BOOT_STREAM, 0); word j % 4 gives (word * n) >> 32.  With ``starts`` and ``perm`` (``stratification``) draw j stays
    in the segment that contains j: perm[starts[s] + ((word * n_s) >> 32)]."""
    from oracle.philox import philox4x32_10 as philox          # checker only, like the head-phase masks
    j = np.arange(n, dtype=np.uint64)
    words = philox([j >> np.uint64(2), np.full(n, r, np.uint64), np.full(n, native.EVAL_BOOT_STREAM, np.uint64), np.zeros(n, np.uint64)],
                   [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    word = np.stack(words, axis=1)[np.arange(n), (j & np.uint64(3)).astype(np.int64)]
    if starts is None:
        return ((word * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    starts, perm = np.asarray(starts, dtype=np.int64), np.asarray(perm, dtype=np.int64)
    seg = np.searchsorted(starts[:-1], np.arange(n), side='right') - 1
    size = (starts[seg + 1] - starts[seg]).astype(np.uint64)
    return perm[starts[seg] + ((word * size) >> np.uint64(32)).astype(np.int64)]


def table_row_from_block(blk: np.ndarray, num_classes: int, n_bins: int) -> np.ndarray:
    """One row of the bootstrap's metric table (EVAL_BOOT_* columns) from a result block, through ``metrics_from_block``."""
    m = metrics_from_block(blk, num_classes, n_bins)
    row = np.zeros(native.EVAL_BOOT_COLS, dtype=np.float64)
    for name, col in BOOT_METRICS:
        row[col] = m[name]
    for k, col in BOOT_CLASS_METRICS:
        row[col:col + num_classes] = [c[k] for c in m['per_class']]
    return row


def bootstrap_reference(arrays: Dict, num_classes: int, n_bins: int = 10, num_resamples: int = 1000, seed: int = 0,
                        stratified: bool = False):
    """The bootstrap on the host in fp64: ``arrays`` as ``EvalAccumulator.arrays()`` returns them; each replicate is a numpy resample
    (``bootstrap_indices``) put through ``result_block_from_arrays`` and ``metrics_from_block``.  Returns (table (R, EVAL_BOOT_COLS)
    float64, blocks (R, 272) int64): the oracle of the kernel, and what ``bootstrap()`` runs for CPU tensors."""
    y_true, y_pred = np.asarray(arrays['y_true']), np.asarray(arrays['y_pred'])
    probs, st, sp = np.asarray(arrays['y_probs']), np.asarray(arrays['severity_true']), np.asarray(arrays['severity_pred'])
    n = len(y_true)
    perm, starts = stratification(y_true, num_classes) if stratified else (None, None)
    table = np.zeros((num_resamples, native.EVAL_BOOT_COLS), dtype=np.float64)
    blocks = np.zeros((num_resamples, native.EVAL_RESULT_WORDS), dtype=np.int64)
    for r in range(num_resamples):
        idx = bootstrap_indices(n, r, seed, starts, perm)
        blocks[r] = result_block_from_arrays(y_true[idx], y_pred[idx], probs[idx], st[idx], sp[idx], num_classes, n_bins)
        table[r] = table_row_from_block(blocks[r], num_classes, n_bins)
    return table, blocks


def _interval(col: np.ndarray, value: float, confidence: float) -> Dict[str, float]:
    """value, mean, se (ddof = 1) and the percentile interval of one column of the table; NaN replicates are left out."""
    ok = col[~np.isnan(col)]
    if ok.size == 0:
        return {'value': value, 'mean': float('nan'), 'se': float('nan'), 'lo': float('nan'), 'hi': float('nan')}
    lo, hi = np.quantile(ok, [(1.0 - confidence) / 2.0, (1.0 + confidence) / 2.0])          # = np.nanquantile(col, ...), linear
    return {'value': value, 'mean': float(ok.mean()), 'se': float(ok.std(ddof=1)) if ok.size > 1 else float('nan'), 'lo': float(lo),
            'hi': float(hi)}


def mcnemar_exact(b01: int, b10: int) -> float:
    """McNemar's exact two-sided test on the discordant counts: p = min(1, 2 P[X <= min(b01, b10)]), X ~ Binomial(b01 + b10, 1/2).
    Exact integers up to 1024 discordant rows, log-gamma beyond."""
    n, k = int(b01) + int(b10), min(int(b01), int(b10))
    if n == 0:
        return 1.0
    if n <= 1024:
        return min(1.0, 2 * sum(math.comb(n, i) for i in range(k + 1)) / 2 ** n)
    i = torch.arange(k + 1, dtype=torch.float64)
    logs = math.lgamma(n + 1) - torch.lgamma(i + 1) - torch.lgamma(n - i + 1) - n * math.log(2.0)
    return min(1.0, 2.0 * float(torch.exp(torch.logsumexp(logs, 0))))


def _paired(diffs: np.ndarray, a: float, b: float, confidence: float) -> Dict[str, float]:
    """b - a with the percentile interval of the replicate differences and the two-sided bootstrap p-value
    min(1, 2 min(#{d <= 0} + 1, #{d >= 0} + 1) / (R + 1)) over the replicates whose difference is a number."""
    ok = diffs[~np.isnan(diffs)]
    if ok.size == 0:
        return {'a': a, 'b': b, 'diff': b - a, 'lo': float('nan'), 'hi': float('nan'), 'p_value': float('nan')}
    lo, hi = np.quantile(ok, [(1.0 - confidence) / 2.0, (1.0 + confidence) / 2.0])
    p = min(1.0, 2.0 * min(int((ok <= 0).sum()) + 1, int((ok >= 0).sum()) + 1) / (ok.size + 1))
    return {'a': a, 'b': b, 'diff': b - a, 'lo': float(lo), 'hi': float(hi), 'p_value': p}


def paired_bootstrap(acc_a: 'EvalAccumulator', acc_b: 'EvalAccumulator', num_resamples: int = 1000, seed: int = 0, confidence: float = 0.95,
                     stratified: bool = False) -> Dict:
    """Paired bootstrap of two models scored on the same test rows: both accumulators are resampled with the same seed, hence the same
    rows, and each metric's replicate differences b - a give ``{'a', 'b', 'diff', 'lo', 'hi', 'p_value'}`` (per class under
    ``'per_class'``).  ``'mcnemar'`` holds McNemar's exact two-sided test on the discordant counts (b01: a right and b wrong, b10 the
    reverse).  Needs the same device, the same number of rows and the same class labels row for row (checked on the device: the flag
    travels in the call's one device-to-host copy)."""
    R = _check_bootstrap_args(num_resamples, seed, confidence)
    for acc in (acc_a, acc_b):
        if not isinstance(acc, EvalAccumulator) or acc.n < 1:
            raise RovitHipError('paired_bootstrap: two EvalAccumulators with recorded rows are needed')
    if acc_a.n != acc_b.n:
        raise RovitHipError(f'paired_bootstrap: {acc_a.n} rows against {acc_b.n}: the models must be scored on the same test rows')
    if (acc_a.num_classes, acc_a.n_bins) != (acc_b.num_classes, acc_b.n_bins) or acc_a.device != acc_b.device:
        raise RovitHipError('paired_bootstrap: the accumulators differ in classes, calibration bins or device')
    n, C, W, COLS = acc_a.n, acc_a.num_classes, native.EVAL_RESULT_WORDS, native.EVAL_BOOT_COLS
    if acc_a.device.type != 'cuda':
        arr = [acc.arrays() for acc in (acc_a, acc_b)]
        differ = not np.array_equal(arr[0]['y_true'], arr[1]['y_true'])
        right = [x['y_pred'] == x['y_true'] for x in arr]
        b01, b10 = int((right[0] & ~right[1]).sum()), int((~right[0] & right[1]).sum())
        tables = [None, None] if differ else [bootstrap_reference(x, C, acc_a.n_bins, R, seed, stratified)[0] for x in arr]
    else:
        out = torch.empty(2 * W + 2 * R * COLS + 3, dtype=torch.int64, device=acc_a.device)
        for k, acc in enumerate((acc_a, acc_b)):
            t0 = 2 * W + k * R * COLS
            out[k * W:(k + 1) * W].copy_(acc._bootstrap_launch(R, seed, stratified, out[t0:t0 + R * COLS], None))
        la, lb = acc_a._rec['label'][:n], acc_b._rec['label'][:n]
        ra, rb = acc_a._rec['pred'][:n] == la, acc_b._rec['pred'][:n] == lb
        out[-3:] = torch.stack([(la != lb).sum(), (ra & ~rb).sum(), (~ra & rb).sum()])
        host = out.cpu().numpy()                             # the call's single device-to-host copy
        for k, acc in enumerate((acc_a, acc_b)):
            if acc._block is None:
                acc._block = host[k * W:(k + 1) * W].copy()
        differ, b01, b10 = bool(host[-3]), int(host[-2]), int(host[-1])
        tables = [host[2 * W + k * R * COLS:2 * W + (k + 1) * R * COLS].view(np.float64).reshape(R, COLS) for k in range(2)]
    if differ:
        raise RovitHipError('paired_bootstrap: the class labels of the two accumulators differ: not the same test rows in the same order')
    ma, mb = acc_a.compute(), acc_b.compute()
    d = tables[1] - tables[0]
    res = {name: _paired(d[:, col], ma[name], mb[name], confidence) for name, col in BOOT_METRICS}
    res['per_class'] = [{k: _paired(d[:, col + c], ma['per_class'][c][k], mb['per_class'][c][k], confidence) for k, col in BOOT_CLASS_METRICS}
                        for c in range(C)]
    res['mcnemar'] = {'b01': b01, 'b10': b10, 'p_value': mcnemar_exact(b01, b10)}
    res.update(num_resamples=R, seed=seed, confidence=confidence, stratified=bool(stratified))
    return res


def validate(model: torch.nn.Module, loader, loss_fn, n_bins: int = 10) -> Dict[str, float]:
    """The reference's ``Trainer.val_epoch`` (training/trainer.py:183-231) with one synchronisation: eval mode, no_grad,
    ``loss_fn(outputs, class_labels, severity_labels, stage=4)`` per batch; returns loss, cls_loss, ord_loss, unc_loss, kan_loss as means
    over batches and accuracy (percent) over samples."""
    model.eval()
    dev = next(model.parameters()).device
    acc: Optional[EvalAccumulator] = None
    with torch.no_grad():
        for images, class_labels, severity_labels in loader:
            images = images.to(dev, non_blocking=True)
            class_labels = class_labels.to(dev, non_blocking=True)
            severity_labels = severity_labels.to(dev, non_blocking=True)
            outputs = model(images)
            losses = loss_fn(outputs, class_labels, severity_labels, stage=4)
            if acc is None:
                acc = EvalAccumulator(int(outputs['cls_logits'].shape[1]), n_bins)
            acc.update(outputs, class_labels, severity_labels, losses=losses)
    if acc is None:
        raise RovitHipError('validate: the loader yielded no batch')
    m = acc.compute()
    out = {k: m[k] for k in ('loss', 'cls_loss', 'ord_loss', 'unc_loss', 'kan_loss')}
    out['accuracy'] = 100. * m['correct'] / m['n']          # the trainer's own expression (trainer.py:228), to the last bit
    return out


def class_table(per_class: Sequence[Dict], class_names: Sequence[str]) -> Dict[str, Dict]:
    """The per-class list of ``compute()`` keyed by class name, as evaluation/metrics.py's ``per_class_metrics`` returns it."""
    return {name: dict(per_class[i]) for i, name in enumerate(class_names)}
