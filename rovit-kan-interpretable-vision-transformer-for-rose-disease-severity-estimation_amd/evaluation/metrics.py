"""The reference's evaluation/metrics.py (:9-122) on the package's own fp64 code paths: same names, signatures and return units
(percent where the reference returns percent), numpy arrays in.  No sklearn, no scipy: the classification metrics come from an integer
confusion matrix, Spearman's rho from counted ranks (``rovit_hip.evaluation``)."""
import time
from typing import Sequence, Tuple

import numpy as np
import torch

from rovit_hip import evaluation as _ev


def _confusion(y_true, y_pred, labels=None) -> np.ndarray:
    """Integer confusion matrix over ``labels`` (default: the sorted values that occur in either array, as sklearn takes them);
    samples whose label or prediction is outside ``labels`` are left out."""
    y_true, y_pred = np.asarray(y_true).reshape(-1), np.asarray(y_pred).reshape(-1)
    labels = np.unique(np.concatenate([y_true, y_pred])) if labels is None else np.asarray(list(labels))
    k = len(labels)
    order = np.argsort(labels, kind='stable')
    srt = labels[order]

    def index(v):
        pos = np.clip(np.searchsorted(srt, v), 0, k - 1)
        return np.where(srt[pos] == v, order[pos], -1)

    it, ip = index(y_true), index(y_pred)
    ok = (it >= 0) & (ip >= 0)
    return np.bincount(it[ok] * k + ip[ok], minlength=k * k).reshape(k, k).astype(np.int64)


def accuracy(y_true: np.ndarray, y_pred: np.ndarray) -> float:
    return float(np.mean(np.asarray(y_true) == np.asarray(y_pred))) * 100


def macro_f1(y_true: np.ndarray, y_pred: np.ndarray) -> float:
    return _ev.f1_averages(_confusion(y_true, y_pred))[0] * 100


def weighted_f1(y_true: np.ndarray, y_pred: np.ndarray) -> float:
    """``f1_score(average='weighted') * 100``, which the reference's Evaluator calls directly (evaluator.py:80)."""
    return _ev.f1_averages(_confusion(y_true, y_pred))[1] * 100


def mae(y_true: np.ndarray, y_pred: np.ndarray) -> float:
    return float(np.mean(np.abs(np.asarray(y_true, dtype=np.float64) - np.asarray(y_pred, dtype=np.float64))))


def spearman_rho(y_true: np.ndarray, y_pred: np.ndarray) -> float:
    return _ev.rho_from_rank_sums(*_ev.rank_sums(y_true, y_pred))


def brier_score(y_true: np.ndarray, y_proba: np.ndarray) -> float:
    p = np.asarray(y_proba, dtype=np.float64)
    onehot = np.zeros_like(p)
    onehot[np.arange(len(p)), np.asarray(y_true).astype(np.int64)] = 1.0
    return float(np.mean(np.sum((p - onehot) ** 2, axis=1)))


def ece(y_true: np.ndarray, y_conf: np.ndarray, n_bins: int = 10) -> float:
    """Expected calibration error over ``n_bins`` equal-width bins (lo < confidence <= hi).  2-D ``y_conf``: class probabilities
    (prediction = first argmax); 1-D: the confidence of the positive class of a binary problem."""
    y_true = np.asarray(y_true).reshape(-1)
    c = np.asarray(y_conf, dtype=np.float64)
    if c.ndim > 1:
        pred, conf = np.argmax(c, axis=1), np.max(c, axis=1)
    else:
        pred, conf = (c > 0.5).astype(int), c
    hit = (pred == y_true).astype(np.float64)
    edges = _ev.bin_edges(n_bins)
    total = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        m = (conf > lo) & (conf <= hi)
        cnt = int(m.sum())
        if cnt > 0:
            total += abs(conf[m].sum() / cnt - hit[m].sum() / cnt) * (cnt / len(conf))
    return float(total)


def fps(model: torch.nn.Module, input_size: Tuple[int, int, int, int], device: torch.device, n: int = 100) -> float:
    """Images per second of ``n`` forwards on one random input of ``input_size`` after 10 warm-up forwards (metrics.py:63-93)."""
    device = torch.device(device)
    model.eval()
    x = torch.randn(input_size).to(device)
    sync = torch.cuda.synchronize if device.type == 'cuda' else (lambda: None)
    with torch.no_grad():
        for _ in range(10):
            model(x)
        sync()
        t0 = time.time()
        for _ in range(n):
            model(x)
        sync()
    return n * input_size[0] / (time.time() - t0)


def count_params(model: torch.nn.Module) -> int:
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def compute_confusion_matrix(y_true: np.ndarray, y_pred: np.ndarray, class_names: Sequence[str]) -> np.ndarray:
    return _confusion(y_true, y_pred, labels=range(len(class_names)))


def per_class_metrics(y_true: np.ndarray, y_pred: np.ndarray, class_names: Sequence[str]) -> dict:
    prec, rec, f1, support = _ev.prf_from_confusion(compute_confusion_matrix(y_true, y_pred, class_names))
    return {name: {'precision': float(prec[i]) * 100, 'recall': float(rec[i]) * 100, 'f1': float(f1[i]) * 100, 'support': int(support[i])}
            for i, name in enumerate(class_names)}
