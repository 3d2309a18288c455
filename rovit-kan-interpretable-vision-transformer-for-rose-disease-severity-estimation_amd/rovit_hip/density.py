"""Feature-space density: Mahalanobis and relative-Mahalanobis OOD scores of the backbone features, and AUROC / AUPR / FPR@TPR.

Every score of the evaluation card (``max p``, entropy, sigma, MC-dropout spread) reads what the HEADS say about the 192 backbone
features.  None can answer whether an image is anything like the training images.  The standard answer needs ``outputs['features']``
alone: the squared distance of a feature row from class-conditional Gaussians with a tied covariance (Lee et al., NeurIPS 2018), its
"relative" form that subtracts the distance under one class-agnostic Gaussian (Ren et al. 2021), reported as every OOD paper reports
it: AUROC, AUPR and FPR at 95 % TPR of in-distribution against out-of-distribution scores.  The reference has none of it.

Definitions (fp64 on the host unless said otherwise), for the valid rows f_i with labels y_i in [0, C):
  mu_c, mu       class means and the mean of all valid rows
  S_w            sum_i (f_i - mu32_{y_i})(f_i - mu32_{y_i})^T, mu32 the class mean rounded to fp32 (what the device subtracts)
  S_t            S_w + sum_c n_c (mu_c - mu)(mu_c - mu)^T                                 (host; never computed on the device)
  Sigma          (1 - a) S_w / (n_valid - C) + a tr(S_w / (n_valid - C)) / E I,  a = shrinkage      ("parity unpinned": this rule is
  Sigma0         the same from S_t / (n_valid - 1)                                                  this repository's own)
  W = L^-1, Sigma = L L^T (Cholesky);  M_c = W mu_c;  W0, m0 likewise from Sigma0 and mu.  The four tables go to the device as fp32.
  d_c(f) = ||W f - M_c||^2 = (f - mu_c)^T Sigma^-1 (f - mu_c);  d0(f) = ||W0 f - m0||^2
  mahalanobis = min_c d_c, nearest_class = argmin (lowest index), relative_mahalanobis = min_c (d_c - d0)
  energy = -logsumexp(cls_logits), max_prob_score = 1 - max softmax(cls_logits)

Why shrinkage: the final LayerNorm with a near-uniform gamma puts the features close to a 191-dimensional affine subspace, so S_w is
singular to working precision.  Why fp32 and not bf16: W amplifies operand error by sqrt(cond(Sigma)) (about 80 at shrinkage 1e-3).

``FeatureDensity.update`` copies rows to a row offset the host knows (no synchronisation); ``fit`` launches ``rovit_density_moments``
(csrc/density.hip) and makes ONE device-to-host copy; ``score`` is one launch.  ``ood_metrics`` is one call of ``rovit_ood_metrics`` and one
copy.  On CPU tensors the same entry points run the numpy fp64 statements below (``density_reference``, ``score_reference``,
``ood_metrics_reference``), the kernels' oracle, as every other accumulator here does: the host logic is testable without a GPU.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import native
from .native import RovitHipError

TABLE_KEYS = ('whitening', 'class_means', 'background_whitening', 'background_mean')
STAT_KEYS = ('counts', 'class_means', 'mean', 'scatter_within', 'scatter_total', 'covariance', 'background_covariance')


def _np(t, dtype=None) -> np.ndarray:
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dtype is None else a.astype(dtype, copy=False)


def check_shape(E: int, C: int) -> None:
    if not (isinstance(E, int) and 32 <= E <= 256 and E % 32 == 0):
        raise RovitHipError(f'FeatureDensity: embed_dim must be a multiple of 32 in 32..256, got {E!r}')
    if not (isinstance(C, int) and 2 <= C <= native.EVAL_MAX_CLASSES):
        raise RovitHipError(f'FeatureDensity: num_classes must be in 2..{native.EVAL_MAX_CLASSES}, got {C!r}')


# ---- host statements (fp64) ----------------------------------------------------------------------------------------------------------

def moments_block_from_arrays(features, labels, num_classes: int) -> np.ndarray:
    """The result block of ``rovit_density_moments`` (include/rovit_hip.h) as int64 words, the fp64 part bit for bit, from (n, E) rows
    and (n,) labels on the host: sums over whole arrays in fp64, so the block cannot depend on how the rows arrived."""
    x32 = _np(features, np.float32)
    y = _np(labels).astype(np.int64).reshape(-1)
    if x32.ndim != 2 or y.shape[0] != x32.shape[0] or x32.shape[0] < 1:
        raise RovitHipError(f'density: features must be (n >= 1, E) with n labels, got {x32.shape} and {y.shape}')
    n, E = x32.shape
    C = num_classes
    check_shape(E, C)
    o = native.density_offsets(E, C)
    blk = np.zeros(o['words'], dtype=np.int64)
    f = blk.view(np.float64)
    in_range = (y >= 0) & (y < C)
    finite = np.isfinite(x32).all(axis=1)
    valid = in_range & finite
    blk[native.DENSITY_N], blk[native.DENSITY_N_VALID] = n, int(valid.sum())
    blk[native.DENSITY_BAD_LABELS], blk[native.DENSITY_BAD_ROWS] = int((~in_range).sum()), int((in_range & ~finite).sum())
    x = x32.astype(np.float64)
    means = np.zeros((C, E))
    S = np.zeros((E, E))
    for c in range(C):
        rows = x[valid & (y == c)]
        blk[native.DENSITY_COUNTS + c] = rows.shape[0]
        if rows.shape[0]:
            means[c] = rows.sum(axis=0) / rows.shape[0]
            d = rows - means[c].astype(np.float32).astype(np.float64)
            S += d.T @ d
    f[o['means']:o['mean']] = means.reshape(-1)
    f[o['mean']:o['scatter']] = x[valid].sum(axis=0) / max(int(valid.sum()), 1) if valid.any() else 0.0
    f[o['scatter']:] = (0.5 * (S + S.T)).reshape(-1)
    return blk


def stats_from_block(blk: np.ndarray, E: int, C: int) -> Dict:
    """The block's words by name: ``n``, ``n_valid``, ``bad_labels``, ``bad_rows`` (ints), ``counts`` (C,) int64, ``class_means`` (C, E),
    ``mean`` (E,), ``scatter_within`` (E, E), and the host's ``scatter_total`` = S_w + sum_c n_c (mu_c - mu)(mu_c - mu)^T."""
    blk = np.asarray(blk, dtype=np.int64)
    o = native.density_offsets(E, C)
    f = blk.view(np.float64)
    counts = blk[native.DENSITY_COUNTS:native.DENSITY_COUNTS + C].copy()
    means = f[o['means']:o['mean']].reshape(C, E).copy()
    mean = f[o['mean']:o['scatter']].copy()
    Sw = f[o['scatter']:o['words']].reshape(E, E).copy()
    dm = means - mean[None]
    St = Sw + (dm * counts[:, None].astype(np.float64)).T @ dm
    return {'n': int(blk[native.DENSITY_N]), 'n_valid': int(blk[native.DENSITY_N_VALID]), 'bad_labels': int(blk[native.DENSITY_BAD_LABELS]),
            'bad_rows': int(blk[native.DENSITY_BAD_ROWS]), 'counts': counts, 'class_means': means, 'mean': mean, 'scatter_within': Sw,
            'scatter_total': 0.5 * (St + St.T)}


def check_stats(s: Dict, C: int) -> None:
    """The refusals of ``fit``: after the copy, naming the counts."""
    head = f"n = {s['n']}, n_valid = {s['n_valid']}, bad_labels = {s['bad_labels']}, bad_rows = {s['bad_rows']}, counts = {s['counts'].tolist()}"
    if s['bad_rows'] > 0:
        raise RovitHipError(f'FeatureDensity.fit: {s["bad_rows"]} rows hold a non-finite feature ({head})')
    if (s['counts'] < 1).any():
        raise RovitHipError(f'FeatureDensity.fit: a class has no valid row ({head})')
    if s['n_valid'] <= C:
        raise RovitHipError(f'FeatureDensity.fit: n_valid must exceed the {C} classes ({head})')


def shrunk_covariance(scatter: np.ndarray, dof: int, shrinkage: float) -> np.ndarray:
    cov = np.asarray(scatter, dtype=np.float64) / dof
    E = cov.shape[0]
    return (1.0 - shrinkage) * cov + shrinkage * (np.trace(cov) / E) * np.eye(E)


def whitening_of(cov: np.ndarray) -> np.ndarray:
    """W = L^-1 with cov = L L^T, lower-triangular (the upper triangle exactly zero)."""
    try:
        L = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError as e:
        raise RovitHipError(f'FeatureDensity.fit: the covariance is not positive definite ({e}); raise the shrinkage') from None
    return np.tril(np.linalg.solve(L, np.eye(cov.shape[0])))


def tables_from_stats(s: Dict, shrinkage: float) -> Dict:
    """Covariances, condition number and the four tables (fp64 here; ``FeatureDensity`` uploads them as fp32) from ``stats_from_block``."""
    C = s['class_means'].shape[0]
    cov = shrunk_covariance(s['scatter_within'], s['n_valid'] - C, shrinkage)
    cov0 = shrunk_covariance(s['scatter_total'], s['n_valid'] - 1, shrinkage)
    W, W0 = whitening_of(cov), whitening_of(cov0)
    ev = np.linalg.eigvalsh(cov)
    return {'covariance': cov, 'background_covariance': cov0, 'condition_number': float(ev[-1] / ev[0]),
            'whitening': W, 'class_means': s['class_means'] @ W.T, 'background_whitening': W0, 'background_mean': W0 @ s['mean']}


def density_reference(features, labels, num_classes: int, shrinkage: float = 1e-3) -> Dict:
    """The whole fit in numpy fp64: the statistics of ``stats_from_block``, then ``covariance``, ``background_covariance``,
    ``condition_number`` and ``tables`` (the four fp32 tables ``score_reference`` and the score kernel read).  Raises as ``fit`` does."""
    x = _np(features, np.float32)
    s = stats_from_block(moments_block_from_arrays(x, labels, num_classes), x.shape[1], num_classes)
    check_stats(s, num_classes)
    t = tables_from_stats(s, shrinkage)
    s.update({k: t[k] for k in ('covariance', 'background_covariance', 'condition_number')})
    s['tables'] = {k: t[k].astype(np.float32) for k in TABLE_KEYS}
    return s


def score_reference(features, tables: Dict, logits=None) -> Dict[str, np.ndarray]:
    """The score kernel's outputs in fp64 from fp32 feature rows and the fp32 tables AS GIVEN (so a test against the kernel never
    involves the host's Cholesky): ``class_distances`` (B, C), ``background_distance``, ``mahalanobis``, ``nearest_class`` (int64),
    ``relative_mahalanobis``, and with ``logits`` ``energy`` and ``max_prob_score`` (-(m + log1p(r)) and r / (1 + r) with m the first
    maximum and r the sum of exp(l - m) over the other classes)."""
    f = _np(features, np.float32).astype(np.float64)
    W, M, W0, m0 = (_np(tables[k], np.float32).astype(np.float64) for k in TABLE_KEYS)
    z, z0 = f @ W.T, f @ W0.T
    d = ((z[:, None, :] - M[None]) ** 2).sum(-1)
    d0 = ((z0 - m0[None]) ** 2).sum(-1)
    out = {'class_distances': d, 'background_distance': d0, 'mahalanobis': d.min(1), 'nearest_class': d.argmin(1).astype(np.int64),
           'relative_mahalanobis': (d - d0[:, None]).min(1)}
    if logits is not None:
        l = _np(logits, np.float32).astype(np.float64)
        am = l.argmax(1)
        m = l[np.arange(l.shape[0]), am]
        e = np.exp(l - m[:, None])
        e[np.arange(l.shape[0]), am] = 0.0
        r = e.sum(1)
        out['energy'] = -(m + np.log1p(r))
        out['max_prob_score'] = r / (1.0 + r)
    return out


def tpr_ranks(tpr_levels: Sequence[float], n_in: int):
    levels = [float(v) for v in tpr_levels]
    if len(levels) > native.OOD_MAX_LEVELS or any(not (0.0 < v <= 1.0) for v in levels):
        raise RovitHipError(f'ood_metrics: at most {native.OOD_MAX_LEVELS} TPR levels, each in (0, 1], got {tpr_levels!r}')
    return levels, [min(max(int(math.ceil(v * n_in)), 1), n_in) for v in levels]


def ood_block_reference(scores_in, scores_out, tpr_levels: Sequence[float] = (0.95,)) -> np.ndarray:
    """The result block of ``rovit_ood_metrics`` on the host, by counting on sorted copies (fp32 compares, fp64 terms)."""
    a, b = _np(scores_in, np.float32).reshape(-1), _np(scores_out, np.float32).reshape(-1)
    n_in, n_out = a.shape[0], b.shape[0]
    if n_in < 1 or n_out < 1 or n_in + n_out > native.EVAL_MAX_ROWS:
        raise RovitHipError(f'ood_metrics: {n_in} + {n_out} scores (each >= 1, together at most {native.EVAL_MAX_ROWS})')
    levels, ks = tpr_ranks(tpr_levels, n_in)
    blk = np.zeros(native.OOD_WORDS, dtype=np.int64)
    f = blk.view(np.float64)
    blk[native.OOD_N_IN], blk[native.OOD_N_OUT] = n_in, n_out
    blk[native.OOD_BAD] = int((~np.isfinite(a)).sum() + (~np.isfinite(b)).sum())
    for l, k in enumerate(ks):
        blk[native.OOD_K + l] = k
    if blk[native.OOD_BAD]:
        return blk
    sa, sb = np.sort(a), np.sort(b)
    less_in_b, le_in_b = np.searchsorted(sa, b, 'left').astype(np.int64), np.searchsorted(sa, b, 'right').astype(np.int64)
    blk[native.OOD_TWO_U] = int((less_in_b + le_in_b).sum())                  # 2 less + eq
    ge_out, ge_in = n_out - np.searchsorted(sb, b, 'left').astype(np.int64), n_in - less_in_b
    f[native.OOD_AP_OUT_SUM] = float((ge_out / (ge_out + ge_in).astype(np.float64)).sum())
    le_in, le_out = np.searchsorted(sa, a, 'right').astype(np.int64), np.searchsorted(sb, a, 'right').astype(np.int64)
    f[native.OOD_AP_IN_SUM] = float((le_in / (le_in + le_out).astype(np.float64)).sum())
    for l, k in enumerate(ks):
        t = sa[k - 1]
        f[native.OOD_THRESHOLD + l] = float(t) + 0.0                              # -0 is written as +0
        blk[native.OOD_OUT_BELOW + l] = int(np.searchsorted(sb, t, 'right'))
    return blk


def ood_from_block(blk: np.ndarray, tpr_levels: Sequence[float]) -> Dict:
    blk = np.asarray(blk, dtype=np.int64)
    f = blk.view(np.float64)
    n_in, n_out, bad = int(blk[native.OOD_N_IN]), int(blk[native.OOD_N_OUT]), int(blk[native.OOD_BAD])
    if bad:
        raise RovitHipError(f'ood_metrics: {bad} non-finite scores among {n_in} + {n_out}')
    levels = [float(v) for v in tpr_levels]
    return {'auroc': int(blk[native.OOD_TWO_U]) / (2.0 * n_in * n_out), 'aupr_out': float(f[native.OOD_AP_OUT_SUM]) / n_out,
            'aupr_in': float(f[native.OOD_AP_IN_SUM]) / n_in,
            'fpr_at_tpr': {v: int(blk[native.OOD_OUT_BELOW + l]) / n_out for l, v in enumerate(levels)},
            'thresholds': {v: float(f[native.OOD_THRESHOLD + l]) for l, v in enumerate(levels)}, 'n_in': n_in, 'n_out': n_out}


def ood_metrics_reference(scores_in, scores_out, tpr_levels: Sequence[float] = (0.95,)) -> Dict:
    """``ood_metrics`` in numpy: see there."""
    return ood_from_block(ood_block_reference(scores_in, scores_out, tpr_levels), tpr_levels)


# ---- device entry points -------------------------------------------------------------------------------------------------------------

def ood_block(scores_in: torch.Tensor, scores_out: torch.Tensor, tpr_levels: Sequence[float] = (0.95,), max_workgroups: int = 0,
              rank: str = 'auto') -> np.ndarray:
    """``rovit_ood_metrics``' result block as int64 words on the host (one launch sequence, one device-to-host copy); CPU tensors run
    ``ood_block_reference``.  ``rank``: ``'count'``, ``'sort'`` or ``'auto'`` (by n_in + n_out), how the ranks are found; the block
    does not depend on it."""
    if rank not in native.RANK_METHODS:
        raise RovitHipError(f"ood_metrics: rank must be one of {sorted(native.RANK_METHODS)}, got {rank!r}")
    if not scores_in.is_cuda:
        return ood_block_reference(scores_in, scores_out, tpr_levels)
    a, b = scores_in.detach().float().reshape(-1).contiguous(), scores_out.detach().float().reshape(-1).contiguous()
    if b.device != a.device:
        raise RovitHipError(f'ood_metrics: scores on {a.device} and {b.device}')
    n_in, n_out = a.shape[0], b.shape[0]
    if n_in < 1 or n_out < 1 or n_in + n_out > native.EVAL_MAX_ROWS:
        raise RovitHipError(f'ood_metrics: {n_in} + {n_out} scores (each >= 1, together at most {native.EVAL_MAX_ROWS})')
    levels, _ = tpr_ranks(tpr_levels, n_in)
    lib = native.load()
    nbytes = lib.rovit_ood_metrics_workspace_bytes(n_in, n_out)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    result = torch.empty(native.OOD_WORDS, dtype=torch.int64, device=a.device)
    d = native.Ood()
    d.n_in, d.n_out, d.num_levels, d.max_workgroups = n_in, n_out, len(levels), max_workgroups
    for l, v in enumerate(levels):
        d.tpr_levels[l] = v
    d.scores_in, d.scores_out, d.workspace, d.workspace_bytes, d.result = native.ptr(a), native.ptr(b), native.ptr(ws), nbytes, native.ptr(result)
    method = native.rank_method(rank, n_in + n_out, 'ood_metrics')
    rank_bytes = lib.rovit_ood_metrics_rank_workspace_bytes(n_in, n_out) if method == native.RANK_SORT else 0
    rank_ws = torch.empty(rank_bytes, dtype=torch.uint8, device=a.device) if rank_bytes else None
    native.call('rovit_ood_metrics_ex', ctypes.byref(d), method, native.ptr(rank_ws), rank_bytes, native.stream_ptr())
    return result.cpu().numpy()                                   # the single device-to-host copy


def ood_metrics(scores_in: torch.Tensor, scores_out: torch.Tensor, tpr_levels: Sequence[float] = (0.95,), rank: str = 'auto') -> Dict:
    """How well a score separates out-of-distribution rows (higher = more anomalous, the positives) from in-distribution rows:
    ``auroc`` = P(out > in) + P(out == in) / 2 exactly (a ratio of integers); ``aupr_out`` / ``aupr_in``: average precision with the
    out / the in rows as the positives, tied scores entering a threshold together; ``fpr_at_tpr[level]``: the share of out rows at or
    below ``thresholds[level]``, the ceil(level n_in)-th smallest in-distribution score (the detector that flags scores ABOVE it keeps
    that share of the in rows); ``n_in``, ``n_out``.  Non-finite scores raise, after the copy.  ``rank``: see ``ood_block``."""
    return ood_from_block(ood_block(scores_in, scores_out, tpr_levels, rank=rank), tpr_levels)


class FeatureDensity:
    """Class-conditional Gaussian density of feature rows with a tied, shrunk covariance; see the module docstring.  ``update`` never
    synchronises; ``fit`` copies one block to the host; ``score`` is one launch."""

    def __init__(self, num_classes: int, embed_dim: int = 192, shrinkage: float = 1e-3, capacity: int = 4096):
        check_shape(embed_dim, num_classes)
        if not (isinstance(shrinkage, (int, float)) and 0.0 <= float(shrinkage) <= 1.0):
            raise RovitHipError(f'FeatureDensity: shrinkage must be in [0, 1], got {shrinkage!r}')
        if not (isinstance(capacity, int) and 1 <= capacity <= native.KAN_STATS_MAX_ROWS):
            raise RovitHipError(f'FeatureDensity: capacity must be in 1..{native.KAN_STATS_MAX_ROWS}, got {capacity!r}')
        self.num_classes, self.embed_dim, self.shrinkage, self._capacity0 = num_classes, embed_dim, float(shrinkage), capacity
        self.max_workgroups = 0                                    # > 0 caps every grid (tests); the results do not depend on it
        self.reset()

    def reset(self) -> None:
        self.n = 0
        self.device: Optional[torch.device] = None
        self._rows: Optional[torch.Tensor] = None
        self._labels: Optional[torch.Tensor] = None
        self._cpu = []
        self._clear_fit()

    def _clear_fit(self) -> None:
        self._block: Optional[np.ndarray] = None
        self.tables: Optional[Dict[str, torch.Tensor]] = None
        self._tables_on: Dict[torch.device, Dict[str, torch.Tensor]] = {}
        self.n_valid = self.bad_labels = 0
        self.counts = self.class_means = self.mean = self.scatter_within = self.scatter_total = None
        self.covariance = self.background_covariance = self.condition_number = None

    @property
    def fitted(self) -> bool:
        return self.tables is not None

    def _reserve(self, rows: int) -> None:
        cap = self._rows.shape[0] if self._rows is not None else 0
        if rows <= cap:
            return
        if rows > native.KAN_STATS_MAX_ROWS:
            raise RovitHipError(f'FeatureDensity: {rows} rows exceed the limit of {native.KAN_STATS_MAX_ROWS}')
        new_cap = min(native.KAN_STATS_MAX_ROWS, max(rows, 2 * cap, self._capacity0))
        new = torch.empty((new_cap, self.embed_dim), dtype=torch.float32, device=self.device)
        lab = torch.empty(new_cap, dtype=torch.int32, device=self.device)
        if self._rows is not None:
            new[:self.n].copy_(self._rows[:self.n])                # device-to-device, stream-ordered: no synchronisation
            lab[:self.n].copy_(self._labels[:self.n])
        self._rows, self._labels = new, lab

    def update(self, features: torch.Tensor, class_labels: torch.Tensor) -> None:
        """Record a batch of (B, E) feature rows with their (B,) integer class labels."""
        x, y = features.detach(), class_labels.detach().reshape(-1)
        if x.dim() != 2 or x.shape[1] != self.embed_dim or x.shape[0] < 1 or y.shape[0] != x.shape[0]:
            raise RovitHipError(f'FeatureDensity.update: features must be (B >= 1, {self.embed_dim}) with B labels, got {tuple(x.shape)} '
                                f'and {tuple(class_labels.shape)}')
        if y.is_floating_point() or y.dtype == torch.bool:
            raise RovitHipError(f'FeatureDensity.update: class labels must be integers, got {y.dtype}')
        if self.device is None:
            self.device = x.device
        elif x.device != self.device:
            raise RovitHipError(f'FeatureDensity.update: batch on {x.device}, earlier batches on {self.device}; reset() first')
        self._clear_fit()
        B = x.shape[0]
        if not x.is_cuda:
            self._cpu.append((x.float().clone(), y.cpu().to(torch.int64).clone()))
        else:
            self._reserve(self.n + B)
            self._rows[self.n:self.n + B].copy_(x)
            self._labels[self.n:self.n + B].copy_(y, non_blocking=True)          # converts to int32; a host tensor is copied up
        self.n += B

    def result_block(self) -> np.ndarray:
        """``rovit_density_moments``' block as int64 words on the host (fp64 part bit for bit).  On the device this is the one
        synchronising call; the block is kept until the next ``update`` or ``reset``."""
        if self._block is not None:
            return self._block
        if self.n < 1:
            raise RovitHipError('FeatureDensity: nothing recorded yet')
        E, C = self.embed_dim, self.num_classes
        if self.device.type != 'cuda':
            self._block = moments_block_from_arrays(torch.cat([b[0] for b in self._cpu]).numpy(), torch.cat([b[1] for b in self._cpu]).numpy(), C)
            return self._block
        lib = native.load()
        nbytes = lib.rovit_density_workspace_bytes(self.n, E, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        result = torch.empty(native.density_offsets(E, C)['words'], dtype=torch.int64, device=self.device)
        d = native.DensityFit()
        d.n, d.embed, d.num_classes, d.max_workgroups = self.n, E, C, self.max_workgroups
        d.features, d.labels = native.ptr(self._rows), native.ptr(self._labels)
        d.workspace, d.workspace_bytes, d.result = native.ptr(ws), nbytes, native.ptr(result)
        native.call('rovit_density_moments', ctypes.byref(d), native.stream_ptr())
        self._block = result.cpu().numpy()                        # the single device-to-host copy
        return self._block

    def fit(self) -> 'FeatureDensity':
        """Moments on the device, one copy, then covariance, Cholesky and the four tables on the host in fp64; the tables are uploaded as
        fp32.  Raises ``RovitHipError`` after the copy, naming the counts, when a class has no valid row, when n_valid <= C or when a
        recorded row holds a non-finite feature.  Rows with a label outside [0, C) are left out and counted in ``bad_labels``."""
        blk = self.result_block()
        s = stats_from_block(blk, self.embed_dim, self.num_classes)
        check_stats(s, self.num_classes)
        t = tables_from_stats(s, self.shrinkage)
        self.n_valid, self.bad_labels = s['n_valid'], s['bad_labels']
        for k in ('counts', 'class_means', 'mean', 'scatter_within', 'scatter_total'):
            setattr(self, k, s[k])
        self.covariance, self.background_covariance, self.condition_number = t['covariance'], t['background_covariance'], t['condition_number']
        self.tables = {k: torch.from_numpy(t[k].astype(np.float32)).contiguous().to(self.device) for k in TABLE_KEYS}
        self._tables_on = {}
        return self

    def _tables_for(self, device: torch.device) -> Dict[str, torch.Tensor]:
        if self.tables is None:
            raise RovitHipError('FeatureDensity.score: fit() (or load_state_dict) first')
        if self.tables['whitening'].device == device:
            return self.tables
        if device not in self._tables_on:
            self._tables_on[device] = {k: v.to(device) for k, v in self.tables.items()}
        return self._tables_on[device]

    def score(self, features: torch.Tensor, cls_logits: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Per row of (B, E) features: ``class_distances`` (B, C), ``background_distance``, ``mahalanobis``, ``nearest_class`` (int32),
        ``relative_mahalanobis``, and with ``cls_logits`` (B, C) also ``energy`` and ``max_prob_score``; tensors on the features' device
        from one launch, nothing copied to the host."""
        x = features.detach()
        E, C = self.embed_dim, self.num_classes
        if x.dim() != 2 or x.shape[1] != E or x.shape[0] < 1:
            raise RovitHipError(f'FeatureDensity.score: features must be (B >= 1, {E}), got {tuple(x.shape)}')
        if cls_logits is not None and (tuple(cls_logits.shape) != (x.shape[0], C) or cls_logits.device != x.device):
            raise RovitHipError(f'FeatureDensity.score: cls_logits must be ({x.shape[0]}, {C}) on {x.device}, got {tuple(cls_logits.shape)} on '
                                f'{cls_logits.device}')
        t = self._tables_for(x.device)
        B = x.shape[0]
        if not x.is_cuda:
            ref = score_reference(x.float().numpy(), t, None if cls_logits is None else cls_logits.detach().float().numpy())
            return {k: torch.from_numpy(v.astype(np.int32 if k == 'nearest_class' else np.float32)) for k, v in ref.items()}
        x = x.float().contiguous()
        lg = None if cls_logits is None else cls_logits.detach().float().contiguous()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        out = {'class_distances': f32(B, C), 'background_distance': f32(B), 'mahalanobis': f32(B),
               'nearest_class': torch.empty(B, dtype=torch.int32, device=x.device), 'relative_mahalanobis': f32(B)}
        if lg is not None:
            out['energy'], out['max_prob_score'] = f32(B), f32(B)
        d = native.DensityScores()
        d.batch, d.embed, d.num_classes, d.max_workgroups = B, E, C, self.max_workgroups
        d.features, d.cls_logits = native.ptr(x), native.ptr(lg)
        d.whitening, d.class_means, d.background_whitening, d.background_mean = (native.ptr(t[k]) for k in TABLE_KEYS)
        for k, v in out.items():
            setattr(d, k, native.ptr(v))
        native.call('rovit_density_score', ctypes.byref(d), native.stream_ptr())
        return out

    def state_dict(self) -> Dict:
        """The fit as tensors and plain numbers (``torch.save`` takes it): the four fp32 tables and the fp64 statistics."""
        if self.tables is None:
            raise RovitHipError('FeatureDensity.state_dict: fit() first')
        sd = {'num_classes': self.num_classes, 'embed_dim': self.embed_dim, 'shrinkage': self.shrinkage, 'n': self.n, 'n_valid': self.n_valid,
              'bad_labels': self.bad_labels, 'condition_number': self.condition_number}
        sd.update({f'tables.{k}': v.detach().cpu().clone() for k, v in self.tables.items()})
        sd.update({f'stats.{k}': torch.from_numpy(np.array(getattr(self, k))) for k in STAT_KEYS})
        return sd

    def load_state_dict(self, sd: Dict, device=None) -> 'FeatureDensity':
        """Restore a fit (not the recorded rows): ``score`` works at once, on ``device`` (default: where the tables were saved from, the
        CPU) or wherever the features are."""
        if (sd['num_classes'], sd['embed_dim']) != (self.num_classes, self.embed_dim):
            raise RovitHipError(f"FeatureDensity.load_state_dict: the state holds {sd['num_classes']} classes of {sd['embed_dim']} features, "
                                f'this object {self.num_classes} of {self.embed_dim}')
        self.reset()
        self.shrinkage, self.n, self.n_valid, self.bad_labels = float(sd['shrinkage']), int(sd['n']), int(sd['n_valid']), int(sd['bad_labels'])
        self.condition_number = float(sd['condition_number'])
        for k in STAT_KEYS:
            setattr(self, k, sd[f'stats.{k}'].numpy().copy())
        self.tables = {k: sd[f'tables.{k}'].to(torch.float32).contiguous().to(device or 'cpu') for k in TABLE_KEYS}
        return self


def fit_model_density(model, x_or_loader, labels=None, shrinkage: float = 1e-3, chunk: int = 256) -> FeatureDensity:
    """``FeatureDensity`` of the model's own backbone features in eval mode under no_grad, ``chunk`` images at a time: an image tensor
    with ``labels``, or an iterable of batches ``(images, class_labels, ...)`` (host batches of a loader are copied to the model's device)."""
    if not (isinstance(chunk, int) and chunk >= 1):
        raise RovitHipError(f'fit_feature_density: chunk must be a positive integer, got {chunk!r}')
    is_tensor = isinstance(x_or_loader, torch.Tensor)
    if is_tensor and labels is None:
        raise RovitHipError('fit_feature_density: an image tensor needs labels')
    dev = next(model.parameters()).device
    fd = FeatureDensity(model.classification_head.fc2.out_features, model.backbone.embed_dim, shrinkage)
    batches = [(x_or_loader, labels)] if is_tensor else x_or_loader
    was_training = model.backbone.training
    model.backbone.eval()
    try:
        with torch.no_grad():
            for batch in batches:
                images, y = batch[0], batch[1]
                if is_tensor:
                    native.ptr(images)                              # a CPU tensor raises: the backbone has no CPU path
                else:
                    images = images.to(dev, non_blocking=True)
                for r0 in range(0, images.shape[0], chunk):
                    fd.update(model.backbone(images[r0:r0 + chunk]), y[r0:r0 + chunk])
    finally:
        model.backbone.train(was_training)
    return fd.fit()
