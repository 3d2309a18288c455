"""Nearest neighbours in feature space: a fused kNN search over recorded backbone features, the kNN out-of-distribution score and the
neighbour-weighted vote.

The uncertainty tool kit built on ``outputs['features']`` is parametric: one tied Gaussian per class (``rovit_hip.density``), one
temperature, one quantile.  Three things users of a vision backbone expect are the same non-parametric operation, the k nearest
recorded rows of a query row: explanation by example ("which training leaves does this one look like, and what were their labels and
severities?"), the distance to the k-th nearest training feature as an OOD score (Sun et al., ICML 2022), and the weighted kNN
classifier that reads the backbone with no head at all (Wu et al. 2018; the DINO evaluation protocol).  The recipe ``q @ r.T`` +
``torch.topk`` materialises a (B, N) matrix, has no tie rule and changes its bits with the chunking; ``csrc/neighbors.hip`` keeps no
such matrix and returns the same bits for every grid, split and batch split.

Definitions.  Reference rows r_j, j in [0, N), and query rows q_i are fp32.
  metric 'l2'      d(q, r) = max(0, (|q|^2 + |r|^2) - 2 q.r)
  metric 'cosine'  d(q, r) = max(0, 1 - q^.r^), x^ = x / sqrt(|x|^2); the reference rows are normalised once in ``build``, the query
                   rows when they are staged.  (The max only removes a rounding excess of q^.r^ over 1: the key below needs d >= 0.)
  On the device every term is fp32, q.r and the squared norms are fma chains in ascending feature index, and the operations run in
  exactly the order written: d is a function of the two rows alone, not of the tile, wave, workgroup or split that computes it.
  Bad rows: a reference row with a non-finite feature (or a squared norm that is not finite in fp32; with 'cosine' also a zero one) can
  never be a neighbour and is counted in ``bad_rows`` by ``build``, on the device.  A query row that is bad in the same sense returns
  index -1 and distance +inf in every slot.  Fewer valid references than k: the remaining slots are index -1 and distance +inf.  On
  the device a pair whose fp32 distance is not finite ('l2' with |q|^2 + |r|^2 or 2 q.r above the fp32 range, about 1.7e38) is no
  candidate; the fp64 statements below have no such limit, so they are the oracle for squared norms below 1.7e38 only.
  Order: the 64-bit key (bits(d) << 32) | j.  d >= 0, so the fp32 bits order as unsigned integers; keys of distinct references are
  distinct; the k smallest keys are the answer, ascending: ties in distance go to the lower index.
  ``exclude`` (B,) int32: per query one reference index that is left out; ``arange(N)`` makes a search of the index against itself
  leave-one-out.  1 <= k <= KNN_MAX_K = 32.
  Vote over the valid slots of a query, in fp64 in slot order: w_j = exp(-(d_j - d_1) / temperature) (with 'cosine' the DINO weight
  exp(sim / T) up to a factor that cancels); class_probs[c] = sum w_j [y_j = c] / sum w_j (labels outside [0, C) carry no vote); class
  = the first argmax of the fp64 sums (-1 without a valid slot); severity = sum w_j s_j / sum w_j; kth_distance = the distance in the
  last valid slot, the OOD score; mean_distance = the mean over the valid slots (both +inf without one).

``FeatureIndex.update`` copies rows to a row offset the host knows (no synchronisation); ``build`` is one launch; ``counts`` the one
device-to-host copy; ``search`` returns device tensors with nothing copied to the host.  On CPU tensors the same entry points run the
numpy statements below (``build_reference``, ``search_reference``, ``vote_reference``: fp64 distances from the fp32 rows, the same key
order, the same vote), the kernels' oracle: the host logic is testable without a GPU.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import native
from .native import RovitHipError

METRICS = {'l2': native.KNN_L2, 'cosine': native.KNN_COSINE}
DEFAULT_TEMPERATURE = 0.07


def _np(t, dtype=None) -> np.ndarray:
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dtype is None else a.astype(dtype, copy=False)


def check_shape(E, num_classes, metric) -> None:
    if not (isinstance(E, int) and 32 <= E <= 256 and E % 32 == 0):
        raise RovitHipError(f'FeatureIndex: embed_dim must be a multiple of 32 in 32..256, got {E!r}')
    if num_classes is not None and not (isinstance(num_classes, int) and 1 <= num_classes <= native.KNN_MAX_CLASSES):
        raise RovitHipError(f'FeatureIndex: num_classes must be None or in 1..{native.KNN_MAX_CLASSES}, got {num_classes!r}')
    if metric not in METRICS:
        raise RovitHipError(f'FeatureIndex: metric must be one of {sorted(METRICS)}, got {metric!r}')


def check_k(k, temperature) -> None:
    if not (isinstance(k, int) and 1 <= k <= native.KNN_MAX_K):
        raise RovitHipError(f'FeatureIndex.search: k must be in 1..{native.KNN_MAX_K}, got {k!r}')
    if not (isinstance(temperature, (int, float)) and 0.0 < float(temperature) < float('inf')):
        raise RovitHipError(f'FeatureIndex.search: temperature must be positive, got {temperature!r}')


# ---- host statements -------------------------------------------------------------------------------------------------------------------

def squared_norms_f32(rows: np.ndarray) -> np.ndarray:
    """|x|^2 of fp32 rows as the device forms it: one fp32 fma chain in ascending feature index (each step a product that is exact in
    fp64 plus the running sum, rounded to fp32)."""
    x = _np(rows, np.float32).astype(np.float64)
    s = np.zeros(x.shape[0], dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for e in range(x.shape[1]):
            s = (x[:, e] * x[:, e] + s.astype(np.float64)).astype(np.float32)
    return s


def valid_rows(rows: np.ndarray, metric: str) -> np.ndarray:
    x = _np(rows, np.float32)
    n2 = squared_norms_f32(x)
    ok = np.isfinite(x).all(axis=1) & np.isfinite(n2)
    return ok & (n2 > 0) if metric == 'cosine' else ok


def build_reference(features, metric: str = 'cosine') -> Dict:
    """What ``rovit_knn_build`` leaves behind, on the host: ``norms`` (fp32, the device's chain), ``valid`` (bool), the counts ``n``,
    ``n_valid``, ``bad_rows``, and with 'cosine' ``normalized``, the rows over their fp64 length (zeros for a row that is not valid)."""
    x = _np(features, np.float32)
    if x.ndim != 2 or x.shape[0] < 1:
        raise RovitHipError(f'build_reference: features must be (n >= 1, E), got {x.shape}')
    check_shape(int(x.shape[1]), None, metric)
    ok = valid_rows(x, metric)
    out = {'norms': squared_norms_f32(x), 'valid': ok, 'n': int(x.shape[0]), 'n_valid': int(ok.sum()), 'bad_rows': int((~ok).sum())}
    if metric == 'cosine':
        out['normalized'] = _unit_rows(x, ok)
    return out


def _unit_rows(x32: np.ndarray, ok: np.ndarray) -> np.ndarray:
    x = np.where(ok[:, None], x32, 0).astype(np.float64)
    length = np.sqrt((x * x).sum(axis=1))
    return x / np.where(ok, length, 1.0)[:, None]


def distance_matrix(queries, rows, metric: str) -> np.ndarray:
    """(B, N) fp64 distances of the definition from fp32 rows; +inf where the query or the reference row is bad."""
    q32, r32 = _np(queries, np.float32), _np(rows, np.float32)
    qok, rok = valid_rows(q32, metric), valid_rows(r32, metric)
    if metric == 'cosine':
        d = 1.0 - _unit_rows(q32, qok) @ _unit_rows(r32, rok).T
    else:
        q, r = np.where(qok[:, None], q32, 0).astype(np.float64), np.where(rok[:, None], r32, 0).astype(np.float64)
        d = ((q * q).sum(1)[:, None] + (r * r).sum(1)[None]) - 2.0 * (q @ r.T)
    d = np.maximum(d, 0.0)
    d[~qok] = np.inf
    d[:, ~rok] = np.inf
    return d


def vote_reference(distances, indices, labels=None, severities=None, num_classes: Optional[int] = None,
                   temperature: float = DEFAULT_TEMPERATURE) -> Dict[str, np.ndarray]:
    """The vote of the definition in fp64 from (B, k) ``distances`` and ``indices`` (slot valid iff index >= 0, valid slots first) and the
    neighbours' (B, k) ``labels`` / ``severities``: ``kth_distance``, ``mean_distance``, with labels and ``num_classes`` ``class_probs``
    and ``class`` (int64), with severities ``severity``."""
    d, idx = _np(distances).astype(np.float64), _np(indices).astype(np.int64)
    B, k = d.shape
    out = {'kth_distance': np.full(B, np.inf), 'mean_distance': np.full(B, np.inf)}
    vote = labels is not None and num_classes is not None
    if vote:
        y = _np(labels).astype(np.int64)
        out['class_probs'], out['class'] = np.zeros((B, num_classes)), np.full(B, -1, dtype=np.int64)
    if severities is not None:
        s = _np(severities).astype(np.float64)
        out['severity'] = np.full(B, np.nan)
    for i in range(B):
        nv = int((idx[i] >= 0).sum())
        if nv == 0:
            continue
        sw = ss = sd = 0.0
        cls = np.zeros(num_classes) if vote else None
        for j in range(nv):
            w = float(np.exp(-(d[i, j] - d[i, 0]) / float(temperature)))
            sw += w
            sd += d[i, j]
            if vote and 0 <= y[i, j] < num_classes:
                cls[y[i, j]] += w
            if severities is not None:
                ss += w * s[i, j]
        out['kth_distance'][i], out['mean_distance'][i] = d[i, nv - 1], sd / nv
        if vote:
            out['class'][i], out['class_probs'][i] = int(np.argmax(cls)), cls / sw
        if severities is not None:
            out['severity'][i] = ss / sw
    return out


def search_reference(queries, rows, k: int = 10, metric: str = 'cosine', exclude=None, class_labels=None, severity=None,
                     num_classes: Optional[int] = None, temperature: float = DEFAULT_TEMPERATURE, chunk: int = 512) -> Dict[str, np.ndarray]:
    """``FeatureIndex.search`` in numpy: fp64 distances from the fp32 rows, the k smallest by (distance, index) ascending per query
    (a stable sort: ties go to the lower index), ``indices`` int64 with -1 and ``distances`` +inf in the empty slots, ``labels`` (-1)
    and ``severities`` (NaN) of the neighbours when the columns are given, and ``vote_reference`` on top."""
    q32, r32 = _np(queries, np.float32), _np(rows, np.float32)
    if q32.ndim != 2 or r32.ndim != 2 or q32.shape[1] != r32.shape[1] or q32.shape[0] < 1 or r32.shape[0] < 1:
        raise RovitHipError(f'search_reference: queries (B >= 1, E) and rows (N >= 1, E), got {q32.shape} and {r32.shape}')
    check_shape(int(r32.shape[1]), num_classes, metric)
    check_k(k, temperature)
    B, N = q32.shape[0], r32.shape[0]
    ex = None if exclude is None else _np(exclude).astype(np.int64).reshape(-1)
    if ex is not None and ex.shape[0] != B:
        raise RovitHipError(f'search_reference: exclude must hold {B} indices, got {ex.shape[0]}')
    dist, idx = np.full((B, k), np.inf), np.full((B, k), -1, dtype=np.int64)
    for r0 in range(0, B, chunk):
        d = distance_matrix(q32[r0:r0 + chunk], r32, metric)
        if ex is not None:
            e = ex[r0:r0 + chunk]
            hit = np.nonzero((e >= 0) & (e < N))[0]
            d[hit, e[hit]] = np.inf
        order = np.argsort(d, axis=1, kind='stable')[:, :k]
        got = np.take_along_axis(d, order, axis=1)
        kk = order.shape[1]
        dist[r0:r0 + chunk, :kk] = got
        idx[r0:r0 + chunk, :kk] = np.where(np.isfinite(got), order, -1)
    out = {'distances': dist, 'indices': idx}
    safe = np.maximum(idx, 0)
    if class_labels is not None:
        out['labels'] = np.where(idx >= 0, _np(class_labels).astype(np.int64).reshape(-1)[safe], -1)
    if severity is not None:
        out['severities'] = np.where(idx >= 0, _np(severity).astype(np.float32).reshape(-1).astype(np.float64)[safe], np.nan)
    out.update(vote_reference(dist, idx, out.get('labels'), out.get('severities'), num_classes, temperature))
    return out


_OUT_DTYPES = {'indices': np.int32, 'labels': np.int32, 'class': np.int32}


# ---- the index -------------------------------------------------------------------------------------------------------------------------

class FeatureIndex:
    """Recorded feature rows (with optional class labels and severities) and the fused k-nearest-neighbour search over them; see the
    module docstring.  ``update`` never synchronises; ``build`` is one launch; ``counts`` the one copy; ``search`` copies nothing."""

    def __init__(self, embed_dim: int = 192, num_classes: Optional[int] = None, metric: str = 'cosine', capacity: int = 4096):
        check_shape(embed_dim, num_classes, metric)
        if not (isinstance(capacity, int) and 1 <= capacity <= native.KAN_STATS_MAX_ROWS):
            raise RovitHipError(f'FeatureIndex: capacity must be in 1..{native.KAN_STATS_MAX_ROWS}, got {capacity!r}')
        self.embed_dim, self.num_classes, self.metric, self._capacity0 = embed_dim, num_classes, metric, capacity
        self.max_workgroups = 0                                    # > 0 caps every grid (tests); the results do not depend on it
        self.reset()

    def reset(self) -> None:
        self.n = 0
        self.device: Optional[torch.device] = None
        self.has_labels: Optional[bool] = None                     # fixed by the first update
        self.has_severity: Optional[bool] = None
        self._rows = self._labels = self._severity = None
        self._clear_build()

    def _clear_build(self) -> None:
        self._norms = self._valid = self._normalized = self._result = None
        self._counts: Optional[Dict[str, int]] = None
        self._host: Optional[Dict] = None

    @property
    def built(self) -> bool:
        return self._result is not None or self._host is not None

    def _reserve(self, rows: int) -> None:
        cap = self._rows.shape[0] if self._rows is not None else 0
        if rows <= cap:
            return
        if rows > native.KAN_STATS_MAX_ROWS:
            raise RovitHipError(f'FeatureIndex: {rows} rows exceed the limit of {native.KAN_STATS_MAX_ROWS}')
        new_cap = min(native.KAN_STATS_MAX_ROWS, max(rows, 2 * cap, self._capacity0))
        grown = [torch.empty((new_cap, self.embed_dim), dtype=torch.float32, device=self.device),
                 torch.empty(new_cap, dtype=torch.int32, device=self.device) if self.has_labels else None,
                 torch.empty(new_cap, dtype=torch.float32, device=self.device) if self.has_severity else None]
        for new, old in zip(grown, (self._rows, self._labels, self._severity)):
            if new is not None and old is not None:
                new[:self.n].copy_(old[:self.n])                   # device-to-device (or host), stream-ordered: no synchronisation
        self._rows, self._labels, self._severity = grown

    def update(self, features: torch.Tensor, class_labels: Optional[torch.Tensor] = None, severity: Optional[torch.Tensor] = None) -> None:
        """Record a batch of (B, E) feature rows, with their (B,) integer class labels and (B,) or (B, 1) severities when the index
        keeps them (the first batch decides which columns exist)."""
        x = features.detach()
        if x.dim() != 2 or x.shape[1] != self.embed_dim or x.shape[0] < 1:
            raise RovitHipError(f'FeatureIndex.update: features must be (B >= 1, {self.embed_dim}), got {tuple(x.shape)}')
        B = x.shape[0]
        y = None if class_labels is None else class_labels.detach().reshape(-1)
        s = None if severity is None else severity.detach().reshape(-1)
        if y is not None and (y.shape[0] != B or y.is_floating_point() or y.dtype == torch.bool):
            raise RovitHipError(f'FeatureIndex.update: class labels must be {B} integers, got {tuple(class_labels.shape)} of {y.dtype}')
        if s is not None and s.shape[0] != B:
            raise RovitHipError(f'FeatureIndex.update: severity must hold {B} values, got {tuple(severity.shape)}')
        if self.device is None:
            self.device, self.has_labels, self.has_severity = x.device, y is not None, s is not None
        elif x.device != self.device:
            raise RovitHipError(f'FeatureIndex.update: batch on {x.device}, earlier batches on {self.device}; reset() first')
        if (y is not None) != self.has_labels or (s is not None) != self.has_severity:
            raise RovitHipError('FeatureIndex.update: every batch carries the columns of the first one (class labels: '
                                f'{self.has_labels}, severity: {self.has_severity})')
        self._clear_build()
        self._reserve(self.n + B)
        self._rows[self.n:self.n + B].copy_(x)
        if y is not None:
            self._labels[self.n:self.n + B].copy_(y, non_blocking=True)          # converts to int32; a host tensor is copied up
        if s is not None:
            self._severity[self.n:self.n + B].copy_(s, non_blocking=True)
        self.n += B

    def rows(self) -> torch.Tensor:
        """The recorded (n, E) rows, a view."""
        if self.n < 1:
            raise RovitHipError('FeatureIndex: nothing recorded yet')
        return self._rows[:self.n]

    def build(self) -> 'FeatureIndex':
        """One launch over the recorded rows: squared norms, validity flags, with 'cosine' the normalised copy, and the counts, which stay
        on the device until ``counts()``."""
        if self.n < 1:
            raise RovitHipError('FeatureIndex: nothing recorded yet')
        self._clear_build()
        if self.device.type != 'cuda':
            self._host = build_reference(self._rows[:self.n].numpy(), self.metric)
            return self
        n, E = self.n, self.embed_dim
        self._norms = torch.empty(n, dtype=torch.float32, device=self.device)
        self._valid = torch.empty(n, dtype=torch.int32, device=self.device)
        self._normalized = torch.empty((n, E), dtype=torch.float32, device=self.device) if self.metric == 'cosine' else None
        result = torch.empty(native.KNN_WORDS, dtype=torch.int64, device=self.device)
        d = native.KnnIndex()
        d.n, d.embed, d.metric, d.max_workgroups = n, E, METRICS[self.metric], self.max_workgroups
        d.features, d.norms, d.valid, d.normalized, d.result = (native.ptr(t) for t in (self._rows, self._norms, self._valid, self._normalized, result))
        native.call('rovit_knn_build', ctypes.byref(d), native.stream_ptr())
        self._result = result
        return self

    def counts(self) -> Dict[str, int]:
        """``n``, ``n_valid`` and ``bad_rows`` of the built index: the one device-to-host copy (kept until the next ``update``)."""
        if not self.built:
            self.build()
        if self._counts is None:
            if self._host is not None:
                self._counts = {k: self._host[k] for k in ('n', 'n_valid', 'bad_rows')}
            else:
                w = self._result.cpu().numpy()                     # the single device-to-host copy
                self._counts = {'n': int(w[native.KNN_N]), 'n_valid': int(w[native.KNN_N_VALID]), 'bad_rows': int(w[native.KNN_BAD_ROWS])}
        return self._counts

    def search(self, features: torch.Tensor, k: int = 10, exclude: Optional[torch.Tensor] = None,
               temperature: float = DEFAULT_TEMPERATURE) -> Dict[str, torch.Tensor]:
        """The k nearest recorded rows of every row of (B, E) ``features``: ``distances`` (B, k) fp32 and ``indices`` (B, k) int32,
        ascending in the key; ``labels`` (B, k) int32 and ``severities`` (B, k) fp32 of the neighbours when the index keeps the columns;
        ``kth_distance`` and ``mean_distance`` (B,); with labels and ``num_classes`` ``class_probs`` (B, C) and ``class`` (B,) int32;
        with severities ``severity`` (B,).  Tensors on the features' device, nothing copied to the host."""
        x = features.detach()
        E = self.embed_dim
        if x.dim() != 2 or x.shape[1] != E or x.shape[0] < 1:
            raise RovitHipError(f'FeatureIndex.search: features must be (B >= 1, {E}), got {tuple(x.shape)}')
        check_k(k, temperature)
        if self.n < 1:
            raise RovitHipError('FeatureIndex: nothing recorded yet')
        if x.device != self.device:
            raise RovitHipError(f'FeatureIndex.search: features on {x.device}, the index on {self.device}')
        B = x.shape[0]
        if exclude is not None:
            if exclude.dim() != 1 or exclude.shape[0] != B or exclude.is_floating_point() or exclude.dtype == torch.bool:
                raise RovitHipError(f'FeatureIndex.search: exclude must be ({B},) integers, got {tuple(exclude.shape)} of {exclude.dtype}')
        if not self.built:
            self.build()
        vote = bool(self.has_labels) and self.num_classes is not None
        if not x.is_cuda:
            ref = search_reference(x.float().numpy(), self._rows[:self.n].numpy(), k, self.metric, None if exclude is None else exclude.numpy(),
                                   self._labels[:self.n].numpy() if self.has_labels else None,
                                   self._severity[:self.n].numpy() if self.has_severity else None,
                                   self.num_classes if vote else None, temperature)
            return {name: torch.from_numpy(np.ascontiguousarray(v.astype(_OUT_DTYPES.get(name, np.float32)))) for name, v in ref.items()}
        x = x.float().contiguous()
        ex = None if exclude is None else exclude.detach().to(device=x.device, dtype=torch.int32).contiguous()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=x.device)
        out = {'distances': f32(B, k), 'indices': i32(B, k)}
        if self.has_labels:
            out['labels'] = i32(B, k)
        if self.has_severity:
            out['severities'] = f32(B, k)
        out['kth_distance'], out['mean_distance'] = f32(B), f32(B)
        if vote:
            out['class_probs'], out['class'] = f32(B, self.num_classes), i32(B)
        if self.has_severity:
            out['severity'] = f32(B)
        lib = native.load()
        nbytes = lib.rovit_knn_workspace_bytes(B, self.n, E, k)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        d = native.KnnQuery()
        d.batch, d.n, d.embed, d.k, d.metric, d.max_workgroups = B, self.n, E, k, METRICS[self.metric], self.max_workgroups
        d.num_classes, d.temperature = (self.num_classes if vote else 0), float(temperature)
        d.queries, d.norms, d.valid, d.exclude = native.ptr(x), native.ptr(self._norms), native.ptr(self._valid), native.ptr(ex)
        d.rows = native.ptr(self._normalized if self.metric == 'cosine' else self._rows)
        d.ref_labels = native.ptr(self._labels) if self.has_labels else None
        d.ref_severity = native.ptr(self._severity) if self.has_severity else None
        d.workspace, d.workspace_bytes = native.ptr(ws), nbytes
        for name, t in out.items():
            setattr(d, 'cls' if name == 'class' else name, native.ptr(t))
        native.call('rovit_knn_search', ctypes.byref(d), native.stream_ptr())
        return out

    def state_dict(self) -> Dict:
        """The recorded rows and columns as CPU tensors and plain numbers (``torch.save`` takes it)."""
        if self.n < 1:
            raise RovitHipError('FeatureIndex.state_dict: nothing recorded yet')
        sd = {'embed_dim': self.embed_dim, 'num_classes': self.num_classes, 'metric': self.metric, 'n': self.n,
              'rows': self._rows[:self.n].detach().cpu().clone()}
        if self.has_labels:
            sd['class_labels'] = self._labels[:self.n].detach().cpu().clone()
        if self.has_severity:
            sd['severity'] = self._severity[:self.n].detach().cpu().clone()
        return sd

    def load_state_dict(self, sd: Dict, device=None) -> 'FeatureIndex':
        """Restore the recorded rows on ``device`` (default: the CPU) and build: ``search`` works at once."""
        if sd['embed_dim'] != self.embed_dim:
            raise RovitHipError(f"FeatureIndex.load_state_dict: the state holds {sd['embed_dim']} features, this object {self.embed_dim}")
        check_shape(self.embed_dim, sd['num_classes'], sd['metric'])
        self.reset()
        self.num_classes, self.metric = sd['num_classes'], sd['metric']
        dev = torch.device(device or 'cpu')
        on = lambda key: sd[key].to(dev) if key in sd else None
        self.update(sd['rows'].to(torch.float32).to(dev), on('class_labels'), on('severity'))
        return self.build()


def fit_model_index(model, x_or_loader, labels=None, severity=None, metric: str = 'cosine', chunk: int = 256) -> FeatureIndex:
    """``FeatureIndex`` of the model's own backbone features in eval mode under no_grad, ``chunk`` images at a time: an image tensor with
    optional ``labels`` and ``severity``, or an iterable of batches ``(images, class_labels, severity_labels, ...)`` (host batches of a
    loader are copied to the model's device; a batch of one or two elements records fewer columns)."""
    if not (isinstance(chunk, int) and chunk >= 1):
        raise RovitHipError(f'fit_feature_index: chunk must be a positive integer, got {chunk!r}')
    is_tensor = isinstance(x_or_loader, torch.Tensor)
    dev = next(model.parameters()).device
    fi = FeatureIndex(model.backbone.embed_dim, model.classification_head.fc2.out_features, metric)
    batches = [(x_or_loader, labels, severity)] if is_tensor else x_or_loader
    was_training = model.backbone.training
    model.backbone.eval()
    try:
        with torch.no_grad():
            for batch in batches:
                batch = tuple(batch) if isinstance(batch, (tuple, list)) else (batch,)
                images, y, s = batch[0], (batch[1] if len(batch) > 1 else None), (batch[2] if len(batch) > 2 else None)
                if is_tensor:
                    native.ptr(images)                              # a CPU tensor raises: the backbone has no CPU path
                else:
                    images = images.to(dev, non_blocking=True)
                for r0 in range(0, images.shape[0], chunk):
                    fi.update(model.backbone(images[r0:r0 + chunk]), None if y is None else y[r0:r0 + chunk],
                              None if s is None else s[r0:r0 + chunk])
    finally:
        model.backbone.train(was_training)
    return fi.build()
