"""k-means of the feature space: k-means++ seeding, Lloyd iterations with the exact stopping rule, medoids, and the cluster-by-class
score card.

The feature-space tools answer what needs a label or a query (``density``, ``neighbors``, ``influence``, ``embedding``).  The
unsupervised questions are one algorithm: which sub-populations do the features form (``KMeans.fit``), which real leaves are their
prototypes (``medoids_``), do the clusters agree with the disease labels (``score_card``: purity, NMI, ARI from the contingency table:
a label audit that needs no trained head), and which m of many unlabelled photographs should be labelled first (``kmeans_pp``: the D^2
seeding alone is the standard diversity sampler).  The recipe ``torch.cdist`` + ``argmin`` + ``index_add_`` materialises n x k
distances, has no tie rule and sums centroids with atomics; ``csrc/kmeans.hip`` keeps no such matrix and returns the same bits for
every grid and from run to run.

Definitions (include/rovit_hip.h states them for the device; the numpy statements below follow them in fp64).
  Rows: (n, E) fp32, E a multiple of 32 up to 256, 1 <= n <= 2^20, 1 <= k <= 256.  Validity is ``FeatureIndex``'s: a row with a
  non-finite feature or squared norm (with 'cosine' also a zero row) is absent: label -1, distances +inf, silhouette 0, counted in
  ``bad_rows``; it enters no sum and no pick.
  Distance of a row x to a centroid c: 'l2' max(0, (|x|^2 + |c|^2) - 2 x.c); 'cosine' max(0, 1 - x^.c) on the unit rows with unit
  centroids (spherical k-means).  On the device every term is fp32 and the chains ascend in feature index, in the seeding kernel
  (vector units) and in the assignment kernel (matrix instruction) alike: the same bits.
  Order: a row belongs to the centroid with the smallest key (bits(d) << 32) | c: ties go to the lower cluster index.  The second
  smallest key gives ``second_distance`` (+inf with k = 1).
  Seeding (Arthur & Vassilvitskii 2007, one trial per seed), exact in integers.  Seed j of restart r draws r64 = (w.x << 32) | w.y
  from Philox4x32-10(key = seed, counter = (j, r, "KMns", 0)).  Seed 0 is the floor(r64 n_valid / 2^64)-th valid row.  Seed j > 0:
  d_i = the smallest distance to the seeds so far (fp32), max d_i = m 2^e with m in [1/2, 1), w_i = floor(d_i 2^(40 - e)), W = sum w_i,
  t = floor(r64 W / 2^64), the seed is the smallest i with sum_{i' <= i} w_i' > t.  W = 0: w_i = 1 for every valid row (``w0_events``).
  Lloyd: assign; when no label changed the run stops (``n_iter_`` = that iteration); else every centroid becomes the fp64 mean of its
  members in ascending row order (segments of 1024 members, added in order), rounded once to fp32; with 'cosine' the fp64 mean of the
  unit rows over its fp64 length, rounded once.  An empty cluster keeps its centroid, and so does a 'cosine' cluster whose mean has
  zero length; both are counted.  NOT built: relocation of empty clusters (sklearn's), a centroid-shift tolerance, mini-batches, k > 256.
  Final pass: one more assign against the final centroids; ``labels_``, ``distances_``, ``inertia_`` (fp64 sum of the fp32 distances),
  ``counts_``, ``medoids_`` (the member with the smallest key (bits(d) << 32) | row; -1 for an empty cluster), ``radii_`` (the largest
  member distance) come from it.  ``n_init`` restarts run one after the other; the lowest inertia is kept, ties go to the lower restart.
  Silhouette (simplified): (b - a) / max(a, b), a, b the square roots of the two distances with 'l2', the distances with 'cosine';
  0 with k = 1, with max(a, b) = 0 and for an absent row; the mean is taken over the valid rows.
  Score card: purity, homogeneity, completeness, NMI (arithmetic normalisation) and ARI in fp64 on the host from the k x C int64
  contingency table, which the device fills with integer atomics; rows with a label outside [0, C) (or absent) are left out and counted.

``fit`` enqueues everything and waits for nothing (a given ``init`` tensor, k x E values, is first brought to the host, where with
'cosine' it is normalised in fp64); the one device-to-host copy of results (the status blocks of all restarts) happens on the first
access of an attribute that needs it.  CPU tensors run through the same entry points on the numpy statements.
"""
from __future__ import annotations

import ctypes
from typing import Dict

import numpy as np
import torch

from . import native
from .native import RovitHipError
from .neighbors import METRICS, _np, _unit_rows, valid_rows

MASK32 = 0xFFFFFFFF


def _check(E, k, metric, who='KMeans') -> None:
    if not (isinstance(E, int) and 32 <= E <= 256 and E % 32 == 0):
        raise RovitHipError(f'{who}: the rows must hold a multiple of 32 features in 32..256, got {E!r}')
    if not (isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= native.KMEANS_MAX_K):
        raise RovitHipError(f'{who}: the number of clusters or seeds must be in 1..{native.KMEANS_MAX_K}, got {k!r}')
    if metric not in METRICS:
        raise RovitHipError(f'{who}: metric must be one of {sorted(METRICS)}, got {metric!r}')


def _check_rows(x, who) -> None:
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[0] > native.KMEANS_MAX_ROWS:
        raise RovitHipError(f'{who}: features must be (1 <= n <= {native.KMEANS_MAX_ROWS}, E), got {tuple(x.shape)}')


# ---- host statements -------------------------------------------------------------------------------------------------------------------

def philox_r64(seed: int, j: int, restart: int = 0) -> int:
    """r64 = (w.x << 32) | w.y of Philox4x32-10(key = seed, counter = (j, restart, "KMns", 0)) in Python integers."""
    c = [j & MASK32, restart & MASK32, native.KMEANS_STREAM, 0]
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK32, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + 0x9E3779B9) & MASK32, (k1 + 0xBB67AE85) & MASK32
    return (c[0] << 32) | c[1]


def seed_reference(min_distance, valid, r64: int) -> Dict:
    """One pick of the integer seeding rule.  ``min_distance``: the fp32 d_i it is given, or None for seed 0; ``valid`` (n,) bool.
    Returns ``index`` (-1 without a valid row), the integer ``weights``, ``W``, ``t`` and ``w0`` (the W = 0 rule was taken)."""
    ok = np.asarray(valid, dtype=bool)
    w = np.zeros(ok.shape[0], dtype=object)
    w0 = False
    if min_distance is not None:
        d = np.where(ok, np.asarray(min_distance, dtype=np.float32), np.float32(0))
        dmax = float(d.max()) if ok.any() else 0.0
        if dmax > 0:
            e = int(np.frexp(dmax)[1])
            w = np.array([int(np.ldexp(float(v), 40 - e)) if g else 0 for v, g in zip(d, ok)], dtype=object)
        w0 = int(w.sum()) == 0
    if min_distance is None or w0:
        w = np.array([1 if g else 0 for g in ok], dtype=object)
    W = int(w.sum())
    if W == 0:
        return {'index': -1, 'weights': w, 'W': 0, 't': 0, 'w0': w0}
    t = (int(r64) * W) >> 64
    run, index = 0, -1
    for i, v in enumerate(w):
        run += int(v)
        if run > t:
            index = i
            break
    return {'index': index, 'weights': w, 'W': W, 't': t, 'w0': w0}


def _rows64(x32: np.ndarray, ok: np.ndarray, metric: str) -> np.ndarray:
    """The rows the distances are taken on, in fp64: the unit rows with 'cosine'; zeros for a row that is absent."""
    return _unit_rows(x32, ok) if metric == 'cosine' else np.where(ok[:, None], x32, 0).astype(np.float64)


def centroid_distances(features, centroids, metric: str) -> np.ndarray:
    """(n, k) fp64 distances of the definition from fp32 rows and fp32 centroids; +inf for an absent row."""
    x32, c = _np(features, np.float32), _np(centroids, np.float32).astype(np.float64)
    ok = valid_rows(x32, metric)
    x = _rows64(x32, ok, metric)
    d = 1.0 - x @ c.T if metric == 'cosine' else ((x * x).sum(1)[:, None] + (c * c).sum(1)[None]) - 2.0 * (x @ c.T)
    d = np.maximum(d, 0.0)
    d[~ok] = np.inf
    return d


def silhouette_reference(d1, d2, metric: str) -> np.ndarray:
    d1, d2 = np.asarray(d1, dtype=np.float64), np.asarray(d2, dtype=np.float64)
    fin = np.isfinite(d1) & np.isfinite(d2)
    a, b = (np.where(fin, v, 0.0) if metric == 'cosine' else np.sqrt(np.where(fin, v, 0.0)) for v in (d1, d2))
    m = np.maximum(a, b)
    return np.where(fin & (m > 0), (b - a) / np.where(m > 0, m, 1.0), 0.0)


def assign_reference(features, centroids, metric: str = 'l2') -> Dict[str, np.ndarray]:
    """``labels`` (int64, -1 for an absent row), ``distance``, ``second_distance`` (+inf with k = 1), ``silhouette`` and ``margin``
    (second minus first distance) in fp64 by the key order: the smallest (distance, cluster index)."""
    d = centroid_distances(features, centroids, metric)
    n, k = d.shape
    labels = np.argmin(d, axis=1)                                   # the first minimum: ties go to the lower index
    d1 = d[np.arange(n), labels]
    rest = d.copy()
    rest[np.arange(n), labels] = np.inf
    d2 = rest.min(axis=1) if k > 1 else np.full(n, np.inf)
    ok = np.isfinite(d1)
    d2 = np.where(ok, d2, np.inf)
    with np.errstate(invalid='ignore'):
        margin = np.where(ok, d2 - d1, np.inf)
    return {'labels': np.where(ok, labels, -1).astype(np.int64), 'distance': d1, 'second_distance': d2,
            'silhouette': silhouette_reference(d1, d2, metric), 'margin': margin}


def update_reference(features, labels, centroids, metric: str = 'l2') -> Dict:
    """The update of the definition: ``centroids`` (k, E) fp32 (the fp64 member mean rounded once; an empty cluster and a zero-length
    'cosine' mean keep the row of ``centroids``), ``means`` in fp64 before the rounding, ``counts``, ``empty``, ``zero_means``."""
    x32, y = _np(features, np.float32), _np(labels).astype(np.int64)
    old = _np(centroids, np.float32)
    k = old.shape[0]
    x = _rows64(x32, valid_rows(x32, metric), metric)
    new, means = old.copy(), old.astype(np.float64)
    counts = np.bincount(y[(y >= 0) & (y < k)], minlength=k).astype(np.int64)
    zero = 0
    for c in range(k):
        if counts[c] == 0:
            continue
        m = x[y == c].sum(axis=0) / counts[c]
        if metric == 'cosine':
            nn = float((m * m).sum())
            if not (nn > 0 and np.isfinite(nn)):
                zero += 1
                continue
            m = m / np.sqrt(nn)
        means[c], new[c] = m, m.astype(np.float32)
    return {'centroids': new, 'means': means, 'counts': counts, 'empty': int((counts == 0).sum()), 'zero_means': zero}


def cluster_stats_reference(labels, distance, k: int) -> Dict[str, np.ndarray]:
    """``counts``, ``medoids`` (the member with the smallest (distance, row); -1 for an empty cluster), ``radii`` (largest member
    distance, 0 for an empty cluster) and ``inertia`` per cluster from the labels and the distances it is given."""
    y, d = _np(labels).astype(np.int64), np.asarray(_np(distance), dtype=np.float64)
    counts, medoids, radii, inertia = np.zeros(k, np.int64), np.full(k, -1, np.int64), np.zeros(k), np.zeros(k)
    for c in range(k):
        rows = np.nonzero(y == c)[0]
        counts[c] = rows.size
        if rows.size:
            medoids[c] = rows[np.argmin(d[rows])]                   # the first minimum: the lowest row among equal distances
            radii[c], inertia[c] = d[rows].max(), d[rows].sum()
    return {'counts': counts, 'medoids': medoids, 'radii': radii, 'inertia': inertia}


def kmeans_pp_reference(features, m: int, metric: str = 'l2', seed: int = 0, restart: int = 0) -> Dict:
    """The whole seeding in numpy: fp64 distances rounded to fp32, then the integer rule.  ``seeds`` (m,) int64, ``taps`` (m, n) fp32 (row
    j >= 1: the d_i seed j was drawn from), ``w0_events``, ``picks`` (every pick's ``seed_reference`` result)."""
    x32 = _np(features, np.float32)
    _check_rows(x32, 'kmeans_pp_reference')
    _check(int(x32.shape[1]), m, metric, 'kmeans_pp_reference')
    ok = valid_rows(x32, metric)
    x = _rows64(x32, ok, metric)
    n = x32.shape[0]
    seeds, taps, picks, w0 = [], np.full((m, n), np.inf, dtype=np.float32), [], 0
    mind = None
    for j in range(m):
        if j > 0:
            c = x[seeds[-1]] if seeds[-1] >= 0 else None
            if c is None:
                d = np.zeros(n)
            elif metric == 'cosine':
                d = 1.0 - x @ c
            else:
                d = ((x * x).sum(1) + (c * c).sum()) - 2.0 * (x @ c)
            d = np.maximum(d, 0.0).astype(np.float32)
            mind = d if mind is None else np.minimum(mind, d)
            taps[j] = np.where(ok, mind, np.inf)
        pick = seed_reference(mind, ok, philox_r64(seed, j, restart))
        w0 += int(pick['w0'])
        picks.append(pick)
        seeds.append(pick['index'])
    return {'seeds': np.asarray(seeds, dtype=np.int64), 'taps': taps, 'w0_events': w0, 'picks': picks}


def fit_reference(features, n_clusters: int, metric: str = 'l2', max_iter: int = 100, n_init: int = 1, seed: int = 0, init=None) -> Dict:
    """``KMeans.fit`` in numpy fp64.  Returns the kept restart's ``cluster_centers`` (fp32), ``labels``, ``distances``,
    ``second_distances``, ``silhouette``, ``counts``, ``medoids``, ``radii``, ``seeds``, ``inertia``, ``n_iter``, ``restart``,
    ``min_margin`` (the smallest margin of a valid row over all its assigns), ``centers_trace`` (the centroids of every assign, the
    final one included), ``inertias`` and ``runs`` of all restarts and the counters."""
    x32 = _np(features, np.float32)
    _check_rows(x32, 'fit_reference')
    _check(int(x32.shape[1]), n_clusters, metric, 'fit_reference')
    ok = valid_rows(x32, metric)
    if n_clusters > int(ok.sum()):
        raise RovitHipError(f'fit_reference: {n_clusters} clusters for {int(ok.sum())} valid rows')
    runs = []
    for r in range(n_init if init is None else 1):
        if init is None:
            pp = kmeans_pp_reference(x32, n_clusters, metric, seed, r)
            seeds, w0 = pp['seeds'], pp['w0_events']
            c = _rows64(x32, ok, metric)[seeds].astype(np.float32)
        else:
            seeds, w0, c = np.full(n_clusters, -1, np.int64), 0, _prepare_init(_np(init, np.float32), metric)
        prev, n_iter, margin, empty_events, zero_means, trace, converged = None, max_iter, np.inf, 0, 0, [], False
        for it in range(1, max_iter + 1):
            trace.append(c.copy())
            a = assign_reference(x32, c, metric)
            margin = min(margin, float(a['margin'][ok].min()) if ok.any() else np.inf)
            if prev is not None and np.array_equal(prev, a['labels']) or not ok.any():
                n_iter, converged = it, True
                break
            prev = a['labels']
            u = update_reference(x32, prev, c, metric)
            c, empty_events, zero_means = u['centroids'], empty_events + u['empty'], zero_means + u['zero_means']
        trace.append(c.copy())
        a = assign_reference(x32, c, metric)
        margin = min(margin, float(a['margin'][ok].min()) if ok.any() else np.inf)
        st = cluster_stats_reference(a['labels'], a['distance'], n_clusters)
        runs.append({'cluster_centers': c, 'labels': a['labels'], 'distances': a['distance'], 'second_distances': a['second_distance'],
                     'silhouette': a['silhouette'], 'seeds': seeds, 'centers_trace': trace, 'converged': converged, 'n_iter': n_iter, 'min_margin': margin, 'w0_events': w0,
                     'empty_events': empty_events, 'zero_means': zero_means, 'empty': int((st['counts'] == 0).sum()),
                     'inertia': float(st['inertia'].sum()), 'counts': st['counts'], 'medoids': st['medoids'], 'radii': st['radii'],
                     'mean_silhouette': float(a['silhouette'][ok].mean()) if ok.any() else 0.0})
    inertias = [run['inertia'] for run in runs]
    best = int(np.argmin(inertias))                                 # the first minimum: ties go to the lower restart
    out = dict(runs[best])
    out.update(restart=best, inertias=inertias, n_valid=int(ok.sum()), bad_rows=int((~ok).sum()), runs=runs)
    return out


def _prepare_init(c32: np.ndarray, metric: str) -> np.ndarray:
    """A given init as the run takes it: as it is with 'l2'; over its fp64 length, rounded once, with 'cosine'."""
    if metric != 'cosine':
        return np.ascontiguousarray(c32, dtype=np.float32)
    c = c32.astype(np.float64)
    length = np.sqrt((c * c).sum(axis=1, keepdims=True))
    if not (np.isfinite(length).all() and (length > 0).all()):
        raise RovitHipError('KMeans: with cosine every row of a given init needs a finite positive length')
    return (c / length).astype(np.float32)


def contingency_reference(clusters, classes, k: int, num_classes: int):
    """The (k, C) int64 table and the number of rows left out (cluster outside [0, k) or class outside [0, C))."""
    a, y = _np(clusters).astype(np.int64).reshape(-1), _np(classes).astype(np.int64).reshape(-1)
    keep = (a >= 0) & (a < k) & (y >= 0) & (y < num_classes)
    table = np.zeros((k, num_classes), dtype=np.int64)
    np.add.at(table, (a[keep], y[keep]), 1)
    return table, int((~keep).sum())


def partition_scores_reference(table) -> Dict[str, float]:
    """Purity, homogeneity, completeness, NMI (arithmetic normalisation: 2 I / (H(cluster) + H(class))) and ARI (Hubert & Arabie 1985)
    in fp64 from a (k, C) contingency table of counts.  An empty table scores 1 everywhere, as identical trivial partitions do."""
    t = np.asarray(table, dtype=np.float64)
    n = t.sum()
    if n <= 0:
        return {'n': 0, 'purity': 1.0, 'homogeneity': 1.0, 'completeness': 1.0, 'nmi': 1.0, 'ari': 1.0}
    a, b = t.sum(axis=1), t.sum(axis=0)

    def entropy(v):
        p = v[v > 0] / n
        return float(-(p * np.log(p)).sum())
    h_k, h_c = entropy(a), entropy(b)
    nz = t > 0
    mi = float((t[nz] / n * np.log(t[nz] * n / np.outer(a, b)[nz])).sum())
    mi = max(mi, 0.0)
    homogeneity = mi / h_c if h_c > 0 else 1.0
    completeness = mi / h_k if h_k > 0 else 1.0
    nmi = 2.0 * mi / (h_k + h_c) if (h_k + h_c) > 0 else 1.0
    comb = lambda v: float((v * (v - 1.0) / 2.0).sum())
    s_t, s_a, s_b, total = comb(t), comb(a), comb(b), n * (n - 1.0) / 2.0
    expected = s_a * s_b / total if total > 0 else 0.0
    denom = 0.5 * (s_a + s_b) - expected
    ari = (s_t - expected) / denom if denom != 0 else 1.0
    return {'n': int(n), 'purity': float(t.max(axis=1).sum() / n), 'homogeneity': float(homogeneity), 'completeness': float(completeness),
            'nmi': float(nmi), 'ari': float(ari)}


# ---- the estimator ---------------------------------------------------------------------------------------------------------------------

_RUN_FIELDS = ('labels', 'distance', 'second_distance', 'silhouette')


class KMeans:
    """k-means with k-means++ seeding on recorded feature rows; see the module docstring.  ``fit`` waits for nothing; the first access of
    an attribute that needs the status blocks makes the one device-to-host copy."""

    def __init__(self, n_clusters: int, metric: str = 'l2', max_iter: int = 100, n_init: int = 1, seed: int = 0, init='k-means++'):
        _check(32, n_clusters, metric)
        if not (isinstance(max_iter, int) and 1 <= max_iter <= native.KMEANS_MAX_ITER):
            raise RovitHipError(f'KMeans: max_iter must be in 1..{native.KMEANS_MAX_ITER}, got {max_iter!r}')
        if not (isinstance(n_init, int) and 1 <= n_init <= 64):
            raise RovitHipError(f'KMeans: n_init must be in 1..64, got {n_init!r}')
        if not (isinstance(seed, int) and 0 <= seed < 2 ** 64):
            raise RovitHipError(f'KMeans: seed must be an integer in [0, 2^64), got {seed!r}')
        if not (isinstance(init, torch.Tensor) or init == 'k-means++'):
            raise RovitHipError("KMeans: init must be 'k-means++' or a (k, E) tensor")
        self.n_clusters, self.metric, self.max_iter, self.n_init, self.seed, self.init = n_clusters, metric, max_iter, n_init, seed, init
        self.max_workgroups = 0                                    # > 0 caps every grid (tests); the results do not depend on it
        self._clear()

    def _clear(self) -> None:
        self._runs = self._status_dev = self._host = self._best = self._status = self._centers = None
        self.n = self.embed_dim = None

    # -- fitting
    def fit(self, features: torch.Tensor) -> 'KMeans':
        x = features.detach()
        _check_rows(x, 'KMeans.fit')
        n, E, k = int(x.shape[0]), int(x.shape[1]), self.n_clusters
        _check(E, k, self.metric, 'KMeans.fit')
        if k > n:
            raise RovitHipError(f'KMeans.fit: {k} clusters for {n} rows')
        given = self.init if isinstance(self.init, torch.Tensor) else None
        if given is not None and tuple(given.shape) != (k, E):
            raise RovitHipError(f'KMeans.fit: the given init must be ({k}, {E}), got {tuple(given.shape)}')
        self._clear()
        self.n, self.embed_dim = n, E
        if not x.is_cuda:
            self._host = fit_reference(x.float().numpy(), k, self.metric, self.max_iter, self.n_init, self.seed,
                                       None if given is None else given.detach().cpu().numpy())
            self._best = self._host['restart']
            return self
        x = x.float().contiguous()
        dev = x.device
        restarts = self.n_init if given is None else 1
        words = native.KMEANS_WORDS
        self._status_dev = torch.zeros((restarts, 2 * words + 5 * k), dtype=torch.int64, device=dev)
        ws, nbytes, normalized = self._workspace(n, E, k, dev)
        init32 = None if given is None else torch.from_numpy(_prepare_init(given.detach().cpu().float().numpy(), self.metric)).to(dev)
        self._runs = []
        for r in range(restarts):
            run = {'centers': torch.empty((k, E), dtype=torch.float32, device=dev), 'seeds': torch.full((k,), -1, dtype=torch.int32, device=dev),
                   'labels': torch.empty(n, dtype=torch.int32, device=dev)}
            for name in _RUN_FIELDS[1:]:
                run[name] = torch.empty(n, dtype=torch.float32, device=dev)
            d = self._problem(x, normalized, ws, nbytes, run, k)
            d.restart, d.m = r, k
            if init32 is None:
                d.seeds, d.status = native.ptr(run['seeds']), native.ptr(self._status_dev[r, :words])
                native.call('rovit_kmeans_seed', ctypes.byref(d), native.stream_ptr())
            else:
                run['centers'].copy_(init32)
            d.status = native.ptr(self._status_dev[r, words:])
            native.call('rovit_kmeans_run', ctypes.byref(d), native.stream_ptr())
            self._runs.append(run)
        if restarts == 1:
            self._best = 0
        return self

    def _workspace(self, n, E, k, dev):
        nbytes = native.load().rovit_kmeans_workspace_bytes(n, E, k)
        if nbytes == 0:
            raise RovitHipError(f'KMeans: n = {n}, E = {E}, k = {k} are outside the limits')
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        normalized = torch.empty((n, E), dtype=torch.float32, device=dev) if self.metric == 'cosine' else None
        return ws, nbytes, normalized

    def _problem(self, x, normalized, ws, nbytes, run, k) -> 'native.KMeansProblem':
        d = native.KMeansProblem()
        d.n, d.embed, d.k, d.metric, d.max_iter, d.max_workgroups = int(x.shape[0]), int(x.shape[1]), k, METRICS[self.metric], self.max_iter, \
            self.max_workgroups
        d.seed = self.seed
        d.features, d.normalized, d.centroids = native.ptr(x), native.ptr(normalized), native.ptr(run['centers'])
        d.labels, d.distance, d.second_distance, d.silhouette = (native.ptr(run[name]) for name in _RUN_FIELDS)
        d.workspace, d.workspace_bytes = native.ptr(ws), nbytes
        return d

    def fit_predict(self, features: torch.Tensor) -> torch.Tensor:
        return self.fit(features).labels_

    # -- results
    def _need_fit(self) -> None:
        if self._runs is None and self._host is None and self._centers is None:
            raise RovitHipError('KMeans: not fitted yet')

    def _resolve(self) -> Dict:
        """The status blocks of all restarts in ONE device-to-host copy, and the kept restart."""
        self._need_fit()
        if self._status is None:
            k, words = self.n_clusters, native.KMEANS_WORDS
            if self._host is not None:
                h = self._host
                self._status = {key: h[key] for key in ('n_valid', 'bad_rows', 'n_iter', 'converged', 'empty', 'empty_events', 'zero_means', 'w0_events',
                                                        'inertia', 'inertias', 'restart', 'counts', 'medoids', 'radii', 'mean_silhouette')}
                self._status.update(n=self.n, short=0)
            elif self._runs is None:
                raise RovitHipError('KMeans: loaded from a state: only cluster_centers_ and predict are available')
            else:
                raw = self._status_dev.cpu().numpy()               # the single device-to-host copy
                blocks = []
                for row in raw:
                    sw, rw, tail = row[:words], row[words:2 * words], row[2 * words:]
                    inertia_c = tail[2 * k:3 * k].view(np.float64)
                    blocks.append({'n': int(rw[native.KMEANS_N]), 'n_valid': int(rw[native.KMEANS_N_VALID]),
                                   'bad_rows': int(rw[native.KMEANS_BAD_ROWS]), 'n_iter': int(rw[native.KMEANS_N_ITER]),
                                   'converged': bool(rw[native.KMEANS_DONE]),
                                   'empty': int(rw[native.KMEANS_EMPTY]), 'empty_events': int(rw[native.KMEANS_EMPTY_EVENTS]),
                                   'zero_means': int(rw[native.KMEANS_ZERO_MEANS]), 'w0_events': int(sw[native.KMEANS_W0_EVENTS]),
                                   'short': int(sw[native.KMEANS_SHORT]), 'counts': tail[:k].copy(), 'medoids': tail[k:2 * k].copy(),
                                   'inertia': float(sum(float(v) for v in inertia_c)),         # clusters in ascending order, fp64
                                   'silhouette_sum': float(sum(float(v) for v in tail[3 * k:4 * k].view(np.float64))),
                                   'radii': tail[4 * k:5 * k].view(np.float64).astype(np.float32)})
                inertias = [b['inertia'] for b in blocks]
                best = int(np.argmin(inertias))
                self._best = best
                self._status = dict(blocks[best])
                nv = self._status['n_valid']
                self._status.update(inertias=inertias, restart=best, mean_silhouette=self._status.pop('silhouette_sum') / nv if nv else 0.0)
        return self._status

    def _kept(self) -> Dict:
        if self._best is None:
            self._resolve()
        return self._runs[self._best]

    def _host_tensor(self, key, dtype) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(np.asarray(self._host[key]).astype(dtype)))

    @property
    def status_(self) -> Dict:
        return self._resolve()

    @property
    def cluster_centers_(self) -> torch.Tensor:
        self._need_fit()
        if self._centers is not None:
            return self._centers
        return self._host_tensor('cluster_centers', np.float32) if self._host is not None else self._kept()['centers']

    @property
    def labels_(self) -> torch.Tensor:
        self._need_fit()
        return self._host_tensor('labels', np.int32) if self._host is not None else self._kept()['labels']

    @property
    def distances_(self) -> torch.Tensor:
        self._need_fit()
        return self._host_tensor('distances', np.float32) if self._host is not None else self._kept()['distance']

    @property
    def second_distances_(self) -> torch.Tensor:
        self._need_fit()
        return self._host_tensor('second_distances', np.float32) if self._host is not None else self._kept()['second_distance']

    @property
    def silhouette_(self) -> torch.Tensor:
        self._need_fit()
        return self._host_tensor('silhouette', np.float32) if self._host is not None else self._kept()['silhouette']

    @property
    def seeds_(self) -> torch.Tensor:
        self._need_fit()
        return self._host_tensor('seeds', np.int32) if self._host is not None else self._kept()['seeds']

    @property
    def counts_(self) -> torch.Tensor:
        return torch.from_numpy(np.asarray(self._resolve()['counts'], dtype=np.int64).copy())

    @property
    def medoids_(self) -> torch.Tensor:
        return torch.from_numpy(np.asarray(self._resolve()['medoids'], dtype=np.int64).copy())

    @property
    def radii_(self) -> torch.Tensor:
        return torch.from_numpy(np.asarray(self._resolve()['radii'], dtype=np.float32).copy())

    @property
    def inertia_(self) -> float:
        return float(self._resolve()['inertia'])

    @property
    def n_iter_(self) -> int:
        return int(self._resolve()['n_iter'])

    # -- out-of-sample rows
    def predict(self, features: torch.Tensor) -> Dict[str, torch.Tensor]:
        """``labels`` (int32), ``distance``, ``second_distance`` and ``silhouette`` of (B, E) rows against the fitted centroids, on the
        rows' device; nothing is copied to the host."""
        centers = self.cluster_centers_
        x = features.detach()
        _check_rows(x, 'KMeans.predict')
        k, E = int(centers.shape[0]), int(centers.shape[1])
        if x.shape[1] != E:
            raise RovitHipError(f'KMeans.predict: the rows hold {x.shape[1]} features, the centroids {E}')
        if not x.is_cuda:
            ref = assign_reference(x.float().numpy(), centers.detach().cpu().numpy(), self.metric)
            return {'labels': torch.from_numpy(ref['labels'].astype(np.int32)),
                    **{name: torch.from_numpy(ref[name].astype(np.float32)) for name in _RUN_FIELDS[1:]}}
        x = x.float().contiguous()
        n, dev = int(x.shape[0]), x.device
        ws, nbytes, normalized = self._workspace(n, E, k, dev)
        run = {'centers': centers.to(dev).float().contiguous(), 'labels': torch.empty(n, dtype=torch.int32, device=dev)}
        for name in _RUN_FIELDS[1:]:
            run[name] = torch.empty(n, dtype=torch.float32, device=dev)
        status = torch.empty(native.KMEANS_WORDS, dtype=torch.int64, device=dev)
        d = self._problem(x, normalized, ws, nbytes, run, k)
        d.status = native.ptr(status)
        native.call('rovit_kmeans_assign', ctypes.byref(d), native.stream_ptr())
        return {name: run[name] for name in _RUN_FIELDS}

    # -- score card
    def contingency(self, labels: torch.Tensor, num_classes: int) -> torch.Tensor:
        """(k * C + 1,) int64 on the labels' device: the table row-major, then the number of rows left out."""
        y = labels.detach().reshape(-1)
        k = self.n_clusters
        if not (isinstance(num_classes, int) and 1 <= num_classes <= native.KNN_MAX_CLASSES):
            raise RovitHipError(f'KMeans.score_card: num_classes must be in 1..{native.KNN_MAX_CLASSES}, got {num_classes!r}')
        mine = self.labels_
        if y.shape[0] != mine.shape[0] or y.is_floating_point() or y.dtype == torch.bool:
            raise RovitHipError(f'KMeans.score_card: labels must be {mine.shape[0]} integers, got {tuple(labels.shape)} of {y.dtype}')
        if not mine.is_cuda:
            table, left = contingency_reference(mine.numpy(), y.cpu().numpy(), k, num_classes)
            return torch.from_numpy(np.concatenate([table.reshape(-1), [left]]).astype(np.int64))
        y = y.to(device=mine.device, dtype=torch.int32).contiguous()
        out = torch.empty(k * num_classes + 1, dtype=torch.int64, device=mine.device)
        native.call('rovit_kmeans_contingency', native.ptr(mine), native.ptr(y), int(mine.shape[0]), k, num_classes, native.ptr(out),
                    native.stream_ptr())
        return out

    def score_card(self, labels: torch.Tensor, num_classes: int) -> Dict:
        """The cluster-by-class ``table`` (k, C) int64, ``left_out``, and ``purity``, ``homogeneity``, ``completeness``, ``nmi``, ``ari`` from
        it in fp64 on the host (one copy of the table), with the run's ``inertia`` and ``mean_silhouette``."""
        flat = self.contingency(labels, num_classes).cpu().numpy()
        table = flat[:-1].reshape(self.n_clusters, num_classes)
        out = {'table': table, 'left_out': int(flat[-1])}
        out.update(partition_scores_reference(table))
        st = self._resolve()
        out.update(inertia=float(st['inertia']), mean_silhouette=float(st['mean_silhouette']))
        return out

    # -- persistence
    def state_dict(self) -> Dict:
        return {'n_clusters': self.n_clusters, 'metric': self.metric, 'max_iter': self.max_iter, 'n_init': self.n_init, 'seed': self.seed,
                'cluster_centers': self.cluster_centers_.detach().cpu().clone()}

    def load_state_dict(self, sd: Dict, device=None) -> 'KMeans':
        """Restore the centroids on ``device`` (default: the CPU): ``cluster_centers_`` and ``predict`` work at once."""
        _check(int(sd['cluster_centers'].shape[1]), sd['n_clusters'], sd['metric'], 'KMeans.load_state_dict')
        self.n_clusters, self.metric, self.max_iter, self.n_init, self.seed = (sd[key] for key in ('n_clusters', 'metric', 'max_iter', 'n_init',
                                                                                                     'seed'))
        self._clear()
        self._centers = sd['cluster_centers'].to(torch.float32).to(torch.device(device or 'cpu'))
        self.embed_dim = int(self._centers.shape[1])
        return self


def kmeans_pp(features: torch.Tensor, m: int, metric: str = 'l2', seed: int = 0, return_tap: bool = False, max_workgroups: int = 0):
    """The k-means++ seeding alone: ``m`` row indices (int32, on the rows' device) that spread over the feature space: the rows to label
    first.  With ``return_tap`` also the (m, n) fp32 tap (row j >= 1: the min-distances seed j was drawn from) and the status words."""
    x = features.detach()
    _check_rows(x, 'kmeans_pp')
    n, E = int(x.shape[0]), int(x.shape[1])
    _check(E, m, metric, 'kmeans_pp')
    if not x.is_cuda:
        ref = kmeans_pp_reference(x.float().numpy(), m, metric, seed)
        seeds = torch.from_numpy(ref['seeds'].astype(np.int32))
        return (seeds, torch.from_numpy(ref['taps']), {'w0_events': ref['w0_events']}) if return_tap else seeds
    x = x.float().contiguous()
    dev = x.device
    nbytes = native.load().rovit_kmeans_workspace_bytes(n, E, m)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    normalized = torch.empty((n, E), dtype=torch.float32, device=dev) if metric == 'cosine' else None
    seeds, centers = torch.full((m,), -1, dtype=torch.int32, device=dev), torch.empty((m, E), dtype=torch.float32, device=dev)
    tap = torch.full((m, n), float('inf'), dtype=torch.float32, device=dev) if return_tap else None
    status = torch.empty(native.KMEANS_WORDS, dtype=torch.int64, device=dev)
    d = native.KMeansProblem()
    d.n, d.embed, d.k, d.m, d.metric, d.max_iter, d.max_workgroups, d.restart, d.seed = n, E, m, m, METRICS[metric], 1, max_workgroups, 0, seed
    d.features, d.normalized, d.centroids, d.seeds, d.tap = native.ptr(x), native.ptr(normalized), native.ptr(centers), native.ptr(seeds), \
        native.ptr(tap)
    d.workspace, d.workspace_bytes, d.status = native.ptr(ws), nbytes, native.ptr(status)
    native.call('rovit_kmeans_seed', ctypes.byref(d), native.stream_ptr())
    if not return_tap:
        return seeds
    w = status.cpu().numpy()
    return seeds, tap, {'n_valid': int(w[native.KMEANS_N_VALID]), 'bad_rows': int(w[native.KMEANS_BAD_ROWS]),
                        'w0_events': int(w[native.KMEANS_W0_EVENTS]), 'short': int(w[native.KMEANS_SHORT])}


def cluster_model_features(model, x_or_loader, n_clusters: int, labels=None, chunk: int = 256, **kw) -> Dict:
    """k-means of the model's own backbone features, gathered as ``fit_feature_index`` gathers them (eval mode, no_grad, ``chunk`` images at
    a time).  Returns ``kmeans`` (the fitted object), ``features``, ``labels``, ``distances``, ``cluster_centers``, ``medoids``,
    ``counts``, ``silhouette``, and with class ``labels`` (or a loader that carries them) the ``score_card``."""
    from . import neighbors
    fi = neighbors.fit_model_index(model, x_or_loader, labels, None, metric='l2', chunk=chunk)
    feats = fi.rows().clone()
    km = KMeans(n_clusters, **kw).fit(feats)
    out = {'kmeans': km, 'features': feats, 'labels': km.labels_, 'distances': km.distances_, 'cluster_centers': km.cluster_centers_,
           'medoids': km.medoids_, 'counts': km.counts_, 'silhouette': km.silhouette_}
    if fi.has_labels:
        out['score_card'] = km.score_card(fi._labels[:fi.n], fi.num_classes)
    return out
