"""Data makers shared by tests/test_neighbors_cpu.py and tests/test_gpu_neighbors.py (no test in here)."""
import numpy as np

from density_cases import make

U32 = 2.0 ** -24


def integer_rows(n: int, E: int, seed: int) -> np.ndarray:
    """(n, E) fp32 rows with integer entries in [-3, 3]: every product, norm and l2 distance is an integer below 2^24, exact in fp32 in
    any order.  Few distinct distances: heavy ties."""
    return np.random.default_rng(seed).integers(-3, 4, (n, E)).astype(np.float32)


def float_case(N: int, E: int, C: int, B: int, seed: int):
    """N reference rows with labels and severities and B query rows of the same classes, all from ``density_cases.make``."""
    x, y = make(N + B, E, C, seed=seed)
    sev = (y + np.random.default_rng(seed + 7).uniform(-0.4, 0.4, N + B)).astype(np.float32)
    return x[:N], y[:N], sev[:N], x[N:]


def brute_force(queries, rows, k, metric, exclude=None):
    """The definition as a double loop in fp64, the k smallest (distance, index) pairs by a Python sort of tuples: indices (-1) and distances
    (+inf) per query.  Bad rows: a non-finite feature, and with cosine a zero norm."""
    q, r = np.asarray(queries, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    bad = lambda v: (not np.isfinite(v).all()) or (metric == 'cosine' and not (v * v).sum() > 0)
    idx, dist = np.full((q.shape[0], k), -1, dtype=np.int64), np.full((q.shape[0], k), np.inf)
    for i in range(q.shape[0]):
        if bad(q[i]):
            continue
        pairs = []
        for j in range(r.shape[0]):
            if bad(r[j]) or (exclude is not None and int(exclude[i]) == j):
                continue
            if metric == 'cosine':
                d = 1.0 - (q[i] / np.sqrt((q[i] * q[i]).sum())) @ (r[j] / np.sqrt((r[j] * r[j]).sum()))
            else:
                d = ((q[i] * q[i]).sum() + (r[j] * r[j]).sum()) - 2.0 * (q[i] @ r[j])
            pairs.append((max(d, 0.0), j))
        for s, (d, j) in enumerate(sorted(pairs)[:k]):
            idx[i, s], dist[i, s] = j, d
    return dist, idx


def distance_bounds(queries, rows, metric):
    """(B, N) bound on |device distance - fp64 distance| from the fp32 operations of the definition, u = 2^-24:
    l2: 2 (E + 1) u sum |q_k r_k| + (E + 1) u (|q|^2 + |r|^2) + 3 u (|q|^2 + |r|^2 + 2 sum |q_k r_k|); cosine: (2 E + 10) u."""
    q, r = np.asarray(queries, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    E = q.shape[1]
    if metric == 'cosine':
        return np.full((q.shape[0], r.shape[0]), (2 * E + 10) * U32)
    absdot = np.abs(q) @ np.abs(r).T
    norms = (q * q).sum(1)[:, None] + (r * r).sum(1)[None]
    return 2 * (E + 1) * U32 * absdot + (E + 1) * U32 * norms + 3 * U32 * (norms + 2 * absdot)
