"""Makers, bounds and recorded seeds shared by tests/test_kmeans_cpu.py and tests/test_gpu_kmeans.py (no test in here)."""
import numpy as np

from density_cases import make
from neighbors_cases import integer_rows  # noqa: F401  (every l2 distance of these rows is an integer, exact in fp32)

U32 = 2.0 ** -24

# (n, E, C, data seed) of the float cases of the whole-run tests, k = C = 4
FLOAT_CASES = [(257, 192, 4, 0), (257, 32, 4, 0), (65, 32, 4, 0), (1025, 192, 4, 0)]

# KMeans seeds chosen with fit_reference (Philox streams), per (float case, metric): one whose run recovers the four planted classes
# (ARI 1) and one that stops in a local optimum that splits a class (ARI about 0.6); None where no seed in 0..11 met the conditions.
# tests/test_kmeans_cpu.py asserts both properties, the margin condition (no row under 2 x bound in any assign of the run) and that no
# seeding pick lies within 1e-4 W of a boundary of the cumulative weights (the device's fp32 distances move them by less).
RECOVERING_SEED = {((257, 192, 4, 0), 'l2'): 1, ((257, 32, 4, 0), 'l2'): 0, ((65, 32, 4, 0), 'l2'): 0, ((1025, 192, 4, 0), 'l2'): 4,
                   ((257, 192, 4, 0), 'cosine'): 1, ((257, 32, 4, 0), 'cosine'): 11, ((65, 32, 4, 0), 'cosine'): 2,
                   ((1025, 192, 4, 0), 'cosine'): 5}
LOCAL_OPTIMUM_SEED = {((257, 192, 4, 0), 'l2'): 11, ((257, 32, 4, 0), 'l2'): 3, ((65, 32, 4, 0), 'l2'): 5, ((1025, 192, 4, 0), 'l2'): 1,
                      ((257, 192, 4, 0), 'cosine'): None, ((257, 32, 4, 0), 'cosine'): 0, ((65, 32, 4, 0), 'cosine'): 3,
                      ((1025, 192, 4, 0), 'cosine'): None}
# the n_init = 3 test: on RESTART_CASE with 'l2' the three restarts of this seed end in inertias 402.3, 299.7, 386.4: restart 1 is kept
RESTART_CASE, RESTART_SEED, RESTART_KEPT = (65, 32, 4, 0), 24, 1


def run_cases():
    """(case, metric, seed, recovers) of every recorded whole run."""
    out = []
    for table, recovers in ((RECOVERING_SEED, True), (LOCAL_OPTIMUM_SEED, False)):
        out += [(case, metric, seed, recovers) for (case, metric), seed in table.items() if seed is not None]
    return out


def float_rows(case):
    n, E, C, seed = case
    return make(n, E, C, seed)


def distance_bound(features, centroids, metric='l2'):
    """(n,) bound on |device fp32 distance - fp64 distance| of every row against any of the centroids: (E + 3) 2^-24 (|x| + |c|max)^2.
    Three fma chains of E terms each (the two squared norms and the cross term, Cauchy-Schwarz on the latter: |x.c| <= |x| |c|) give
    E 2^-24 (|x|^2 + |c|^2 + 2 |x| |c|), and the three combining roundings (the sum of the norms, the doubling is exact, the
    difference, and with 'cosine' the two normalisations instead of the norms) 3 2^-24 of the same magnitude.  With 'cosine' the rows
    and the centroids have unit length."""
    x, c = np.asarray(features, dtype=np.float64), np.asarray(centroids, dtype=np.float64)
    E = x.shape[1]
    if metric == 'cosine':
        nx, nc = np.ones(x.shape[0]), 1.0
    else:
        nx, nc = np.sqrt((x * x).sum(1)), float(np.sqrt((c * c).sum(1)).max())
    return (E + 3) * U32 * (nx + nc) ** 2


def duplicate_rows(n, E, seed):
    """n copies of one integer row: every distance is 0 and the seeding takes the W = 0 path from seed 1 on."""
    return np.repeat(integer_rows(1, E, seed), n, axis=0)


# (n, E, k) of the assignment tests: the smallest shapes at which the tiles can go wrong (row tiles of 64, centroid tiles of 64 and
# their 32-wide halves, one and several workgroups), k <= n
ASSIGN_SHAPES = [(1, 32, 1), (5, 32, 2), (5, 192, 4), (63, 32, 31), (64, 192, 32), (65, 256, 33), (257, 192, 64), (257, 32, 65),
                 (257, 256, 256), (1025, 192, 4), (1025, 32, 65), (1025, 256, 2)]


def assign_case(n, E, k, metric, seed=1):
    """Float rows and k centroids taken from k distinct rows (unit length, rounded once, with 'cosine').  tests/test_kmeans_cpu.py
    asserts that with this data seed no shape leaves out more than 1 % of its rows."""
    x, _ = make(n, E, 4, seed)
    pick = np.random.default_rng(seed + 7).permutation(n)[:k]
    c = x[pick].astype(np.float64)
    if metric == 'cosine':
        c = c / np.sqrt((c * c).sum(1, keepdims=True))
    return x, c.astype(np.float32)


def integer_assign_case(n, E, k, seed=0):
    """Integer rows with small entries (heavy distance ties) and centroids taken from the first k rows, some of them twice."""
    x = integer_rows(n, E, seed)
    c = x[np.arange(k) % max(1, (k + 1) // 2)].copy()              # duplicates: equal distances to two cluster indices
    return x, c
