"""Data makers and error bounds shared by tests/test_tsne_cpu.py and tests/test_gpu_tsne.py (no test in here)."""
import functools

import numpy as np
import torch

from density_cases import make
from neighbors_cases import integer_rows  # noqa: F401  (re-exported for the GPU tests)

from rovit_hip import embedding as EM

U32 = 2.0 ** -24

PERPLEXITY_CASES = [(5, 2.0), (65, 2.0), (65, 5.0), (65, 15.0), (257, 2.0), (257, 5.0), (257, 15.0), (257, 80.0)]
STEP_CASES = [(n, s, alpha, m) for n in (5, 65, 257) for s in (1e-4, 10.0) for alpha, m in ((12.0, 0.5), (1.0, 0.8))]
STEP_ETA = 50.0                                  # max(n / 12 / 4, 50) at every n of STEP_CASES


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def float_rows(n: int, E: int):
    return frozen(make(n, E, 4, seed=n + E)[0])


@functools.lru_cache(maxsize=None)
def duplicate_rows():
    """40 copies of one row followed by 25 rows of ``make``: 65 rows of 32 features.  (The seed is one at which the copied row is the nearest
    neighbour of no other row: such a row sees 40 equal smallest distances and is unconverged too, by the same definition.)"""
    x = make(26, 32, 4, seed=13)[0]
    return frozen(np.concatenate([np.repeat(x[:1], 40, axis=0), x[1:]], axis=0))


@functools.lru_cache(maxsize=None)
def step_case(n: int, s: float):
    """P from the oracle on ``make`` rows (perplexity 5; 2 at n = 5), Y ~ N(0, s^2), V ~ 0.1 s N(0, 1), G = 1, all fp32-representable."""
    P = EM.affinities_reference(float_rows(n, 32), 2.0 if n == 5 else 5.0)['P'].astype(np.float32)
    rng = np.random.default_rng(1000 + n)
    Y = (s * rng.standard_normal((n, 2))).astype(np.float32)
    V = (0.1 * s * rng.standard_normal((n, 2))).astype(np.float32)
    return frozen(P, Y, V, np.ones((n, 2), dtype=np.float32))


def gradient_bound(ref, n: int, alpha: float) -> np.ndarray:
    """Per gradient component: 4 (n + 16) u (sum |attraction terms| + 2 sum |repulsion terms| / Z), the attraction terms with their alpha."""
    return 4.0 * (n + 16) * U32 * (alpha * ref['abs_a'] + 2.0 * ref['abs_r'] / ref['Z'])


@functools.lru_cache(maxsize=None)
def step_reference(n: int, s: float, alpha: float, m: float):
    P, Y, V, G = step_case(n, s)
    return EM.step_reference(P, Y, V, G, alpha, m, STEP_ETA)


@functools.lru_cache(maxsize=None)
def whole_run():
    """make(257, 192, 4, seed=0), perplexity 15, 300 iterations of which 100 exaggerated, the 'pca' init of the oracle: rows, labels,
    the oracle's P, the init and the oracle's run."""
    x, y = make(257, 192, 4, seed=0)
    P = EM.affinities_reference(x, 15.0)['P']
    Y0 = EM.pca_init(torch.from_numpy(x)).numpy()
    run = EM.run_reference(P, Y0.astype(np.float64), 300, 12.0, 100, 'auto', 50)
    frozen(x, y, P, Y0, run['map'], run['kl_trace'])
    return x, y, P, Y0, run


def purity(Y: np.ndarray, labels: np.ndarray, k: int = 10) -> float:
    """The share of each row's k nearest map neighbours (fp64, itself excluded) that carry the row's label."""
    Y = np.asarray(Y, dtype=np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind='stable')[:, :k]
    return float((labels[nn] == labels[:, None]).mean())


def knn_sets(rows: np.ndarray, k: int) -> np.ndarray:
    rows = np.asarray(rows, dtype=np.float64)
    d = ((rows[:, None, :] - rows[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind='stable')[:, :k]


def knn_overlap(features: np.ndarray, Y: np.ndarray, k: int) -> float:
    """The mean overlap of the k nearest neighbours in feature space and in the map, by a numpy count in fp64."""
    a, b = knn_sets(features, k), knn_sets(Y, k)
    return sum(len(set(a[i]) & set(b[i])) for i in range(a.shape[0])) / float(a.shape[0] * k)
