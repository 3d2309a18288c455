"""Data makers shared by tests/test_density_cpu.py and tests/test_gpu_density.py (no test in here)."""
import numpy as np


def make(n: int, E: int, C: int, seed: int):
    """(n, E) fp32 feature rows and (n,) int64 labels that look like the backbone's: class means of norm 3, Gaussian noise through a random
    orthogonal basis with covariance eigenvalues from 1 down to 1e-3, then every row's own mean subtracted: the LayerNorm-like singular
    direction (the rows lie in a hyperplane, so the covariance is singular without shrinkage).  The first min(n, C) labels are 0 .. C - 1,
    so that no class is empty when n >= C."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((C, E))
    mu *= 3.0 / np.linalg.norm(mu, axis=1, keepdims=True)
    Q, _ = np.linalg.qr(rng.standard_normal((E, E)))
    ev = np.geomspace(1.0, 1e-3, E)
    labels = rng.integers(0, C, n)
    labels[:min(n, C)] = np.arange(min(n, C))
    rows = mu[labels] + (rng.standard_normal((n, E)) * np.sqrt(ev)[None]) @ Q.T
    rows -= rows.mean(axis=1, keepdims=True)
    return rows.astype(np.float32), labels.astype(np.int64)


def with_bad_labels(labels: np.ndarray, C: int, seed: int, share: float = 0.05) -> np.ndarray:
    """A copy with about ``share`` of the labels (never one of the first C) set to -1, C or C + 3: rows the fit must leave out."""
    rng = np.random.default_rng(seed + 1000)
    out = labels.copy()
    pick = np.nonzero(rng.random(labels.shape[0]) < share)[0]
    pick = pick[pick >= C]
    out[pick] = rng.choice([-1, C, C + 3], size=pick.shape[0])
    return out


def logits(n: int, C: int, seed: int) -> np.ndarray:
    """(n, C) fp32 logits with a spread of a few units and some confident rows."""
    rng = np.random.default_rng(seed + 2000)
    l = rng.standard_normal((n, C)) * 2.0
    l[::7] *= 6.0
    return l.astype(np.float32)


def score_populations(n_in: int, n_out: int, kind: str, seed: int):
    """Two fp32 score populations: 'ties' (rounded to one decimal: heavy ties inside and across the populations), 'equal' (every score the
    same) and 'separated' (every out score above every in score)."""
    rng = np.random.default_rng(seed + 3000)
    if kind == 'ties':
        a, b = np.round(rng.standard_normal(n_in), 1), np.round(rng.standard_normal(n_out) + 0.7, 1)
    elif kind == 'equal':
        a, b = np.full(n_in, 0.25), np.full(n_out, 0.25)
    elif kind == 'separated':
        a, b = rng.random(n_in), 2.0 + rng.random(n_out)
    else:
        raise ValueError(kind)
    return a.astype(np.float32), b.astype(np.float32)


def sorted_definitions(a: np.ndarray, b: np.ndarray, level: float = 0.95):
    """AUROC, the two average precisions and FPR@TPR straight from their sort-based definitions in fp64, tied scores entering a threshold
    together: the independent statement the counting formulas are checked against."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    auroc = ((b[:, None] > a[None]).sum() + 0.5 * (b[:, None] == a[None]).sum()) / (a.size * b.size)

    def average_precision(pos, neg):
        # detector "score >= t": at each distinct threshold (descending) precision = TP / (TP + FP), weighted by the recall step
        total = 0.0
        for t in np.unique(pos)[::-1]:
            tp, fp = (pos >= t).sum(), (neg >= t).sum()
            total += (pos == t).sum() * tp / (tp + fp)
        return total / pos.size
    aupr_out = average_precision(b, a)
    aupr_in = average_precision(-a, -b)
    k = min(max(int(np.ceil(level * a.size)), 1), a.size)
    t = np.sort(a)[k - 1]
    return {'auroc': float(auroc), 'aupr_out': float(aupr_out), 'aupr_in': float(aupr_in), 'threshold': float(t), 'fpr': float((b <= t).mean())}
