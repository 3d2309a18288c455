"""Case generators of the Laplace tests (tests/test_laplace_cpu.py, tests/test_gpu_laplace.py): small heads, feature rows, the model's
own kind of logits, rows with a non-finite input, and the fp32 numpy evaluations that set the tolerances.

The tolerance rule (the one tests/test_gpu_corrupt.py uses): the error of an fp32 numpy evaluation of the same formulas against their
fp64 evaluation, maximum over a matrix, times four.  It is computed from the references alone, never from the code under test.
"""
import numpy as np

from rovit_hip import laplace as L


def head(E, hid, C, seed):
    """fc1 (hid, E), b1 (hid), last layer (C, hid), bias (C): fp32, scaled so the hidden units are O(1) and about half of them active."""
    g = np.random.default_rng(seed)
    return ((g.standard_normal((hid, E)) / np.sqrt(E)).astype(np.float32), (0.1 * g.standard_normal(hid)).astype(np.float32),
            (g.standard_normal((C, hid)) / np.sqrt(hid)).astype(np.float32), (0.1 * g.standard_normal(C)).astype(np.float32))


def features(n, E, seed):
    return np.random.default_rng(seed).standard_normal((n, E)).astype(np.float32)


def outputs(x, w1, b1, w2, b2, scale=3.0):
    """The last layer's outputs on the rows x, fp32 (evaluated in fp64): logits of some spread for a classification head."""
    a = L.augmented_hidden(x, w1, b1)
    return (scale * (a[:, :-1] @ w2.astype(np.float64).T + b2.astype(np.float64)[None])).astype(np.float32)


def with_bad_rows(x, lg, seed):
    """Copies with a non-finite feature in some rows and a non-finite logit in others (and both in one, when there is room)."""
    x, lg = x.copy(), lg.copy()
    n = x.shape[0]
    g = np.random.default_rng(seed)
    if n >= 4:
        rows = g.choice(n, size=min(n, 4), replace=False)
        x[rows[0], g.integers(x.shape[1])] = np.nan
        x[rows[1], g.integers(x.shape[1])] = np.inf
        lg[rows[2], g.integers(lg.shape[1])] = -np.inf
        lg[rows[3], g.integers(lg.shape[1])] = np.nan
        x[rows[3], 0] = np.nan
    else:
        x[0, 0] = np.nan
    return x, lg


def gram_fp32(x, w1, b1, w):
    """rovit_laplace_gram's formulas evaluated by numpy in fp32 over the valid rows: (K, D, D)."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32).reshape(x.shape[0], -1)
    valid = np.isfinite(x).all(axis=1) & np.isfinite(w).all(axis=1)
    a = L.augmented_hidden(x[valid], w1, b1, dtype=np.float32)
    return np.stack([a.T @ (a * w[valid, k][:, None]) for k in range(w.shape[1])])


def predict_fp32(x, w1, b1, W, C):
    """rovit_laplace_predict's logit_cov evaluated by numpy in fp32: (B, C, C)."""
    a = L.augmented_hidden(x, w1, b1, dtype=np.float32)
    W = np.asarray(W, np.float32)
    P = W.shape[0] // C
    ap = np.zeros((a.shape[0], P), dtype=np.float32)
    ap[:, :a.shape[1]] = a
    z = np.stack([ap @ W[:, c * P:(c + 1) * P].T for c in range(C)], axis=1)
    return np.einsum('bct,bdt->bcd', z, z)


def tolerance(fp32_value, fp64_value, axes):
    """Four times the largest error of the fp32 evaluation over ``axes``, kept broadcastable against the values."""
    return 4.0 * np.abs(np.asarray(fp32_value, np.float64) - fp64_value).max(axis=axes, keepdims=True)


def splits_of(n, parts, seed):
    """Row boundaries [0, ..., n] of ``parts`` uneven pieces."""
    if n < parts:
        return [0, n]
    cuts = np.sort(np.random.default_rng(seed).choice(np.arange(1, n), size=parts - 1, replace=False))
    return [0] + [int(c) for c in cuts] + [n]
