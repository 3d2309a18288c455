"""Case generators of the influence tests (tests/test_influence_cpu.py, tests/test_gpu_influence.py): fitted heads with their whitening
tables, recorded rows with labels and a few bad ones, integer-valued search problems, and the fp32 numpy evaluations that set the
tolerances (the rule of tests/laplace_cases.py: four times the error of an fp32 evaluation of the same formulas against fp64, computed
from the references alone, never from the code under test).
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import laplace_cases as cases
from rovit_hip import influence as I
from rovit_hip import laplace as L


@functools.lru_cache(maxsize=None)
def fitted_head(E, hid, C, n_fit=200, tau=1.0):
    """A head (fc1, b1, last layer, bias), the rows its Laplace fit was made on and the fit (``laplace_reference``): C > 1 a
    classification head, C = 1 the Gaussian head (its ``outputs`` are log_var; mu comes from ``mu_head``)."""
    w1, b1, w2, b2 = cases.head(E, hid, C, seed=E + hid + C)
    x = cases.features(n_fit, E, seed=C + 11)
    out = cases.outputs(x, w1, b1, w2, b2, scale=3.0 if C > 1 else 1.0)
    theta = np.concatenate([w2.ravel(), b2])
    fit = L.laplace_reference(x, out, w1, b1, theta, tau) if C > 1 else L.laplace_reference(x, None, w1, b1, theta, tau, log_var=out[:, 0])
    for a in (w1, b1, w2, b2, fit['whitening']):
        a.setflags(write=False)
    return w1, b1, w2, b2, fit


def recorded(n, E, hid, C, seed, bad=True):
    """n rows for the head ``fitted_head(E, hid, C)``: features, and for C > 1 logits and labels (the argmax, a fifth of them moved), for
    C = 1 mu, log_var and severity.  With ``bad`` and n >= 4 a few rows carry a non-finite input or a label outside the range."""
    w1, b1, w2, b2, _ = fitted_head(E, hid, C)
    g = np.random.default_rng(seed)
    x = cases.features(n, E, seed=seed + 1)
    out = cases.outputs(x, w1, b1, w2, b2, scale=3.0 if C > 1 else 1.0)
    if C > 1:
        y = out.argmax(axis=1).astype(np.int32)
        move = g.random(n) < 0.2
        y[move] = (y[move] + 1 + g.integers(C - 1, size=int(move.sum()))) % C
        cols = {'cls_logits': out, 'labels': y}
        if bad and n >= 4:
            x, out = cases.with_bad_rows(x, out, seed)
            cols['cls_logits'] = out
            rows = g.choice(n, size=2, replace=False)
            y[rows[0]], y[rows[1]] = C, -1
    else:
        mu = (0.5 * g.standard_normal(n) + 1.5).astype(np.float32)
        sev = g.integers(0, 4, size=n).astype(np.float32)
        cols = {'mu': mu, 'log_var': out[:, 0].copy(), 'severity': sev}
        if bad and n >= 4:
            rows = g.choice(n, size=4, replace=False)
            x[rows[0], 0] = np.nan
            cols['mu'][rows[1]] = np.inf
            cols['log_var'][rows[2]] = -200.0                      # exp(200) is not finite in fp32
            cols['severity'][rows[3]] = np.nan
    return x, cols


def embed_fp32(x, w1, b1, W, C, residual):
    """rovit_influence_embed's rows evaluated by numpy in fp32 from the fp32 residual: (n, C P); rows with a NaN residual are zeros."""
    x = np.asarray(x, np.float32)
    good = np.isfinite(x).all(axis=1) & np.isfinite(residual).all(axis=1)
    a = L.augmented_hidden(np.where(np.isfinite(x), x, 0), w1, b1, dtype=np.float32)
    W = np.asarray(W, np.float32)
    P = W.shape[0] // C
    g = np.zeros((x.shape[0], C, P), dtype=np.float32)
    g[:, :, :a.shape[1]] = np.where(good[:, None], residual, 0).astype(np.float32)[:, :, None] * a[:, None, :]
    g[~good] = 0
    return g.reshape(x.shape[0], C * P) @ W.T


def embed_case(n, E, hid, C, head=None, target='loss', bad=True, seed=None):
    """(x, cols, reference, tolerance): ``embed_reference`` of ``recorded`` rows and four times the largest error of ``embed_fp32``."""
    head = head or ('cls' if C > 1 else 'mu')
    w1, b1, _, _, fit = fitted_head(E, hid, C)
    x, cols = recorded(n, E, hid, C, seed if seed is not None else n + C, bad)
    ref = I.embed_reference(x, w1, b1, fit['whitening'], C, head, target, **cols)
    u32 = embed_fp32(x, w1, b1, fit['whitening'], C, ref['residual'])
    u32[~ref['valid']] = 0
    tol = float(cases.tolerance(u32, ref['rows'], (0, 1)).max())
    return x, cols, ref, tol


def lin(i, o, w, b, device):
    m = torch.nn.Linear(i, o)
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(np.array(w).reshape(o, i)))
        m.bias.copy_(torch.from_numpy(np.array(b)))
    return m.to(device)


def fitted_laplace(E, hid, C, device, gaussian=True, tau=1.0):
    """A fitted ``HeadLaplace`` on ``device`` over the heads of ``fitted_head(E, hid, C)`` and, with ``gaussian``, ``fitted_head(E, hid,
    1)``, on the rows those were fitted on."""
    w1, b1, w2, b2, _ = fitted_head(E, hid, C)
    u1, c1, u2, c2, _ = fitted_head(E, hid, 1)
    heads = (SimpleNamespace(fc1=lin(E, hid, w1, b1, device), fc2=lin(hid, C, w2, b2, device)),
             SimpleNamespace(fc1=lin(E, hid, u1, c1, device), fc_mu=lin(hid, 1, u2, c2, device)) if gaussian else None)
    la = L.HeadLaplace(heads, capacity=64)
    x = cases.features(200, E, seed=C + 11)
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    la.update(on(x), on(cases.outputs(x, w1, b1, w2, b2)), on(cases.outputs(x, u1, c1, u2, c2, scale=1.0)) if gaussian else None)
    return la.fit(tau)


def integer_rows(n, B, dim, seed, invalid=True):
    """Rows and queries with integer entries in [-3, 3] (every dot product is exact in fp32 and ties abound), their exact squared norms,
    and validity flags: with ``invalid`` and n >= 4 a tenth of the rows (at least one) are invalid and stored as zeros, as an embed leaves
    them."""
    g = np.random.default_rng(seed)
    rows = g.integers(-3, 4, size=(n, dim)).astype(np.float32)
    q = g.integers(-3, 4, size=(B, dim)).astype(np.float32)
    valid = np.ones(n, dtype=np.int32)
    if invalid and n >= 4:
        valid[g.choice(n, size=max(1, n // 10), replace=False)] = 0
    valid[~(rows != 0).any(axis=1)] = 0
    rows[valid == 0] = 0
    return q, rows, (rows.astype(np.float64) ** 2).sum(axis=1).astype(np.float32), valid


def auroc(score, positive):
    """P(score of a positive > score of a negative) + half the ties, by ranks."""
    s, p = np.asarray(score, dtype=np.float64), np.asarray(positive, dtype=bool)
    order = np.argsort(s, kind='stable')
    ranks = np.empty(len(s))
    ranks[order] = np.arange(1, len(s) + 1)
    for v in np.unique(s):
        tie = s == v
        if tie.sum() > 1:
            ranks[tie] = ranks[tie].mean()
    n1, n0 = p.sum(), (~p).sum()
    return (ranks[p].sum() - n1 * (n1 + 1) / 2) / (n1 * n0)
