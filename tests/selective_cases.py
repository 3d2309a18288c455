"""Data shared by tests/test_evaluation_selective_cpu.py and tests/test_gpu_evaluation_selective.py: ``bootstrap_cases.make_data`` plus the
uncertainty head's ``mu`` and ``log_var`` columns, a ``feed`` that passes them, and the brute-force tie average the definitions rest on."""
import itertools

import numpy as np
import torch

from bootstrap_cases import make_data as _make_data


def make_data(n, C, seed, ties=False):
    """``bootstrap_cases.make_data`` with ``mu`` (the severity plus noise) and ``log_var`` (larger where mu is further off, plus noise;
    rounded to one decimal with ``ties``, so sigma has tie groups)."""
    d = _make_data(n, C, seed, ties)
    g = torch.Generator().manual_seed(seed + 7919)
    d['mu'] = d['sev_true'].float() + torch.randn(n, generator=g) * 0.6
    d['log_var'] = torch.log((d['mu'] - d['sev_true'].float()).abs() + 0.1) + torch.randn(n, generator=g) * 0.5
    if ties:
        d['log_var'] = (d['log_var'] * 10).round() / 10
    return d


def feed(acc, d, sizes=(1 << 30,), device=None, extra=('mu',)):
    """Record ``d`` in batches of ``sizes`` (cycled) on ``device`` (None: the CPU path) with ``mu`` and ``log_var`` in the outputs and
    the columns named in ``extra`` (keys of ``d``) as extra columns."""
    to = (lambda t: t) if device is None else (lambda t: t.to(device))
    i, k, n = 0, 0, d['logits'].shape[0]
    while i < n:
        j = min(n, i + sizes[k % len(sizes)])
        k += 1
        out = {'cls_logits': to(d['logits'][i:j]), 'kan_severity': to(d['sev_pred'][i:j].reshape(-1, 1)),
               'mu': to(d['mu'][i:j].reshape(-1, 1)), 'log_var': to(d['log_var'][i:j].reshape(-1, 1))}
        acc.update(out, to(d['labels'][i:j]), to(d['sev_true'][i:j]),
                   extra={name: to(d[name][i:j].reshape(-1, 1)) for name in extra} if extra else None)
        i = j
    return acc


def brute_force_risks(u, l):
    """r_1..r_n as the plain average, over EVERY order of the rows that is ascending in ``u``, of the mean risk of the first k rows."""
    u, l = np.asarray(u), np.asarray(l, dtype=np.float64)
    n = len(u)
    total, count = np.zeros(n), 0
    for perm in itertools.permutations(range(n)):
        us = u[list(perm)]
        if np.all(us[:-1] <= us[1:]):
            total += np.cumsum(l[list(perm)]) / np.arange(1, n + 1)
            count += 1
    return total / count
