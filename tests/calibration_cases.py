"""Data shared by tests/test_evaluation_calibration_cpu.py and tests/test_gpu_evaluation_calibration.py: ``selective_cases.make_data`` with
scaled logits (an over- and an under-confident classifier), ``bootstrap_cases.exact_data`` with an uncertainty head, a plain bisection of
g to convergence, and the recorded columns of an accumulator in the shape ``calibration_block`` takes.  Everything is seeded."""
import math

import numpy as np
import torch

from bootstrap_cases import exact_data as _exact_data
from selective_cases import feed, make_data  # noqa: F401  (re-exported)

U_MAX = math.log(32.0)

# (n, C, seed, logit scale): the sizes and class counts of the issue, the logits as drawn, times 3 (over-confident) and divided by 3
# (under-confident).  Seed 500 is one whose first five rows put the root inside (1/32, 32) for every class count and scale (five rows that are
# mostly wrong sit at T = 32); the tests derive the status they expect from g at the two ends (``expected_status``).
CPU_CASES = [(n, C, 500 if n == 5 else 100 * n + C, s) for n in (5, 257, 1027) for C in (2, 4, 8) for s in (1.0, 3.0, 1.0 / 3.0)]


def scaled_data(n, C, seed, scale=1.0):
    d = make_data(n, C, seed)
    d['logits'] = d['logits'] * scale
    return d


def exact_case(n=600, C=4, seed=41):
    """``exact_data`` (probabilities 1/m and exact zeros, the same bits on every device) plus a mu and a log_var column."""
    d = _exact_data(n, C, seed)
    g = torch.Generator().manual_seed(seed + 7919)
    d['mu'] = d['sev_true'].float() + torch.randn(n, generator=g) * 0.6
    d['log_var'] = torch.randn(n, generator=g) * 0.5
    return d


def log_probs(probs):
    """max(log p, ln 2^-100) in fp64, written out again here so that the bisection shares no code with the module under test."""
    with np.errstate(divide='ignore'):
        return np.maximum(np.log(np.asarray(probs, dtype=np.float32).astype(np.float64)), -100.0 * math.log(2.0))


def g_of(l, y, u):
    w = np.exp(math.exp(u) * (l - l.max(axis=1, keepdims=True)))
    w = w / w.sum(axis=1, keepdims=True)
    return float(((w * l).sum(axis=1) - l[np.arange(len(y)), y]).sum())


def expected_status(l, y):
    """From g at the two ends of [-ln 32, ln 32] alone: g is non-decreasing in u = -ln T."""
    if g_of(l, y, -U_MAX) >= 0.0:
        return 'at_max'
    if g_of(l, y, U_MAX) < 0.0:
        return 'at_min'
    return 'interior'


def bisect_u(l, y, steps=200):
    """The root of g in [-ln 32, ln 32] by plain bisection, to convergence (200 halvings of a 6.9-wide bracket end at adjacent doubles)."""
    lo, hi = -U_MAX, U_MAX
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        if g_of(l, y, mid) >= 0.0:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


def recorded(acc):
    """(arrays, extras) of an accumulator's OWN record, device or CPU, for ``calibration_block`` / ``calibration_reference``."""
    extras = {k: acc._extra_column(k) for k in (acc._extra_names or ())}
    return acc.arrays(), extras
