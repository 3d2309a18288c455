"""Data shared by tests/test_evaluation_conformal_cpu.py and tests/test_gpu_evaluation_conformal.py: ``selective_cases.make_data`` plus the
adversarial columns of the radix select (keys that differ in one byte only, negatives, -0.0, denormals, non-finite values), tied rows,
probabilities with ties inside a row and a class without rows."""
import numpy as np
import torch

from selective_cases import feed, make_data  # noqa: F401  (feed is re-exported)

DEFAULT = ('lac', 'aps', 'raps', 'kan_abs', 'mu_abs', 'mu_scaled')
# name: (n, C, what is special, keyword arguments of conformal())
CASES = {
    'n1_c4': (1, 4, None, dict(alphas=(0.5, 0.1))),
    'n2_c2': (2, 2, None, dict(alphas=(0.1,))),
    'n9_c4': (9, 4, None, dict(alphas=(0.1, 0.05))),                             # k = 9: the largest score; k = 10 > 9: trivial
    'n19_c8': (19, 8, None, dict(alphas=(0.1,))),
    'n20_c4': (20, 4, None, dict(alphas=(0.1,), randomized=False)),
    'n255_c2': (255, 2, None, dict(alphas=(0.1, 0.05, 0.2), class_conditional=True)),
    'n256_c4_all_tied': (256, 4, 'tied', dict(alphas=(0.1,))),
    'n257_c8_two_decimals': (257, 8, 'rounded', dict(alphas=(0.1, 0.3), raps_lambda=0.05, raps_k=2)),
    'n1027_c4_class_absent': (1027, 4, 'absent', dict(alphas=(0.1, 0.05, 0.25), class_conditional=True)),
    'n4099_c4_columns': (4099, 4, 'columns', dict(alphas=(0.1, 0.01, 0.5), scores=('lac', 'aps', 'mu_scaled', 'low', 'high', 'wild', 'mu'))),
    'n4099_c8_class_conditional': (4099, 8, 'bad_rows', dict(alphas=(0.1, 0.2, 0.001), class_conditional=True)),
}


def adversarial_columns(n, seed):
    """'low': keys that differ in the lowest byte only.  'high': keys that differ in the highest byte only (both signs, from a denormal
    to 1e38; the exponent's last bit is 0, so every value is finite).  'wild': negatives, -0.0, +0.0, denormals, ties, and a few NaN
    and infinities, which the fit has to leave out and count."""
    rng = np.random.default_rng(seed)
    low = (np.uint32(0x3F800000) | rng.integers(0, 256, n, dtype=np.uint32)).view(np.float32)
    high = ((rng.integers(0, 256, n, dtype=np.uint32) << np.uint32(24)) | np.uint32(0x00123456)).view(np.float32)
    wild = (np.round(rng.standard_normal(n) * 4) / 4).astype(np.float32)
    special = np.array([-0.0, 0.0, 1e-40, -1e-42, 1.4e-45, -1.4e-45, np.nan, np.inf, -np.inf, np.nan], dtype=np.float32)
    at = rng.permutation(n)[:min(n, 3 * len(special))]
    wild[at] = np.resize(special, len(at))
    return {'low': torch.from_numpy(low.copy()), 'high': torch.from_numpy(high.copy()), 'wild': torch.from_numpy(wild)}


def make_case(name):
    """(data, extra column names, keyword arguments of ``conformal()``) of one case."""
    n, C, special, kw = CASES[name]
    d = make_data(n, C, seed=500 + n + C, ties=True)
    extra = ('mu',)
    if special == 'tied':
        for k in ('logits', 'sev_pred', 'mu', 'log_var'):
            d[k] = d[k][:1].expand(n, *d[k].shape[1:]).clone()
        d['labels'] = torch.full((n,), 2)
        d['sev_true'] = torch.full((n,), 1)
    if special == 'rounded':
        p = (torch.softmax(d['logits'], dim=1) * 100).round() / 100          # ties inside a row: the order falls back on the index
        d['logits'] = torch.log(p.clamp_min(1e-12))
    if special == 'absent':
        d['labels'] = torch.where(d['labels'] == 2, torch.zeros_like(d['labels']), d['labels'])
    if special == 'columns':
        d.update(adversarial_columns(n, seed=n))
        extra = ('mu', 'low', 'high', 'wild')
    if special == 'bad_rows':
        d['labels'][5], d['labels'][4000] = C, -3                             # left out everywhere
        d['log_var'][7] = float('inf')                                        # sigma = inf: out of 'mu_scaled' only
        d['mu'][9] = float('nan')                                             # out of both mu scores
        d['logits'][11] = float('nan')                                        # NaN probabilities: out of the class scores
    kw = dict(kw)
    kw.setdefault('scores', DEFAULT)
    return d, extra, kw


def held_out_rows(name, seed_shift=1):
    """Another draw of the same case's distribution: the test split of ``Conformal.evaluate``."""
    n, C, special, _ = CASES[name]
    d = make_data(n + 3, C, seed=900 + n + C + seed_shift, ties=True)
    if special == 'columns':
        d.update(adversarial_columns(n + 3, seed=n + 77))
    return d
