"""Columns shared by tests/test_rank_cpu.py, tests/test_gpu_rank.py and tests/test_gpu_rank_consumers.py: the contents and sizes at
which a radix sort can go wrong (ties, one bucket, one digit, the specials, NaNs), the brute-force O(n^2) statement of the ranks, and the
wide selective case."""
import numpy as np
import torch

TILE = 2048                                     # ROVIT_SORT_TILE (asserted against native.SORT_TILE by the tests)
# 1, 2, around the 256-row chunk, around one tile, two tiles + 1, and a column of more than 32 tiles
SIZES = (1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 65537)
CPU_SIZES = (1, 2, 255, 256, 257, 300)

NEG_NAN, PAYLOAD_NAN = 0xFFC00000, 0x7F800001   # a negative quiet NaN and a positive NaN with the smallest payload


def _bits(a):
    return np.asarray(a, dtype=np.uint32).view(np.float32)


def _one_byte(byte):
    def make(n, rng):
        r = rng.integers(0, 256, n).astype(np.uint32)
        if byte < 3:
            return _bits(np.uint32(0x40000000) | (r << np.uint32(8 * byte)))       # positive floats, the key is the bits with bit 31 set
        return _bits((r << np.uint32(24)) | np.uint32(0x00400000))                  # both signs, exponent at most 0xFE: finite
    return make


def _specials(n, rng):
    pool = np.concatenate([_bits([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000]),
                           np.float32([-1.5, -1e-30, 1e-30, 2.0, -3.4e38, 3.4e38])])
    return pool[rng.integers(0, len(pool), n)]


def _nans(n, rng):
    x = (rng.standard_normal(n) * 4).round(1).astype(np.float32)
    x[0] = np.float32('nan')
    x[n - 1] = _bits([NEG_NAN])[0]
    x[n // 2] = _bits([PAYLOAD_NAN])[0]
    if n > 8:
        x[n // 3] = -np.float32(0.0)
        x[n // 3 + 1] = np.float32(0.0)
    return x


CONTENTS = {
    'distinct': lambda n, rng: (rng.permutation(n).astype(np.float32) - np.float32(n // 2)),
    'all_equal': lambda n, rng: np.full(n, 1.5, dtype=np.float32),
    'two_values': lambda n, rng: rng.integers(0, 2, n).astype(np.float32),
    'two_decimals': lambda n, rng: rng.standard_normal(n).round(2).astype(np.float32),
    'ascending': lambda n, rng: np.sort(rng.standard_normal(n).round(3).astype(np.float32)),
    'descending': lambda n, rng: np.sort(rng.standard_normal(n).round(3).astype(np.float32))[::-1].copy(),
    'byte0': _one_byte(0), 'byte1': _one_byte(1), 'byte2': _one_byte(2), 'byte3': _one_byte(3),
    'specials': _specials,
    'nans': _nans,
}


def column(content, n, seed=0):
    """The fp32 column of ``n`` rows with the named content; a function of (content, n, seed)."""
    rng = np.random.default_rng([seed, n, sorted(CONTENTS).index(content)])
    x = np.ascontiguousarray(CONTENTS[content](n, rng), dtype=np.float32)
    assert x.shape == (n,)
    return x


def brute_force_ranks(x):
    """less, eq and before by their O(n^2) definitions with fp32 compares (a NaN compares false), as int64."""
    x = np.asarray(x, dtype=np.float32)
    lt = x[None, :] < x[:, None]                  # [i, j]: x_j < x_i
    eq = x[None, :] == x[:, None]
    earlier = np.tri(len(x), k=-1, dtype=bool)    # [i, j]: j < i
    return lt.sum(1).astype(np.int64), eq.sum(1).astype(np.int64), (eq & earlier).sum(1).astype(np.int64)


def u32(t):
    """An int32 tensor of the library as a uint32 numpy array."""
    return t.detach().cpu().numpy().view(np.uint32)


WIDE = (['confidence', 'entropy', 'sigma', 'mu', 'c1', 'c2', 'c3', 'c4'], ['error', 'abs_err', 'mu_abs_err', 'r3'])


def add_wide_columns(d, n):
    """Four extra score columns with negative keys, -0.0 and ties, and a fourth risk; returns the names of the extra columns to feed."""
    g = torch.Generator().manual_seed(n)
    for k in range(1, 5):
        d[f'c{k}'] = (torch.randn(n, generator=g) * k).round() / k
    d['c1'][::7] = -0.0
    d['c1'][3::7] = 0.0
    d['r3'] = torch.rand(n, generator=g) * 7
    return ('c1', 'c2', 'c3', 'c4', 'r3', 'mu')
