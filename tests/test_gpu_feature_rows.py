"""GPU test of the row scan the feature-space kernels share (csrc/feature_tiles.h: row_scan): the kNN index build, k-means and t-SNE
agree on which rows exist, and that set is the numpy statement of the rule evaluated in fp32.

The rule.  s = the squared norm of the fp32 row as one fp32 fma chain in ascending feature index; a row is good when every feature is
finite, s is finite and, with 'cosine', s > 0.  Hence of the hard rows below the all-zero row and the row of subnormals (its products
underflow: s = 0) are valid with 'l2' and absent with 'cosine'; the rows with a NaN, with +inf and of 1e20 entries (s overflows) are
absent with both.  n = 70 rows: the scan is a thread per row, so the rows cross a wave, and the hard rows sit on both sides of it.

Each module reports through what it already has: the index its counts and what a search of the rows themselves returns (a row that
exists finds itself), k-means the label -1 and the status counts, t-SNE the rows and columns of P that are all zero (P_ij >= 1e-12
between valid rows) and its status counts.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rovit_hip import clustering as cl  # noqa: E402
from rovit_hip import embedding as EM  # noqa: E402
from rovit_hip import neighbors as NB  # noqa: E402

pytestmark = pytest.mark.gpu

N, E = 70, 32
NAN_ROW, INF_ROW, ZERO_ROW, HUGE_ROW, TINY_ROW = 3, 20, 63, 64, 69


def rows():
    x = np.random.default_rng(2024).standard_normal((N, E)).astype(np.float32)
    x[NAN_ROW, 5] = np.nan
    x[INF_ROW, 31] = np.inf
    x[ZERO_ROW] = 0.0
    x[HUGE_ROW] = 1e20                                             # finite features, 32e40 overflows fp32
    x[TINY_ROW] = 1e-40                                            # subnormals: every product underflows to 0
    return x


def good_rows(x, metric):
    """The rule in numpy: the fma chain in fp32 (a product of two fp32 values is exact in fp64; the sum is rounded to fp32 each step)."""
    s = np.zeros(x.shape[0], dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for e in range(x.shape[1]):
            s = (x[:, e].astype(np.float64) ** 2 + s.astype(np.float64)).astype(np.float32)
    good = np.isfinite(x).all(axis=1) & np.isfinite(s)
    return good & (s > 0) if metric == 'cosine' else good


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda:0'))


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_the_three_consumers_of_the_row_scan_agree_on_which_rows_exist(metric):
    x = rows()
    want = good_rows(x, metric)
    absent = {NAN_ROW, INF_ROW, HUGE_ROW} | ({ZERO_ROW, TINY_ROW} if metric == 'cosine' else set())
    assert set(np.flatnonzero(~want).tolist()) == absent            # the statement says what the issue says

    fi = NB.FeatureIndex(E, None, metric, capacity=N)
    fi.update(cuda(x))
    fi.build()
    knn = fi.search(cuda(x), k=1)['indices'].cpu().numpy()[:, 0] != -1   # a row that exists finds itself, a row that does not finds nothing
    assert fi.counts() == {'n': N, 'n_valid': int(knn.sum()), 'bad_rows': int((~knn).sum())}

    km = cl.KMeans(3, metric=metric, max_iter=2, seed=1).fit(cuda(x))
    kmeans = km.labels_.cpu().numpy() != -1
    st = km.status_
    assert (st['n'], st['n_valid'], st['bad_rows']) == (N, int(kmeans.sum()), int((~kmeans).sum()))

    out = EM.TSNE(perplexity=5.0, metric=metric).affinities(cuda(x))
    P = out['P'].cpu().numpy()
    tsne = (P != 0).any(axis=1)
    assert np.array_equal(tsne, (P != 0).any(axis=0))
    status = EM.decode_status(out['status'])
    assert (status['n'], status['n_valid'], status['bad_rows']) == (N, int(tsne.sum()), int((~tsne).sum()))

    print(f'feature rows {metric}: valid {int(want.sum())} of {N}; absent kNN {np.flatnonzero(~knn).tolist()}, '
          f'k-means {np.flatnonzero(~kmeans).tolist()}, t-SNE {np.flatnonzero(~tsne).tolist()}')
    assert np.array_equal(knn, kmeans) and np.array_equal(kmeans, tsne)
    assert np.array_equal(knn, want)
