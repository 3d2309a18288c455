"""GPU tests of csrc/neighbors.hip through rovit_hip.neighbors: the fused k-nearest-neighbour search against the numpy fp64 statements
(bit for bit where fp32 is exact, within derived bounds elsewhere), its determinism, exclude, bad rows, the vote, and the model /
Evaluator entry points end to end.

Measured on the MI355X over the cases below (printed by the tests before they assert):
  distances  max |d - d_ref| / derived bound = 1.387e-01 (N = 1000, E = 32, l2, k = 32; 1.2e-02 .. 1.4e-01 over the 30 cases: the bound is
             a worst case over E roundings of one sign, and E = 32 leaves the least room for them to cancel)
  decided    the smallest share of decided queries = 0.942 (N = 5197, E = 192, l2, k = 32); it depends on the data (density_cases.make with
             seed N + E + C) and the bound alone, not on the device
  end to end: kNN AUROC of Gaussian-noise images against the 48 recorded images = 0.7804
"""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbors_cases as cases  # noqa: E402
from oracle import ref_cpu  # noqa: E402  (checker only)

from rovit_hip import neighbors as NB  # noqa: E402

pytestmark = pytest.mark.gpu

# The largest error / bound the MI355X gave over the bounded cases of this file (None: not measured yet, the derived bounds alone then hold).
MEASURED_DISTANCE_RATIO = 1.387e-01

FLOAT_CASES = [(33, 32, 2), (1000, 32, 4), (1000, 192, 4), (5197, 192, 4), (1000, 256, 8)]
QUERIES = 257


def dev():
    return torch.device('cuda:0')


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(out):
    return {name: t.cpu().numpy() for name, t in out.items()}


def make_index(rows, metric, labels=None, severity=None, num_classes=None, edges=None, max_workgroups=0):
    fi = NB.FeatureIndex(rows.shape[1], num_classes, metric, capacity=64)
    fi.max_workgroups = max_workgroups
    edges = [0, rows.shape[0]] if edges is None else edges
    for r0, r1 in zip(edges[:-1], edges[1:]):
        fi.update(cuda(rows[r0:r1]), None if labels is None else cuda(labels[r0:r1]), None if severity is None else cuda(severity[r0:r1]))
    return fi.build()


def check_order(got, n):
    """Ascending in the device's own key (bits(d) << 32) | j, valid slots first, distinct indices inside [0, n)."""
    d, idx = got['distances'], got['indices'].astype(np.int64)
    valid = idx >= 0
    assert (idx[valid] < n).all() and np.isinf(d[~valid]).all() and (d[valid] >= 0).all()
    assert (valid[:, :-1] | ~valid[:, 1:]).all()
    key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (idx & 0xffffffff).astype(np.uint64)
    both = valid[:, :-1] & valid[:, 1:]
    assert (key[:, :-1][both] < key[:, 1:][both]).all()


# ---- 1: exact ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', [1, 31, 32, 33, 1000])
@pytest.mark.parametrize('E', [32, 192])
def test_l2_on_integer_rows_equals_the_reference_bit_for_bit(E, N):
    """Entries in [-3, 3]: every product, norm and distance is an integer below 2^24, exact in fp32 in any order, and ties are heavy.
    B in {1, 63, 64, 65, 257} and k in {1, 5, 32}; k > N whenever N < k."""
    rows, q = cases.integer_rows(N, E, seed=N + E), cases.integer_rows(257, E, seed=N + E + 1)
    fi = make_index(rows, 'l2')
    assert fi.counts() == {'n': N, 'n_valid': N, 'bad_rows': 0}
    for k in (1, 5, 32):
        ref = NB.search_reference(q, rows, k, 'l2')
        for B in (1, 63, 64, 65, 257):
            got = host(fi.search(cuda(q[:B]), k=k))
            assert got['distances'].dtype == np.float32 and got['indices'].dtype == np.int32 and got['indices'].shape == (B, k)
            assert np.array_equal(got['indices'], ref['indices'][:B]), (k, B)
            assert np.array_equal(got['distances'], ref['distances'][:B].astype(np.float32)), (k, B)
            assert np.array_equal(got['kth_distance'], ref['kth_distance'][:B].astype(np.float32))
            check_order(got, N)
        assert (got['indices'][:, N:] == -1).all()


@pytest.mark.parametrize('k', [1, 5, 31])
def test_a_tie_pair_cut_by_k_keeps_the_lower_index(k):
    """Every reference row sits at j and at j + N / 2: each distance comes twice, and an odd k cuts a pair."""
    half = cases.integer_rows(500, 192, seed=77)
    rows, q = np.concatenate([half, half]), cases.integer_rows(65, 192, seed=78)
    got = host(make_index(rows, 'l2').search(cuda(q), k=k))
    ref = NB.search_reference(q, rows, k, 'l2')
    assert np.array_equal(got['indices'], ref['indices']) and np.array_equal(got['distances'], ref['distances'].astype(np.float32))
    low = got['indices'] < 500
    partner = np.where(low, got['indices'] + 500, got['indices'] - 500)
    present = (partner[:, :, None] == got['indices'][:, None, :]).any(-1)
    assert (present | low).all()                                    # an upper copy never appears without its lower copy
    assert (~present).any()                                         # and the cut happens


# ---- 2: bounded --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def float_case(N, E, C):
    rows, y, sev, q = cases.float_case(N, E, C, QUERIES, seed=N + E + C)
    for a in (rows, y, sev, q):
        a.setflags(write=False)
    return rows, y.astype(np.int32), sev, q


@functools.lru_cache(maxsize=None)
def float_reference(N, E, C, metric):
    rows, y, sev, q = float_case(N, E, C)
    D, b = NB.distance_matrix(q, rows, metric), cases.distance_bounds(q, rows, metric)
    D.setflags(write=False)
    b.setflags(write=False)
    return D, b, np.sort(D, axis=1)


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
@pytest.mark.parametrize('N,E,C', FLOAT_CASES)
def test_float_rows_against_the_fp64_reference_within_the_derived_bounds(N, E, C, metric):
    """Per returned distance |d - d_ref| <= b, b = 2 (E + 1) u sum |q_k r_k| + (E + 1) u (|q|^2 + |r|^2) + 3 u (|q|^2 + |r|^2 + 2 sum |q_k r_k|)
    for l2 (the product's fma chain, the two norms' chains, the three roundings of the combination) and (2 E + 10) u for cosine (two
    normalisations of (E / 2 + 2) u each, the chain, the subtraction), u = 2^-24; under that cap 4 x the measured maximum of error / bound.
    Membership for EVERY query: no returned index lies above the reference's k-th distance plus b, no missing index below the device's k-th
    distance minus b.  The index sets equal the reference's for every decided query (reference gap between the k-th and the (k + 1)-th
    distance above 2 max b); at least 90 % of the queries are decided."""
    rows, y, sev, q = float_case(N, E, C)
    D, b, Ds = float_reference(N, E, C, metric)
    fi = make_index(rows, metric)
    factor = 1.0 if MEASURED_DISTANCE_RATIO is None else min(1.0, 4 * MEASURED_DISTANCE_RATIO)
    rows_i = np.arange(QUERIES)[:, None]
    for k in (1, 5, 32):
        got = host(fi.search(cuda(q), k=k))
        check_order(got, N)
        idx = got['indices'].astype(np.int64)
        kk = min(k, N)
        assert (idx[:, :kk] >= 0).all() and (idx[:, kk:] == -1).all()
        idx, dd = idx[:, :kk], got['distances'][:, :kk].astype(np.float64)
        err, bound = np.abs(dd - D[rows_i, idx]), b[rows_i, idx]
        ratio = float((err / bound).max())
        print(f'distance ratio N={N} E={E} {metric} k={k}: {ratio:.3e}')
        assert (err <= factor * bound).all()
        assert (D[rows_i, idx] <= Ds[:, kk - 1][:, None] + bound).all()
        missing = np.ones((QUERIES, N), dtype=bool)
        missing[rows_i, idx] = False
        assert (~missing | (D >= dd[:, -1][:, None] - b)).all()
        if kk < N:
            decided = (Ds[:, kk] - Ds[:, kk - 1]) > 2 * b.max()
            print(f'decided share N={N} E={E} {metric} k={k}: {decided.mean():.3f}')
            assert decided.mean() >= 0.9
            want = np.argsort(D, axis=1, kind='stable')[:, :kk]
            assert np.array_equal(np.sort(idx[decided], axis=1), np.sort(want[decided], axis=1))


# ---- 3: determinism ----------------------------------------------------------------------------------------------------------------------

def test_every_output_is_bit_identical_across_runs_splits_grids_and_query_batches():
    N, E, C = FLOAT_CASES[3]
    rows, y, sev, q = float_case(N, E, C)
    for metric in ('cosine', 'l2'):
        first = make_index(rows, metric, y, sev, C).search(cuda(q), k=10)
        assert list(first) == ['distances', 'indices', 'labels', 'severities', 'kth_distance', 'mean_distance', 'class_probs', 'class', 'severity']

        def check(other, what):
            assert [name for name in first if not torch.equal(first[name], other[name])] == [], (metric, what)
        check(make_index(rows, metric, y, sev, C).search(cuda(q), k=10), 'second run')
        for edges in ([0, 1, N], [0, 255, 256, 3000, N], [0] + list(range(100, N, 700)) + [N]):
            check(make_index(rows, metric, y, sev, C, edges=edges).search(cuda(q), k=10), edges)
        for cap in (1, 3, 0):
            check(make_index(rows, metric, y, sev, C, max_workgroups=cap).search(cuda(q), k=10), cap)
        fi = make_index(rows, metric, y, sev, C)
        for row in (0, 200, 256):                                   # a one-row batch: one query tile
            one = fi.search(cuda(q[row:row + 1]), k=10)
            assert all(torch.equal(one[name][0], first[name][row]) for name in first), (metric, row)
        # another number of reference splits for the same rows: 82 reference tiles run as 41 splits for 5 query tiles (257 queries, the
        # cap of 64 and two tiles per split) and as 28 splits for 17 query tiles (1025 queries, three tiles per split)
        many = fi.search(cuda(np.concatenate([q, rows[:768]])), k=10)
        assert all(torch.equal(many[name][:QUERIES], first[name]) for name in first), (metric, 'query tiles')


# ---- 4: exclude --------------------------------------------------------------------------------------------------------------------------

def test_leave_one_out_of_the_index_against_itself():
    rows = cases.integer_rows(1000, 32, seed=5)
    me = np.arange(1000)
    got = host(make_index(rows, 'l2').search(cuda(rows), k=5, exclude=cuda(me.astype(np.int32))))
    ref = NB.search_reference(rows, rows, 5, 'l2', exclude=me)
    assert not (got['indices'] == me[:, None]).any()
    assert np.array_equal(got['indices'], ref['indices']) and np.array_equal(got['distances'], ref['distances'].astype(np.float32))
    frows, y, sev, _ = float_case(1000, 192, 4)
    got = host(make_index(frows, 'cosine').search(cuda(frows), k=5, exclude=cuda(me.astype(np.int32))))
    ref = NB.search_reference(frows, frows, 5, 'cosine', exclude=me)
    assert not (got['indices'] == me[:, None]).any()
    D = NB.distance_matrix(frows, frows, 'cosine')
    D[me, me] = np.inf
    Ds = np.sort(D, axis=1)
    decided = (Ds[:, 5] - Ds[:, 4]) > 2 * (2 * 192 + 10) * cases.U32
    assert decided.mean() >= 0.9 and np.array_equal(np.sort(got['indices'][decided], axis=1), np.sort(ref['indices'][decided], axis=1))
    without = host(make_index(frows, 'cosine').search(cuda(frows), k=1))
    assert np.array_equal(without['indices'][:, 0], me)             # and without exclude every row finds itself


# ---- 5: bad rows -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_bad_reference_rows_are_counted_and_never_returned_and_a_bad_query_row_returns_nothing(metric):
    rows = cases.integer_rows(200, 64, seed=9) + 0.5
    rows[17, 3], rows[130, 63], rows[64] = np.inf, np.nan, 0.0
    q = rows[[17, 18, 130, 64, 5]].copy()                           # inf, fine, NaN, zero, fine
    fi = make_index(rows, metric)
    bad = 3 if metric == 'cosine' else 2
    assert fi.counts() == {'n': 200, 'n_valid': 200 - bad, 'bad_rows': bad}
    for k in (3, 32):
        got = host(fi.search(cuda(q), k=k))
        ref = NB.search_reference(q, rows, k, metric)
        assert not np.isin(got['indices'], [17, 130] + ([64] if metric == 'cosine' else [])).any()
        for row in (0, 2) + ((3,) if metric == 'cosine' else ()):
            assert (got['indices'][row] == -1).all() and np.isposinf(got['distances'][row]).all()
            assert np.isposinf(got['kth_distance'][row]) and np.isposinf(got['mean_distance'][row])
        assert got['indices'][1, 0] == 18 and got['indices'][4, 0] == 5 and (got['indices'][[1, 4]] >= 0).all()
        if metric == 'l2':                                          # halves: still exact in fp32
            assert np.array_equal(got['indices'], ref['indices']) and np.array_equal(got['distances'], ref['distances'].astype(np.float32))
    few = host(make_index(rows[15:19], metric).search(cuda(q), k=5))          # three valid rows, k = 5
    assert (few['indices'][1, :3] >= 0).all() and (few['indices'][1, 3:] == -1).all() and np.isposinf(few['distances'][1, 3:]).all()


# ---- 6: vote -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_the_vote_equals_the_fp64_statement_on_the_devices_own_neighbours(metric):
    """class_probs, severity, mean_distance within 4 fp32 ulp of the fp64 host vote on the device's distances, labels and severities;
    class, kth_distance, labels and severities exact."""
    N, E, C = FLOAT_CASES[2]
    rows, y, sev, q = float_case(N, E, C)
    y = y.copy()
    y[::13] = C + 2                                                 # labels outside [0, C): no vote
    fi = make_index(rows, metric, y, sev, C)
    for k, tau in ((1, 0.07), (10, 0.07), (32, 0.5)):
        got = host(fi.search(cuda(q), k=k, temperature=tau))
        idx = got['indices'].astype(np.int64)
        assert np.array_equal(got['labels'], y[idx]) and np.array_equal(got['severities'], sev[idx])
        want = NB.vote_reference(got['distances'], idx, got['labels'], got['severities'], C, tau)
        assert np.array_equal(got['class'], want['class']) and got['class'].dtype == np.int32
        assert np.array_equal(got['kth_distance'], got['distances'][:, -1])
        for name in ('class_probs', 'severity', 'mean_distance'):
            w32 = want[name].astype(np.float32)
            assert (np.abs(got[name].astype(np.float64) - want[name]) <= 4 * np.spacing(np.abs(w32)).astype(np.float64)).all(), name
        assert (got['class_probs'].sum(1) <= 1.0 + 1e-6).all() and (got['class_probs'].sum(1) < 0.999).any()


# ---- 7: end to end -----------------------------------------------------------------------------------------------------------------------

CLASS_NAMES = ['Healthy Leaf', 'Leaf Holes', 'Black Spot', 'Dry Leaf']


def test_model_and_evaluator_end_to_end(tmp_path):
    """48 smooth images in batches of 16 on the oracle-initialised model: fit_feature_index on a loader equals an index fed the same
    features by hand, bit for bit; an image added twice is its own nearest neighbour under leave-one-out; Gaussian-noise images lie
    farther from the recorded features than the recorded images (AUROC > 0.5: a direction, not a quality claim); the Evaluator's keys
    with and without an index and the order of the OOD cards."""
    from evaluation.evaluator import Evaluator
    from models.rovit_kan import RoViTKAN
    from rovit_hip.density import ood_metrics
    model = RoViTKAN(pretrained=False)
    model.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    model = model.to(dev()).eval()
    g = torch.Generator().manual_seed(0)
    smooth = torch.nn.functional.interpolate(torch.randn(48, 3, 7, 7, generator=g), size=224, mode='bilinear', align_corners=False)
    labels = torch.arange(48) % 4
    loader = [(smooth[i:i + 16], labels[i:i + 16], labels[i:i + 16]) for i in range(0, 48, 16)]
    fi = model.fit_feature_index(loader)
    by_hand = NB.FeatureIndex(192, 4)
    with torch.no_grad():
        for images, y, s in loader:
            by_hand.update(model.backbone(images.to(dev())), y, s)
    by_hand.build()
    assert fi.n == 48 and fi.counts() == {'n': 48, 'n_valid': 48, 'bad_rows': 0} and fi.has_labels and fi.has_severity
    assert torch.equal(fi.rows(), by_hand.rows())
    a, b = fi.search(fi.rows(), k=5), by_hand.search(by_hand.rows(), k=5)
    assert all(torch.equal(a[name], b[name]) for name in a)
    from_tensor = model.fit_feature_index(smooth.to(dev()), labels, labels.float(), chunk=16)
    assert torch.equal(from_tensor.rows(), fi.rows())
    twice = model.fit_feature_index(torch.cat([smooth, smooth[7:8]]).to(dev()), torch.cat([labels, labels[7:8]]), chunk=16)
    loo = twice.search(twice.rows(), k=1, exclude=torch.arange(49, dtype=torch.int32, device=dev()))
    assert int(loo['indices'][7, 0]) == 48 and int(loo['indices'][48, 0]) == 7
    near = model.nearest_examples(smooth[:8].to(dev()), fi, k=5)
    assert set(near) == {'distances', 'indices', 'labels', 'severities', 'kth_distance', 'mean_distance', 'class_probs', 'class', 'severity',
                         'head_class', 'head_ordinal_severity'}
    assert near['indices'][:, 0].tolist() == list(range(8)) and near['labels'][:, 0].tolist() == labels[:8].tolist()
    with torch.no_grad():
        inside = fi.search(model.backbone(smooth.to(dev())), k=5)['kth_distance']
        outside = fi.search(model.backbone(torch.randn(48, 3, 224, 224, generator=g).to(dev())), k=5)['kth_distance']
    card = ood_metrics(inside, outside)
    print(f"kNN AUROC of noise against the recorded images: {card['auroc']:.4f}")
    assert card['auroc'] > 0.5
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=CLASS_NAMES, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    plain = Evaluator(model, loader, cfg, dev()).evaluate(selective=True)
    assert set(plain) == {'accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece', 'fps', 'params',
                          'params_m', 'per_class', 'selective'}
    assert list(plain['selective']['scores']) == ['confidence', 'entropy', 'sigma']
    ev = Evaluator(model, loader, cfg, dev())
    assert ev.fit_index(loader) is ev.index and torch.equal(ev.index.rows(), fi.rows())
    with_index = ev.evaluate(selective=True, index=ev.index, knn_k=3)
    assert set(with_index) == set(plain) | {'knn'} and set(with_index['knn']) == {'k', 'accuracy', 'severity_mae', 'agreement'}
    assert list(with_index['selective']['scores']) == ['confidence', 'entropy', 'sigma', 'knn_distance']
    assert with_index['knn']['k'] == 3 and 0.0 <= with_index['knn']['agreement'] <= 1.0 and 0.0 <= with_index['knn']['accuracy'] <= 100.0
    assert 'Nearest neighbours (k = 3):' in (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    ev.fit_density(loader)
    cards = ev.evaluate_ood([torch.randn(16, 3, 224, 224, generator=g) for _ in range(2)], density=ev.density, index=ev.index)
    assert list(cards) == ['max_prob', 'entropy', 'energy', 'sigma', 'mahalanobis', 'relative_mahalanobis', 'knn']
    assert all(c['n_in'] == 48 and c['n_out'] == 32 for c in cards.values()) and cards['knn']['auroc'] > 0.5
