"""The numpy statements of rovit_hip.clustering on their own, and the conditions the GPU tests rely on (no GPU needed)."""
import numpy as np
import pytest
import torch

import kmeans_cases as kc
from oracle import philox
from rovit_hip import clustering as cl
from rovit_hip import native
from rovit_hip.native import RovitHipError


def test_binding_has_the_entry_points():
    lib = native.load()
    for name in ('rovit_kmeans_workspace_bytes', 'rovit_kmeans_seed', 'rovit_kmeans_run', 'rovit_kmeans_assign', 'rovit_kmeans_contingency'):
        assert hasattr(lib, name)
    assert lib.rovit_kmeans_workspace_bytes(257, 192, 4) > 0
    for n, E, k in ((0, 192, 4), (257, 48, 4), (257, 192, 0), (257, 192, 257), (2 ** 20 + 1, 192, 4), (257, 288, 4)):
        assert lib.rovit_kmeans_workspace_bytes(n, E, k) == 0
    assert native.KMEANS_STREAM == int.from_bytes(b'KMns', 'big')
    p = native.KMeansProblem()
    p.n, p.embed, p.k, p.m = 0, 192, 4, 4                           # refused before any launch, with the entry's name in the message
    with pytest.raises(RovitHipError, match='kmeans_run'):
        native.call('rovit_kmeans_run', None, None)
    import ctypes
    with pytest.raises(RovitHipError, match='kmeans_seed: 0 rows'):
        native.call('rovit_kmeans_seed', ctypes.byref(p), None)


def test_philox_words_match_the_oracle():
    for seed, j, r in ((0, 0, 0), (5, 3, 2), (2 ** 63 + 11, 255, 63)):
        w = philox.philox4x32_10([j, r, native.KMEANS_STREAM, 0], [seed & 0xFFFFFFFF, seed >> 32])
        assert cl.philox_r64(seed, j, r) == (int(w[0]) << 32) | int(w[1])


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_assign_reference_against_brute_force(metric):
    x, c = kc.assign_case(65, 32, 33, metric)
    x = x.copy()
    x[3, 5] = np.nan
    x[9] = 0.0
    got = cl.assign_reference(x, c, metric)
    for i in range(x.shape[0]):
        xi = x[i].astype(np.float64)
        bad = not np.isfinite(xi).all() or (metric == 'cosine' and not (xi * xi).sum() > 0)
        if bad:
            assert got['labels'][i] == -1 and np.isinf(got['distance'][i]) and np.isinf(got['second_distance'][i]) and got['silhouette'][i] == 0
            continue
        best = (np.inf, -1)
        second = np.inf
        for j in range(c.shape[0]):
            cj = c[j].astype(np.float64)
            if metric == 'cosine':
                d = 1.0 - float((xi / np.sqrt((xi * xi).sum())) @ cj)
            else:
                d = float((xi * xi).sum() + (cj * cj).sum() - 2.0 * (xi @ cj))
            d = max(d, 0.0)
            if d < best[0]:
                second, best = best[0], (d, j)
            elif d < second:
                second = d
        assert got['labels'][i] == best[1]
        assert abs(got['distance'][i] - best[0]) <= 1e-12 * max(1.0, best[0])
        assert abs(got['second_distance'][i] - second) <= 1e-12 * max(1.0, second)
        # the silhouette formula on the statement's own distances (a row that is a centroid has a ~ 1e-8, not 0, in fp64)
        d1, d2 = got['distance'][i], got['second_distance'][i]
        a, b = (d1, d2) if metric == 'cosine' else (np.sqrt(d1), np.sqrt(d2))
        assert abs(got['silhouette'][i] - (b - a) / max(a, b)) < 1e-15


def test_assign_reference_ties_go_to_the_lower_cluster():
    x, c = kc.integer_assign_case(64, 32, 8)
    got = cl.assign_reference(x, c, 'l2')
    assert (got['labels'] < 4).all()                               # centroids 4..7 repeat 0..3
    assert (got['distance'] == np.round(got['distance'])).all()
    one = cl.assign_reference(x, c[:1], 'l2')
    assert np.isinf(one['second_distance']).all() and (one['silhouette'] == 0).all() and (one['labels'] == 0).all()


def test_seeding_rule_on_a_hand_worked_case():
    d = np.array([0.0, 1.0, 3.0, 4.0, 0.5], dtype=np.float32)      # dmax = 4 = 0.5 * 2^3: e = 3, w = d * 2^37
    ok = np.ones(5, dtype=bool)
    unit = 2 ** 36
    pick = cl.seed_reference(d, ok, 2 ** 63)
    assert [int(v) for v in pick['weights']] == [0, 2 * unit, 6 * unit, 8 * unit, unit]
    assert pick['W'] == 17 * unit and pick['t'] == 17 * unit // 2 and pick['index'] == 3 and not pick['w0']
    edge = -((-8 * 2 ** 64) // 17)                                 # the smallest r64 with t >= 8 * 2^36, the cumulative weight of rows 0..2
    assert cl.seed_reference(d, ok, edge)['t'] == 8 * unit and cl.seed_reference(d, ok, edge)['index'] == 3
    assert cl.seed_reference(d, ok, edge - 1)['t'] == 8 * unit - 1 and cl.seed_reference(d, ok, edge - 1)['index'] == 2
    assert cl.seed_reference(d, ok, 0)['index'] == 1               # row 0 has weight 0 and is never drawn
    assert cl.seed_reference(d, ok, 2 ** 64 - 1)['index'] == 4
    # an absent row carries no weight whatever its distance says
    assert cl.seed_reference(np.array([9, 1, 3, 4, .5], np.float32), np.array([0, 1, 1, 1, 1], bool), 0)['index'] == 1


def test_seeding_w0_rule_and_the_ordinal_rule_of_seed_0():
    ok = np.array([False, False, True, True, True])
    zeros = np.zeros(5, dtype=np.float32)
    for r64, want in ((0, 2), (2 ** 64 // 3, 2), (2 ** 64 // 3 + 1, 3), (2 ** 64 - 1, 4)):
        w0 = cl.seed_reference(zeros, ok, r64)
        first = cl.seed_reference(None, ok, r64)
        assert w0['w0'] and not first['w0'] and w0['W'] == first['W'] == 3
        assert w0['index'] == first['index'] == want
    none = cl.seed_reference(None, np.zeros(5, bool), 7)
    assert none['index'] == -1 and none['W'] == 0
    pp = cl.kmeans_pp_reference(kc.duplicate_rows(9, 32, 3), 4, 'l2', seed=1)
    assert pp['w0_events'] == 3 and ((pp['seeds'] >= 0) & (pp['seeds'] < 9)).all()
    assert (pp['taps'][1:] == 0).all()


def test_seeding_on_integer_rows_is_exact_and_spreads():
    x = kc.integer_rows(65, 32, 0)
    pp = cl.kmeans_pp_reference(x, 8, 'l2', seed=3)
    assert len(set(pp['seeds'].tolist())) == 8                     # a chosen row has weight 0 afterwards
    assert (pp['taps'][1:] == np.round(pp['taps'][1:])).all()
    for j in range(1, 8):
        assert pp['taps'][j][pp['seeds'][:j]].max() == 0
    again = cl.kmeans_pp_reference(x, 8, 'l2', seed=3)
    other = cl.kmeans_pp_reference(x, 8, 'l2', seed=4)
    assert (again['seeds'] == pp['seeds']).all() and (other['seeds'] != pp['seeds']).any()


def test_score_card_on_hand_computed_tables():
    same = cl.partition_scores_reference(np.diag([5, 3, 9]))
    assert same['ari'] == 1.0 and abs(same['nmi'] - 1.0) < 1e-15 and same['purity'] == 1.0
    assert abs(same['homogeneity'] - 1.0) < 1e-15 and abs(same['completeness'] - 1.0) < 1e-15
    perm = cl.partition_scores_reference(np.array([[0, 4, 0], [0, 0, 6], [2, 0, 0]]))
    assert perm['ari'] == 1.0 and abs(perm['nmi'] - 1.0) < 1e-15
    for a, b, c, d in ((3, 1, 1, 3), (10, 0, 2, 5), (4, 4, 4, 4), (7, 2, 0, 1)):
        got = cl.partition_scores_reference(np.array([[a, b], [c, d]]))
        # the pair-counting closed form (Hubert & Arabie; Steinley 2004): pairs together in both, in one, in neither
        pairs = lambda v: v * (v - 1) // 2
        n11 = pairs(a) + pairs(b) + pairs(c) + pairs(d)
        n10, n01 = pairs(a + b) + pairs(c + d) - n11, pairs(a + c) + pairs(b + d) - n11
        n00 = pairs(a + b + c + d) - n11 - n10 - n01
        want = 2.0 * (n00 * n11 - n01 * n10) / ((n00 + n01) * (n01 + n11) + (n00 + n10) * (n10 + n11))
        assert abs(got['ari'] - want) < 1e-14, (a, b, c, d)
        assert got['purity'] == (max(a, b) + max(c, d)) / (a + b + c + d)
    # [[3, 1], [1, 3]] by hand: 6 pairs together in both, 12 and 12 in each, 28 in all: (6 - 144 / 28) / (12 - 144 / 28) = 1 / 8
    assert abs(cl.partition_scores_reference(np.array([[3, 1], [1, 3]]))['ari'] - 0.125) < 1e-15
    even = cl.partition_scores_reference(np.array([[4, 4], [4, 4]]))
    assert abs(even['nmi']) < 1e-15 and abs(even['homogeneity']) < 1e-15
    one = cl.partition_scores_reference(np.array([[5, 3, 2]]))       # k = 1
    assert one['ari'] == 0.0 and one['homogeneity'] == 0.0 and one['completeness'] == 1.0 and one['nmi'] == 0.0 and one['purity'] == 0.5
    # a 2 x 3 table by hand: clusters {a a a b}, {b c c c}
    t = np.array([[3, 1, 0], [0, 1, 3]])
    got = cl.partition_scores_reference(t)
    h_k, h_c = np.log(2), -(2 * 3 / 8 * np.log(3 / 8) + 2 / 8 * np.log(2 / 8))
    mi = 2 * (3 / 8 * np.log((3 / 8) / (1 / 2 * 3 / 8)) + 1 / 8 * np.log((1 / 8) / (1 / 2 * 2 / 8)))
    assert abs(got['nmi'] - 2 * mi / (h_k + h_c)) < 1e-14 and abs(got['homogeneity'] - mi / h_c) < 1e-14
    assert abs(got['completeness'] - mi / h_k) < 1e-14
    assert abs(got['ari'] - (6 - 12 * 7 / 28) / (0.5 * (12 + 7) - 12 * 7 / 28)) < 1e-14


def test_score_card_against_sklearn_where_it_imports():
    metrics = pytest.importorskip('sklearn.metrics')
    rng = np.random.default_rng(0)
    for k, C, n in ((3, 4, 200), (1, 3, 50), (5, 2, 77)):
        a, y = rng.integers(0, k, n), rng.integers(0, C, n)
        table, left = cl.contingency_reference(a, y, k, C)
        got = cl.partition_scores_reference(table)
        assert left == 0 and table.sum() == n
        assert abs(got['ari'] - metrics.adjusted_rand_score(y, a)) < 1e-12
        assert abs(got['nmi'] - metrics.normalized_mutual_info_score(y, a)) < 1e-12
        h, c, _ = metrics.homogeneity_completeness_v_measure(y, a)
        assert abs(got['homogeneity'] - h) < 1e-12 and abs(got['completeness'] - c) < 1e-12


def test_contingency_leaves_out_and_counts_bad_labels():
    table, left = cl.contingency_reference([0, 1, 1, -1, 2, 0], [0, 1, 5, 1, -1, 0], 3, 2)
    assert left == 3 and table.tolist() == [[2, 0], [0, 1], [0, 0]]


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_bad_rows_and_empty_clusters(metric):
    x, y = kc.float_rows((65, 32, 4, 0))
    x = x.copy()
    x[7, 0] = np.inf
    x[11] = 0.0
    bad = [7, 11] if metric == 'cosine' else [7]
    fit = cl.fit_reference(x, 4, metric, seed=2)
    assert fit['bad_rows'] == len(bad) and fit['n_valid'] == 65 - len(bad)
    assert (fit['labels'][bad] == -1).all() and np.isinf(fit['distances'][bad]).all() and (fit['silhouette'][bad] == 0).all()
    assert fit['counts'].sum() == 65 - len(bad) and not np.isin(fit['seeds'], bad).any()
    clean = cl.fit_reference(np.delete(x, bad, axis=0), 4, metric, seed=2)          # the bad rows disturb nothing but the indices
    keep = np.delete(np.arange(65), bad)
    if (keep[clean['seeds']] == fit['seeds']).all():
        assert (clean['labels'] == fit['labels'][keep]).all() and clean['inertia'] == fit['inertia']
    # a given init that leaves a cluster empty: the centroid keeps its place and is counted
    if metric == 'l2':                                             # a far centroid stays empty to the end and has medoid -1
        init = np.stack([x[0], x[1], x[2], -50.0 * np.ones(32, np.float32) + np.arange(32, dtype=np.float32)])
        got = cl.fit_reference(x, 4, metric, init=init)
        assert got['counts'][3] == 0 and got['medoids'][3] == -1 and got['empty'] == 1 and got['empty_events'] >= 1
    else:                                                          # a repeated centroid loses every tie to the lower index
        init = np.stack([x[0], x[1], x[2], x[0]])
        got = cl.fit_reference(x, 4, metric, max_iter=1, init=init)
        assert got['empty_events'] == 1 and got['n_iter'] == 1
    assert (got['cluster_centers'][3] == cl._prepare_init(init, metric)[3]).all()
    with pytest.raises(RovitHipError):
        cl.fit_reference(x[:3], 4, metric)                           # k > n_valid is refused where it is known


def test_update_reference_is_the_member_mean():
    x, y = kc.float_rows((65, 32, 4, 0))
    old = np.zeros((5, 32), np.float32)
    old[4] = 7.0
    u = cl.update_reference(x, y, old, 'l2')
    for c in range(4):
        assert np.allclose(u['means'][c], x[y == c].astype(np.float64).mean(0), rtol=0, atol=1e-14)
        assert (u['centroids'][c] == u['means'][c].astype(np.float32)).all()
    assert (u['centroids'][4] == 7.0).all() and u['empty'] == 1
    s = cl.update_reference(x, y, old, 'cosine')
    assert np.allclose((s['means'][:4] ** 2).sum(1), 1.0, atol=1e-14)


def test_cpu_tensors_run_through_the_public_entry_points():
    case = kc.FLOAT_CASES[2]
    x, y = kc.float_rows(case)
    seed = kc.RECOVERING_SEED[(case, 'l2')]
    km = cl.KMeans(4, seed=seed).fit(torch.from_numpy(x))
    ref = cl.fit_reference(x, 4, seed=seed)
    assert (km.labels_.numpy() == ref['labels']).all() and km.n_iter_ == ref['n_iter'] and km.inertia_ == ref['inertia']
    assert (km.medoids_.numpy() == ref['medoids']).all() and (km.seeds_.numpy() == ref['seeds']).all()
    card = km.score_card(torch.from_numpy(y), 4)
    assert card['ari'] == 1.0 and card['left_out'] == 0 and card['table'].sum() == 65
    pred = km.predict(torch.from_numpy(x[:9]))
    assert (pred['labels'].numpy() == ref['labels'][:9]).all()
    again = cl.KMeans(4).load_state_dict(km.state_dict())
    assert (again.predict(torch.from_numpy(x[:9]))['labels'] == pred['labels']).all()
    assert (cl.kmeans_pp(torch.from_numpy(x), 4, seed=seed).numpy() == ref['seeds']).all()
    for bad in (dict(n_clusters=0), dict(n_clusters=257), dict(n_clusters=4, metric='l1'), dict(n_clusters=4, max_iter=0),
                dict(n_clusters=4, n_init=0), dict(n_clusters=4, seed=-1), dict(n_clusters=4, init='random')):
        with pytest.raises(RovitHipError):
            cl.KMeans(**bad)
    with pytest.raises(RovitHipError):
        cl.KMeans(4).fit(torch.zeros(3, 32))                        # k > n
    with pytest.raises(RovitHipError):
        cl.KMeans(4).fit(torch.zeros(9, 40))                        # E no multiple of 32
    with pytest.raises(RovitHipError):
        cl.KMeans(4).labels_                                        # not fitted


def _pick_margin(x, k, metric, seed, restart=0):
    """The smallest distance of a pick's t to a boundary of its row's cumulative-weight interval, over W."""
    pp = cl.kmeans_pp_reference(x, k, metric, seed, restart)
    worst = 1.0
    for p in pp['picks'][1:]:
        cs = np.cumsum([int(v) for v in p['weights']])
        hi = int(cs[p['index']])
        lo = hi - int(p['weights'][p['index']])
        worst = min(worst, min(hi - p['t'], p['t'] - lo + 1) / p['W'])
    return worst


def _worst_margin(x, run, metric):
    """min over the run's assigns and rows of margin - 2 bound: positive when no row has to be left out."""
    worst = np.inf
    for c in run['centers_trace']:
        a = cl.assign_reference(x, c, metric)
        worst = min(worst, float((a['margin'] - 2 * kc.distance_bound(x, c, metric)).min()))
    return worst


@pytest.mark.parametrize('case,metric,seed,recovers', kc.run_cases())
def test_conditions_of_the_recorded_runs(case, metric, seed, recovers):
    """What tests/test_gpu_kmeans.py relies on: the recorded seed recovers the planted classes (or stops in a local optimum), no row of
    any assign of the run is nearer than 2 x bound to a second centroid, and no seeding pick is within 1e-4 W of a boundary."""
    x, y = kc.float_rows(case)
    ref = cl.fit_reference(x, 4, metric, seed=seed)
    table, left = cl.contingency_reference(ref['labels'], y, 4, 4)
    ari = cl.partition_scores_reference(table)['ari']
    assert left == 0 and ref['n_iter'] < 100
    assert (ari == 1.0) if recovers else (0.5 < ari < 0.7)
    assert _worst_margin(x, ref, metric) > 0
    assert _pick_margin(x, 4, metric, seed) > 1e-4


def test_conditions_of_the_restart_run():
    x, _ = kc.float_rows(kc.RESTART_CASE)
    ref = cl.fit_reference(x, 4, 'l2', n_init=3, seed=kc.RESTART_SEED)
    assert ref['restart'] == kc.RESTART_KEPT
    others = [v for r, v in enumerate(ref['inertias']) if r != kc.RESTART_KEPT]
    assert min(others) - ref['inertia'] > 1.0                       # no tie for fp32 distances to break differently
    for r, run in enumerate(ref['runs']):
        assert _worst_margin(x, run, 'l2') > 0 and _pick_margin(x, 4, 'l2', kc.RESTART_SEED, r) > 1e-4


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_conditions_of_the_assign_cases(metric):
    """The float assignment cases of the GPU test leave out at most 1 % of their rows (margin under 2 x bound)."""
    for n, E, k in kc.ASSIGN_SHAPES:
        x, c = kc.assign_case(n, E, k, metric)
        a = cl.assign_reference(x, c, metric)
        out = int((a['margin'] <= 2 * kc.distance_bound(x, c, metric)).sum())
        assert out <= n // 100, (n, E, k, out)
