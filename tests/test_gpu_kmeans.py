"""GPU tests of csrc/kmeans.hip through rovit_hip.clustering: the assignment (bit for bit on integer rows, within the derived bound on
float rows, and against the neighbour search), the update, the integer seeding, whole runs at the recorded seeds, determinism, bad rows
and edge cases, the contingency table and the score card, the silhouette and the model entry.

Bound on a distance: (E + 3) 2^-24 (|x| + |c|)^2 (tests/kmeans_cases.py: distance_bound).  Labels are compared on every row whose
reference margin exceeds 2 x bound; at most 1 % of the rows may be left out (tests/test_kmeans_cpu.py shows the cases leave out far
fewer), and in the whole runs none.

Measured on the MI355X over the cases below (printed by the tests before they assert; profiles/kmeans_error.jsonl):
  distances        max |d - d_ref| / bound = 7.540e-02 with l2, 3.562e-02 with cosine (second distance: 4.917e-02); the seeding's
                   min-distance tap: 4.782e-02.  Asserted: <= 1, the derived bound.
  l2 centroid      max error / (2^-24 |c| + n 2^-53 sum |x|) = 9.983e-01 (the bound is the final rounding to fp32).  Asserted: <= 1.
  cosine centroid  max |c - c_ref| per element after one update = 2.275e-08 (n = 257, E = 192, k = 33; 1.4e-08 on the converged run
                   with bad rows)
  silhouette       max |s - s_ref| per row = 1.351e-06 on the fitted runs (n = 65, E = 32, cosine), 9.973e-06 on the depth-2 model's
                   features; of the mean = 5.129e-08 (n = 257, E = 32, l2)
For the errors with no derived bound (the 'cosine' centroid, whose rows are the fp32 unit rows; the silhouette against the fp64
statement) the asserted tolerance is 4 x the measured value, capped at 1e-3; a None would mean not measured yet, and the cap alone
would hold.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_cases as kc  # noqa: E402
from density_cases import with_bad_labels  # noqa: E402
from oracle import ref_cpu  # noqa: E402  (checker only)

from rovit_hip import clustering as cl  # noqa: E402
from rovit_hip import neighbors  # noqa: E402
from rovit_hip.native import RovitHipError  # noqa: E402

pytestmark = pytest.mark.gpu

U = kc.U32
CAP = 1e-3
MEASURED_COSINE_CENTROID = 2.275e-08
MEASURED_SILHOUETTE = 9.973e-06
MEASURED_SILHOUETTE_MEAN = 5.129e-08


def tolerance(measured):
    return CAP if measured is None else min(4.0 * measured, CAP)


def dev():
    return torch.device('cuda:0')


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy()


def assign(x, c, metric, max_workgroups=0):
    """The assignment alone: the centroids enter through load_state_dict, the rows through predict."""
    km = cl.KMeans(int(c.shape[0]), metric=metric)
    km.load_state_dict({'n_clusters': int(c.shape[0]), 'metric': metric, 'max_iter': 1, 'n_init': 1, 'seed': 0,
                        'cluster_centers': torch.from_numpy(np.ascontiguousarray(c))}, device=dev())
    km.max_workgroups = max_workgroups
    return {k: host(v) for k, v in km.predict(cuda(x)).items()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. assign on integer rows: bit for bit, the tie rule ------------------------------------------------------------------------------

@pytest.mark.parametrize('n,E,k', kc.ASSIGN_SHAPES)
def test_assign_integer_rows_bit_equal(n, E, k):
    x, c = kc.integer_assign_case(n, E, k)
    got, ref = assign(x, c, 'l2'), cl.assign_reference(x, c, 'l2')
    assert (got['labels'] == ref['labels']).all()
    assert (bits(got['distance']) == bits(ref['distance'])).all()
    assert (bits(got['second_distance']) == bits(ref['second_distance'])).all()
    if k > 1:
        assert (got['labels'] < (k + 1) // 2).all()                # the repeated centroids lose every tie to the lower index
    else:
        assert np.isinf(got['second_distance']).all() and (got['silhouette'] == 0).all()


# ---- 2. assign on float rows: within the bound -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('metric', ['l2', 'cosine'])
@pytest.mark.parametrize('n,E,k', kc.ASSIGN_SHAPES)
def test_assign_float_rows_within_the_bound(n, E, k, metric):
    x, c = kc.assign_case(n, E, k, metric)
    got, ref = assign(x, c, metric), cl.assign_reference(x, c, metric)
    bound = kc.distance_bound(x, c, metric)
    ratio = np.abs(got['distance'] - ref['distance']) / bound
    ratio2 = float((np.abs(got['second_distance'] - ref['second_distance']) / bound).max()) if k > 1 else 0.0
    print(f'assign {metric} n={n} E={E} k={k}: distance error / bound = {ratio.max():.3e}, second = {ratio2:.3e}')
    assert ratio.max() <= 1.0 and ratio2 <= 1.0
    if k == 1:
        assert np.isinf(got['second_distance']).all()
    safe = ref['margin'] > 2 * bound
    assert (~safe).sum() <= n // 100
    assert (got['labels'][safe] == ref['labels'][safe]).all()
    # the silhouette is the fp32 formula on the device's own distances: a square root, a difference and a division, each rounded once
    own = cl.silhouette_reference(got['distance'], got['second_distance'], metric)
    assert np.abs(got['silhouette'] - own).max() <= 8 * U


# ---- 3. assign against the neighbour search over the centroids --------------------------------------------------------------------------

@pytest.mark.parametrize('metric', ['l2', 'cosine'])
@pytest.mark.parametrize('n,E,k', [(65, 32, 33), (257, 192, 64), (1025, 256, 65)])
def test_assign_equals_the_neighbour_search_over_the_centroids(n, E, k, metric):
    x, c = kc.assign_case(n, E, k, metric)
    fi = neighbors.FeatureIndex(E, None, metric)
    fi.update(cuda(c))
    fi.build()
    if metric == 'cosine':                                         # the index normalises its rows once more: take the rows it searches
        c = host(fi._normalized)
    nn = fi.search(cuda(x), k=1)
    got = assign(x, c, metric)
    assert (got['labels'] == host(nn['indices'])[:, 0]).all()
    assert (bits(got['distance']) == bits(host(nn['distances'])[:, 0])).all()


# ---- 4. update -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('metric', ['l2', 'cosine'])
@pytest.mark.parametrize('n,E,k', [(5, 32, 2), (65, 32, 4), (257, 192, 33), (1025, 256, 4), (3000, 64, 2)])
def test_update_and_cluster_statistics(n, E, k, metric):
    """One iteration from a given init: the centroids are the update of the device's own first labels; counts, medoids and radii are
    the reference on the device's own final labels and distances.  n = 3000 with k = 2 has clusters of more than one segment."""
    x, c0 = kc.assign_case(n, E, k, metric)
    c0 = cl._prepare_init(c0, metric)                               # the centroids as the run takes them
    first = assign(x, c0, metric)
    km = cl.KMeans(k, metric=metric, max_iter=1, init=torch.from_numpy(c0)).fit(cuda(x))
    ref = cl.update_reference(x, first['labels'], c0, metric)
    got = host(km.cluster_centers_)
    err = np.abs(got - ref['means'])
    if metric == 'l2':
        sums = np.stack([np.abs(x[first['labels'] == j].astype(np.float64)).sum(0) for j in range(k)])
        bound = U * np.abs(ref['means']) + n * 2.0 ** -53 * sums
        print(f'update l2 n={n} E={E} k={k}: centroid error / bound = {(err / np.maximum(bound, 1e-300)).max():.3e}')
        assert (err <= bound).all()
    else:
        print(f'update cosine n={n} E={E} k={k}: max centroid error = {err.max():.3e}')
        assert err.max() <= tolerance(MEASURED_COSINE_CENTROID)
    labels, dist = host(km.labels_), host(km.distances_)
    final = assign(x, got, metric)
    assert (labels == final['labels']).all() and (bits(dist) == bits(final['distance'])).all()
    st = cl.cluster_stats_reference(labels, dist, k)
    assert (host(km.counts_) == st['counts']).all() and (host(km.medoids_) == st['medoids']).all()
    assert (bits(host(km.radii_)) == bits(st['radii'])).all()
    total = float(dist.astype(np.float64).sum())
    assert abs(km.inertia_ - total) <= n * 2.0 ** -53 * total
    assert km.n_iter_ == 1 and km.status_['n_valid'] == n and km.status_['empty_events'] == ref['empty']


# ---- 5. seeding ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,E,m', [(1, 32, 1), (5, 32, 5), (65, 192, 8), (257, 32, 33), (1025, 256, 8)])
def test_seeding_on_integer_rows_equals_the_reference(n, E, m):
    x = kc.integer_rows(n, E, 1)
    ref = cl.kmeans_pp_reference(x, m, 'l2', seed=5)
    for mw in (0, 1, 7):
        seeds, tap, st = cl.kmeans_pp(cuda(x), m, 'l2', seed=5, return_tap=True, max_workgroups=mw)
        assert (host(seeds) == ref['seeds']).all()
        assert (bits(host(tap)[1:]) == bits(ref['taps'][1:])).all()
        assert st['w0_events'] == ref['w0_events'] and st['n_valid'] == n and st['short'] == 0


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
@pytest.mark.parametrize('n,E,m', [(65, 32, 4), (257, 192, 8), (1025, 192, 4)])
def test_seeding_on_float_rows(n, E, m, metric):
    """The min-distance tap is within the bound of the fp64 distances to the device's own earlier seeds, and every pick is the integer
    rule applied to the device's own tap."""
    x, _ = kc.float_rows((n, E, 4, 0))
    seeds, tap, st = cl.kmeans_pp(cuda(x), m, metric, seed=9, return_tap=True)
    seeds, tap = host(seeds), host(tap)
    ok = np.ones(n, dtype=bool)
    assert seeds[0] == cl.seed_reference(None, ok, cl.philox_r64(9, 0))['index']
    rows = cl._rows64(x, ok, metric).astype(np.float32) if metric == 'cosine' else x
    for j in range(1, m):
        c = rows[seeds[:j]]
        d = cl.centroid_distances(x, c, metric).min(axis=1)
        ratio = np.abs(tap[j] - d) / kc.distance_bound(x, c, metric)
        print(f'seeding {metric} n={n} E={E} seed {j}: tap error / bound = {ratio.max():.3e}')
        assert ratio.max() <= 1.0
        assert seeds[j] == cl.seed_reference(tap[j], ok, cl.philox_r64(9, j))['index']
    assert st['w0_events'] == 0


def test_seeding_of_duplicate_rows_takes_the_w0_path():
    x = kc.duplicate_rows(70, 32, 3)
    ref = cl.kmeans_pp_reference(x, 4, 'l2', seed=1)
    seeds, tap, st = cl.kmeans_pp(cuda(x), 4, 'l2', seed=1, return_tap=True)
    assert st['w0_events'] == 3 == ref['w0_events'] and (host(seeds) == ref['seeds']).all() and (host(tap)[1:] == 0).all()


# ---- 6. whole runs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case,metric,seed,recovers', kc.run_cases())
def test_whole_run_equals_the_reference(case, metric, seed, recovers):
    x, y = kc.float_rows(case)
    ref = cl.fit_reference(x, 4, metric, seed=seed)
    km = cl.KMeans(4, metric=metric, seed=seed).fit(cuda(x))
    assert (host(km.seeds_) == ref['seeds']).all()
    assert (host(km.labels_) == ref['labels']).all() and km.n_iter_ == ref['n_iter']
    card = km.score_card(cuda(y), 4)
    table, _ = cl.contingency_reference(ref['labels'], y, 4, 4)
    assert card['ari'] == cl.partition_scores_reference(table)['ari'] and ((card['ari'] == 1.0) == recovers)
    assert abs(km.inertia_ - ref['inertia']) <= kc.distance_bound(x, ref['cluster_centers'], metric).sum()   # a bound per member
    own = cl.cluster_stats_reference(host(km.labels_), host(km.distances_), 4)
    assert (host(km.counts_) == ref['counts']).all() and (host(km.medoids_) == own['medoids']).all()
    sil = host(km.silhouette_)
    err, mean_err = np.abs(sil - ref['silhouette']).max(), abs(card['mean_silhouette'] - ref['mean_silhouette'])
    print(f'run {case} {metric} seed {seed}: silhouette error = {err:.3e}, of the mean = {mean_err:.3e}')
    assert err <= tolerance(MEASURED_SILHOUETTE) and mean_err <= tolerance(MEASURED_SILHOUETTE_MEAN)


def test_restarts_keep_the_restart_the_reference_keeps():
    x, _ = kc.float_rows(kc.RESTART_CASE)
    ref = cl.fit_reference(x, 4, 'l2', n_init=3, seed=kc.RESTART_SEED)
    km = cl.KMeans(4, n_init=3, seed=kc.RESTART_SEED).fit(cuda(x))
    st = km.status_
    assert st['restart'] == ref['restart'] == kc.RESTART_KEPT
    for r, run in enumerate(ref['runs']):
        assert abs(st['inertias'][r] - run['inertia']) <= kc.distance_bound(x, run['cluster_centers']).sum()
    assert (host(km.labels_) == ref['labels']).all() and (host(km.seeds_) == ref['seeds']).all() and km.n_iter_ == ref['n_iter']


# ---- 7. determinism --------------------------------------------------------------------------------------------------------------------

def _everything(km):
    st = km.status_
    return [host(km.cluster_centers_), host(km.labels_), host(km.distances_), host(km.second_distances_), host(km.silhouette_),
            host(km.seeds_), host(km.counts_), host(km.medoids_), host(km.radii_), np.float64(km.inertia_), np.int64(km.n_iter_),
            np.float64(st['mean_silhouette'])]


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_bits_do_not_depend_on_the_run_the_grid_or_the_recording(metric):
    x, _ = kc.float_rows((1025, 192, 4, 0))
    runs = []
    for mw in (0, 0, 1, 7):
        km = cl.KMeans(33, metric=metric, seed=3, max_iter=8)
        km.max_workgroups = mw
        runs.append(_everything(km.fit(cuda(x))))
    fi = neighbors.FeatureIndex(192, None, metric)                  # the rows recorded in several calls instead of one
    for r0, r1 in ((0, 1), (1, 300), (300, 1025)):
        fi.update(cuda(x[r0:r1]))
    runs.append(_everything(cl.KMeans(33, metric=metric, seed=3, max_iter=8).fit(fi.rows())))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 8. bad rows and edge cases --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_bad_rows_are_absent(metric):
    x, _ = kc.float_rows((257, 32, 4, 0))
    x = x.copy()
    x[70, 3] = np.nan
    x[200] = 0.0
    bad = [70, 200] if metric == 'cosine' else [70]
    km = cl.KMeans(4, metric=metric, seed=6).fit(cuda(x))
    labels = host(km.labels_)
    assert km.status_['bad_rows'] == len(bad) and km.status_['n_valid'] == 257 - len(bad) and km.status_['n'] == 257
    assert (labels[bad] == -1).all() and np.isinf(host(km.distances_)[bad]).all() and np.isinf(host(km.second_distances_)[bad]).all()
    assert (host(km.silhouette_)[bad] == 0).all() and host(km.counts_).sum() == 257 - len(bad)
    assert not np.isin(host(km.seeds_), bad).any() and km.status_['short'] == 0
    centers = host(km.cluster_centers_)
    ref = cl.assign_reference(x, centers, metric)                   # the bad rows disturb nothing else
    safe = ref['margin'] > 2 * kc.distance_bound(np.nan_to_num(x), centers, metric)
    assert safe.sum() > 200 and (labels[safe] == ref['labels'][safe]).all() and (ref['labels'][bad] == -1).all()
    again = cl.update_reference(x, labels, centers, metric)         # converged: the centroids are the means of their members
    slack = tolerance(MEASURED_COSINE_CENTROID) if metric == 'cosine' else U * np.abs(centers).max() + 1e-12
    print(f'bad rows {metric}: converged centroid error = {np.abs(again["means"] - centers).max():.3e}')
    assert km.n_iter_ < 100 and np.abs(again['means'] - centers).max() <= slack


def test_every_row_its_own_cluster_and_a_single_cluster():
    x, _ = kc.float_rows((5, 32, 4, 0))
    km = cl.KMeans(5, seed=2).fit(cuda(x))
    assert sorted(host(km.labels_).tolist()) == [0, 1, 2, 3, 4] and (host(km.counts_) == 1).all()
    assert sorted(host(km.seeds_).tolist()) == [0, 1, 2, 3, 4] and (host(km.medoids_) == host(km.seeds_)).all()
    # a centroid is its one member, rounded from its own fp64 value: |x|^2 + |c|^2 - 2 x.c is the same chain three times, exactly 0
    assert km.inertia_ == 0.0 and (host(km.distances_) == 0).all() and km.status_['short'] == 0 and km.n_iter_ == 2
    x, _ = kc.float_rows((65, 192, 4, 0))
    one = cl.KMeans(1).fit(cuda(x))
    mean = x.astype(np.float64).mean(0)
    assert (host(one.labels_) == 0).all() and np.isinf(host(one.second_distances_)).all() and (host(one.silhouette_) == 0).all()
    assert np.abs(host(one.cluster_centers_) - mean).max() <= U * np.abs(mean).max() + 65 * 2.0 ** -53 * np.abs(x).sum(0).max()
    assert one.n_iter_ == 2 and host(one.counts_).tolist() == [65]
    # more clusters than valid rows cannot be known before the rows are looked at: the status block says so
    x = x[:5].copy()
    x[1:3] = np.nan
    short = cl.KMeans(4, max_iter=2).fit(cuda(x))
    assert short.status_['short'] == 1 and short.status_['n_valid'] == 3


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_a_given_init_that_leaves_a_cluster_empty(metric):
    x, _ = kc.float_rows((65, 32, 4, 0))
    if metric == 'l2':
        init = np.stack([x[0], x[1], x[2], -50.0 * np.ones(32, np.float32) + np.arange(32, dtype=np.float32)])
        km = cl.KMeans(4, metric=metric, init=torch.from_numpy(init)).fit(cuda(x))      # the far centroid stays empty to the end
        assert host(km.counts_)[3] == 0 and host(km.medoids_)[3] == -1 and km.status_['empty'] == 1 and host(km.radii_)[3] == 0
        assert km.status_['empty_events'] == km.n_iter_ - 1        # one per update
    else:
        init = np.stack([x[0], x[1], x[2], x[0]])                   # a repeated centroid loses every tie to the lower index
        km = cl.KMeans(4, metric=metric, max_iter=1, init=torch.from_numpy(init)).fit(cuda(x))
        assert km.status_['empty_events'] == 1 and km.n_iter_ == 1
    assert (host(km.cluster_centers_)[3] == cl._prepare_init(init, metric)[3]).all()
    assert (host(km.seeds_) == -1).all() and host(km.counts_).sum() == 65


def test_predict_on_new_rows_and_the_refusals():
    case = (257, 192, 4, 0)
    x, _ = kc.float_rows(case)
    km = cl.KMeans(4, seed=kc.RECOVERING_SEED[(case, 'l2')]).fit(cuda(x))
    new, _ = kc.float_rows((65, 192, 4, 5))
    pred = km.predict(cuda(new))
    ref = cl.assign_reference(new, host(km.cluster_centers_), 'l2')
    safe = ref['margin'] > 2 * kc.distance_bound(new, host(km.cluster_centers_))
    assert safe.sum() > 32 and (host(pred['labels'])[safe] == ref['labels'][safe]).all()
    assert pred['labels'].is_cuda and pred['labels'].dtype == torch.int32 and set(pred) == {'labels', 'distance', 'second_distance', 'silhouette'}
    again = cl.KMeans(4).load_state_dict(km.state_dict(), device=dev()).predict(cuda(new))
    assert all(torch.equal(pred[name], again[name]) for name in pred)
    with pytest.raises(RovitHipError):
        cl.KMeans(4).fit(cuda(x[:3]))                               # k > n
    with pytest.raises(RovitHipError):
        cl.KMeans(4).fit(cuda(x[:, :40]))                           # E no multiple of 32
    with pytest.raises(RovitHipError):
        km.predict(cuda(new[:, :32]))
    with pytest.raises(RovitHipError):
        km.score_card(cuda(np.zeros(5, np.int64)), 4)
    with pytest.raises(RovitHipError):
        cl.kmeans_pp(cuda(x), 257)


# ---- 9. contingency table and score card -----------------------------------------------------------------------------------------------

def test_contingency_table_and_score_card():
    case = (1025, 192, 4, 0)
    x, y = kc.float_rows(case)
    y = with_bad_labels(y, 4, 0)
    km = cl.KMeans(7, seed=1).fit(cuda(x))
    card = km.score_card(cuda(y), 4)
    table, left = cl.contingency_reference(host(km.labels_), y, 7, 4)
    assert (card['table'] == table).all() and card['left_out'] == left > 0 and table.sum() + left == 1025
    ref = cl.partition_scores_reference(table)
    assert all(card[name] == ref[name] for name in ('purity', 'homogeneity', 'completeness', 'nmi', 'ari'))
    assert card['inertia'] == km.inertia_


# ---- 10. silhouette, and the model entry -----------------------------------------------------------------------------------------------

def test_model_cluster_features():
    from models.backbone import DeiTTiny
    from models.rovit_kan import RoViTKAN
    model = RoViTKAN(pretrained=False)
    model.backbone.model = DeiTTiny(depth=2)
    model.load_state_dict(ref_cpu.init_rovit_state(depth=2, seed=23), strict=True)
    model = model.to(dev()).train()
    g = torch.Generator().manual_seed(0)
    images = torch.nn.functional.interpolate(torch.randn(48, 3, 7, 7, generator=g), size=224, mode='bilinear', align_corners=False).to(dev())
    y = torch.arange(48) % 4
    out = model.cluster_features(images, 3, labels=y, chunk=16, seed=1)
    assert model.training and all(p.grad is None for p in model.parameters())
    feats = host(out['features'])
    assert feats.shape == (48, 192) and out['labels'].shape == (48,) and out['cluster_centers'].shape == (3, 192)
    km = out['kmeans']
    ref = cl.assign_reference(feats, host(km.cluster_centers_), 'l2')
    safe = ref['margin'] > 2 * kc.distance_bound(feats, host(km.cluster_centers_))
    assert (host(out['labels'])[safe] == ref['labels'][safe]).all()
    sil = host(out['silhouette'])
    print(f'model: silhouette error = {np.abs(sil - ref["silhouette"])[safe].max():.3e}')
    assert np.abs(sil - ref['silhouette'])[safe].max() <= tolerance(MEASURED_SILHOUETTE)
    card = out['score_card']
    table, left = cl.contingency_reference(host(out['labels']), y.numpy(), 3, 4)
    assert (card['table'] == table).all() and left == 0 and card['ari'] == cl.partition_scores_reference(table)['ari']
    assert host(out['counts']).sum() == 48 and (host(out['medoids']) >= 0).all()
