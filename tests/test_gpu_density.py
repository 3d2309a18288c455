"""GPU tests of csrc/density.hip through rovit_hip.density: the moments kernel, the score kernel and the OOD-metric kernel against the
numpy fp64 statements, their determinism, and the model / Evaluator entry points end to end.

Measured on the MI355X over the cases below (printed by the tests before they assert):
  scatter   max |S - S_ref| / sum_i |x_ia x_ib|  = 6.684e-07 (n = 300, E = 256, C = 2; 1.0e-07 .. 6.7e-07 over the eight cases), against the
            cap (R + 2) 2^-24 = 1.54e-05
  score     max error / derived bound over all class and background distances = 2.043e-02 (30 cases; 1.2e-03 .. 2.0e-02)
  AP sums   max relative difference from the reference = 2.569e-16 (the first 12 cases; MEASURED_AP_REL below stays at that figure);
            3.517e-16 over all 21 with n_in = 1023, 1024, 1025 around the rank kernel's 1024-row tile (n_in = 1025, `equal`)
  end to end: Mahalanobis AUROC of Gaussian-noise images against the 48 fitted images = 1.0000
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
import density_cases as cases  # noqa: E402
from oracle import ref_cpu  # noqa: E402  (checker only)

from rovit_hip import native  # noqa: E402
from rovit_hip import density as D  # noqa: E402
from rovit_hip.native import RovitHipError  # noqa: E402

pytestmark = pytest.mark.gpu

R, TILE = native.DENSITY_CHUNK_ROWS, native.DENSITY_SCORE_TILE
U32 = 2.0 ** -24

# The largest ratios the MI355X gave over the cases of this file (None: not measured yet, the derived caps alone then hold).
MEASURED_SCATTER_RATIO = 6.684e-07
MEASURED_SCORE_RATIO = 2.043e-02
MEASURED_AP_REL = 2.569e-16

MOMENT_CASES = [(3, 32, 2), (5, 32, 4), (R - 1, 64, 4), (R, 64, 4), (R + 1, 64, 4), (5 * R + 77, 192, 4), (300, 192, 8), (300, 256, 2)]


def dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def moment_case(n, E, C):
    x, y = cases.make(n, E, C, seed=n + E + C)
    if n >= R - 1:
        y = cases.with_bad_labels(y, C, seed=n)
    blk = D.moments_block_from_arrays(x, y, C)
    blk.setflags(write=False)
    return x, y, blk


def device_block(x, y, C, splits=None, max_workgroups=0):
    fd = D.FeatureDensity(C, x.shape[1], capacity=64)
    fd.max_workgroups = max_workgroups
    edges = [0, x.shape[0]] if splits is None else splits
    for r0, r1 in zip(edges[:-1], edges[1:]):
        fd.update(torch.from_numpy(x[r0:r1]).to(dev()), torch.from_numpy(y[r0:r1]).to(dev()))
    return fd.result_block()


@pytest.mark.parametrize('n,E,C', MOMENT_CASES)
def test_moments_against_the_fp64_reference(n, E, C):
    """Integer words exact; each mean within n_c 2^-53 (capped at 1e-12) of the column's largest magnitude, against an 80-bit sum;
    |S - S_ref|[a,b] <= min((R + 2) 2^-24, 4 x measured) sum_i |x_ia x_ib|: the first term is the worst case of an fp32 fma chain of R
    products plus the two centring roundings.  S exactly symmetric."""
    x, y, ref = moment_case(n, E, C)
    blk = device_block(x, y, C)
    o = native.density_offsets(E, C)
    assert np.array_equal(blk[:native.DENSITY_HEADER], ref[:native.DENSITY_HEADER])
    s, sr = D.stats_from_block(blk, E, C), D.stats_from_block(ref, E, C)
    assert s['bad_labels'] == int(((y < 0) | (y >= C)).sum()) and (n < R - 1 or s['bad_labels'] > 0)
    valid = (y >= 0) & (y < C)
    xl = x.astype(np.longdouble)
    for c in range(C):
        rows = xl[valid & (y == c)]
        if rows.shape[0] == 0:
            assert not s['class_means'][c].any()
            continue
        exact = (rows.sum(0) / rows.shape[0]).astype(np.float64)
        tol = min(rows.shape[0] * 2.0 ** -53, 1e-12) * np.abs(rows).max(0).astype(np.float64)
        assert (np.abs(s['class_means'][c] - exact) <= tol).all(), c
    exact = (xl[valid].sum(0) / valid.sum()).astype(np.float64)
    assert (np.abs(s['mean'] - exact) <= min(int(valid.sum()) * 2.0 ** -53, 1e-12) * np.abs(x[valid]).max(0)).all()
    S, Sref = s['scatter_within'], sr['scatter_within']
    assert np.array_equal(S, S.T)
    centred = np.abs(x[valid].astype(np.float64) - sr['class_means'][y[valid]].astype(np.float32).astype(np.float64))
    denom = centred.T @ centred
    ratio = float((np.abs(S - Sref) / denom).max())
    print(f'scatter ratio n={n} E={E} C={C}: {ratio:.3e}')
    cap = (native.density_chunk_rows(n) + 2) * U32
    bound = cap if MEASURED_SCATTER_RATIO is None else min(cap, 4 * MEASURED_SCATTER_RATIO)
    assert ratio <= bound
    assert blk.shape == (o['words'],)


def test_moments_block_is_bit_identical_across_runs_splits_and_grids():
    n, E, C = MOMENT_CASES[5]
    x, y, _ = moment_case(n, E, C)
    first = device_block(x, y, C)
    assert np.array_equal(first, device_block(x, y, C))
    for splits in ([0, 1, n], [0, R - 3, R + 5, 3 * R, n], [0] + list(range(100, n, 100)) + [n]):
        assert np.array_equal(first, device_block(x, y, C, splits=splits)), splits
    for cap in (1, 3):
        assert np.array_equal(first, device_block(x, y, C, max_workgroups=cap)), cap
    n, E, C = MOMENT_CASES[7]
    x, y, _ = moment_case(n, E, C)
    assert np.array_equal(device_block(x, y, C), device_block(x, y, C, splits=[0, 7, n], max_workgroups=1))


def test_fit_on_the_device_raises_after_the_copy_and_matches_the_host_fit():
    x, y = cases.make(400, 64, 4, seed=11)
    fd = D.FeatureDensity(4, 64)
    fd.update(torch.from_numpy(x).to(dev()), torch.from_numpy(y))                    # host labels are copied up
    fd.fit()
    ref = D.density_reference(x, y, 4)
    assert fd.counts.tolist() == ref['counts'].tolist() and fd.tables['whitening'].is_cuda
    np.testing.assert_allclose(fd.covariance, ref['covariance'], rtol=0, atol=2e-6 * np.abs(ref['covariance']).max())
    # the smallest eigenvalue is the shrinkage floor, ~1e-4 of the largest: a scatter error of 1e-6 of the largest moves it by a per cent
    assert fd.condition_number == pytest.approx(ref['condition_number'], rel=5e-2)
    bad = x.copy()
    bad[17, 5] = np.inf
    fd.reset()
    fd.update(torch.from_numpy(bad).to(dev()), torch.from_numpy(y).to(dev()))
    with pytest.raises(RovitHipError, match='1 rows hold a non-finite feature'):
        fd.fit()
    fd.reset()
    fd.update(torch.from_numpy(x).to(dev()), torch.from_numpy(np.where(y == 3, 9, y)).to(dev()))
    with pytest.raises(RovitHipError, match='no valid row'):
        fd.fit()


@functools.lru_cache(maxsize=None)
def score_case(E, C):
    """A host fit on 600 rows, 257 more rows of the same classes to score, logits, and the fp64 reference on the fp32 tables."""
    x, y = cases.make(600 + 257, E, C, seed=E + C)
    host = D.FeatureDensity(C, E)
    host.update(torch.from_numpy(x[:600]), torch.from_numpy(y[:600]))
    host.fit()
    fd = D.FeatureDensity(C, E).load_state_dict(host.state_dict(), device=dev())
    rows, lg = x[600:], cases.logits(257, C, seed=E)
    ref = D.score_reference(rows, host.tables, lg)
    f = rows.astype(np.float64)
    bounds = {}
    for name, wk, mk in (('class', 'whitening', 'class_means'), ('background', 'background_whitening', 'background_mean')):
        W, M = host.tables[wk].numpy().astype(np.float64), host.tables[mk].numpy().astype(np.float64).reshape(-1, E)
        z, az = f @ W.T, np.abs(f) @ np.abs(W).T
        t = np.abs(z[:, None, :] - M[None])
        d = (t ** 2).sum(-1)
        bounds[name] = 2.0 * (t * ((E + 1) * U32 * az + U32 * np.abs(z))[:, None, :]).sum(-1) + (E + 2) * U32 * d
    return fd, rows, lg, ref, bounds


@pytest.mark.parametrize('E,C', [(32, 2), (32, 4), (32, 8), (192, 2), (192, 4), (192, 8)])
@pytest.mark.parametrize('B', [1, TILE - 1, TILE, TILE + 1, 257])
def test_score_against_the_fp64_reference_on_the_same_tables(B, E, C):
    """Per distance: error <= 2 sum_k |z_k - M_ck| ((E + 1) u (|W||f|)_k + u |z_k|) + (E + 2) u d_c, u = 2^-24 (the whitening's fma chain
    of at most E products, the subtraction, the squares' chain), and under that cap 4 x the measured maximum of error / bound."""
    fd, rows, lg, ref, bounds = score_case(E, C)
    out = fd.score(torch.from_numpy(rows[:B]).to(dev()), torch.from_numpy(lg[:B]).to(dev()))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got['class_distances'].shape == (B, C) and got['nearest_class'].dtype == np.int32
    factor = 1.0 if MEASURED_SCORE_RATIO is None else min(1.0, 4 * MEASURED_SCORE_RATIO)
    err = np.abs(got['class_distances'].astype(np.float64) - ref['class_distances'][:B])
    err0 = np.abs(got['background_distance'].astype(np.float64) - ref['background_distance'][:B])
    bc, b0 = bounds['class'][:B], bounds['background'][:B, 0]
    print(f'score ratio B={B} E={E} C={C}: {max(float((err / bc).max()), float((err0 / b0).max())):.3e}')
    assert (err <= factor * bc).all() and (err0 <= factor * b0).all()
    # the minimum and its index are those of the device's own distances, the lowest index on a tie
    assert np.array_equal(got['mahalanobis'], got['class_distances'].min(1)) and np.array_equal(got['nearest_class'], got['class_distances'].argmin(1))
    rel = (got['class_distances'] - got['background_distance'][:, None]).min(1)
    assert np.array_equal(got['relative_mahalanobis'], rel)
    srt = np.sort(ref['class_distances'][:B], axis=1)
    decided = (srt[:, 1] - srt[:, 0]) > 2 * bc.max(1)
    assert decided.mean() >= 0.95 and np.array_equal(got['nearest_class'][decided], ref['nearest_class'][:B][decided])
    for k in ('energy', 'max_prob_score'):
        want = ref[k][:B].astype(np.float32)
        assert (np.abs(got[k].astype(np.float64) - want.astype(np.float64)) <= 4 * np.spacing(np.abs(want)).astype(np.float64)).all(), k
    again = fd.score(torch.from_numpy(rows[:B]).to(dev()), torch.from_numpy(lg[:B]).to(dev()))
    assert all(torch.equal(again[k], out[k]) for k in out)
    if B == 257:
        fd.max_workgroups = 2
        try:
            capped = fd.score(torch.from_numpy(rows[:B]).to(dev()))
        finally:
            fd.max_workgroups = 0
        assert set(capped) == set(out) - {'energy', 'max_prob_score'} and all(torch.equal(capped[k], out[k]) for k in capped)


@pytest.mark.parametrize('n_in,n_out', [(1, 1), (2, 3), (255, 257), (1027, 600), (1023, 600), (1024, 600), (1025, 600)])
@pytest.mark.parametrize('kind', ['ties', 'equal', 'separated'])
def test_ood_metrics_against_the_reference(n_in, n_out, kind):
    """Every integer word and every threshold equal to the reference's; the two AP sums within min(1e-9, 8 x measured) relative; the
    block bit-identical across runs and grids."""
    a, b = cases.score_populations(n_in, n_out, kind, seed=n_in)
    levels = (0.5, 0.95, 1.0)
    ref = D.ood_block_reference(a, b, levels)
    ta, tb = torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev())
    blk = D.ood_block(ta, tb, levels)
    assert np.array_equal(blk[:native.OOD_AP_OUT_SUM], ref[:native.OOD_AP_OUT_SUM])
    f, fr = blk.view(np.float64), ref.view(np.float64)
    rel = max(abs(f[i] - fr[i]) / fr[i] for i in (native.OOD_AP_OUT_SUM, native.OOD_AP_IN_SUM))
    print(f'AP relative difference n_in={n_in} n_out={n_out} {kind}: {rel:.3e}')
    assert rel <= (1e-9 if MEASURED_AP_REL is None else min(1e-9, max(8 * MEASURED_AP_REL, 2.0 ** -52)))
    assert np.array_equal(blk, D.ood_block(ta, tb, levels))
    for cap in (1, 3):
        assert np.array_equal(blk, D.ood_block(ta, tb, levels, max_workgroups=cap)), cap
    got, want = D.ood_metrics(ta, tb, levels), cases.sorted_definitions(a, b, 0.95)
    assert got['auroc'] == want['auroc'] and got['fpr_at_tpr'][0.95] == want['fpr'] and got['thresholds'][0.95] == want['threshold']
    assert got['aupr_out'] == pytest.approx(want['aupr_out'], rel=1e-9) and got['aupr_in'] == pytest.approx(want['aupr_in'], rel=1e-9)


def test_ood_metrics_raises_on_non_finite_scores_after_the_copy():
    a, b = cases.score_populations(255, 257, 'ties', seed=4)
    a[200], b[3] = np.nan, np.inf
    with pytest.raises(RovitHipError, match='2 non-finite scores among 255 \\+ 257'):
        D.ood_metrics(torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev()))


CLASS_NAMES = ['Healthy Leaf', 'Leaf Holes', 'Black Spot', 'Dry Leaf']


def test_model_and_evaluator_end_to_end(tmp_path):
    """48 images in batches of 16 on the oracle-initialised model: fit_feature_density on a loader equals FeatureDensity fed the same
    features by hand, bit for bit; Gaussian-noise images lie farther from the fitted features than the fitted images (AUROC > 0.5: a sanity
    direction, not a quality claim); the Evaluator lists the two new scores with a density and keeps its keys without one."""
    from evaluation.evaluator import Evaluator
    from models.rovit_kan import RoViTKAN
    model = RoViTKAN(pretrained=False)
    model.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    model = model.to(dev()).eval()
    g = torch.Generator().manual_seed(0)
    smooth = torch.nn.functional.interpolate(torch.randn(48, 3, 7, 7, generator=g), size=224, mode='bilinear', align_corners=False)
    labels = torch.arange(48) % 4
    loader = [(smooth[i:i + 16], labels[i:i + 16], labels[i:i + 16]) for i in range(0, 48, 16)]
    fd = model.fit_feature_density(loader)
    by_hand = D.FeatureDensity(4, 192)
    with torch.no_grad():
        for images, y, _ in loader:
            by_hand.update(model.backbone(images.to(dev())), y)
    by_hand.fit()
    assert fd.n == 48 and fd.n_valid == 48 and np.array_equal(fd.result_block(), by_hand.result_block())
    assert all(torch.equal(fd.tables[k], by_hand.tables[k]) for k in D.TABLE_KEYS)
    from_tensor = model.fit_feature_density(smooth.to(dev()), labels, chunk=16)
    assert np.array_equal(from_tensor.result_block(), fd.result_block())
    inside = model.ood_scores(smooth.to(dev()), fd)
    outside = model.ood_scores(torch.randn(48, 3, 224, 224, generator=g).to(dev()), fd)
    assert set(inside) == {'class_distances', 'background_distance', 'mahalanobis', 'nearest_class', 'relative_mahalanobis', 'energy', 'max_prob_score'}
    card = D.ood_metrics(inside['mahalanobis'], outside['mahalanobis'])
    print(f"mahalanobis AUROC of noise against the fitted images: {card['auroc']:.4f}")
    assert card['auroc'] > 0.5
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=CLASS_NAMES, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    plain = Evaluator(model, loader, cfg, dev()).evaluate(selective=True)
    assert set(plain) == {'accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece', 'fps', 'params',
                          'params_m', 'per_class', 'selective'}
    assert list(plain['selective']['scores']) == ['confidence', 'entropy', 'sigma']
    ev = Evaluator(model, loader, cfg, dev())
    assert ev.fit_density(loader) is ev.density and np.array_equal(ev.density.result_block(), fd.result_block())
    with_density = ev.evaluate(selective=True, density=ev.density)
    assert set(with_density) == set(plain)
    assert list(with_density['selective']['scores']) == ['confidence', 'entropy', 'sigma', 'mahalanobis', 'relative_mahalanobis']
    cards = ev.evaluate_ood([torch.randn(16, 3, 224, 224, generator=g) for _ in range(2)], density=ev.density)
    assert list(cards) == ['max_prob', 'entropy', 'energy', 'sigma', 'mahalanobis', 'relative_mahalanobis']
    assert all(c['n_in'] == 48 and c['n_out'] == 32 for c in cards.values()) and cards['mahalanobis']['auroc'] > 0.5
