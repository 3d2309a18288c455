"""CPU tests of rovit_hip.density: the numpy fp64 statements that are the kernels' oracle (moments, covariance and Cholesky tables, scores,
OOD metrics), every refusal, the state dict, FeatureDensity / ood_metrics end to end on CPU tensors, and the Evaluator's defaults."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_cases as cases  # noqa: E402

from rovit_hip import native  # noqa: E402
from rovit_hip import density as D  # noqa: E402
from rovit_hip.native import RovitHipError  # noqa: E402


@pytest.fixture(scope='module')
def fitted():
    x, y = cases.make(600, 64, 4, seed=1)
    return x, y, D.density_reference(x, y, 4, 1e-3)


def test_reference_moments_against_a_direct_computation_and_np_cov(fitted):
    x, y, ref = fitted
    x64 = x.astype(np.float64)
    assert ref['n'] == ref['n_valid'] == 600 and ref['bad_labels'] == ref['bad_rows'] == 0
    assert ref['counts'].tolist() == [int((y == c).sum()) for c in range(4)]
    Sw = np.zeros((64, 64))
    for c in range(4):
        rows = x64[y == c]
        np.testing.assert_allclose(ref['class_means'][c], rows.mean(0), rtol=0, atol=1e-14)
        Sw += np.cov(rows, rowvar=False, bias=True) * rows.shape[0]
    np.testing.assert_allclose(ref['mean'], x64.mean(0), rtol=0, atol=1e-14)
    # centring on the class mean rounded to fp32 (what the device subtracts) moves S_w by n_c (mu - mu32)^2 ~ 1e-13 at most
    np.testing.assert_allclose(ref['scatter_within'], Sw, rtol=0, atol=1e-10)
    assert np.array_equal(ref['scatter_within'], ref['scatter_within'].T)
    # S_t = S_w + between-class scatter = the scatter about the global mean
    np.testing.assert_allclose(ref['scatter_total'], np.cov(x64, rowvar=False, bias=True) * 600, rtol=0, atol=1e-9)
    assert np.array_equal(ref['scatter_total'], ref['scatter_total'].T)


def test_covariance_is_symmetric_positive_definite_on_the_singular_rows(fitted):
    x, y, ref = fitted
    raw = ref['scatter_within'] / (600 - 4)
    assert np.linalg.eigvalsh(raw)[0] < 1e-9 * np.linalg.eigvalsh(raw)[-1]           # the LayerNorm direction: singular without shrinkage
    for k in ('covariance', 'background_covariance'):
        cov = ref[k]
        assert np.array_equal(cov, cov.T) and np.linalg.eigvalsh(cov)[0] > 0
    want = 0.999 * raw + 1e-3 * np.trace(raw) / 64 * np.eye(64)
    np.testing.assert_allclose(ref['covariance'], want, rtol=1e-14, atol=0)
    ev = np.linalg.eigvalsh(ref['covariance'])
    assert ref['condition_number'] == pytest.approx(ev[-1] / ev[0]) and 1e2 < ref['condition_number'] < 1e5


def test_cholesky_tables_reproduce_the_quadratic_form(fitted):
    x, y, ref = fitted
    s = D.stats_from_block(D.moments_block_from_arrays(x, y, 4), 64, 4)
    t = D.tables_from_stats(s, 1e-3)                                               # the fp64 tables
    assert np.array_equal(t['whitening'], np.tril(t['whitening'])) and np.array_equal(t['background_whitening'], np.tril(t['background_whitening']))
    f = x[:50].astype(np.float64)
    inv, inv0 = np.linalg.inv(t['covariance']), np.linalg.inv(t['background_covariance'])
    for c in range(4):
        d = f - s['class_means'][c][None]
        want = np.einsum('na,ab,nb->n', d, inv, d)
        got = (((f @ t['whitening'].T) - t['class_means'][c][None]) ** 2).sum(1)
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
    d = f - s['mean'][None]
    np.testing.assert_allclose((((f @ t['background_whitening'].T) - t['background_mean'][None]) ** 2).sum(1),
                               np.einsum('na,ab,nb->n', d, inv0, d), rtol=1e-9, atol=0)


def test_score_reference_definitions(fitted):
    x, y, ref = fitted
    lg = cases.logits(40, 4, seed=2)
    out = D.score_reference(x[:40], ref['tables'], lg)
    d = out['class_distances']
    assert d.shape == (40, 4) and np.array_equal(out['mahalanobis'], d.min(1)) and np.array_equal(out['nearest_class'], d.argmin(1))
    np.testing.assert_array_equal(out['relative_mahalanobis'], (d - out['background_distance'][:, None]).min(1))
    l = lg.astype(np.float64)
    lse = np.log(np.exp(l - l.max(1, keepdims=True)).sum(1)) + l.max(1)
    p = np.exp(l - lse[:, None])
    np.testing.assert_allclose(out['energy'], -lse, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(out['max_prob_score'], 1.0 - p.max(1), rtol=0, atol=1e-14)
    assert (out['nearest_class'] == y[:40]).mean() > 0.9                            # the rows were drawn around their class means
    assert 'energy' not in D.score_reference(x[:3], ref['tables'])


def test_every_refusal():
    x, y = cases.make(40, 32, 4, seed=3)
    with pytest.raises(RovitHipError, match='no valid row'):
        D.density_reference(x, np.where(y == 2, 0, y), 4)
    with pytest.raises(RovitHipError, match='no valid row.*bad_labels = 10'):
        D.density_reference(x, np.where(np.arange(40) % 4 == 1, 7, np.where(y == 1, 0, y)), 4)
    with pytest.raises(RovitHipError, match='n_valid must exceed'):
        D.density_reference(x[:4], np.arange(4), 4)
    bad = x.copy()
    bad[7, 3] = np.nan
    bad[9, 0] = np.inf
    with pytest.raises(RovitHipError, match='2 rows hold a non-finite feature'):
        D.density_reference(bad, y, 4)
    blk = D.moments_block_from_arrays(bad, np.where(np.arange(40) == 9, -1, y), 4)  # a bad label wins over a bad row
    assert blk[native.DENSITY_BAD_LABELS] == 1 and blk[native.DENSITY_BAD_ROWS] == 1 and blk[native.DENSITY_N_VALID] == 38
    for E, C in ((48, 4), (16, 4), (288, 4), (64, 1), (64, 9)):
        with pytest.raises(RovitHipError, match='embed_dim|num_classes'):
            D.FeatureDensity(C, E)
    for kw in ({'shrinkage': -0.1}, {'shrinkage': 2}, {'capacity': 0}):
        with pytest.raises(RovitHipError):
            D.FeatureDensity(4, 64, **kw)
    fd = D.FeatureDensity(4, 32)
    with pytest.raises(RovitHipError, match='nothing recorded'):
        fd.fit()
    with pytest.raises(RovitHipError, match='fit\\(\\)'):
        fd.score(torch.zeros(2, 32))
    with pytest.raises(RovitHipError, match='fit\\(\\)'):
        fd.state_dict()
    with pytest.raises(RovitHipError, match='features must be'):
        fd.update(torch.zeros(2, 31), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RovitHipError, match='features must be'):
        fd.update(torch.zeros(2, 32), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RovitHipError, match='integers'):
        fd.update(torch.zeros(2, 32), torch.zeros(2))


def test_feature_density_on_cpu_tensors_end_to_end_and_state_dict(tmp_path, fitted):
    x, y, ref = fitted
    fd = D.FeatureDensity(4, 64, capacity=16)
    for r0, r1 in ((0, 1), (1, 257), (257, 600)):                                    # the split of the rows changes nothing
        fd.update(torch.from_numpy(x[r0:r1]), torch.from_numpy(y[r0:r1]))
    assert fd.fit() is fd and fd.fitted and fd.n == 600 and fd.n_valid == 600
    assert np.array_equal(fd.result_block(), D.moments_block_from_arrays(x, y, 4))
    for k in ('counts', 'class_means', 'mean', 'scatter_within', 'covariance'):
        assert np.array_equal(getattr(fd, k), ref[k]), k
    assert fd.condition_number == ref['condition_number']
    for k in D.TABLE_KEYS:
        assert fd.tables[k].dtype == torch.float32 and np.array_equal(fd.tables[k].numpy(), ref['tables'][k])
    lg = cases.logits(33, 4, seed=5)
    out = fd.score(torch.from_numpy(x[:33]), torch.from_numpy(lg))
    want = D.score_reference(x[:33], ref['tables'], lg)
    assert set(out) == set(want) == {'class_distances', 'background_distance', 'mahalanobis', 'nearest_class', 'relative_mahalanobis', 'energy',
                                     'max_prob_score'}
    assert out['nearest_class'].dtype == torch.int32 and np.array_equal(out['nearest_class'].numpy(), want['nearest_class'])
    for k in want:
        if k != 'nearest_class':
            assert out[k].dtype == torch.float32 and np.array_equal(out[k].numpy(), want[k].astype(np.float32)), k
    assert set(fd.score(torch.from_numpy(x[:2]))) == set(want) - {'energy', 'max_prob_score'}
    torch.save(fd.state_dict(), tmp_path / 'density.pt')
    back = D.FeatureDensity(4, 64).load_state_dict(torch.load(tmp_path / 'density.pt'))
    assert back.fitted and back.n == 600 and back.shrinkage == fd.shrinkage and back.condition_number == fd.condition_number
    for k in D.STAT_KEYS:
        assert np.array_equal(getattr(back, k), getattr(fd, k)), k
    again = back.score(torch.from_numpy(x[:33]), torch.from_numpy(lg))
    assert all(torch.equal(again[k], out[k]) for k in out)
    with pytest.raises(RovitHipError, match='classes'):
        D.FeatureDensity(3, 64).load_state_dict(fd.state_dict())
    fd.update(torch.from_numpy(x[:1]), torch.from_numpy(y[:1]))                      # new rows invalidate the fit
    assert not fd.fitted


@pytest.mark.parametrize('n_in,n_out', [(1, 1), (2, 3), (40, 55), (255, 257)])
@pytest.mark.parametrize('kind', ['ties', 'equal', 'separated'])
def test_ood_metrics_reference_against_the_sorted_definitions(n_in, n_out, kind):
    a, b = cases.score_populations(n_in, n_out, kind, seed=n_in)
    got = D.ood_metrics_reference(a, b, tpr_levels=(0.95,))
    want = cases.sorted_definitions(a, b, 0.95)
    assert got['n_in'] == n_in and got['n_out'] == n_out
    assert got['auroc'] == want['auroc']                                             # a ratio of integers on both sides
    assert got['aupr_out'] == pytest.approx(want['aupr_out'], rel=1e-12) and got['aupr_in'] == pytest.approx(want['aupr_in'], rel=1e-12)
    assert got['thresholds'][0.95] == want['threshold'] and got['fpr_at_tpr'][0.95] == want['fpr']
    if kind == 'equal':
        assert got['auroc'] == 0.5 and got['fpr_at_tpr'][0.95] == 1.0
        assert got['aupr_out'] == pytest.approx(n_out / (n_in + n_out), rel=1e-12)
    if kind == 'separated':
        assert got['auroc'] == 1.0 and got['fpr_at_tpr'][0.95] == 0.0 and got['aupr_out'] == pytest.approx(1.0, rel=1e-12)
        assert got['aupr_in'] == pytest.approx(1.0, rel=1e-12)


def test_ood_metrics_on_cpu_tensors_levels_and_refusals():
    a, b = cases.score_populations(300, 200, 'ties', seed=9)
    got = D.ood_metrics(torch.from_numpy(a), torch.from_numpy(b), tpr_levels=(0.5, 0.95, 1.0))
    assert got == D.ood_metrics_reference(a, b, (0.5, 0.95, 1.0))
    assert list(got['fpr_at_tpr']) == [0.5, 0.95, 1.0] and got['thresholds'][1.0] == float(a.max())
    assert got['fpr_at_tpr'][0.5] <= got['fpr_at_tpr'][0.95] <= got['fpr_at_tpr'][1.0]
    blk = D.ood_block_reference(a, b, (0.5, 0.95, 1.0))
    assert blk[native.OOD_K:native.OOD_K + 3].tolist() == [150, 285, 300] and blk.shape == (native.OOD_WORDS,)
    bad = b.copy()
    bad[3] = np.nan
    with pytest.raises(RovitHipError, match='1 non-finite'):
        D.ood_metrics(torch.from_numpy(a), torch.from_numpy(bad))
    with pytest.raises(RovitHipError, match='TPR levels'):
        D.ood_metrics(torch.from_numpy(a), torch.from_numpy(b), tpr_levels=(0.0,))
    with pytest.raises(RovitHipError, match='TPR levels'):
        D.ood_metrics(torch.from_numpy(a), torch.from_numpy(b), tpr_levels=tuple([0.5] * 9))
    with pytest.raises(RovitHipError, match='scores'):
        D.ood_metrics(torch.from_numpy(a[:0]), torch.from_numpy(b))


def test_binding_matches_the_header():
    import ctypes
    lib = native.load()
    assert lib.rovit_density_workspace_bytes(0, 192, 4) == 0 and lib.rovit_density_workspace_bytes(10, 48, 4) == 0
    assert lib.rovit_density_workspace_bytes(10, 192, 9) == 0 and lib.rovit_ood_metrics_workspace_bytes(0, 5) == 0
    assert lib.rovit_ood_metrics_workspace_bytes(1 << 19, (1 << 19) + 1) == 0
    small, large = lib.rovit_density_workspace_bytes(256, 192, 4), lib.rovit_density_workspace_bytes(257, 192, 4)
    assert large - small >= 21 * 1024 * 4 and lib.rovit_density_workspace_bytes(1 << 22, 256, 8) < 64 << 20
    assert native.density_chunk_rows(65536) == 256 and native.density_chunk_rows(65537) == 512 and native.density_chunk_rows(1 << 22) == 16384
    assert native.density_offsets(192, 4)['words'] == 16 + 5 * 192 + 192 * 192
    # a bad descriptor is refused before any launch (no GPU is touched here)
    for d, name in ((native.DensityFit(), 'rovit_density_moments'), (native.DensityScores(), 'rovit_density_score'), (native.Ood(), 'rovit_ood_metrics')):
        assert getattr(lib, name)(ctypes.byref(d), None) != 0
        assert getattr(lib, name)(None, None) != 0


def test_cpu_evaluator_defaults_are_unchanged_and_density_adds_two_scores(tmp_path, capsys):
    from evaluation.evaluator import Evaluator

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(3)
            self.cls, self.sev = torch.nn.Linear(32, 4), torch.nn.Linear(32, 1)

        def forward(self, x):
            f = x.flatten(1)[:, :32]
            return {'cls_logits': self.cls(f), 'features': f, 'kan_severity': self.sev(f), 'mu': self.sev(f), 'log_var': -self.sev(f)}

    torch.manual_seed(5)
    data = [(torch.randn(b, 3, 224, 224), torch.randint(0, 4, (b,)), torch.randint(0, 4, (b,))) for b in (16, 16, 9)]
    names = ['Healthy Leaf', 'Leaf Holes', 'Black Spot', 'Dry Leaf']
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=names, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    fps_free = lambda t: [line for line in t.splitlines() if not line.startswith('FPS:')]
    ev = Evaluator(Tiny(), data, cfg, torch.device('cpu'))
    assert ev.density is None
    m = ev.evaluate()
    assert set(m) == {'accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece', 'fps', 'params',
                      'params_m', 'per_class'}
    text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    plain_sel = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate(selective=True)
    assert list(plain_sel['selective']['scores']) == ['confidence', 'entropy', 'sigma']
    fd = D.FeatureDensity(4, 32)
    model = Tiny()
    with torch.no_grad():
        for images, y, _ in data:
            fd.update(model(images)['features'], y)
    fd.fit()
    with_density = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate(density=fd)
    assert set(with_density) == set(m) and all(with_density[k] == m[k] for k in ('accuracy', 'macro_f1', 'mae', 'brier_score', 'ece', 'per_class'))
    assert fps_free((tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')) == fps_free(text)
    s = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate(selective=True, density=fd)
    assert list(s['selective']['scores']) == ['confidence', 'entropy', 'sigma', 'mahalanobis', 'relative_mahalanobis']
    assert s['selective']['scores']['sigma'] .keys() == plain_sel['selective']['scores']['sigma'].keys()
    assert 'relative_mahalanobis' in (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    capsys.readouterr()
    ood = [torch.randn(b, 3, 224, 224) * 4.0 for b in (16, 5)]
    cards = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate_ood(ood, density=fd)
    assert list(cards) == ['max_prob', 'entropy', 'energy', 'sigma', 'mahalanobis', 'relative_mahalanobis']
    assert all(c['n_in'] == 41 and c['n_out'] == 21 and 0.0 <= c['auroc'] <= 1.0 for c in cards.values())
    assert cards['mahalanobis']['auroc'] > 0.9                                       # four times the spread: far from the fitted rows
    printed = capsys.readouterr().out
    assert 'Out-of-distribution detection:' in printed and 'FPR@95%TPR' in printed and 'relative_mahalanobis' in printed
    assert list(Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate_ood(ood)) == ['max_prob', 'entropy', 'energy', 'sigma']
