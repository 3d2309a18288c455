"""CPU tests of rovit_hip.neighbors: the numpy statements that are the kernels' oracle against a brute-force double loop (the tie rule,
exclude, k > n_valid, bad rows, zero norms, the vote by hand), FeatureIndex end to end on CPU tensors, every refusal, and the Evaluator's
defaults."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbors_cases as cases  # noqa: E402

from rovit_hip import native  # noqa: E402
from rovit_hip import neighbors as NB  # noqa: E402
from rovit_hip.native import RovitHipError  # noqa: E402


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
@pytest.mark.parametrize('k', [1, 3, 7])
def test_search_reference_against_the_double_loop(metric, k):
    rows, y, sev, q = cases.float_case(40, 32, 3, 9, seed=k)
    ref = NB.search_reference(q, rows, k, metric)
    dist, idx = cases.brute_force(q, rows, k, metric)
    assert np.array_equal(ref['indices'], idx)
    np.testing.assert_allclose(ref['distances'], dist, rtol=0, atol=1e-12)
    assert ref['indices'].dtype == np.int64 and (np.diff(ref['distances'], axis=1) >= 0).all()


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_ties_on_duplicated_rows_go_to_the_lower_index(metric):
    base = cases.integer_rows(6, 32, seed=2) + 5.0                   # no zero row, no two rows parallel
    rows = np.concatenate([base, base])                              # row j and row j + 6 are the same
    ref = NB.search_reference(base, rows, 3, metric)
    assert np.array_equal(ref['indices'][:, 0], np.arange(6)) and np.array_equal(ref['indices'][:, 1], np.arange(6) + 6)
    assert (ref['distances'][:, 0] == ref['distances'][:, 1]).all()
    one = NB.search_reference(base, rows, 1, metric)                 # the pair cut by k keeps the lower index
    assert np.array_equal(one['indices'][:, 0], np.arange(6))
    dist, idx = cases.brute_force(base, rows, 3, metric)
    assert np.array_equal(ref['indices'], idx)


def test_exclude_bad_rows_and_k_above_the_valid_rows():
    rows = cases.integer_rows(7, 32, seed=3) + 4.0
    rows[2, 5], rows[4, 0] = np.inf, np.nan
    rows[6] = 0.0                                                    # a zero row: bad under cosine only
    q = np.concatenate([rows[:2], rows[2:3], np.zeros((1, 32), np.float32)])      # rows 0 and 1, the inf row, a zero row
    for metric, n_valid in (('l2', 5), ('cosine', 4)):
        b = NB.build_reference(rows, metric)
        assert (b['n'], b['n_valid'], b['bad_rows']) == (7, n_valid, 7 - n_valid)
        assert not b['valid'][2] and not b['valid'][4] and b['valid'][6] == (metric == 'l2')
        ref = NB.search_reference(q, rows, 6, metric)
        dist, idx = cases.brute_force(q, rows, 6, metric)
        assert np.array_equal(ref['indices'], idx)
        assert (ref['indices'][:2, :n_valid] >= 0).all() and (ref['indices'][:2, n_valid:] == -1).all()
        assert np.isinf(ref['distances'][:2, n_valid:]).all()
        assert not np.isin(ref['indices'], [2, 4]).any()
        assert (ref['indices'][2] == -1).all() and np.isinf(ref['distances'][2]).all()            # the bad query row
        assert ((ref['indices'][3] == -1).all()) == (metric == 'cosine')                          # a zero query is fine for l2
        assert ref['indices'][0, 0] == 0 and ref['indices'][1, 0] == 1
        ex = NB.search_reference(q, rows, 6, metric, exclude=np.array([0, 1, -1, 99]))
        dist, idx = cases.brute_force(q, rows, 6, metric, exclude=[0, 1, -1, 99])
        assert np.array_equal(ex['indices'], idx) and 0 not in ex['indices'][0] and 1 not in ex['indices'][1]
        assert ex['kth_distance'][0] == ex['distances'][0, n_valid - 2] and np.isinf(ex['kth_distance'][2])
    b = NB.build_reference(rows, 'cosine')
    assert not b['normalized'][6].any() and abs(np.linalg.norm(b['normalized'][0]) - 1.0) < 1e-12


def test_vote_against_a_hand_computation():
    d = np.array([[0.10, 0.17, 0.24, np.inf]])
    idx = np.array([[5, 2, 9, -1]])
    labels, sev = np.array([[1, 0, 1, -1]]), np.array([[2.0, 0.5, 3.0, np.nan]])
    v = NB.vote_reference(d, idx, labels, sev, num_classes=3, temperature=0.07)
    w = np.exp(-np.array([0.0, 0.07, 0.14]) / 0.07)                  # 1, 1/e, 1/e^2
    assert v['class_probs'][0] == pytest.approx([w[1] / w.sum(), (w[0] + w[2]) / w.sum(), 0.0], rel=1e-12)
    assert v['class'][0] == 1 and v['severity'][0] == pytest.approx((2.0 * w[0] + 0.5 * w[1] + 3.0 * w[2]) / w.sum(), rel=1e-12)
    assert v['kth_distance'][0] == 0.24 and v['mean_distance'][0] == pytest.approx(0.17, rel=1e-12)
    # a label outside [0, C) carries no vote but stays in the denominator; a tie goes to the lower class; no valid slot: -1, NaN, +inf
    v = NB.vote_reference(np.array([[0.2, 0.2], [np.inf, np.inf]]), np.array([[0, 1], [-1, -1]]), np.array([[7, 2], [-1, -1]]),
                          np.array([[1.0, 3.0], [np.nan, np.nan]]), num_classes=3)
    assert v['class_probs'][0].tolist() == [0.0, 0.0, 0.5] and v['class'].tolist() == [2, -1] and v['severity'][0] == 2.0
    assert np.isnan(v['severity'][1]) and np.isinf(v['kth_distance'][1]) and np.isinf(v['mean_distance'][1]) and not v['class_probs'][1].any()
    v = NB.vote_reference(np.array([[0.3, 0.3]]), np.array([[4, 8]]), np.array([[2, 1]]), None, num_classes=3)
    assert v['class'][0] == 1 and 'severity' not in v


@pytest.mark.parametrize('metric', ['l2', 'cosine'])
def test_feature_index_on_cpu_tensors_splits_and_state_dict(tmp_path, metric):
    rows, y, sev, q = cases.float_case(300, 64, 4, 33, seed=5)
    t = torch.from_numpy

    def index(edges):
        fi = NB.FeatureIndex(64, 4, metric, capacity=16)
        for r0, r1 in zip(edges[:-1], edges[1:]):
            fi.update(t(rows[r0:r1]), t(y[r0:r1]), t(sev[r0:r1]))
        return fi.build()
    fi = index([0, 300])
    out = fi.search(t(q), k=5)
    assert list(out) == ['distances', 'indices', 'labels', 'severities', 'kth_distance', 'mean_distance', 'class_probs', 'class', 'severity']
    assert out['indices'].dtype == torch.int32 and out['class'].dtype == torch.int32 and out['distances'].dtype == torch.float32
    ref = NB.search_reference(q, rows, 5, metric, class_labels=y, severity=sev, num_classes=4)
    assert np.array_equal(out['indices'].numpy(), ref['indices']) and np.array_equal(out['class'].numpy(), ref['class'])
    assert np.array_equal(out['labels'].numpy(), y[ref['indices']])
    for edges in ([0, 1, 300], [0, 17, 18, 200, 300]):
        other = index(edges).search(t(q), k=5)
        assert all(torch.equal(other[name], out[name]) for name in out), edges
    assert fi.counts() == {'n': 300, 'n_valid': 300, 'bad_rows': 0}
    torch.save(fi.state_dict(), tmp_path / 'index.pt')
    back = NB.FeatureIndex(64).load_state_dict(torch.load(tmp_path / 'index.pt'))
    assert back.metric == metric and back.num_classes == 4 and back.n == 300
    again = back.search(t(q), k=5)
    assert all(torch.equal(again[name], out[name]) for name in out)
    loo = fi.search(t(rows), k=3, exclude=torch.arange(300))
    assert not (loo['indices'] == torch.arange(300)[:, None]).any()
    bare = NB.FeatureIndex(64, None, metric)
    bare.update(t(rows))
    assert list(bare.search(t(q), k=2)) == ['distances', 'indices', 'kth_distance', 'mean_distance']
    fi.reset()
    assert fi.n == 0 and not fi.built


def test_every_refusal():
    t = torch.from_numpy
    rows = cases.integer_rows(10, 32, seed=1)
    for bad in (dict(embed_dim=48), dict(embed_dim=288), dict(num_classes=0), dict(num_classes=native.KNN_MAX_CLASSES + 1), dict(metric='dot'),
                dict(capacity=0)):
        with pytest.raises(RovitHipError):
            NB.FeatureIndex(**bad)
    fi = NB.FeatureIndex(32, 3)
    with pytest.raises(RovitHipError, match='nothing recorded'):
        fi.search(t(rows))
    with pytest.raises(RovitHipError, match='nothing recorded'):
        fi.build()
    with pytest.raises(RovitHipError, match='features must be'):
        fi.update(t(rows[:, :16]))
    with pytest.raises(RovitHipError, match='integers'):
        fi.update(t(rows), torch.zeros(10))
    fi.update(t(rows), torch.zeros(10, dtype=torch.int64))
    with pytest.raises(RovitHipError, match='columns of the first'):
        fi.update(t(rows))
    with pytest.raises(RovitHipError, match='columns of the first'):
        fi.update(t(rows), torch.zeros(10, dtype=torch.int64), torch.zeros(10))
    for k in (0, native.KNN_MAX_K + 1, 2.0):
        with pytest.raises(RovitHipError, match='k must be'):
            fi.search(t(rows), k=k)
    with pytest.raises(RovitHipError, match='temperature'):
        fi.search(t(rows), temperature=0.0)
    with pytest.raises(RovitHipError, match='exclude'):
        fi.search(t(rows), exclude=torch.arange(9))
    with pytest.raises(RovitHipError, match='exclude'):
        fi.search(t(rows), exclude=torch.zeros(10))
    with pytest.raises(RovitHipError, match='features must be'):
        fi.search(t(rows[:, :16]))
    with pytest.raises(RovitHipError):
        NB.search_reference(rows, rows[:, :16], 3)
    assert native.KNN_MAX_K == 32


def test_binding_matches_the_header():
    lib = native.load()
    assert lib.rovit_knn_workspace_bytes(0, 100, 192, 10) == 0 and lib.rovit_knn_workspace_bytes(5, 100, 48, 10) == 0
    assert lib.rovit_knn_workspace_bytes(5, 100, 192, 33) == 0 and lib.rovit_knn_workspace_bytes(5, 100, 192, 0) == 0
    assert lib.rovit_knn_workspace_bytes(5, (1 << 22) + 1, 192, 10) == 0
    # the keys of every split: 65 536 queries against 65 536 rows need one split, one tile of queries 64 of them
    big, wide = lib.rovit_knn_workspace_bytes(65536, 65536, 192, 10), lib.rovit_knn_workspace_bytes(64, 65536, 192, 10)
    assert big == 65536 * (4 + 4 + 16 * 8) and wide == 64 * (4 + 4 + 64 * 16 * 8)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rovit_hip.h')).read()
    assert f'#define ROVIT_KNN_MAX_K {native.KNN_MAX_K}\n' in header and f'#define ROVIT_KNN_QUERY_TILE {native.KNN_QUERY_TILE}\n' in header
    # a bad descriptor is refused before any launch (no GPU is touched here)
    for d, name in ((native.KnnIndex(), 'rovit_knn_build'), (native.KnnQuery(), 'rovit_knn_search')):
        assert getattr(lib, name)(ctypes.byref(d), None) != 0
        assert getattr(lib, name)(None, None) != 0


def test_cpu_evaluator_defaults_are_unchanged_and_an_index_adds_its_card(tmp_path, capsys):
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
    fps_free = lambda text: [line for line in text.splitlines() if not line.startswith('FPS:')]
    plain_keys = {'accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece', 'fps', 'params', 'params_m',
                  'per_class'}
    ev = Evaluator(Tiny(), data, cfg, torch.device('cpu'))
    assert ev.index is None
    m = ev.evaluate()
    assert set(m) == plain_keys
    text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    assert 'Nearest neighbours' not in text and 'Nearest neighbours' not in capsys.readouterr().out
    assert list(Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate(selective=True)['selective']['scores']) == ['confidence', 'entropy', 'sigma']
    fi = NB.FeatureIndex(32, 4)
    model = Tiny()
    with torch.no_grad():
        for images, y, s in data:
            fi.update(model(images)['features'], y, s.float())
    fi.build()
    with_index = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate(index=fi, knn_k=1)
    assert set(with_index) == plain_keys | {'knn'}
    assert all(with_index[k] == m[k] for k in ('accuracy', 'macro_f1', 'mae', 'brier_score', 'ece', 'per_class'))
    # every test row is in the index: its nearest neighbour is itself, so the vote returns its label and its severity
    assert with_index['knn'] == {'k': 1, 'accuracy': 100.0, 'severity_mae': 0.0, 'agreement': pytest.approx(m['accuracy'] / 100.0, rel=1e-12)}
    new_text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    assert fps_free(new_text)[:len(fps_free(text))] == fps_free(text) and 'Nearest neighbours (k = 1):' in new_text
    assert 'Vote accuracy:' in capsys.readouterr().out
    s = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate(selective=True, index=fi)
    assert list(s['selective']['scores']) == ['confidence', 'entropy', 'sigma', 'knn_distance'] and s['knn']['k'] == 10
    ood = [torch.randn(b, 3, 224, 224) * 4.0 for b in (16, 5)]
    cards = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate_ood(ood, index=fi)
    assert list(cards) == ['max_prob', 'entropy', 'energy', 'sigma', 'knn'] and cards['knn']['n_in'] == 41 and cards['knn']['n_out'] == 21
    assert list(Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate_ood(ood)) == ['max_prob', 'entropy', 'energy', 'sigma']
