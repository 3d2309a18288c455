"""CPU tests of the evaluation surface: rovit_eval_accumulate / rovit_eval_finalize refuse bad descriptors before anything is launched;
the host restatement (rovit_hip.evaluation) and every evaluation.metrics function reproduce what the reference's evaluation/metrics.py
returned on tests/golden/eval_metrics.npz (tools/make_eval_golden.py), and sklearn / scipy directly where they import.

Bound of the float comparisons, 1e-9: fp64 sums of at most 4 099 terms of size at most 2 carry at most 4 099 * 2^-52 ~ 1e-12 of rounding
(percent values: 1e-10), so 1e-9 leaves three orders of margin.  Counts and supports must be equal."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

TOL = 1e-9
CASES = ('full', 'absent', 'constant')
FLOATS = ('accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'brier_score', 'ece')


@pytest.fixture(scope='module')
def native():
    from rovit_hip import native as n
    if not os.path.exists(n.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    n.load()
    return n


@pytest.fixture(scope='module')
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, 'eval_metrics.npz'))
    return {c: {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(c + '/')} for c in CASES}, [str(s) for s in z['class_names']]


def close(got, want, tol=TOL):
    got, want = float(got), float(want)
    if np.isnan(want):
        return np.isnan(got)
    return abs(got - want) <= tol


def test_abi_version(native):
    assert native.ABI_VERSION == 440 and native.load().rovit_version() == 440


def _batch(native, **kw):
    d = native.EvalBatch()
    d.batch, d.num_classes, d.offset, d.capacity, d.severity_is_int64, d.loss_row, d.loss_capacity = 8, 4, 0, 64, 1, 0, 4
    # dummy non-null, 16-byte aligned addresses: every call here is refused before a launch, so nothing is dereferenced
    for f in ('cls_logits', 'kan_severity', 'log_var', 'class_labels', 'severity_labels', 'losses', 'probs', 'pred', 'label', 'sev_pred',
              'sev_true', 'uncertainty', 'loss_table'):
        setattr(d, f, 64)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _final(native, **kw):
    d = native.EvalFinal()
    d.n, d.num_classes, d.n_bins, d.n_loss_rows = 100, 4, 10, 0
    for f in ('probs', 'pred', 'label', 'sev_pred', 'sev_true', 'loss_table', 'bin_edges', 'rank_counts', 'partials', 'result'):
        setattr(d, f, 64)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize('kw,match', [({'num_classes': 1}, 'classes'), ({'num_classes': 9}, 'classes'), ({'batch': 0}, 'batch'),
                                      ({'offset': 60}, 'capacity'), ({'offset': -1}, 'capacity'), ({'capacity': (1 << 20) + 1}, 'capacity'),
                                      ({'cls_logits': None}, 'null'), ({'class_labels': None}, 'null'), ({'severity_labels': None}, 'null'),
                                      ({'probs': None}, 'null'), ({'uncertainty': None}, 'null'), ({'loss_row': 4}, 'loss row'),
                                      ({'loss_table': None}, 'loss row'), ({'cls_logits': 66}, 'aligned'), ({'class_labels': 68}, 'aligned'),
                                      ({'severity_labels': 68}, 'aligned'), ({'probs': 72}, '16-byte'), ({'label': 68}, '16-byte')])
def test_accumulate_rejects_bad_descriptors(native, kw, match):
    with pytest.raises(native.RovitHipError, match=match):
        native.call('rovit_eval_accumulate', ctypes.byref(_batch(native, **kw)), None)
    with pytest.raises(native.RovitHipError, match='null descriptor'):
        native.call('rovit_eval_accumulate', None, None)


@pytest.mark.parametrize('kw,match', [({'num_classes': 1}, 'classes'), ({'num_classes': 9}, 'classes'), ({'n': 0}, 'rows'),
                                      ({'n': (1 << 20) + 1}, 'rows'), ({'n_bins': 0}, 'bins'), ({'n_bins': 65}, 'bins'),
                                      ({'n_loss_rows': -1}, 'loss rows'), ({'n_loss_rows': 3, 'loss_table': None}, 'no loss table'),
                                      ({'probs': None}, 'null'), ({'sev_true': None}, 'null'), ({'bin_edges': None}, 'null'),
                                      ({'rank_counts': None}, 'null'), ({'partials': None}, 'null'), ({'result': None}, 'null'),
                                      ({'pred': 68}, '16-byte'), ({'bin_edges': 68}, 'not aligned'), ({'result': 68}, 'not aligned'),
                                      ({'rank_counts': 72}, 'not aligned')])
def test_finalize_rejects_bad_descriptors(native, kw, match):
    with pytest.raises(native.RovitHipError, match=match):
        native.call('rovit_eval_finalize', ctypes.byref(_final(native, **kw)), None)
    with pytest.raises(native.RovitHipError, match='null descriptor'):
        native.call('rovit_eval_finalize', None, None)


def test_partials_size_and_constructor_checks(native):
    from rovit_hip.evaluation import EvalAccumulator
    lib = native.load()
    assert lib.rovit_eval_partials_doubles(1) == 66 and lib.rovit_eval_partials_doubles(257) == 2 * 66 and lib.rovit_eval_partials_doubles(0) == 0
    for kw in ({'num_classes': 1}, {'num_classes': 9}, {'num_classes': 4, 'n_bins': 0}, {'num_classes': 4, 'n_bins': 65},
               {'num_classes': 4, 'capacity': 0}, {'num_classes': 4, 'capacity': (1 << 20) + 1}):
        with pytest.raises(native.RovitHipError):
            EvalAccumulator(**kw)
    acc = EvalAccumulator(4)
    with pytest.raises(native.RovitHipError, match='nothing recorded'):
        acc.compute()
    with pytest.raises(native.RovitHipError, match='cls_logits'):
        acc.update({'cls_logits': torch.zeros(3, 5)}, torch.zeros(3, dtype=torch.long), torch.zeros(3, dtype=torch.long))
    with pytest.raises(native.RovitHipError, match='class_labels'):
        acc.update({'cls_logits': torch.zeros(3, 4)}, torch.zeros(2, dtype=torch.long), torch.zeros(3, dtype=torch.long))


def test_metrics_functions_reproduce_the_reference_results(golden):
    from evaluation import metrics as M
    cases, names = golden
    for c, g in cases.items():
        y, pred, probs = g['labels'], g['pred'], g['probs'].astype(np.float64)
        st, sp = g['sev_true'], g['sev_pred'].astype(np.float64)
        got = {'accuracy': M.accuracy(y, pred), 'macro_f1': M.macro_f1(y, pred), 'weighted_f1': M.weighted_f1(y, pred), 'mae': M.mae(st, sp),
               'spearman_rho': M.spearman_rho(st, sp), 'brier_score': M.brier_score(y, probs), 'ece': M.ece(y, probs),
               'ece_15': M.ece(y, probs, n_bins=15)}
        for k, v in got.items():
            print(c, k, v, float(g[k]), abs(v - float(g[k])))
            assert close(v, g[k]), (c, k, v, float(g[k]))
        assert np.array_equal(M.compute_confusion_matrix(y, pred, names), g['confusion'])
        pc = M.per_class_metrics(y, pred, names)
        assert list(pc) == names
        for i, n in enumerate(names):
            assert pc[n]['support'] == int(g['per_class_support'][i])
            for f in ('precision', 'recall', 'f1'):
                assert close(pc[n][f], g['per_class_' + f][i]), (c, n, f)
    assert np.isnan(M.spearman_rho(cases['constant']['sev_true'], cases['constant']['sev_pred']))


def test_host_restatement_reproduces_the_reference_results(golden):
    from rovit_hip import native as N
    from rovit_hip.evaluation import metrics_from_block, result_block_from_arrays
    cases, names = golden
    for c, g in cases.items():
        blk = result_block_from_arrays(g['labels'], g['pred'], g['probs'], g['sev_true'], g['sev_pred'], 4, 10)
        m = metrics_from_block(blk, 4, 10)
        for k in FLOATS:
            print(c, k, m[k], float(g[k]))
            assert close(m[k], g[k]), (c, k, m[k], float(g[k]))
        assert m['spearman'] == m['spearman_rho'] or (np.isnan(m['spearman']) and np.isnan(m['spearman_rho']))
        assert np.array_equal(m['confusion_matrix'], g['confusion']) and m['n'] == len(g['labels'])
        assert int(blk[N.EVAL_BIN_COUNT:N.EVAL_BIN_COUNT + 10].sum()) == len(g['labels'])
        for i in range(4):
            assert m['per_class'][i]['support'] == int(g['per_class_support'][i])
            for f in ('precision', 'recall', 'f1'):
                assert close(m['per_class'][i][f], g['per_class_' + f][i]), (c, i, f)
        m15 = metrics_from_block(result_block_from_arrays(g['labels'], g['pred'], g['probs'], g['sev_true'], g['sev_pred'], 4, 15), 4, 15)
        assert close(m15['ece'], g['ece_15'])


def _feed(acc, g, sizes, with_losses=False):
    i, k = 0, 0
    n = len(g['labels'])
    while i < n:
        b = sizes[k % len(sizes)]
        k += 1
        j = min(n, i + b)
        out = {'cls_logits': torch.from_numpy(g['logits'][i:j]), 'kan_severity': torch.from_numpy(g['sev_pred'][i:j]).reshape(-1, 1),
               'mu': torch.zeros(j - i, 1), 'log_var': torch.from_numpy(g['logits'][i:j, :1].copy())}
        losses = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5]) * (k + 1) if with_losses else None
        acc.update(out, torch.from_numpy(g['labels'][i:j]), torch.from_numpy(g['sev_true'][i:j]), losses=losses)
        i = j


def test_cpu_accumulator_matches_the_metrics_functions_and_is_independent_of_the_batch_split(golden):
    from evaluation import metrics as M
    from rovit_hip.evaluation import EvalAccumulator
    cases, names = golden
    for c, g in cases.items():
        blocks = []
        for sizes in ((1,), (7,), (256,), (5, 1, 33)):
            acc = EvalAccumulator(4, capacity=16)
            _feed(acc, g, sizes)
            blocks.append(acc.result_block().copy())
        assert all(b.tobytes() == blocks[0].tobytes() for b in blocks), c          # identical result block for every split
        m, a = acc.compute(), acc.arrays()
        assert np.abs(a['y_probs'] - g['probs']).max() < 1e-6 and np.array_equal(a['y_true'], g['labels'])
        assert np.array_equal(a['severity_pred'], g['sev_pred']) and a['severity_true'].dtype == np.float32
        assert np.allclose(a['uncertainty'], np.exp(0.5 * g['logits'][:, 0]), rtol=1e-6)
        p64 = a['y_probs'].astype(np.float64)
        want = {'accuracy': M.accuracy(a['y_true'], a['y_pred']), 'macro_f1': M.macro_f1(a['y_true'], a['y_pred']),
                'weighted_f1': M.weighted_f1(a['y_true'], a['y_pred']), 'mae': M.mae(a['severity_true'], a['severity_pred']),
                'spearman_rho': M.spearman_rho(a['severity_true'], a['severity_pred']), 'brier_score': M.brier_score(a['y_true'], p64),
                'ece': M.ece(a['y_true'], p64)}
        for k, v in want.items():
            assert close(m[k], v), (c, k, m[k], v)
        if np.array_equal(a['y_probs'], g['probs']):                                # this machine's softmax is the golden's, bit for bit
            for k in FLOATS:
                assert close(m[k], g[k]), (c, k, m[k], float(g[k]))


def test_cpu_accumulator_substitutes_labels_for_a_missing_kan_head_and_averages_losses_over_batches(golden):
    from rovit_hip.evaluation import EvalAccumulator
    g = golden[0]['full']
    acc = EvalAccumulator(4)
    acc.update({'cls_logits': torch.from_numpy(g['logits']), 'kan_severity': None, 'mu': None, 'log_var': None},
               torch.from_numpy(g['labels']), torch.from_numpy(g['sev_true']))
    m, a = acc.compute(), acc.arrays()
    assert m['mae'] == 0.0 and close(m['spearman_rho'], 1.0) and a['uncertainty'] is None and 'loss' not in m
    acc.reset()
    _feed(acc, g, (100,), with_losses=True)              # 3 batches (100, 100, 57), loss vectors (k + 1) * [.1 .. .5], k = 1, 2, 3
    m = acc.compute()
    base = np.array([0.1, 0.2, 0.3, 0.4, 0.5], dtype=np.float32).astype(np.float64)
    want = sum(np.float32(k + 1) * np.array([0.1, 0.2, 0.3, 0.4, 0.5], dtype=np.float32) for k in (1, 2, 3)).astype(np.float64) / 3
    for i, k in enumerate(('cls_loss', 'ord_loss', 'unc_loss', 'kan_loss', 'loss')):
        assert abs(m[k] - want[i]) < 1e-6 * base[i] * 4, (k, m[k], want[i])
    # a dict of five separate 0-dim tensors, as a loss module on the CPU returns it
    acc.reset()
    acc.update({'cls_logits': torch.from_numpy(g['logits'][:8]), 'kan_severity': None}, torch.from_numpy(g['labels'][:8]),
               torch.from_numpy(g['sev_true'][:8]),
               losses={'cls_loss': torch.tensor(1.0), 'ord_loss': torch.tensor(2.0), 'unc_loss': torch.tensor(3.0), 'kan_loss': torch.tensor(4.0),
                       'total_loss': torch.tensor(5.5)})
    m = acc.compute()
    assert (m['cls_loss'], m['ord_loss'], m['unc_loss'], m['kan_loss'], m['loss']) == (1.0, 2.0, 3.0, 4.0, 5.5)


def test_non_finite_severity_gives_nan_rho_and_leaves_the_rest_finite(golden):
    from rovit_hip.evaluation import EvalAccumulator
    g = golden[0]['full']
    sp = g['sev_pred'].copy()
    sp[17] = np.inf
    acc = EvalAccumulator(4)
    acc.update({'cls_logits': torch.from_numpy(g['logits']), 'kan_severity': torch.from_numpy(sp)}, torch.from_numpy(g['labels']),
               torch.from_numpy(g['sev_true']))
    m = acc.compute()
    assert np.isnan(m['spearman_rho']) and all(np.isfinite(m[k]) for k in ('accuracy', 'macro_f1', 'brier_score', 'ece'))
    acc.reset()
    bad = g['labels'].copy()
    bad[3] = 4
    acc.update({'cls_logits': torch.from_numpy(g['logits'])}, torch.from_numpy(bad), torch.from_numpy(g['sev_true']))
    from rovit_hip.native import RovitHipError
    with pytest.raises(RovitHipError, match='outside'):
        acc.compute()


def test_against_sklearn_and_scipy_on_random_inputs_with_ties_and_an_absent_class():
    sk = pytest.importorskip('sklearn.metrics')
    st = pytest.importorskip('scipy.stats')
    from evaluation import metrics as M
    names = ['a', 'b', 'c', 'd', 'e']
    for seed, n in ((0, 50), (1, 333), (2, 2048)):
        rng = np.random.default_rng(seed)
        y = rng.integers(0, 4, size=n)                    # class 4 never a label
        pred = np.where(rng.random(n) < 0.6, y, rng.integers(0, 4, size=n))
        pred[y == 2] = rng.integers(0, 2, size=int((y == 2).sum()))      # class 2 never predicted: zero_division in its precision
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            assert close(M.macro_f1(y, pred), sk.f1_score(y, pred, average='macro') * 100)
            assert close(M.weighted_f1(y, pred), sk.f1_score(y, pred, average='weighted') * 100)
            p, r, f, s = sk.precision_recall_fscore_support(y, pred, labels=range(5), zero_division=0)
        assert np.array_equal(M.compute_confusion_matrix(y, pred, names), sk.confusion_matrix(y, pred, labels=range(5)))
        pc = M.per_class_metrics(y, pred, names)
        for i, nm in enumerate(names):
            assert pc[nm]['support'] == int(s[i])
            assert close(pc[nm]['precision'], p[i] * 100) and close(pc[nm]['recall'], r[i] * 100) and close(pc[nm]['f1'], f[i] * 100)
        a = rng.integers(0, 4, size=n).astype(np.float64)
        b = np.round(a + rng.normal(size=n), 1)
        assert abs(M.spearman_rho(a, b) - st.spearmanr(a, b)[0]) < 1e-12
        assert abs(M.spearman_rho(b, rng.normal(size=n)) - st.spearmanr(b, rng.normal(size=n))[0]) < 1.0      # finite on untied input
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            assert np.isnan(M.spearman_rho(a, np.ones(n))) and np.isnan(st.spearmanr(a, np.ones(n))[0])
        conf1d = rng.random(n)
        assert 0.0 <= M.ece((y > 1).astype(int), conf1d) <= 1.0


def test_evaluator_end_to_end_on_a_cpu_model_with_a_last_batch_of_one(tmp_path, capsys):
    """The drop-in Evaluator against the metrics functions on its own arrays; 9 samples in batches of 4: the last batch has one sample
    (the reference's squeeze() + concatenate raises there)."""
    from types import SimpleNamespace
    from evaluation import metrics as M
    from evaluation.evaluator import Evaluator

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(3)
            self.cls, self.sev = torch.nn.Linear(12, 4), torch.nn.Linear(12, 1)

        def forward(self, x):
            f = x.flatten(1)[:, :12]
            return {'cls_logits': self.cls(f), 'kan_severity': self.sev(f), 'mu': self.sev(f), 'log_var': -self.sev(f)}

    torch.manual_seed(5)
    data = [(torch.randn(b, 3, 224, 224), torch.randint(0, 4, (b,)), torch.randint(0, 4, (b,))) for b in (4, 4, 1)]
    names = ['Healthy Leaf', 'Leaf Holes', 'Black Spot', 'Dry Leaf']
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=names, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path / 'results'))
    metrics, a = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate(return_arrays=True)
    assert len(a['y_true']) == 9 and a['y_probs'].shape == (9, 4) and a['uncertainty'].shape == (9,)
    assert close(metrics['accuracy'], M.accuracy(a['y_true'], a['y_pred'])) and close(metrics['macro_f1'], M.macro_f1(a['y_true'], a['y_pred']))
    assert close(metrics['brier_score'], M.brier_score(a['y_true'], a['y_probs'].astype(np.float64)))
    assert close(metrics['ece'], M.ece(a['y_true'], a['y_probs'].astype(np.float64))) and close(metrics['mae'], M.mae(a['severity_true'], a['severity_pred']))
    assert metrics['spearman'] == metrics['spearman_rho'] or np.isnan(metrics['spearman'])
    assert metrics['params'] == M.count_params(Tiny()) == 65 and metrics['params_m'] == 65 / 1e6 and metrics['fps'] > 0
    assert list(metrics['per_class']) == names and sum(c['support'] for c in metrics['per_class'].values()) == 9
    text = (tmp_path / 'results' / 'evaluation_results.txt').read_text()
    assert text.startswith('RoViT-KAN Evaluation Results\n') and f"Accuracy:       {metrics['accuracy']:.2f}%" in text and "Spearman's rho: " in text
    out = capsys.readouterr().out
    assert 'Running Evaluation on Test Set' in out and 'Per-Class Metrics:' in out and f"Macro F1:       {metrics['macro_f1']:.2f}%" in out
    # no results_dir configured: nothing is written, nothing raises
    cfg2 = SimpleNamespace(data=cfg.data)
    assert 'accuracy' in Evaluator(Tiny(), data, cfg2, 'cpu').evaluate()
