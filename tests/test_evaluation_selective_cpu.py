"""CPU tests of the selective-prediction score card (rovit_hip/evaluation.py: selective_reference, EvalAccumulator.selective on CPU
tensors, update(extra=...)) and of the Evaluator's ``selective`` option.

Bounds.  The restatement against the brute-force average over every tie-consistent order: 1e-12 (fp64 on at most six integers).  Row
permutations: n * 2^-50 * max(1, max l), the summation bound of the GPU tests (each of at most n additions is off by at most 2^-53 of a
partial sum of at most n max l, divided by k, on both sides; a factor of 4 for the tie interpolation and the mean)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from selective_cases import brute_force_risks, feed, make_data  # noqa: E402


def _ev():
    from rovit_hip import evaluation
    return evaluation


def test_reference_equals_the_average_over_every_tie_consistent_order():
    ev = _ev()
    rng = np.random.default_rng(0)
    worst = 0.0
    for case in range(20):
        n = int(rng.integers(1, 7))
        u = rng.integers(0, 3, n).astype(np.float32)           # integer keys: many ties
        l = rng.integers(0, 5, n).astype(np.float32)
        worst = max(worst, float(np.abs(ev.selective_risks(u, l) - brute_force_risks(u, l)).max()))
    print(f'max distance to the brute-force tie average: {worst:.3e}')
    assert worst <= 1e-12
    # -0 and +0 are one tie group
    u, l = np.array([0.0, -0.0, 1.0], np.float32), np.array([1.0, 0.0, 0.0], np.float32)
    assert np.allclose(ev.selective_risks(u, l), [0.5, 0.5, 1 / 3], atol=1e-15)


def test_constant_key_perfect_key_and_reversed_key():
    ev = _ev()
    rng = np.random.default_rng(1)
    n = 500
    l = rng.random(n).astype(np.float32)
    flat = ev.selective_reference(np.zeros((1, n), np.float32), l[None], 20)
    assert abs(flat['aurc'][0, 0] - flat['mean'][0]) <= 1e-12 and np.abs(flat['curve'][0, 0] - flat['mean'][0]).max() <= 1e-12
    own = ev.selective_reference(l[None], l[None], 20)
    assert own['aurc'][0, 0] == own['oracle_aurc'][0] and np.array_equal(own['curve'][0, 0], own['oracle_curve'][0])
    # n = 1000, e = 137 errors ordered perfectly: aurc = (1/n) sum_{k > n - e} (k - (n - e)) / k
    n, e = 1000, 137
    err = np.zeros(n, np.float32)
    err[rng.permutation(n)[:e]] = 1.0
    u = (err + rng.random(n) * 0.5).astype(np.float32)         # every wrong row is less certain than every right one
    k = np.arange(n - e + 1, n + 1, dtype=np.float64)
    want = ((k - (n - e)) / k).sum() / n
    got = ev.selective_reference(u[None], err[None], 20)
    print(f'perfect order: |aurc - closed form| = {abs(got["aurc"][0, 0] - want):.3e}')
    assert abs(got['aurc'][0, 0] - want) <= 1e-15 and abs(got['oracle_aurc'][0] - want) <= 1e-15
    d = dict(make_data(n, 4, seed=3), good=torch.from_numpy(u), bad=torch.from_numpy(-u), err=torch.from_numpy(err))
    acc = feed(ev.EvalAccumulator(4), d, sizes=(333,), extra=('good', 'bad', 'err'))
    res = acc.selective(scores=['good', 'bad'], risks=['err'])
    assert abs(res['scores']['good']['err']['e_aurc']) <= 1e-15 and abs(res['scores']['good']['err']['normalized']) <= 1e-12
    assert res['scores']['bad']['err']['normalized'] > 1.0
    assert abs(res['risks']['err']['mean'] - e / n) <= 1e-15


def test_row_permutation_changes_nothing_beyond_the_summation_bound():
    ev = _ev()
    n = 4099
    d = make_data(n, 4, seed=5, ties=True)
    acc = feed(ev.EvalAccumulator(4), d)
    a = acc.selective(return_keys=True)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    b = feed(ev.EvalAccumulator(4), {k: v[perm] for k, v in d.items()}, sizes=(300,)).selective(return_keys=True)
    bound = n * 2.0 ** -50 * max(1.0, float(a['risk_values'].max()))
    off = _native().eval_selective_offsets(3, 2, 20)
    assert np.array_equal(a['block'][:8], b['block'][:8])
    dist = float(np.abs(a['block'][8:].view(np.float64) - b['block'][8:].view(np.float64)).max())
    print(f'row permutation at n = {n}: max distance {dist:.3e} (bound {bound:.3e})')
    assert dist <= bound and off['words'] == len(a['block'])
    assert np.array_equal(a['scores']['sigma']['thresholds'], b['scores']['sigma']['thresholds'])


def _native():
    from rovit_hip import native
    return native


@pytest.mark.parametrize('P', [1, 3, 20, 256])
def test_coverage_counts_and_thresholds(P):
    ev = _ev()
    for n in (1, 2, 5, 7, 100):
        kp = ev.coverage_counts(n, P)
        assert kp.tolist() == [-(-p * n // P) for p in range(1, P + 1)] and kp[-1] == n and kp.min() >= 1 and np.all(np.diff(kp) >= 0)
        u = np.random.default_rng(n).permutation(n).astype(np.float32)
        l = np.ones(n, np.float32)
        ref = ev.selective_reference(u[None], l[None], P)
        assert np.array_equal(ref['thresholds'][0], (kp - 1).astype(np.float64)) and np.array_equal(ref['coverages'], kp / n)
        assert ref['thresholds'].dtype == np.float64 and ref['curve'].shape == (1, 1, P)
        # the deployer's rule: accepting u <= t keeps exactly k_p rows (no ties here)
        assert [(u <= t).sum() for t in ref['thresholds'][0]] == kp.tolist()


def test_cpu_selective_structure_defaults_and_columns():
    ev = _ev()
    d = make_data(300, 4, seed=9, ties=True)
    acc = feed(ev.EvalAccumulator(4), d, sizes=(64,))
    res = acc.selective(return_keys=True)
    assert list(res['scores']) == ['confidence', 'entropy', 'sigma'] and list(res['risks']) == ['error', 'abs_err'] and res['n'] == 300
    arr = acc.arrays()
    assert np.array_equal(res['keys'][0], np.float32(1) - arr['y_probs'].max(axis=1))
    assert np.array_equal(res['keys'][2], arr['uncertainty']) and res['keys'].dtype == np.float32
    assert np.array_equal(res['risk_values'][0], (arr['y_pred'] != arr['y_true']).astype(np.float32))
    assert np.array_equal(res['risk_values'][1], np.abs(arr['severity_true'] - arr['severity_pred']))
    ref = ev.selective_reference(res['keys'], res['risk_values'], 20)
    for s, score in enumerate(res['scores']):
        assert np.array_equal(res['scores'][score]['thresholds'], ref['thresholds'][s])
        for k, risk in enumerate(res['risks']):
            e = res['scores'][score][risk]
            assert e['aurc'] == ref['aurc'][s, k] and e['e_aurc'] == ref['aurc'][s, k] - ref['oracle_aurc'][k]
            assert np.array_equal(e['curve'], ref['curve'][s, k]) and 0 <= e['aurc'] and e['e_aurc'] >= -1e-15
    assert abs(res['risks']['error']['mean'] - (arr['y_pred'] != arr['y_true']).mean()) <= 1e-15
    mu = acc.selective(scores=['mu', 'sigma'], risks=['mu_abs_err'], coverages=7, return_keys=True)
    assert np.array_equal(mu['risk_values'][0], np.abs(arr['severity_true'] - d['mu'].numpy())) and len(mu['coverages']) == 7
    assert 'keys' not in acc.selective()
    # without an uncertainty head the default leaves sigma out
    plain = ev.EvalAccumulator(4)
    plain.update({'cls_logits': d['logits'], 'kan_severity': d['sev_pred'], 'mu': None, 'log_var': None}, d['labels'], d['sev_true'])
    assert list(plain.selective()['scores']) == ['confidence', 'entropy']
    with pytest.raises(ev.RovitHipError, match='sigma'):
        plain.selective(scores=['sigma'])


def test_extra_name_set_rule_unknown_names_and_bad_values():
    ev = _ev()
    d = make_data(40, 4, seed=2)
    out = lambda i, j: {'cls_logits': d['logits'][i:j], 'kan_severity': d['sev_pred'][i:j], 'mu': d['mu'][i:j], 'log_var': d['log_var'][i:j]}
    acc = ev.EvalAccumulator(4)
    acc.update(out(0, 10), d['labels'][:10], d['sev_true'][:10], extra={'mu': d['mu'][:10], 'mi': d['log_var'][:10].reshape(-1, 1)})
    for extra, text in ((None, 'none'), ({'mu': d['mu'][10:20]}, 'differ'), ({'mu': d['mu'][10:20], 'other': d['mu'][10:20]}, 'differ'),
                        ({'mu': d['mu'][10:20], 'mi': d['mu'][10:15]}, 'batch of 10'), ({'mu': d['mu'][10:20], 'sigma': d['mu'][10:20]}, 'cannot name')):
        with pytest.raises(ev.RovitHipError, match=text):
            acc.update(out(10, 20), d['labels'][10:20], d['sev_true'][10:20], extra=extra)
    assert acc.n == 10
    acc.update(out(10, 40), d['labels'][10:], d['sev_true'][10:], extra={'mi': d['log_var'][10:], 'mu': d['mu'][10:]})
    assert acc.n == 40 and list(acc.selective(scores=['mi'], risks=['mu_abs_err'])['scores']) == ['mi']
    late = ev.EvalAccumulator(4)
    late.update(out(0, 10), d['labels'][:10], d['sev_true'][:10])
    with pytest.raises(ev.RovitHipError, match='first batch'):
        late.update(out(10, 20), d['labels'][10:20], d['sev_true'][10:20], extra={'mu': d['mu'][10:20]})
    for kw, text in (({'scores': ['nope']}, 'unknown score'), ({'risks': ['nope']}, 'unknown risk'), ({'risks': ['mu_abs_err']}, "'mu'"),
                     ({'scores': []}, 'distinct'), ({'scores': ['entropy', 'entropy']}, 'distinct'), ({'coverages': 0}, 'coverages'),
                     ({'coverages': 257}, 'coverages'), ({'risks': ['error'] * 5}, 'distinct'), ({'scores': 'entropy'}, 'sequences')):
        with pytest.raises(ev.RovitHipError, match=text):
            late.selective(**kw)
    with pytest.raises(ev.RovitHipError, match='nothing recorded'):
        ev.EvalAccumulator(4).selective()
    # a NaN score, a negative risk and a label outside [0, C) raise
    for name, column, text in (('s', torch.tensor([0.1, float('nan'), 0.3]), 'non-finite score'), ('r', torch.tensor([0.1, -1.0, 0.3]), 'negative risk'),
                               ('r', torch.tensor([0.1, float('inf'), 0.3]), 'non-finite risk')):
        bad = ev.EvalAccumulator(4)
        bad.update(out(0, 3), d['labels'][:3], d['sev_true'][:3], extra={name: column})
        with pytest.raises(ev.RovitHipError, match=text):
            bad.selective(scores=[name] if name == 's' else None, risks=[name] if name == 'r' else None)
    bad = ev.EvalAccumulator(4)
    bad.update(out(0, 3), torch.tensor([0, 9, 1]), d['sev_true'][:3])
    with pytest.raises(ev.RovitHipError, match='class labels outside'):
        bad.selective()


def test_cpu_evaluator_defaults_are_unchanged_and_selective_adds_a_section(tmp_path):
    from evaluation.evaluator import RULE, Evaluator

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
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=names, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    m = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate()
    assert set(m) == {'accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece', 'fps', 'params',
                      'params_m', 'per_class'}
    text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    # the file as it has always been written, restated from the returned dict
    want = ['RoViT-KAN Evaluation Results', RULE, '', f"{'Accuracy:':<16}{m['accuracy']:.2f}%", f"{'Macro F1:':<16}{m['macro_f1']:.2f}%",
            f"{'MAE:':<16}{m['mae']:.4f}", "Spearman's rho: " + f"{m['spearman_rho']:.4f}",
            f"{'Brier Score:':<16}{m['brier_score']:.4f}", f"{'ECE:':<16}{m['ece']:.4f}", f"{'FPS:':<16}{m['fps']:.1f}",
            f"{'Parameters:':<16}{m['params']:,}", '', 'Per-Class Metrics:', '-' * 60]
    for name, c in m['per_class'].items():
        want += [f'{name}:', f"  Precision: {c['precision']:.2f}%", f"  Recall:    {c['recall']:.2f}%", f"  F1-Score:  {c['f1']:.2f}%",
                 f"  Support:   {c['support']}", '']
    assert text == '\n'.join(want) + '\n' and 'Selective prediction' not in text
    with pytest.raises(RuntimeError, match='selective=True'):
        Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate(mc_samples=4)
    s = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate(selective=True)
    assert set(s) == set(m) | {'selective'} and all(s[k] == m[k] for k in ('accuracy', 'macro_f1', 'mae', 'brier_score', 'ece', 'per_class'))
    sel = s['selective']
    assert list(sel['scores']) == ['confidence', 'entropy', 'sigma'] and list(sel['risks']) == ['error', 'abs_err', 'mu_abs_err']
    text2 = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    head, _, tail = text2.partition('Selective prediction:\n')
    fps_free = lambda t: [line for line in t.splitlines() if not line.startswith('FPS:')]
    assert tail.count('\n') == 2 + 9 + 1 and 'Risk@80%' in tail and fps_free(head) == fps_free(text)
    assert f"{'sigma':<24}{'mu_abs_err':<12}{sel['scores']['sigma']['mu_abs_err']['aurc']:>10.4f}" in tail
