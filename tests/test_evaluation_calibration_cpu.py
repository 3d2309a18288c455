"""CPU tests of post-hoc calibration (rovit_hip/evaluation.py: calibration_reference, EvalAccumulator.calibrate on CPU tensors, Calibration)
and of the Evaluator's ``calibration`` option.

Bounds.  ln T of the fixed search against a bisection of g to convergence: 5e-7, the width 2 ln 32 / 63^4 = 4.4e-7 of the last bracket
(both roots lie inside it up to the rounding of g).  Refitting after ``apply``: 1e-6 in ln T and in s, which allows for the fp32 rounding
of p' and sigma' (2^-24 relative per entry; the refit averages it over the rows).  ``transform`` + ``update`` against ``apply``: the same
torch expressions on the same tensors, so the records are equal."""
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_cases as cc  # noqa: E402


def _ev():
    from rovit_hip import evaluation
    return evaluation


def _acc(d, C, **kw):
    return cc.feed(_ev().EvalAccumulator(C), d, **kw)


@pytest.fixture(scope='module')
def fits():
    """Every case once: (accumulator, Calibration, l, y) keyed by the case."""
    out = {}
    for case in cc.CPU_CASES:
        n, C, seed, scale = case
        acc = _acc(cc.scaled_data(n, C, seed, scale), C)
        a = acc.arrays()
        out[case] = (acc, acc.calibrate(return_block=True), cc.log_probs(a['y_probs']), a['y_true'])
    return out


def test_reference_temperature_equals_a_bisection_of_g(fits):
    worst = 0.0
    for case, (acc, cal, l, y) in fits.items():
        assert cal.status == cc.expected_status(l, y) == 'interior', case
        dist = abs(-math.log(cal.temperature) - cc.bisect_u(l, y))
        worst = max(worst, dist)
        assert dist <= 5e-7, (case, dist)
        assert cal.diagnostics['nll_calibrated'] <= cal.diagnostics['nll'], case
        assert cal.n == case[0] and cal.bad_labels == 0 and cal.bad_sigma == 0
    print(f'max |ln T - bisection| over {len(fits)} cases: {worst:.3e}')
    # an over-confident classifier is cooled down, an under-confident one sharpened, by about the factor its logits were scaled with
    for n, C in ((257, 4), (1027, 8)):
        t = {s: fits[(n, C, 100 * n + C, s)][1].temperature for s in (1.0, 3.0, 1.0 / 3.0)}
        assert abs(math.log(t[3.0] / t[1.0]) - math.log(3.0)) < 1e-4 and abs(math.log(t[1.0 / 3.0] / t[1.0]) + math.log(3.0)) < 1e-4


def test_status_at_the_bounds():
    ev = _ev()
    one = _acc(cc.make_data(1, 4, 301), 4)                        # one row, and it is right: the NLL falls all the way to T = 1/32
    cal = one.calibrate()
    a = one.arrays()
    assert cc.expected_status(cc.log_probs(a['y_probs']), a['y_true']) == 'at_min'
    assert cal.status == 'at_min' and cal.temperature == 1.0 / 32.0 and cal.diagnostics['nll_calibrated'] <= cal.diagnostics['nll']
    exact = _acc(cc.exact_case(), 4)                              # exact zeros on the label: their clamped log dominates
    cal = exact.calibrate()
    a = exact.arrays()
    assert cc.expected_status(cc.log_probs(a['y_probs']), a['y_true']) == 'at_max'
    assert cal.status == 'at_max' and cal.temperature == 32.0 and cal.diagnostics['nll_calibrated'] <= cal.diagnostics['nll']
    assert math.isfinite(cal.diagnostics['nll']) and cal.sigma_scale is not None
    assert ev.CALIBRATION_STATUS == {0: 'interior', 1: 'at_min', 2: 'at_max'}


def test_sigma_scale_gaussian_nll_and_coverage_counts(fits):
    ev = _ev()
    for case in ((5, 4, 500, 1.0), (257, 4, 25704, 1.0), (1027, 8, 102708, 3.0)):
        acc, cal, _, _ = fits[case]
        a, extras = cc.recorded(acc)
        sigma, mu, st = (np.asarray(x, dtype=np.float64) for x in (a['uncertainty'], extras['mu'], a['severity_true']))
        z = (st - mu) / sigma
        assert cal.sigma_scale == math.sqrt(float((z * z).sum()) / len(z))
        d = cal.diagnostics
        assert abs(d['gaussian_nll'] - float((np.log(sigma) + z * z / 2).mean())) <= 1e-12
        s = cal.sigma_scale
        assert abs(d['gaussian_nll_calibrated'] - float((np.log(s * sigma) + z * z / (2 * s * s)).mean())) <= 1e-12
        assert d['gaussian_nll_calibrated'] <= d['gaussian_nll']
        assert d['levels'] == [k / 10 for k in range(1, 10)]
        widths = ev.coverage_half_widths(9)
        brute = [sum(1 for i in range(len(z)) if abs(st[i] - mu[i]) <= q * sigma[i]) for q in widths]
        assert [int(c) for c in cal.block[ev.native.EVAL_CAL_COVERAGE:]] == brute and d['coverage'] == [c / len(z) for c in brute]
    assert abs(ev.coverage_half_widths(1)[0] - 0.6744897501960817) < 1e-15          # the quartile of the normal distribution
    acc = fits[(257, 4, 25704, 1.0)][0]
    assert len(acc.calibrate(levels=64).diagnostics['coverage']) == 64


def test_apply_then_calibrate_finds_nothing_left_to_fit(fits):
    worst_t = worst_s = 0.0
    for case, (acc, cal, _, _) in fits.items():
        before = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in acc.arrays().items()}
        applied = cal.apply(acc)
        again = applied.calibrate()
        worst_t, worst_s = max(worst_t, abs(math.log(again.temperature))), max(worst_s, abs(again.sigma_scale - 1.0))
        assert abs(math.log(again.temperature)) <= 1e-6 and abs(again.sigma_scale - 1.0) <= 1e-6, case
        after, b = acc.arrays(), applied.arrays()
        assert all(np.array_equal(before[k], after[k]) for k in before)                      # the input accumulator is untouched
        assert all(np.array_equal(after[k], b[k]) for k in ('y_true', 'y_pred', 'severity_true', 'severity_pred'))
        assert np.array_equal(applied._extra_column('mu'), acc._extra_column('mu'))
        assert abs(again.diagnostics['nll'] - cal.diagnostics['nll_calibrated']) <= 1e-6
    print(f'refit after apply: max |ln T| {worst_t:.3e}, max |s - 1| {worst_s:.3e}')
    acc, cal, _, _ = fits[(257, 4, 25704, 3.0)]
    applied = cal.apply(acc)
    assert applied.compute()['ece'] < acc.compute()['ece']                                   # what the feature is for
    assert applied.selective()['n'] == 257 and applied.bootstrap(20)['ece']['value'] == applied.compute()['ece']


def test_transform_then_update_equals_apply(fits):
    ev = _ev()
    case = (257, 4, 25704, 3.0)
    acc, cal, _, _ = fits[case]
    d = cc.scaled_data(*case)
    out = {'cls_logits': d['logits'], 'kan_severity': d['sev_pred'].reshape(-1, 1), 'mu': d['mu'].reshape(-1, 1), 'log_var': d['log_var'].reshape(-1, 1)}
    t = cal.transform(out)
    assert t['mu'] is out['mu'] and t['kan_severity'] is out['kan_severity'] and set(t) == set(out)
    assert torch.equal(t['cls_logits'], out['cls_logits'] / cal.temperature)
    fed = ev.EvalAccumulator(4)
    fed.update(t, d['labels'], d['sev_true'], extra={'mu': d['mu']})
    a, b = cal.apply(acc).arrays(), fed.arrays()
    eps = 2.0 ** -23
    assert np.abs(a['y_probs'] - b['y_probs']).max() <= eps and np.all(np.abs(a['uncertainty'] - b['uncertainty']) <= eps * np.abs(a['uncertainty']))
    assert np.array_equal(a['y_pred'], b['y_pred'])
    # without a sigma scale log_var passes through
    plain = ev.Calibration(2.0)
    assert plain.transform(out)['log_var'] is out['log_var']


def test_to_dict_round_trip_is_json(fits):
    ev = _ev()
    cal = fits[(1027, 8, 102708, 3.0)][1]
    text = json.dumps(cal.to_dict())
    back = ev.Calibration.from_dict(json.loads(text))
    assert (back.temperature, back.status, back.sigma_scale, back.n, back.bad_labels, back.bad_sigma) == \
           (cal.temperature, cal.status, cal.sigma_scale, cal.n, cal.bad_labels, cal.bad_sigma)
    assert back.diagnostics == cal.diagnostics and back.to_dict() == cal.to_dict()
    none = ev.Calibration.from_dict(json.loads(json.dumps(ev.Calibration(1.5).to_dict())))
    assert none.temperature == 1.5 and none.sigma_scale is None and none.status == 'interior'
    with pytest.raises(ev.RovitHipError, match='temperature'):
        ev.Calibration(0.0)
    with pytest.raises(ev.RovitHipError, match='sigma_scale'):
        ev.Calibration(1.0, sigma_scale=float('nan'))


def test_error_paths():
    ev = _ev()
    with pytest.raises(ev.RovitHipError, match='nothing recorded'):
        ev.EvalAccumulator(4).calibrate()
    d = cc.make_data(6, 4, 1)
    acc = _acc(d, 4)
    for levels in (0, 65, 2.5, True):
        with pytest.raises(ev.RovitHipError, match='levels'):
            acc.calibrate(levels=levels)
    bad = dict(d, labels=torch.full((6,), 7))
    with pytest.raises(ev.RovitHipError, match='none of the 6 recorded rows'):
        _acc(bad, 4).calibrate()
    with pytest.raises(ev.RovitHipError, match='recorded rows'):
        ev.Calibration(1.0).apply(ev.EvalAccumulator(4))


def test_bad_rows_are_counted_and_left_out():
    ev = _ev()
    d = cc.make_data(40, 4, 9)
    ref = _acc(dict((k, v[2:]) for k, v in d.items()), 4).calibrate(return_block=True)
    d['labels'][0] = 11                                            # out of range: leaves the classification part only
    d['log_var'][1] = float('nan')                                 # sigma = NaN: leaves the regression part only
    cal = _acc(d, 4).calibrate(return_block=True)
    assert (cal.n, cal.bad_labels, cal.bad_sigma) == (40, 1, 1)
    N = ev.native
    assert int(cal.block[N.EVAL_CAL_N_VALID]) == 39 and int(cal.block[N.EVAL_CAL_N_REG]) == 39
    # rows 0 and 1 are each in one part only, so neither part equals the 38-row fit; dropping row 1's label and row 0's sigma does
    d2 = {k: v.clone() for k, v in d.items()}
    d2['labels'][1] = 11
    d2['log_var'][0] = float('inf')
    both = _acc(d2, 4).calibrate()
    assert (both.bad_labels, both.bad_sigma) == (2, 2)
    assert both.temperature == ref.temperature and abs(both.sigma_scale - ref.sigma_scale) <= 1e-15
    for column, value in (('mu', float('inf')), ('sev_true', None)):
        d3 = {k: v.clone() for k, v in cc.make_data(40, 4, 9).items()}
        if value is None:
            d3['sev_true'] = d3['sev_true'].float()
            d3['sev_true'][3] = float('nan')
        else:
            d3[column][3] = value
        assert _acc(d3, 4).calibrate().bad_sigma == 1
    d4 = cc.make_data(40, 4, 9)
    d4['log_var'][5] = -400.0                                      # exp(-200) underflows: sigma == 0 is not a scale
    assert _acc(d4, 4).calibrate().bad_sigma == 1


def test_missing_regression_part():
    ev = _ev()
    d = cc.make_data(50, 4, 2)
    no_mu = _acc(d, 4, extra=()).calibrate()
    import bootstrap_cases
    no_head = bootstrap_cases.feed(ev.EvalAccumulator(4), d).calibrate()
    full = _acc(d, 4).calibrate()
    for cal in (no_mu, no_head):
        assert cal.sigma_scale is None and cal.diagnostics['coverage'] is None and cal.diagnostics['gaussian_nll'] is None
        assert cal.temperature == full.temperature and cal.diagnostics['nll'] == full.diagnostics['nll'] and cal.bad_sigma == 0
    applied = no_mu.apply(_acc(d, 4, extra=()))
    assert np.array_equal(applied.arrays()['uncertainty'], _acc(d, 4, extra=()).arrays()['uncertainty'])


def test_cpu_evaluator_defaults_are_unchanged_and_calibration_adds_a_section(tmp_path):
    from evaluation.evaluator import RULE, Evaluator

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(3)
            self.cls, self.sev = torch.nn.Linear(12, 4), torch.nn.Linear(12, 1)

        def forward(self, x):
            f = x.flatten(1)[:, :12]
            return {'cls_logits': 4.0 * self.cls(f), 'kan_severity': self.sev(f), 'mu': self.sev(f), 'log_var': -self.sev(f)}

    torch.manual_seed(5)
    batch = lambda b: (torch.randn(b, 3, 224, 224), torch.randint(0, 4, (b,)), torch.randint(0, 4, (b,)))
    data, val = [batch(b) for b in (4, 4, 1)], [batch(b) for b in (8, 8)]
    names = ['Healthy Leaf', 'Leaf Holes', 'Black Spot', 'Dry Leaf']
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=names, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    ev = Evaluator(Tiny(), data, cfg, torch.device('cpu'))
    assert ev.calibration is None
    m = ev.evaluate()
    assert set(m) == {'accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece', 'fps', 'params',
                      'params_m', 'per_class'}
    assert ev.accumulator._extra_names is None                     # nothing more is recorded either
    text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    want = ['RoViT-KAN Evaluation Results', RULE, '', f"{'Accuracy:':<16}{m['accuracy']:.2f}%", f"{'Macro F1:':<16}{m['macro_f1']:.2f}%",
            f"{'MAE:':<16}{m['mae']:.4f}", "Spearman's rho: " + f"{m['spearman_rho']:.4f}",
            f"{'Brier Score:':<16}{m['brier_score']:.4f}", f"{'ECE:':<16}{m['ece']:.4f}", f"{'FPS:':<16}{m['fps']:.1f}",
            f"{'Parameters:':<16}{m['params']:,}", '', 'Per-Class Metrics:', '-' * 60]
    for name, c in m['per_class'].items():
        want += [f'{name}:', f"  Precision: {c['precision']:.2f}%", f"  Recall:    {c['recall']:.2f}%", f"  F1-Score:  {c['f1']:.2f}%",
                 f"  Support:   {c['support']}", '']
    assert text == '\n'.join(want) + '\n' and 'Calibration' not in text

    cal = ev.fit_calibration(val)
    assert ev.calibration is cal and cal.n == 16 and cal.sigma_scale is not None
    c = ev.evaluate(calibration=cal)
    assert set(c) == set(m) | {'calibration'} and all(c[k] == m[k] for k in ('accuracy', 'macro_f1', 'mae', 'brier_score', 'ece', 'per_class'))
    card = c['calibration']
    assert set(card) == {'temperature', 'sigma_scale', 'status', 'before', 'after'}
    assert (card['temperature'], card['sigma_scale'], card['status']) == (cal.temperature, cal.sigma_scale, cal.status)
    for side in ('before', 'after'):
        assert set(card[side]) == {'nll', 'ece', 'brier_score', 'gaussian_nll', 'coverage', 'levels', 'sigma_scale_refit'}
    assert card['before']['ece'] == m['ece'] and card['before']['brier_score'] == m['brier_score']
    applied = cal.apply(ev.accumulator)
    assert card['after']['ece'] == applied.compute()['ece'] and card['after']['nll'] == applied.calibrate().diagnostics['nll']
    assert abs(card['after']['sigma_scale_refit'] * cal.sigma_scale - card['before']['sigma_scale_refit']) <= 1e-6
    text2 = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    head, _, tail = text2.partition('Calibration (temperature ')
    fps_free = lambda t: [line for line in t.splitlines() if not line.startswith('FPS:')]
    assert fps_free(head) == fps_free(text) and tail.startswith(f'{cal.temperature:.4f}, sigma scale {cal.sigma_scale:.4f}, {cal.status}):')
    assert f"{'after':<10}{card['after']['nll']:>10.4f}{card['after']['ece']:>10.4f}" in tail and 'Interval coverage' in tail
    s = ev.evaluate(calibration=cal, selective=True)
    assert set(s['calibration']) == set(card) | {'selective'} and list(s['calibration']['selective']['scores']) == list(s['selective']['scores'])
    # fitted and scored on the same rows, the calibrated NLL cannot be larger
    same = Evaluator(Tiny(), val, cfg, torch.device('cpu'))
    r = same.evaluate(calibration=same.fit_calibration(val))['calibration']
    assert r['after']['nll'] <= r['before']['nll'] + 1e-9 and r['after']['gaussian_nll'] <= r['before']['gaussian_nll'] + 1e-9
