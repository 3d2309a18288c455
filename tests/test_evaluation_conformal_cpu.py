"""CPU tests of split conformal prediction's numpy statement (rovit_hip/evaluation.py: conformal_reference, conformal_block,
conformal_apply_block) and of the host layer built on it (EvalAccumulator.conformal, Conformal.evaluate, Conformal.predict on CPU
tensors): the definitions the kernels are tested against on the GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conformal_cases import CASES, feed, held_out_rows, make_case, make_data  # noqa: E402


def _acc(d, C, extra=('mu',), sizes=(1 << 30,)):
    from rovit_hip.evaluation import EvalAccumulator
    return feed(EvalAccumulator(C), d, sizes, extra=extra)


@pytest.mark.parametrize('name', ['n1_c4', 'n9_c4', 'n20_c4', 'n255_c2', 'n256_c4_all_tied', 'n257_c8_two_decimals', 'n1027_c4_class_absent',
                                  'n4099_c4_columns'])
def test_thresholds_are_order_statistics_of_every_group_and_level(name):
    from rovit_hip.evaluation import conformal_fraction, conformal_rank
    n, C, _, _ = CASES[name]
    d, extra, kw = make_case(name)
    acc = _acc(d, C, extra, sizes=(100, 7))
    cp = acc.conformal(return_scores=True, **kw)
    a = acc._cpu_arrays()
    cc = kw.get('class_conditional', False)
    assert cp.rows == n and cp.score_columns.shape == (len(kw['scores']), n)
    for m, s in enumerate(kw['scores']):
        col = cp.score_columns[m]
        ok = (a['label'] >= 0) & np.isfinite(col)
        if s == 'mu_scaled':
            ok &= np.isfinite(a['uncertainty']) & (a['uncertainty'] > 0)
        assert cp.bad_rows[s] == int(((a['label'] >= 0) & ~ok).sum())
        for g in range(1 + C if cc else 1):
            v = np.sort(col[ok if g == 0 else ok & (a['label'] == g - 1)])
            assert np.asarray(cp.n[s]).reshape(-1)[g] == len(v)
            for alpha in kw['alphas']:
                pick = lambda field: np.asarray(field[s][alpha]).reshape(-1)[g]
                k = conformal_rank(len(v), conformal_fraction(alpha))
                assert pick(cp.k) == k
                if k > len(v):
                    assert pick(cp.status) == 'trivial' and pick(cp.thresholds) == np.inf
                    continue
                q = np.float32(pick(cp.thresholds))
                assert pick(cp.status) == 'ok' and q.view(np.uint32) == v[k - 1].view(np.uint32), 'the threshold is an element of the column'
                less, equal = int(pick(cp.less)), int(pick(cp.equal))
                assert less == (v < q).sum() and equal == (v == q).sum() and less < k <= less + equal
                assert (v <= q).sum() / len(v) >= k / len(v)


def test_rank_for_small_samples_and_inexact_levels():
    """k = n + 1 - floor((n + 1) alpha) for (n, alpha) = (19, 0.1) -> 18, (20, 0.1) -> 19, (1, 0.5) -> 1, (1, 0.1) -> 2 > 1: trivial.
    (9, 0.1) gives 10 - floor(1) = 9 = ceil(10 * 0.9): the largest of the nine scores, which covers a tenth row with probability
    9 / 10, so it is NOT trivial; the feature request listed it as trivial, which contradicts its own formula (and the theory), and
    this test pins what the formula gives.  The first n at which alpha = 0.1 is trivial is 8: k = 9 > 8."""
    from rovit_hip.evaluation import RovitHipError, conformal_fraction, conformal_rank
    fr = conformal_fraction(0.1)
    assert (fr.numerator, fr.denominator) == (1, 10)
    for n, alpha, k in ((19, 0.1, 18), (20, 0.1, 19), (9, 0.1, 9), (8, 0.1, 9), (1, 0.5, 1), (1, 0.1, 2), (199, 0.1, 180), (999, 0.05, 950)):
        assert conformal_rank(n, conformal_fraction(alpha)) == k, (n, alpha)
    assert conformal_rank(8, conformal_fraction(0.1)) > 8 and conformal_rank(1, conformal_fraction(0.1)) > 1          # trivial
    assert conformal_rank(9, conformal_fraction(0.1)) == 9 == int(np.ceil(10 * 0.9))
    # alpha is not exact in binary: ceil((n + 1) (1 - alpha)) in floating point is off by one for (n, alpha) below; the integers are not
    assert int(np.ceil(150 * (1 - 0.18))) == 124 and conformal_rank(149, conformal_fraction(0.18)) == 123 == 150 - 27
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(RovitHipError):
            conformal_fraction(bad)
    acc = _acc(make_data(30, 4, seed=1), 4)
    for kw in (dict(alphas=()), dict(alphas=[0.1] * 2), dict(alphas=np.linspace(0.05, 0.5, 9)), dict(scores=[]), dict(scores=['lac', 'lac']),
               dict(scores=['nope']), dict(scores='lac'), dict(seed=-1), dict(raps_k=9), dict(raps_lambda=float('inf'))):
        with pytest.raises(RovitHipError):
            acc.conformal(**kw)
    from selective_cases import feed as feed_sel
    from bootstrap_cases import feed as feed_plain
    from rovit_hip.evaluation import EvalAccumulator
    plain = feed_plain(EvalAccumulator(4), make_data(30, 4, seed=1))
    assert plain.conformal().scores == ['lac', 'aps', 'raps', 'kan_abs']          # no mu recorded: the default leaves the mu scores out
    with pytest.raises(RovitHipError, match="'mu'"):
        plain.conformal(scores=['mu_abs'])
    assert feed_sel is feed


def test_aps_and_raps_of_a_hand_computed_example():
    from rovit_hip.evaluation import conformal_class_scores
    f = np.float32
    p = np.array([[0.5, 0.25, 0.25], [0.2, 0.2, 0.6], [0.1, 0.7, 0.2]], dtype=f)
    # row 0: order 0, 1, 2 (the tie of classes 1 and 2 goes to the lower index); row 1: order 2, 0, 1; row 2: order 1, 2, 0
    cum = np.array([[f(0.5), f(0.5) + f(0.25), f(0.5) + f(0.25) + f(0.25)],
                    [f(0.6) + f(0.2), f(0.6) + f(0.2) + f(0.2), f(0.6)],
                    [f(0.7) + f(0.2) + f(0.1), f(0.7), f(0.7) + f(0.2)]], dtype=f)
    rank = np.array([[1, 2, 3], [2, 3, 1], [3, 1, 2]])
    s, exact = conformal_class_scores(p, 'aps', None)
    assert np.array_equal(s.view(np.uint32), cum.view(np.uint32)) and np.array_equal(exact, cum.astype(np.float64))
    u = np.array([0.5, 0.25, 1.0], dtype=f)
    s, exact = conformal_class_scores(p, 'aps', u)
    want = cum.astype(np.float64) - u.astype(np.float64)[:, None] * p.astype(np.float64)
    assert np.array_equal(exact, want) and np.array_equal(s, want.astype(f))
    assert exact[0, 2] == 0.875 and exact[0, 1] == 0.625 and exact[0, 0] == 0.25           # 1 - 0.5 * 0.25, 0.75 - 0.5 * 0.25, 0.5 - 0.5 * 0.5
    # RAPS with k_reg = 1, lambda = 0.125: classes of rank 2 and 3 pay 0.125 and 0.25
    s, exact = conformal_class_scores(p, 'raps', u, raps_lambda=0.125, raps_k=1)
    assert np.array_equal(exact, want + 0.125 * np.maximum(0, rank - 1))
    assert exact[0, 2] == 0.875 + 0.25 and exact[2, 0] == want[2, 0] + 0.25 and exact[2, 1] == want[2, 1]
    lac, _ = conformal_class_scores(p, 'lac')
    assert np.array_equal(lac, f(1) - p)
    nan_row, _ = conformal_class_scores(np.array([[np.nan, 0.5, 0.5]], dtype=f), 'aps', None)
    assert np.isnan(nan_row).all()


def test_uniforms_are_the_philox_stream_of_the_row_index():
    from oracle.philox import philox4x32_10
    from rovit_hip import native as N
    from rovit_hip.evaluation import conformal_uniforms
    u = conformal_uniforms(1000, seed=(7 << 32) | 5, row_offset=40)
    assert u.dtype == np.float32 and (u > 0).all() and (u <= 1).all() and abs(float(u.mean()) - 0.5) < 0.05
    w = philox4x32_10([np.uint64(43), np.uint64(0), np.uint64(N.EVAL_CONF_STREAM), np.uint64(0)], [5, 7])[0]
    assert u[3] == (np.float32(int(w) >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert np.array_equal(conformal_uniforms(10, 3, 5), conformal_uniforms(15, 3)[5:])


def test_to_dict_round_trips_through_json_with_infinite_thresholds():
    from rovit_hip.evaluation import Conformal
    d, extra, kw = make_case('n1027_c4_class_absent')
    cp = _acc(d, 4, extra).conformal(**kw)
    small = _acc(make_data(8, 4, seed=3), 4).conformal(alphas=(0.1, 0.5))
    for c in (cp, small):
        text = json.dumps(c.to_dict())
        assert 'Infinity' not in text and '"inf"' in text
        back = Conformal.from_dict(json.loads(text))
        assert back.to_dict() == c.to_dict() and back.alphas == c.alphas and back.scores == c.scores and back.rows == c.rows
        for s in c.scores:
            for alpha in c.alphas:
                assert np.array_equal(np.asarray(back.thresholds[s][alpha]), np.asarray(c.thresholds[s][alpha]))
                assert np.array_equal(np.asarray(back.status[s][alpha]), np.asarray(c.status[s][alpha]))
    assert small.thresholds['lac'][0.1] == np.inf and small.status['lac'][0.1] == 'trivial' and small.status['lac'][0.5] == 'ok'
    held = _acc(held_out_rows('n1027_c4_class_absent'), 4)
    assert np.array_equal(Conformal.from_dict(json.loads(json.dumps(cp.to_dict()))).evaluate(held)['block'], cp.evaluate(held)['block'])


@pytest.mark.parametrize('class_conditional', [False, True])
def test_predict_gives_the_membership_evaluate_counts(class_conditional):
    d = make_data(400, 4, seed=12)
    cp = _acc(d, 4).conformal(alphas=(0.1, 0.3), class_conditional=class_conditional)
    t = make_data(333, 4, seed=13)
    acc = _acc(t, 4, sizes=(50,))
    card = cp.evaluate(acc)
    out = {'cls_logits': t['logits'], 'kan_severity': t['sev_pred'].reshape(-1, 1), 'mu': t['mu'].reshape(-1, 1), 'log_var': t['log_var'].reshape(-1, 1)}
    y = t['labels'].numpy()
    for score in ('lac', 'aps', 'raps'):
        for alpha in (0.1, 0.3):
            got = cp.predict(out, score=score, alpha=alpha, row_offset=cp.rows)
            sets, lv = got['sets'].numpy(), card['scores'][score]['levels'][alpha]
            assert lv['size_histogram'] == np.bincount(sets.sum(axis=1), minlength=5).tolist()
            assert lv['coverage'] == sets[np.arange(333), y].mean() and lv['mean_set_size'] == sets.sum() / 333
            assert lv['coverage_by_class'] == [sets[y == c, c].mean() for c in range(4)]
            assert torch.equal(got['set_size'], got['sets'].sum(dim=1))
    got = cp.predict(out, alpha=0.3)
    q = float(np.float32(np.asarray(cp.thresholds['kan_abs'][0.3]).reshape(-1)[0]))
    assert torch.equal(got['kan_interval'][:, 1] - got['kan_interval'][:, 0], (t['sev_pred'] + q) - (t['sev_pred'] - q))
    lv = card['scores']['kan_abs']['levels'][0.3]
    inside = (t['sev_true'].float() >= got['kan_interval'][:, 0]) & (t['sev_true'].float() <= got['kan_interval'][:, 1])
    assert abs(lv['coverage'] - float(inside.float().mean())) <= 2 / 333 and lv['mean_width'] == 2 * q and not lv['infinite']
    sigma = torch.exp(0.5 * t['log_var'])
    q = float(np.float32(np.asarray(cp.thresholds['mu_scaled'][0.3]).reshape(-1)[0]))
    assert torch.equal(got['mu_interval'], torch.stack([t['mu'] - q * sigma, t['mu'] + q * sigma], dim=1))
    assert abs(card['scores']['mu_scaled']['levels'][0.3]['mean_width'] - 2 * q * float(sigma.double().mean())) < 1e-12
    abs_only = _acc(d, 4).conformal(scores=['lac', 'mu_abs'])
    got = abs_only.predict(out, score='lac')
    q = float(np.float32(abs_only.thresholds['mu_abs'][0.1]))
    assert 'kan_interval' not in got and torch.equal(got['mu_interval'], torch.stack([t['mu'] - q, t['mu'] + q], dim=1))


def test_fit_works_on_a_calibrated_record_and_evaluate_counts_what_it_leaves_out():
    d = make_data(300, 4, seed=21)
    acc = _acc(d, 4)
    cal = acc.calibrate()
    applied = cal.apply(acc)
    cp = applied.conformal(alphas=(0.2,))
    assert cp.scores == ['lac', 'aps', 'raps', 'kan_abs', 'mu_abs', 'mu_scaled'] and cp.status['aps'][0.2] == 'ok'
    raw = acc.conformal(alphas=(0.2,))
    assert cp.thresholds['lac'][0.2] != raw.thresholds['lac'][0.2] and cp.thresholds['kan_abs'][0.2] == raw.thresholds['kan_abs'][0.2]
    t = make_data(100, 4, seed=22)
    t['labels'][3] = 7
    t['mu'][5] = float('nan')
    card = cp.evaluate(cal.apply(_acc(t, 4)))
    assert card['n'] == 100 and card['bad_labels'] == 1
    assert card['scores']['lac']['n'] == 99 and card['scores']['mu_abs']['n'] == 98 and card['scores']['mu_abs']['bad_rows'] == 1
    assert card['scores']['kan_abs']['bad_rows'] == 0 and sum(card['scores']['aps']['levels'][0.2]['size_histogram']) == 99
    from rovit_hip.evaluation import RovitHipError
    with pytest.raises(RovitHipError, match='no valid row|label'):
        bad = make_data(5, 4, seed=1)
        bad['labels'][:] = -1
        _acc(bad, 4).conformal()
    with pytest.raises(RovitHipError):
        cp.evaluate(_acc(t, 4, extra=()))                     # the mu scores need the extra column


def test_finite_sample_guarantee_over_400_splits():
    """400 independent splits of 199 calibration rows and 1000 test rows, logits 2 randn with + 2.5 on the true class, alpha = 0.1: the
    mean test coverage is within 4.6e-3 of k / (n + 1) = 180 / 200 = 0.9.  One split's coverage has variance Var Beta(180, 20) +
    0.09 / 1000 = 4.5e-4 + 0.9e-4 = 5.4e-4, so the mean of 400 has a standard deviation of 1.16e-3, and 4.6e-3 is four of them.  (For
    'lac' the scores have no ties almost surely, so the coverage given the calibration rows is exactly Beta(k, n + 1 - k); the
    randomised 'aps' is exact for the same reason.)"""
    from rovit_hip.evaluation import conformal_apply_block, conformal_reference
    from rovit_hip import native as N
    C, n_cal, n_test, splits = 4, 199, 1000, 400
    rng = np.random.default_rng(2024)
    scores = ['lac', 'aps']
    cover = np.zeros((splits, 2))
    for r in range(splits):
        n = n_cal + n_test
        y = rng.integers(0, C, n)
        z = (2.0 * rng.standard_normal((n, C))).astype(np.float32)
        z[np.arange(n), y] += np.float32(2.5)
        e = np.exp(z - z.max(axis=1, keepdims=True))
        p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        rows = lambda a, b: {'probs': p[a:b], 'label': y[a:b], 'sev_true': np.zeros(b - a, np.float32), 'sev_pred': np.zeros(b - a, np.float32)}
        fit = conformal_reference(rows(0, n_cal), None, C, (0.1,), scores, seed=r)['block']
        e0 = fit[N.EVAL_CONF_ENTRIES:].reshape(2, 1, 1, N.EVAL_CONF_ENTRY_WORDS)
        assert e0[:, 0, 0, 0].tolist() == [199, 199] and e0[:, 0, 0, 1].tolist() == [180, 180]
        thr = e0[..., 4].astype(np.uint32).view(np.float32)
        blk, _ = conformal_apply_block(rows(n_cal, n), None, C, scores, thr, seed=r, row_offset=n_cal)
        for m in range(2):
            base = N.EVAL_CONF_APPLY_SCORES + m * 48
            cover[r, m] = blk[base + 16 + 26] / blk[base]
    mean, sd = cover.mean(axis=0), cover.std(axis=0, ddof=1) / np.sqrt(splits)
    print(f"mean test coverage: lac {mean[0]:.4f}, randomised aps {mean[1]:.4f}; standard deviation of the mean {sd[0]:.1e}, {sd[1]:.1e}")
    assert np.all(np.abs(mean - 0.9) <= 4.6e-3)
