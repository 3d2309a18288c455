"""CPU tests of the bootstrap layer of rovit_hip/evaluation.py: the draw rule, the sort-free rank identity the kernel rests on, the
result structure of ``EvalAccumulator.bootstrap`` and ``paired_bootstrap`` on CPU tensors (the numpy restatement), and McNemar's tail."""
import math

import numpy as np
import pytest
import torch

from bootstrap_cases import PAIR_R, PAIR_SEED, feed, make_data, paired_data

METRICS = ('accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'brier_score', 'ece')


def test_bootstrap_indices_range_reproducibility_and_tail():
    from rovit_hip.evaluation import bootstrap_indices
    for n in (1, 2, 3, 5, 6, 7, 257, 1000):                  # n % 4 in {0, 1, 2, 3}
        a = bootstrap_indices(n, 0, seed=5)
        assert a.shape == (n,) and a.min() >= 0 and a.max() < n
        assert np.array_equal(a, bootstrap_indices(n, 0, seed=5))
    a, b, c = bootstrap_indices(1000, 0, 5), bootstrap_indices(1000, 1, 5), bootstrap_indices(1000, 0, 6)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    # the draw is a function of (seed, r, j, n): draw j uses word j % 4 of the Philox call with counter j // 4, whatever follows it --
    # a tail of 1, 2 or 3 draws takes the first words of the last call
    from oracle.philox import philox4x32_10
    from rovit_hip import native
    for n in (5, 6, 7):
        words = philox4x32_10([1, 3, native.EVAL_BOOT_STREAM, 0], [9, 0])
        want = [(int(words[e]) * n) >> 32 for e in range(n - 4)]
        assert list(bootstrap_indices(n, 3, seed=9)[4:]) == want
    # a 64-bit seed uses both key words
    assert not np.array_equal(bootstrap_indices(100, 0, 5), bootstrap_indices(100, 0, 5 + (1 << 32)))
    # uniform enough: every row of 64 is drawn somewhere in 64 replicates
    assert len(np.unique(np.concatenate([bootstrap_indices(64, r, 0) for r in range(64)]))) == 64


def test_stratified_indices_stay_in_their_class_segment():
    from rovit_hip.evaluation import bootstrap_indices, stratification
    g = np.random.default_rng(3)
    y = g.integers(0, 4, 301)
    y[y == 2] = 1                                            # class 2 is absent
    y[[7, 100]] = -1                                         # two bad labels: a last segment of their own
    perm, starts = stratification(y, 4)
    assert sorted(perm) == list(range(301)) and list(starts[[0, -1]]) == [0, 301] and starts[2] == starts[3]
    for r in range(4):
        idx = bootstrap_indices(301, r, seed=2, starts=starts, perm=perm)
        assert np.array_equal(np.bincount(y[idx] + 1, minlength=5), np.bincount(y + 1, minlength=5))
        key = np.where(y < 0, 4, y)
        assert np.array_equal(key[idx], np.sort(key))          # draw j belongs to the segment that contains j


@pytest.mark.parametrize('n', [1, 2, 5, 257, 1000])
def test_rank_identity_against_rank_sums_of_the_resample(n):
    """With H[less[idx_j]] += 1 and P its exclusive prefix sum, 2 P[v] + H[v] + 1 (v = less[idx_j]) is the doubled tie-averaged rank of
    draw j inside the resample: the three rank sums equal ``rank_sums`` of the resampled arrays, with ties."""
    from rovit_hip.evaluation import bootstrap_indices, rank_sums
    g = np.random.default_rng(n)
    x, y = np.round(g.normal(size=n), 1), g.integers(0, 4, n).astype(np.float64)

    def centred_ranks(v, idx):
        less = np.searchsorted(np.sort(v), v, side='left')
        H = np.bincount(less[idx], minlength=n)
        P = np.cumsum(H) - H
        return (2 * P[less[idx]] + H[less[idx]] + 1 - (n + 1)).astype(object)

    for r in range(4):
        idx = bootstrap_indices(n, r, seed=7)
        da, db = centred_ranks(x, idx), centred_ranks(y, idx)
        assert (int((da * db).sum()), int((da * da).sum()), int((db * db).sum()), 0, 0) == rank_sums(x[idx], y[idx])


def _acc(d, C=4, sizes=(97,)):
    from rovit_hip.evaluation import EvalAccumulator
    return feed(EvalAccumulator(C), d, sizes)


def test_bootstrap_on_cpu_tensors_structure_and_reproducibility():
    from rovit_hip import native
    acc = _acc(make_data(300, 4, seed=1, ties=True))
    point = acc.compute()
    b = acc.bootstrap(num_resamples=40, seed=3, return_table=True, return_blocks=True)
    for k in METRICS:
        assert set(b[k]) >= {'value', 'mean', 'se', 'lo', 'hi'} and b[k]['lo'] <= b[k]['hi'] and b[k]['se'] > 0
        assert b[k]['value'] == point[k]
    assert b['spearman_rho']['n_nan'] == 0 and len(b['per_class']) == 4
    for c in range(4):
        for k in ('precision', 'recall', 'f1'):
            assert b['per_class'][c][k]['value'] == point['per_class'][c][k] and b['per_class'][c][k]['lo'] <= b['per_class'][c][k]['hi']
    assert b['table'].shape == (40, native.EVAL_BOOT_COLS) and b['blocks'].shape == (40, native.EVAL_RESULT_WORDS)
    assert np.all(b['blocks'][:, native.EVAL_N] == 300)
    # se and the percentile interval are numpy's, on the table
    col = b['table'][:, native.EVAL_BOOT_ACCURACY]
    assert b['accuracy']['se'] == float(np.std(col, ddof=1)) and b['accuracy']['lo'] == float(np.nanquantile(col, 0.025))
    again = acc.bootstrap(num_resamples=40, seed=3, return_table=True)
    other = acc.bootstrap(num_resamples=40, seed=4, return_table=True)
    assert np.array_equal(again['table'], b['table'], equal_nan=True) and not np.array_equal(other['table'], b['table'], equal_nan=True)
    assert 'table' not in acc.bootstrap(num_resamples=2)


def test_stratified_bootstrap_keeps_every_class_support():
    from rovit_hip import native
    acc = _acc(make_data(300, 4, seed=2))
    support = [c['support'] for c in acc.compute()['per_class']]
    plain = acc.bootstrap(num_resamples=12, seed=1, return_blocks=True)['blocks']
    strat = acc.bootstrap(num_resamples=12, seed=1, stratified=True, return_blocks=True)['blocks']
    cm = lambda blocks: blocks[:, native.EVAL_CONFUSION:native.EVAL_CONFUSION + 16].reshape(-1, 4, 4).sum(axis=2)
    assert np.all(cm(strat) == np.asarray(support)) and not np.all(cm(plain) == np.asarray(support))


def test_bootstrap_argument_checks_and_bad_labels():
    from rovit_hip.evaluation import EvalAccumulator, RovitHipError
    acc = _acc(make_data(20, 4, seed=3))
    for kw in ({'num_resamples': 0}, {'num_resamples': 65537}, {'seed': -1}, {'confidence': 1.0}):
        with pytest.raises(RovitHipError):
            acc.bootstrap(**kw)
    with pytest.raises(RovitHipError):
        EvalAccumulator(4).bootstrap()
    d = make_data(20, 4, seed=3)
    d['labels'][5] = 9
    with pytest.raises(RovitHipError, match='outside'):
        _acc(d).bootstrap(num_resamples=4)


def test_paired_bootstrap_of_an_accumulator_against_itself():
    from rovit_hip.evaluation import paired_bootstrap
    acc = _acc(make_data(200, 4, seed=4))
    p = paired_bootstrap(acc, acc, num_resamples=30, seed=1)
    for k in METRICS:
        assert (p[k]['diff'], p[k]['lo'], p[k]['hi'], p[k]['p_value']) == (0.0, 0.0, 0.0, 1.0) and p[k]['a'] == p[k]['b']
    assert p['mcnemar'] == {'b01': 0, 'b10': 0, 'p_value': 1.0}


def test_paired_bootstrap_detects_ten_points_of_accuracy():
    from rovit_hip.evaluation import paired_bootstrap
    a, b = paired_data()
    acc_a, acc_b = _acc(a), _acc(b, sizes=(600,))
    assert abs(acc_b.compute()['accuracy'] - acc_a.compute()['accuracy'] - 10.0) < 1e-9          # the construction, checked
    p = paired_bootstrap(acc_a, acc_b, num_resamples=PAIR_R, seed=PAIR_SEED)
    assert abs(p['accuracy']['diff'] - 10.0) < 1e-9 and p['accuracy']['lo'] > 0 and p['accuracy']['p_value'] < 0.05
    assert p['accuracy']['lo'] <= p['accuracy']['diff'] <= p['accuracy']['hi']
    assert p['mae']['diff'] < 0 and p['mae']['hi'] < 0 and p['mae']['p_value'] < 0.05
    assert p['mcnemar']['b01'] == 0 and p['mcnemar']['b10'] == 60 and p['mcnemar']['p_value'] == 2.0 / 2 ** 60
    assert len(p['per_class']) == 4 and set(p['per_class'][0]['f1']) == {'a', 'b', 'diff', 'lo', 'hi', 'p_value'}


def test_paired_score_cards_have_an_exact_softmax():
    """``exact_data``: every recorded probability is exactly 0 or fl(1 / m) with m the number of classes at logit 0, in all four
    calibration bins, and the prediction is the first of those classes."""
    a, b = paired_data()
    for d in (a, b):
        p = _acc(d).arrays()['y_probs']
        m = (d['logits'] == 0).sum(1).numpy()
        want = np.where(d['logits'].numpy() == 0, (np.float32(1) / m.astype(np.float32))[:, None], np.float32(0))
        assert p.dtype == np.float32 and np.array_equal(p, want) and set(m) == {1, 2, 3, 4}
        assert np.array_equal(_acc(d).arrays()['y_pred'], (d['logits'] == 0).int().argmax(1).numpy())


def test_paired_bootstrap_refuses_other_rows():
    from rovit_hip.evaluation import RovitHipError, paired_bootstrap
    d = make_data(50, 4, seed=5)
    acc = _acc(d)
    with pytest.raises(RovitHipError, match='rows'):
        paired_bootstrap(acc, _acc(make_data(49, 4, seed=5)), num_resamples=4)
    other = dict(d, labels=d['labels'].clone())
    other['labels'][10] = (other['labels'][10] + 1) % 4
    with pytest.raises(RovitHipError, match='labels'):
        paired_bootstrap(acc, _acc(other), num_resamples=4)


@pytest.mark.parametrize('b01,b10', [(0, 0), (3, 0), (5, 12)])
def test_mcnemar_tail_against_the_binomial_by_hand(b01, b10):
    from rovit_hip.evaluation import mcnemar_exact
    # P[X <= min] for X ~ Binomial(b01 + b10, 1/2), doubled and capped: 1; 2 * 1/8; 2 * (1 + 17 + 136 + 680 + 2380 + 6188) / 2^17
    want = {(0, 0): 1.0, (3, 0): 0.25, (5, 12): 2 * 9402 / 131072}[(b01, b10)]
    assert mcnemar_exact(b01, b10) == want and mcnemar_exact(b10, b01) == want


def test_mcnemar_log_gamma_branch_agrees_with_the_exact_sum():
    from rovit_hip.evaluation import mcnemar_exact
    exact = min(1.0, 2 * sum(math.comb(1500, i) for i in range(701)) / 2 ** 1500)
    assert abs(mcnemar_exact(700, 800) - exact) <= 1e-9 * exact
