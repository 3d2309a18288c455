"""GPU tests of the bootstrap kernel (csrc/eval_bootstrap.hip) and its Python layer (rovit_hip/evaluation.py: EvalAccumulator.bootstrap,
paired_bootstrap), against the numpy / fp64 restatement ``bootstrap_reference`` on the accumulator's own recorded arrays.

Bounds.  Integer words of a replicate's result block: equal.  fp64 words: n * 2^-50 absolute, the summation bound of the existing
evaluation tests restated per row count (n terms of size at most 2, each addition off by at most 2^-53 of a partial sum of at most
2 n, both sides).  Metric table against ``metrics_from_block`` of the kernel's own blocks: 1e-9 (fp64 arithmetic on identical inputs,
times 100 for the percent values), rho 1e-12, NaN where the restatement is NaN."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref_cpu  # noqa: E402  (checker only)
from bootstrap_cases import PAIR_R, PAIR_SEED, feed, make_data, paired_data, paired_data_random_logits  # noqa: E402

pytestmark = pytest.mark.gpu

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
SEVERITY = {n: i for i, n in enumerate(CLASS_NAMES)}
CASES = {'n1': (1, 2, 1, False), 'n2': (2, 4, 10, False), 'n5': (5, 4, 10, False), 'n257': (257, 3, 15, False), 'n1000': (1000, 4, 10, True),
         'constant': (64, 4, 10, False)}
R_CASES, SEED_CASES = 8, 17


def dev():
    return torch.device('cuda:0')


def _acc(d, C, bins=10, sizes=(1 << 30,)):
    from rovit_hip.evaluation import EvalAccumulator
    return feed(EvalAccumulator(C, n_bins=bins), d, sizes, device=dev())


_cache = {}


def _case(name):
    """(n, C, bins, kernel result, oracle table, oracle blocks) of one case: computed once, shared by the tests, never changed."""
    if name not in _cache:
        from rovit_hip.evaluation import bootstrap_reference
        n, C, bins, ties = CASES[name]
        d = make_data(n, C, seed=100 + n, ties=ties)
        if name == 'constant':
            d['sev_pred'] = torch.full((n,), 1.5)
        acc = _acc(d, C, bins)
        got = acc.bootstrap(num_resamples=R_CASES, seed=SEED_CASES, return_table=True, return_blocks=True)
        table, blocks = bootstrap_reference(acc.arrays(), C, bins, R_CASES, SEED_CASES)
        for a in (got['table'], got['blocks'], table, blocks):
            a.setflags(write=False)
        _cache[name] = (n, C, bins, got, table, blocks)
    return _cache[name]


def _assert_blocks(got, want, n, what=''):
    from rovit_hip import native as N
    assert got.shape == want.shape, what
    I = N.EVAL_BIN_CONF                                       # the first fp64 word
    bad = np.argwhere(got[:, :I] != want[:, :I])
    assert bad.size == 0, f'{what}: integer words differ at (replicate, word) {bad[:5].tolist()}'
    err = np.abs(got[:, I:].view(np.float64) - want[:, I:].view(np.float64))
    print(f'{what} n={n}: max fp64 word error {float(err.max()):.3e} (bound {n * 2.0 ** -50:.3e})')
    assert float(err.max()) <= n * 2.0 ** -50, what


@pytest.mark.parametrize('name', ['n1', 'n2', 'n5', 'n257', 'n1000'])
def test_blocks_against_the_oracle(name):
    n, C, bins, got, _, blocks = _case(name)
    _assert_blocks(got['blocks'], blocks, n, name)


@pytest.mark.parametrize('name', list(CASES))
def test_metric_table_against_metrics_from_block_of_the_same_blocks(name):
    from rovit_hip import native as N
    from rovit_hip.evaluation import table_row_from_block
    n, C, bins, got, table, _ = _case(name)
    want = np.stack([table_row_from_block(b, C, bins) for b in got['blocks']])
    rho = N.EVAL_BOOT_RHO
    assert np.array_equal(np.isnan(got['table']), np.isnan(want)) and np.array_equal(np.isnan(want[:, rho]), np.isnan(table[:, rho]))
    if name in ('n1', 'constant'):
        assert np.isnan(got['table'][:, rho]).all()           # one row; a constant column
    err = np.nan_to_num(np.abs(got['table'] - want), nan=0.0)
    print(f'{name}: max table error {float(err.max()):.3e}, rho {float(err[:, rho].max()):.3e}')
    assert float(err.max()) <= 1e-9 and float(err[:, rho].max()) <= 1e-12
    other = [c for c in range(N.EVAL_BOOT_COLS) if c != rho]
    assert np.isfinite(got['table'][:, other]).all() and np.all(got['table'][:, N.EVAL_BOOT_PRECISION + C:N.EVAL_BOOT_RECALL] == 0)


def test_a_replicate_that_lacks_a_class():
    from rovit_hip import native as N
    from rovit_hip.evaluation import bootstrap_reference
    labels = torch.tensor([0] * 60 + [1] * 3 + [2])
    logits = torch.zeros(64, 3)
    logits[torch.arange(64), labels] = 4.0
    logits[:10, 1] = 6.0                                     # ten rows of class 0 are taken for class 1
    d = {'logits': logits, 'labels': labels, 'sev_true': labels.clone(), 'sev_pred': labels.float() + torch.linspace(-.4, .4, 64)}
    acc = _acc(d, 3)
    got = acc.bootstrap(num_resamples=64, seed=0, return_table=True, return_blocks=True)
    table, blocks = bootstrap_reference(acc.arrays(), 3, 10, 64, 0)
    cm = blocks[:, :9].reshape(64, 3, 3)
    absent = (cm.sum(axis=1)[:, 2] + cm.sum(axis=2)[:, 2]) == 0
    assert absent.any() and not absent.all(), 'seed 0: the restatement must have replicates with and without class 2'
    _assert_blocks(got['blocks'], blocks, 64, 'missing class')
    f1 = got['table'][:, N.EVAL_BOOT_F1:N.EVAL_BOOT_F1 + 3]
    macro = got['table'][:, N.EVAL_BOOT_MACRO_F1]
    assert np.abs(macro - table[:, N.EVAL_BOOT_MACRO_F1]).max() <= 1e-9
    for r in np.flatnonzero(absent):
        present = (cm[r].sum(axis=0) + cm[r].sum(axis=1)) > 0
        assert abs(macro[r] - f1[r][present].mean()) <= 1e-9 and abs(macro[r] - f1[r].sum() / 3) > 1.0, r


def test_both_h_paths_and_persistent_workgroups():
    from rovit_hip import native as N
    from rovit_hip.evaluation import bootstrap_reference
    for n in (N.EVAL_BOOT_LDS_ROWS, N.EVAL_BOOT_LDS_ROWS + 3):
        acc = _acc(make_data(n, 4, seed=n, ties=True), 4)
        got = acc.bootstrap(num_resamples=4, seed=5, return_table=True, return_blocks=True)
        table, blocks = bootstrap_reference(acc.arrays(), 4, 10, 4, 5)
        _assert_blocks(got['blocks'], blocks, n, 'H in LDS' if n == N.EVAL_BOOT_LDS_ROWS else 'H in the workspace')
        assert np.abs(got['table'] - table).max() <= 1e-9
        # a grid smaller than R: one workgroup serves several replicates in turn, and nothing changes
        for cap in (1, 3):
            capped = acc.bootstrap(num_resamples=4, seed=5, return_table=True, return_blocks=True, _max_workgroups=cap)
            assert capped['blocks'].tobytes() == got['blocks'].tobytes() and capped['table'].tobytes() == got['table'].tobytes(), (n, cap)
    assert N.load().rovit_eval_bootstrap_workspace_bytes(N.EVAL_BOOT_LDS_ROWS, 1000) == 0
    assert N.load().rovit_eval_bootstrap_workspace_bytes(N.EVAL_BOOT_LDS_ROWS + 3, 1000) == N.EVAL_BOOT_WORKSPACE_GRID * 8 * (N.EVAL_BOOT_LDS_ROWS + 3)


def test_table_and_blocks_are_bit_identical_across_calls_and_batch_splits():
    d = make_data(4099, 4, seed=5, ties=True)
    out = []
    for sizes in ((4099,), (4099,), (256,), (1, 7, 300)):
        b = _acc(d, 4, sizes=sizes).bootstrap(num_resamples=24, seed=9, return_table=True, return_blocks=True)
        out.append((b['table'].tobytes(), b['blocks'].tobytes()))
    acc = _acc(d, 4)
    acc.compute()                                            # the point block cached first: the same bootstrap
    b = acc.bootstrap(num_resamples=24, seed=9, return_table=True, return_blocks=True)
    out.append((b['table'].tobytes(), b['blocks'].tobytes()))
    assert out[0] == out[1], 'two calls differ'
    assert out[0] == out[2] == out[3] == out[4], 'the bootstrap depends on the batch split'


def test_stratified_resampling():
    from rovit_hip import native as N
    from rovit_hip.evaluation import bootstrap_reference
    d = make_data(1001, 4, seed=8, ties=True)
    absent = dict(d, labels=torch.where(d['labels'] == 2, torch.ones_like(d['labels']), d['labels']))       # class 2 never occurs
    for data in (d, absent):
        acc = _acc(data, 4, sizes=(300,))
        support = np.bincount(data['labels'].numpy(), minlength=4)
        got = acc.bootstrap(num_resamples=8, seed=3, stratified=True, return_table=True, return_blocks=True)
        table, blocks = bootstrap_reference(acc.arrays(), 4, 10, 8, 3, stratified=True)
        assert np.all(got['blocks'][:, N.EVAL_CONFUSION:N.EVAL_CONFUSION + 16].reshape(8, 4, 4).sum(axis=2) == support)
        _assert_blocks(got['blocks'], blocks, 1001, 'stratified')
        assert np.nan_to_num(np.abs(got['table'] - table)).max() <= 1e-9
    assert support[2] == 0


def test_paired_bootstrap_on_the_device_equals_the_cpu_path():
    """The CPU test's two score cards on the device against the same call on CPU tensors: every entry within 1e-9, p-values equal.

    The score cards are ``bootstrap_cases.exact_data``: logits whose fp32 softmax is exactly 1/m and 0 whoever computes it, so both paths
    record the same probabilities (asserted below) and the comparison is one of the two bootstraps.  On random logits the device's
    expf(z - max) / sum and the host's torch.softmax differ in the last bit of some rows, and the point values of Brier score and ECE
    already differ by 8.4e-10 and 1.49e-9 between the two ``compute()`` calls (600 rows, measured on the MI355X)."""
    from rovit_hip.evaluation import EvalAccumulator, paired_bootstrap
    a, b = paired_data()
    on_gpu = paired_bootstrap(_acc(a, 4), _acc(b, 4, sizes=(250,)), num_resamples=PAIR_R, seed=PAIR_SEED)
    cpu_a, cpu_b = feed(EvalAccumulator(4), a), feed(EvalAccumulator(4), b)
    for data, acc in ((a, cpu_a), (b, cpu_b)):                # the premise: identical records on both sides
        assert np.array_equal(_acc(data, 4).arrays()['y_probs'], acc.arrays()['y_probs'])
    on_cpu = paired_bootstrap(cpu_a, cpu_b, num_resamples=PAIR_R, seed=PAIR_SEED)
    assert on_gpu['mcnemar'] == on_cpu['mcnemar'] and on_gpu['accuracy']['p_value'] < 0.05 and on_gpu['accuracy']['lo'] > 0

    worst = {}

    def compare(name, g, c):
        worst[name] = max(abs(g[k] - c[k]) for k in ('a', 'b', 'diff', 'lo', 'hi'))
        print(f"{name}: p {g['p_value']!r} / {c['p_value']!r}, max difference {worst[name]:.3e}")
    for k in ('accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'brier_score', 'ece'):
        compare(k, on_gpu[k], on_cpu[k])
    for c in range(4):
        for k in ('precision', 'recall', 'f1'):
            compare(f'{k}[{c}]', on_gpu['per_class'][c][k], on_cpu['per_class'][c][k])
    for k in ('accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'brier_score', 'ece'):
        assert on_gpu[k]['p_value'] == on_cpu[k]['p_value'] and worst[k] <= 1e-9, (k, worst[k])
    assert max(worst.values()) <= 1e-9


def test_paired_bootstrap_on_the_device_equals_the_restatement_on_the_recorded_arrays():
    from rovit_hip import native as N
    from rovit_hip.evaluation import _paired, bootstrap_reference, paired_bootstrap
    a, b = paired_data_random_logits()
    acc_a, acc_b = _acc(a, 4), _acc(b, 4)
    got = paired_bootstrap(acc_a, acc_b, num_resamples=PAIR_R, seed=PAIR_SEED)
    ta, tb = (bootstrap_reference(acc.arrays(), 4, 10, PAIR_R, PAIR_SEED)[0] for acc in (acc_a, acc_b))
    ma, mb = acc_a.compute(), acc_b.compute()
    for name, col in (('brier_score', N.EVAL_BOOT_BRIER), ('ece', N.EVAL_BOOT_ECE), ('accuracy', N.EVAL_BOOT_ACCURACY)):
        want = _paired(tb[:, col] - ta[:, col], ma[name], mb[name], 0.95)
        assert got[name]['p_value'] == want['p_value']
        for k in ('a', 'b', 'diff', 'lo', 'hi'):
            assert abs(got[name][k] - want[k]) <= 1e-9, (name, k)


class _Copied(Exception):
    pass


@pytest.mark.parametrize('stratified', [False, True])
def test_bootstrap_of_a_fresh_accumulator_copies_once_and_hides_no_synchronisation(monkeypatch, stratified):
    from rovit_hip import native as N
    from rovit_hip.evaluation import paired_bootstrap
    d = make_data(1500, 4, seed=2)
    _acc(d, 4).bootstrap(num_resamples=16, stratified=stratified)          # warm: allocator pools, code objects
    acc, twin = _acc(d, 4), _acc(d, 4)
    real = torch.Tensor.cpu

    def stop(self, *a, **k):
        raise _Copied()
    torch.cuda.synchronize()
    # everything before the copy runs with synchronisation forbidden: a hidden one raises RuntimeError before .cpu() is reached
    monkeypatch.setattr(torch.Tensor, 'cpu', stop)
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(_Copied):
            acc.bootstrap(num_resamples=16, stratified=stratified)
        with pytest.raises(_Copied):
            paired_bootstrap(acc, twin, num_resamples=16, stratified=stratified)
    finally:
        torch.cuda.set_sync_debug_mode('default')
        monkeypatch.undo()
    copies = []
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (copies.append(tuple(self.shape)), real(self, *a, **k))[1])
    fresh = _acc(d, 4)
    b = fresh.bootstrap(num_resamples=16, stratified=stratified)
    m = fresh.compute()                                      # the point block came along: no second copy
    p = paired_bootstrap(_acc(d, 4), _acc(d, 4), num_resamples=16, stratified=stratified)
    monkeypatch.undo()
    W, COLS = N.EVAL_RESULT_WORDS, N.EVAL_BOOT_COLS
    assert copies == [(W + 16 * COLS,), (2 * W + 2 * 16 * COLS + 3,)], copies
    assert b['accuracy']['value'] == m['accuracy'] and np.isfinite(b['ece']['se']) and p['accuracy']['diff'] == 0.0


def test_descriptor_errors_are_refused_before_any_launch():
    from rovit_hip import native as N
    from rovit_hip.evaluation import RovitHipError
    n = 64
    acc = _acc(make_data(n, 4, seed=1), 4)
    acc.compute()
    table = torch.zeros(4 * N.EVAL_BOOT_COLS + 1, dtype=torch.float64, device=dev())

    def descriptor(**kw):
        d = N.EvalBoot()
        d.n, d.num_classes, d.n_bins, d.num_resamples, d.max_workgroups, d.seed = n, 4, 10, 4, 0, 0
        for k in ('probs', 'pred', 'label', 'sev_pred', 'sev_true'):
            setattr(d, k, N.ptr(acc._rec[k]))
        d.bin_edges, d.rank_counts, d.table = N.ptr(acc._edges), N.ptr(acc._rank_counts), N.ptr(table)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    N.call('rovit_eval_bootstrap', ctypes.byref(descriptor()), N.stream_ptr())           # the descriptor itself is sound
    torch.cuda.synchronize()
    for kw, text in (({'num_resamples': 0}, 'resamples'), ({'num_resamples': 65537}, 'resamples'), ({'n': N.EVAL_MAX_ROWS + 1}, 'rows'),
                     ({'n': 0}, 'rows'), ({'num_classes': 9}, 'classes'), ({'n_bins': 65}, 'bins'), ({'table': N.ptr(table) + 4}, 'aligned'),
                     ({'probs': N.ptr(acc._rec['probs']) + 4}, 'aligned'), ({'table': None}, 'null'), ({'rank_counts': None}, 'null'),
                     ({'perm': N.ptr(acc._rec['pred'])}, 'stratified'), ({'n': N.EVAL_BOOT_LDS_ROWS + 1}, 'workspace'),
                     ({'n': N.EVAL_BOOT_LDS_ROWS + 1, 'workspace': N.ptr(table), 'workspace_bytes': 64}, 'workspace')):
        with pytest.raises(RovitHipError, match=text):
            N.call('rovit_eval_bootstrap', ctypes.byref(descriptor(**kw)), N.stream_ptr())
    with pytest.raises(RovitHipError):
        acc.bootstrap(num_resamples=0)


def test_evaluator_with_bootstrap_on_the_depth2_model(tmp_path):
    from data.dataset import create_dataloaders
    from data.transforms import original_transforms
    from evaluation.evaluator import Evaluator
    from models.backbone import DeiTTiny
    from models.rovit_kan import RoViTKAN
    model = RoViTKAN(pretrained=False)
    model.backbone.model = DeiTTiny(depth=2)
    model.load_state_dict(ref_cpu.init_rovit_state(depth=2, seed=23), strict=True)
    model = model.to(dev()).eval()
    _, _, test_loader = create_dataloaders('data/Augmented Image', 'data/Original Image', CLASS_NAMES, SEVERITY,
                                           original_transform=original_transforms(), batch_size=8, synthetic=96, seed=7, device=dev())
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=CLASS_NAMES, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    model.backbone.model.precision = 'fp32'
    try:
        plain = Evaluator(model, test_loader, cfg, dev()).evaluate()
        plain_text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
        boot = Evaluator(model, test_loader, cfg, dev()).evaluate(bootstrap=16, bootstrap_seed=1)
    finally:
        model.backbone.model.precision = 'bf16'
    assert set(plain) == {'accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece', 'fps', 'params',
                          'params_m', 'per_class'}
    assert set(boot) == set(plain) | {'confidence_intervals'}
    ci = boot['confidence_intervals']
    for k in ('accuracy', 'macro_f1', 'weighted_f1', 'mae', 'brier_score', 'ece'):
        assert boot[k] == plain[k] == ci[k]['value']
        assert np.isfinite([ci[k]['lo'], ci[k]['hi'], ci[k]['se']]).all() and ci[k]['lo'] <= ci[k]['hi'], k
    assert ci['num_resamples'] == 16 and list(ci['per_class']) == CLASS_NAMES
    text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    assert '±' in text and '±' not in plain_text and text.count('[') >= 6
