"""GPU tests of the selective-prediction kernels (csrc/selective.hip) and their Python layer (rovit_hip/evaluation.py:
EvalAccumulator.selective, update(extra=...)), against the numpy fp64 restatement ``selective_reference`` on the kernel's OWN fp32 key
and risk matrices (``return_keys=True``).

Bounds.  Integer words and thresholds: equal.  fp64 words: n * 2^-50 * max(1, max l) absolute: each of at most n additions is off by at
most 2^-53 of a partial sum of at most n max l, it is divided by k, and this happens on both sides; a factor of 4 covers the tie
interpolation and the mean.  Keys: confidence, sigma and abs_err are one IEEE operation on recorded fp32 values, so they equal the numpy
float32 expression bit for bit; entropy is within 1e-6 of the fp64 entropy of the recorded probabilities (at most 8 terms of magnitude
at most 0.37, logf within 2 ulp)."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ref_cpu  # noqa: E402  (checker only)
from selective_cases import feed, make_data  # noqa: E402

pytestmark = pytest.mark.gpu

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
SEVERITY = {n: i for i, n in enumerate(CLASS_NAMES)}
BUILTIN = (['confidence', 'entropy', 'sigma'], ['error', 'abs_err'])
ROUNDED = (['conf2', 'ent2', 'sig2'], ['error', 'abs_err'])
WIDE = (['confidence', 'entropy', 'sigma', 'mu', 'c1', 'c2', 'c3', 'c4'], ['error', 'abs_err', 'mu_abs_err', 'r3'])
# name: (n, scores and risks, P)
CASES = {'n1': (1, BUILTIN, 20), 'n2': (2, BUILTIN, 20), 'n5_all_tied': (5, BUILTIN, 20), 'n257': (257, BUILTIN, 20),
         'n1000_two_decimals': (1000, ROUNDED, 20), 'n1027': (1027, BUILTIN, 20), 'n2051': (2051, BUILTIN, 20), 'n257_wide': (257, WIDE, 256),
         # around the 1024-row LDS tile of the counting rank: last tile one short, exactly full, one row in a new tile
         'n1023': (1023, BUILTIN, 20), 'n1024': (1024, BUILTIN, 20), 'n1025': (1025, BUILTIN, 20)}


def dev():
    return torch.device('cuda:0')


def _data(name):
    n, (scores, risks), _ = CASES[name]
    d = make_data(n, 4, seed=300 + n, ties=True)
    g = torch.Generator().manual_seed(n)
    if name == 'n5_all_tied':
        d['logits'] = d['logits'][:1].repeat(n, 1)
        d['log_var'] = torch.full((n,), -0.5)
    if scores is ROUNDED[0]:
        p = torch.softmax(d['logits'], dim=1)
        d['conf2'] = ((1 - p.max(dim=1)[0]) * 100).round() / 100
        d['ent2'] = (-(p * torch.log(p)).sum(dim=1) * 100).round() / 100
        d['sig2'] = (torch.exp(0.5 * d['log_var']) * 100).round() / 100
    if scores is WIDE[0]:
        for k in range(1, 5):
            d[f'c{k}'] = (torch.randn(n, generator=g) * k).round() / k          # negative keys, -0.0 and ties
        d['r3'] = torch.rand(n, generator=g) * 7
    extra = tuple(x for x in scores + risks if x in d and x not in ('mu',)) + ('mu',)
    return d, extra


def _acc(d, extra=('mu',), sizes=(1 << 30,)):
    from rovit_hip.evaluation import EvalAccumulator
    return feed(EvalAccumulator(4), d, sizes, device=dev(), extra=extra)


_cache = {}


def _case(name):
    """(accumulator, selective() result with the kernel's keys and block) of one case: computed once, shared, never changed."""
    if name not in _cache:
        n, (scores, risks), P = CASES[name]
        d, extra = _data(name)
        acc = _acc(d, extra)
        res = acc.selective(scores=scores, risks=risks, coverages=P, return_keys=True)
        for a in (res['keys'], res['risk_values'], res['block']):
            a.setflags(write=False)
        _cache[name] = (acc, res)
    return _cache[name]


@pytest.mark.parametrize('name', list(CASES))
def test_block_against_the_reference_on_the_kernels_own_keys(name):
    from rovit_hip import native as N
    from rovit_hip.evaluation import selective_block, selective_reference
    n, (scores, risks), P = CASES[name]
    _, res = _case(name)
    S, K = len(scores), len(risks)
    assert res['keys'].shape == (S, n) and res['risk_values'].shape == (K, n) and res['keys'].dtype == np.float32
    want = selective_block(res['keys'], res['risk_values'], P)
    got = res['block']
    off = N.eval_selective_offsets(S, K, P)
    assert got.shape == want.shape == (off['words'],)
    H = N.EVAL_SEL_HEADER
    assert got[:H].tolist() == want[:H].tolist() == [0, 0, 0, 0, n, 0, 0, 0]
    assert np.array_equal(got[off['thresholds']:], want[off['thresholds']:]), 'thresholds differ'
    err = np.abs(got[H:off['thresholds']].view(np.float64) - want[H:off['thresholds']].view(np.float64))
    bound = n * 2.0 ** -50 * max(1.0, float(res['risk_values'].max()))
    print(f'{name}: max fp64 word error {float(err.max()):.3e} (bound {bound:.3e})')
    assert float(err.max()) <= bound
    ref = selective_reference(res['keys'], res['risk_values'], P)
    assert np.array_equal(res['coverages'], ref['coverages']) and res['n'] == n
    for s, score in enumerate(scores):
        for k, risk in enumerate(risks):
            e = res['scores'][score][risk]
            assert abs(e['aurc'] - ref['aurc'][s, k]) <= bound and e['e_aurc'] == e['aurc'] - res['risks'][risk]['oracle_aurc']
            assert e['e_aurc'] >= -2 * bound
    if name == 'n5_all_tied':                                  # one tie group: the curve is flat at the mean, aurc = mean
        for score in scores:
            for risk in risks:
                e, mean = res['scores'][score][risk], res['risks'][risk]['mean']
                assert abs(e['aurc'] - mean) <= bound and np.abs(e['curve'] - mean).max() <= bound


def test_keys_are_the_numpy_float32_expressions_of_the_recorded_arrays():
    for name in ('n257', 'n2051'):
        acc, res = _case(name)
        a = acc.arrays()
        assert np.array_equal(res['keys'][0], np.float32(1) - a['y_probs'].max(axis=1)), 'confidence'
        assert np.array_equal(res['keys'][2], a['uncertainty']), 'sigma'
        assert np.array_equal(res['risk_values'][0], (a['y_pred'] != a['y_true']).astype(np.float32)), 'error'
        assert np.array_equal(res['risk_values'][1], np.abs(a['severity_true'] - a['severity_pred'])), 'abs_err'
        p = a['y_probs'].astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            h = -np.where(p == 0, 0.0, p * np.log(p)).sum(axis=1)
        err = float(np.abs(res['keys'][1].astype(np.float64) - h).max())
        print(f'{name}: max entropy error {err:.3e} (bound 1e-6)')
        assert err <= 1e-6
    acc, res = _case('n257_wide')
    a = acc.arrays()
    d, _ = _data('n257_wide')
    assert np.array_equal(res['risk_values'][2], np.abs(a['severity_true'] - d['mu'].numpy())), 'mu_abs_err'
    assert np.array_equal(res['keys'][4], d['c1'].numpy()) and np.array_equal(res['risk_values'][3], d['r3'].numpy())
    # probabilities of exactly 0 and 1: the entropy term at p = 0 is 0, the confidence key of a certain row is 0
    z = make_data(8, 4, seed=1)
    z['logits'] = torch.full((8, 4), -200.0)
    z['logits'][torch.arange(8), z['labels']] = 0.0
    sure = _acc(z).selective(return_keys=True)
    assert np.all(sure['keys'][0] == 0) and np.all(sure['keys'][1] == 0)
    assert sure['scores']['confidence']['error']['aurc'] == sure['risks']['error']['mean'] == 0.0


def test_block_is_bit_identical_across_calls_batch_splits_and_grids():
    d = make_data(4099, 4, seed=5, ties=True)
    out = []
    for sizes in ((4099,), (4099,), (256,), (1, 7, 300)):
        out.append(_acc(d, sizes=sizes).selective(return_keys=True)['block'].tobytes())
    assert out[0] == out[1], 'two calls differ'
    assert out[0] == out[2] == out[3], 'the block depends on the batch split'
    acc = _acc(d)
    for cap in (0, 1, 3):
        assert acc.selective(return_keys=True, _max_workgroups=cap)['block'].tobytes() == out[0], f'max_workgroups = {cap}'
    blk = np.frombuffer(out[0], dtype=np.int64)
    assert blk[4] == 4099 and np.isfinite(blk[8:].view(np.float64)).all()


class _Copied(Exception):
    pass


def test_selective_of_a_fresh_accumulator_copies_once_and_hides_no_synchronisation(monkeypatch):
    from rovit_hip import native as N
    from rovit_hip.evaluation import EvalAccumulator
    n = 1500
    d = {k: v.to(dev()) for k, v in make_data(n, 4, seed=2).items()}
    _acc(d).selective(risks=['error', 'abs_err', 'mu_abs_err'])          # warm: allocator pools, code objects
    real = torch.Tensor.cpu

    def stop(self, *a, **k):
        raise _Copied()
    torch.cuda.synchronize()
    # update(extra=...) and everything before the copy run with synchronisation forbidden: a hidden one raises RuntimeError
    monkeypatch.setattr(torch.Tensor, 'cpu', stop)
    torch.cuda.set_sync_debug_mode('error')
    try:
        acc = feed(EvalAccumulator(4), d, sizes=(700,), extra=('mu',))
        with pytest.raises(_Copied):
            acc.selective(risks=['error', 'abs_err', 'mu_abs_err'])
        with pytest.raises(_Copied):
            acc.selective(return_keys=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
        monkeypatch.undo()
    copies = []
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (copies.append(tuple(self.shape)), real(self, *a, **k))[1])
    fresh = feed(EvalAccumulator(4), d, sizes=(700,), extra=('mu',))
    a = fresh.selective(risks=['error', 'abs_err', 'mu_abs_err'])
    b = fresh.selective(return_keys=True)
    monkeypatch.undo()
    W3, W2 = N.eval_selective_offsets(3, 3, 20)['words'], N.eval_selective_offsets(3, 2, 20)['words']
    assert copies == [(W3,), (W2 + (5 * n + 1) // 2,)], copies
    assert a['scores']['sigma']['error']['aurc'] == b['scores']['sigma']['error']['aurc'] and np.isfinite(a['scores']['sigma']['mu_abs_err']['aurc'])


def test_descriptor_errors_are_refused_before_any_launch():
    from rovit_hip import native as N
    from rovit_hip.evaluation import RovitHipError
    n = 64
    acc = _acc(make_data(n, 4, seed=1))
    S, K, P = 2, 2, 20
    ws_bytes = N.load().rovit_eval_selective_workspace_bytes(n, S, K)
    assert ws_bytes > 0 and ws_bytes % 16 == 0 and N.load().rovit_eval_selective_workspace_bytes(n, 9, K) == 0
    workspace = torch.zeros(ws_bytes + 16, dtype=torch.uint8, device=dev())
    result = torch.zeros(N.eval_selective_offsets(S, K, P)['words'] + 1, dtype=torch.int64, device=dev())
    column = acc._extra['mu']

    def descriptor(kw=None):
        d = N.EvalSel()
        d.n, d.num_classes, d.num_scores, d.num_risks, d.num_coverages, d.max_workgroups = n, 4, S, K, P, 0
        d.score_kind[0], d.score_kind[1] = N.EVAL_SEL_CONFIDENCE, N.EVAL_SEL_SCORE_COLUMN
        d.risk_kind[0], d.risk_kind[1] = N.EVAL_SEL_ABS_ERR, N.EVAL_SEL_RISK_COLUMN
        d.score_column[1], d.risk_column[1] = N.ptr(column), N.ptr(acc._rec['uncertainty'])
        for k in ('probs', 'pred', 'label', 'sev_pred', 'sev_true', 'uncertainty'):
            setattr(d, k, N.ptr(acc._rec[k]))
        d.workspace, d.workspace_bytes, d.result = N.ptr(workspace), ws_bytes, N.ptr(result)
        for k, v in (kw or {}).items():
            if isinstance(k, tuple):
                getattr(d, k[0])[k[1]] = v
            else:
                setattr(d, k, v)
        return d

    N.call('rovit_eval_selective', ctypes.byref(descriptor()), N.stream_ptr())            # the descriptor itself is sound
    torch.cuda.synchronize()
    assert int(result[N.EVAL_SEL_N]) == n
    for kw, text in (({'n': 0}, 'rows'), ({'n': N.EVAL_MAX_ROWS + 1}, 'rows'), ({'num_classes': 9}, 'classes'),
                     ({'num_scores': 0}, 'scores'), ({'num_scores': 9}, 'scores'), ({'num_risks': 0}, 'risks'), ({'num_risks': 5}, 'risks'),
                     ({'num_coverages': 0}, 'coverages'), ({'num_coverages': 257}, 'coverages'), ({'max_workgroups': -1}, 'max_workgroups'),
                     ({('score_kind', 0): 4}, 'unknown kind'), ({('risk_kind', 0): -1}, 'unknown kind'),
                     ({('score_column', 1): None}, 'null'), ({('risk_column', 1): None}, 'null'), ({'probs': None}, 'null'),
                     ({'label': None}, 'null'), ({'sev_true': None}, 'null'), ({'result': None}, 'null'), ({'workspace': None}, 'null'),
                     ({('score_kind', 0): N.EVAL_SEL_SIGMA, 'uncertainty': None}, 'null'),
                     ({('score_column', 1): N.ptr(column) + 2}, 'aligned'), ({('risk_column', 1): N.ptr(column) + 1}, 'aligned'),
                     ({'probs': N.ptr(acc._rec['probs']) + 4}, 'aligned'), ({'result': N.ptr(result) + 4}, 'aligned'),
                     ({'workspace': N.ptr(workspace) + 8}, 'aligned'), ({'keys_out': N.ptr(column) + 2}, 'aligned'),
                     ({'workspace_bytes': ws_bytes - 16}, 'workspace holds'), ({'workspace_bytes': 0}, 'workspace holds')):
        with pytest.raises(RovitHipError, match=text):
            N.call('rovit_eval_selective', ctypes.byref(descriptor(kw)), N.stream_ptr())
    with pytest.raises(RovitHipError, match='null'):
        N.call('rovit_eval_selective', None, N.stream_ptr())


def test_nan_key_negative_risk_and_bad_label_raise_from_selective():
    from rovit_hip.evaluation import RovitHipError
    d = make_data(300, 4, seed=4)
    d['s'] = d['mu'].clone()
    d['s'][17] = float('nan')
    d['r'] = d['mu'].abs()
    d['r'][200] = -0.5
    acc = _acc(d, extra=('mu', 's', 'r'))
    with pytest.raises(RovitHipError, match='1 non-finite score'):
        acc.selective(scores=['confidence', 's'])
    with pytest.raises(RovitHipError, match='1 negative risk'):
        acc.selective(risks=['r'])
    assert np.isfinite(acc.selective(scores=['mu'], risks=['mu_abs_err'])['scores']['mu']['mu_abs_err']['aurc'])
    d['labels'][5] = 9
    with pytest.raises(RovitHipError, match='1 class labels outside'):
        _acc(d, extra=('mu', 's', 'r')).selective(scores=['mu'])
    with pytest.raises(RovitHipError, match='differ'):
        acc.update({'cls_logits': d['logits'][:2].to(dev()), 'kan_severity': None, 'mu': None, 'log_var': None}, d['labels'][:2], d['sev_true'][:2],
                   extra={'mu': d['mu'][:2].to(dev())})


def test_evaluator_with_selective_and_mc_dropout_on_the_depth2_model(tmp_path):
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
        sel = Evaluator(model, test_loader, cfg, dev()).evaluate(selective=True, mc_samples=4)
    finally:
        model.backbone.model.precision = 'bf16'
    assert set(plain) == {'accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece', 'fps', 'params',
                          'params_m', 'per_class'}
    assert set(sel) == set(plain) | {'selective'}
    for k in plain:
        if k != 'fps':                                         # a measured time
            assert sel[k] == plain[k] or (sel[k] != sel[k] and plain[k] != plain[k]), k
    card = sel['selective']
    assert card['n'] == sum(c['support'] for c in plain['per_class'].values()) and list(card['risks']) == ['error', 'abs_err', 'mu_abs_err']
    assert list(card['scores']) == ['confidence', 'entropy', 'sigma', 'predictive_entropy_mc', 'mutual_information', 'epistemic_var', 'uncertainty_std']
    for score in ('confidence', 'entropy', 'sigma', 'mutual_information'):
        for risk in card['risks']:
            e = card['scores'][score][risk]
            assert np.isfinite(e['aurc']) and np.isfinite(e['curve']).all() and e['aurc'] >= card['risks'][risk]['oracle_aurc'] - 1e-12, (score, risk)
        assert np.all(np.diff(card['scores'][score]['thresholds']) >= 0)
    text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    assert 'Selective prediction' in text and 'Selective prediction' not in plain_text and 'mutual_information' in text and 'Risk@90%' in text
