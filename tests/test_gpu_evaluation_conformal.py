"""GPU tests of the conformal kernels (csrc/conformal.hip, csrc/conformal_device.h) and their Python layer (rovit_hip/evaluation.py:
EvalAccumulator.conformal, Conformal.evaluate, Conformal.predict), against the numpy statements ``conformal_block`` and
``conformal_apply_block`` on the kernel's OWN fp32 score columns and thresholds (``return_scores=True``).

Bounds.  Every integer word and every threshold: equal.  Scores: 'lac', 'kan_abs', 'mu_abs' and the non-randomised 'aps' are one IEEE
fp32 operation (or a running fp32 sum in a stated order) on recorded fp32 values, so they equal the numpy float32 expressions bit for
bit.  The randomised 'aps' is fma(-u, p_y, cum): ONE rounding of the exact cum - u p_y, an error of at most 2^-24 |s|.  'raps' rounds
once more after adding lambda max(0, r - k_reg) exactly: at most 2^-24 (|aps| + |raps|) <= 2^-23 |raps|, since 0 <= aps <= raps.
'mu_scaled' is one correctly rounded division: 2^-24 |s|.  Results below the normal range are off by at most 2^-150.  All three are
therefore within 2^-23 max(1, |s|) of the fp64 statement on the same fp32 inputs; the measured distance is printed beside the bound.
The sum of sigma over n rows in fp64: each of at most n additions is off by at most 2^-53 of a partial sum of at most n max sigma, on
both sides: n 2^-50 max sigma covers it."""
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
from conformal_cases import CASES, feed, held_out_rows, make_case, make_data  # noqa: E402

pytestmark = pytest.mark.gpu

CLASS_NAMES = ["Healthy Leaf", "Leaf Holes", "Black Spot", "Dry Leaf"]
SEVERITY = {n: i for i, n in enumerate(CLASS_NAMES)}


def dev():
    return torch.device('cuda:0')


def _acc(d, C, extra=('mu',), sizes=(1 << 30,)):
    from rovit_hip.evaluation import EvalAccumulator
    return feed(EvalAccumulator(C), d, sizes, device=dev(), extra=extra)


def _host(acc):
    """The accumulator's record and extra columns on the host, in the naming the numpy statements read."""
    a = {k: t[:acc.n].cpu().numpy() for k, t in acc._rec.items()}
    return a, {k: t[:acc.n].cpu().numpy() for k, t in acc._extra.items()}


_cache = {}


def _case(name):
    """(accumulator, its host arrays, its extras, fitted Conformal with the kernel's columns and block, kwargs): computed once, shared."""
    if name not in _cache:
        d, extra, kw = make_case(name)
        acc = _acc(d, CASES[name][1], extra)
        cp = acc.conformal(return_scores=True, **kw)
        for a in (cp.score_columns, cp.u, cp.block):
            a.setflags(write=False)
        _cache[name] = (acc, *_host(acc), cp, kw)
    return _cache[name]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _same_numbers(a, b):
    """Bit for bit where both are numbers, and NaN in the same places (a NaN's payload is not part of the definition)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and _same_bits(a[~nan], b[~nan])


@pytest.mark.parametrize('name', list(CASES))
def test_fit_block_equals_the_reference_on_the_kernels_own_columns(name):
    from rovit_hip import native as N
    from rovit_hip.evaluation import conformal_block, conformal_fraction, conformal_valid
    n, C, _, _ = CASES[name]
    acc, a, extras, cp, kw = _case(name)
    scores, alphas, cc = list(kw['scores']), list(kw['alphas']), kw.get('class_conditional', False)
    M, A, G = len(scores), len(alphas), 1 + C if cc else 1
    assert cp.score_columns.shape == (M, n) and cp.score_columns.dtype == np.float32 and cp.u.shape == (n,)
    valid = conformal_valid(cp.score_columns, scores, a['label'], a['uncertainty'], C)
    want = conformal_block(cp.score_columns, valid, a['label'], C, [conformal_fraction(x) for x in alphas], cc)
    assert cp.block.shape == want.shape == (N.eval_conformal_words(M, G, A),)
    assert cp.block.tolist() == want.tolist(), 'a word of the fit block differs'
    e = cp.block[N.EVAL_CONF_ENTRIES:].reshape(M, G, A, N.EVAL_CONF_ENTRY_WORDS)
    for m, s in enumerate(scores):
        for g in range(G):
            rows = valid[m] if g == 0 else valid[m] & (a['label'] == g - 1)
            v = np.sort(cp.score_columns[m][rows])
            for i, alpha in enumerate(alphas):
                n_g, k, less, equal, bits, trivial = (int(x) for x in e[m, g, i])
                q = np.asarray(cp.thresholds[s][alpha], dtype=np.float32).reshape(-1)[g]
                assert n_g == len(v) and q.view(np.uint32) == bits
                if trivial:
                    assert k > n_g and q == np.inf and np.asarray(cp.status[s][alpha]).reshape(-1)[g] == 'trivial'
                else:
                    assert less < k <= less + equal and _same_bits(q, v[k - 1]) and (v <= q).sum() >= k
    if name == 'n9_c4':
        assert all(cp.status[s][0.05] == 'trivial' and cp.thresholds[s][0.05] == np.inf for s in scores)
        assert all(cp.status[s][0.1] == 'ok' and cp.k[s][0.1] == 9 and cp.thresholds[s][0.1] == cp.score_columns[m].max() for m, s in enumerate(scores))
    if name == 'n256_c4_all_tied':
        assert all(cp.less[s][0.1] == 0 and cp.equal[s][0.1] == n for s in ('lac', 'kan_abs', 'mu_abs', 'mu_scaled'))
    if name == 'n1027_c4_class_absent':
        assert cp.n['lac'][3] == 0 and cp.status['lac'][0.1][3] == 'trivial' and cp.status['lac'][0.1][1] == 'ok'
    if name == 'n4099_c4_columns':
        wild = extras['wild']
        assert cp.bad_rows['wild'] == int((~np.isfinite(wild)).sum()) > 0 and cp.bad_rows['low'] == cp.bad_rows['high'] == 0
    if name == 'n4099_c8_class_conditional':
        assert cp.bad_labels == 2 and cp.bad_rows['mu_scaled'] == 2 and cp.bad_rows['mu_abs'] == 1 and cp.bad_rows['kan_abs'] == 0
        assert cp.bad_rows['aps'] == cp.bad_rows['raps'] == 1


@pytest.mark.parametrize('name', ['n19_c8', 'n20_c4', 'n257_c8_two_decimals', 'n4099_c4_columns', 'n4099_c8_class_conditional'])
def test_score_columns_against_numpy(name):
    from rovit_hip.evaluation import conformal_scores, conformal_uniforms
    n, C, _, _ = CASES[name]
    acc, a, extras, cp, kw = _case(name)
    scores = list(kw['scores'])
    p = {k: kw[k] for k in ('randomized', 'seed', 'raps_lambda', 'raps_k') if k in kw}
    ref = conformal_scores(a, extras, C, scores, **p)
    randomized = kw.get('randomized', True)
    assert _same_bits(cp.u, conformal_uniforms(n, kw.get('seed', 0)) if randomized else np.zeros(n, np.float32)), 'u'
    for m, s in enumerate(scores):
        got = cp.score_columns[m]
        if s in ('lac', 'kan_abs', 'mu_abs') or (s == 'aps' and not randomized) or s not in ('aps', 'raps', 'mu_scaled'):
            assert _same_numbers(got, ref['columns'][m]), s
            continue
        nan = np.isnan(ref['exact'][m])
        assert np.array_equal(np.isnan(got), nan), s
        with np.errstate(invalid='ignore'):
            dist = np.abs(got.astype(np.float64) - ref['exact'][m])[~nan & np.isfinite(ref['exact'][m])]
            bound = 2.0 ** -23 * np.maximum(1.0, np.abs(ref['exact'][m]))[~nan & np.isfinite(ref['exact'][m])]
        print(f'{name} {s}: max distance from the fp64 statement {float(dist.max()):.3e} (bound {float(bound.min()):.3e} and up)')
        assert np.all(dist <= bound), s
    if randomized and 'aps' in scores:                      # the same rows without randomisation: the running fp32 sum, bit for bit
        plain = acc.conformal(alphas=kw['alphas'], scores=['aps'], randomized=False, return_scores=True)
        assert _same_numbers(plain.score_columns[0], conformal_scores(a, extras, C, ['aps'], randomized=False)['columns'][0])


@pytest.mark.parametrize('name', ['n2_c2', 'n9_c4', 'n255_c2', 'n257_c8_two_decimals', 'n1027_c4_class_absent', 'n4099_c4_columns',
                                  'n4099_c8_class_conditional'])
def test_evaluate_block_equals_the_reference_given_the_kernels_thresholds(name):
    from rovit_hip import native as N
    from rovit_hip.evaluation import conformal_apply_block
    n, C, special, _ = CASES[name]
    acc, a, extras, cp, kw = _case(name)
    scores, A = list(kw['scores']), len(kw['alphas'])
    extra = tuple(extras)
    other = _acc(held_out_rows(name), C, extra)
    for which, rows in (('the fitted rows', acc), ('held-out rows', other)):
        got = cp.evaluate(rows)
        ra, re = _host(rows)
        want, _ = conformal_apply_block(ra, re, C, scores, cp.threshold_array(), row_offset=cp.rows, **cp.params)
        per = 16 + 32 * A
        sigma_words = [N.EVAL_CONF_APPLY_SCORES + m * per + 2 for m in range(len(scores))]
        keep = np.ones(len(want), dtype=bool)
        keep[sigma_words] = False
        assert got['block'][keep].tolist() == want[keep].tolist(), f'{which}: an integer word differs'
        with np.errstate(invalid='ignore'):
            sg = ra['uncertainty'][np.isfinite(ra['uncertainty'])]
        bound = rows.n * 2.0 ** -50 * float(sg.max())
        err = float(np.abs(got['block'][sigma_words].view(np.float64) - want[sigma_words].view(np.float64)).max())
        print(f'{name}, {which}: sum of sigma off by {err:.3e} (bound {bound:.3e})')
        assert err <= bound
        assert got['n'] == rows.n
        for s in scores:
            for alpha, lv in got['scores'][s]['levels'].items():
                if 'size_histogram' in lv:
                    assert sum(lv['size_histogram']) == got['scores'][s]['n'] and len(lv['size_histogram']) == C + 1
                drawn = s in ('aps', 'raps') and cp.randomized          # evaluate() draws u past the fitted rows' counters: other scores
                if which == 'the fitted rows' and not kw.get('class_conditional') and not drawn and got['scores'][s]['n']:
                    # on the calibration rows themselves the share of rows with s <= q is at least k / n_g
                    assert lv['coverage'] >= min(1.0, cp.k[s][alpha] / cp.n[s]) - 1e-12, (s, alpha)


def test_blocks_are_bit_identical_across_calls_batch_splits_and_grids():
    d, extra, _ = make_case('n4099_c4_columns')
    kw = dict(alphas=(0.1, 0.05, 0.5), scores=('lac', 'aps', 'raps', 'kan_abs', 'mu_scaled', 'wild', 'high'), class_conditional=True)
    held = held_out_rows('n4099_c4_columns')
    fit, ev = [], []
    for sizes in ((4099,), (4099,), (256,), (1, 7, 300)):
        acc = _acc(d, 4, extra, sizes)
        cp = acc.conformal(return_scores=True, **kw)
        fit.append(cp.block.tobytes())
        ev.append(cp.evaluate(_acc(held, 4, extra, sizes))['block'].tobytes())
    assert fit[0] == fit[1] and ev[0] == ev[1], 'two calls differ'
    assert fit[0] == fit[2] == fit[3] and ev[0] == ev[2] == ev[3], 'a block depends on the batch split'
    acc, rows = _acc(d, 4, extra), _acc(held, 4, extra)
    for cap in (0, 1, 3):
        cp = acc.conformal(return_scores=True, _max_workgroups=cap, **kw)
        assert cp.block.tobytes() == fit[0], f'fit, max_workgroups = {cap}'
        assert cp.evaluate(rows, _max_workgroups=cap)['block'].tobytes() == ev[0], f'evaluate, max_workgroups = {cap}'


def test_predict_gives_the_reference_membership_and_the_intervals():
    from rovit_hip.evaluation import conformal_class_scores, conformal_membership, conformal_uniforms
    acc, a, extras, cp, kw = _case('n1027_c4_class_absent')
    d = held_out_rows('n1027_c4_class_absent')
    out = {'cls_logits': d['logits'].to(dev()), 'kan_severity': d['sev_pred'].reshape(-1, 1).to(dev()), 'mu': d['mu'].reshape(-1, 1).to(dev()),
           'log_var': d['log_var'].reshape(-1, 1).to(dev())}
    B = d['logits'].shape[0]
    probs = torch.softmax(out['cls_logits'].float(), dim=1).cpu().numpy()
    for score in ('lac', 'aps', 'raps'):
        for alpha, offset in ((None, 0), (0.25, 1000)):
            got = cp.predict(out, score=score, alpha=alpha, row_offset=offset)
            s, _ = conformal_class_scores(probs, score, conformal_uniforms(B, cp.seed, offset), cp.raps_lambda, cp.raps_k)
            level = cp.alphas[0] if alpha is None else alpha
            want = conformal_membership(s, cp.threshold_array([score], [level])[0, :, 0], True)
            assert got['sets'].is_cuda and got['sets'].dtype == torch.bool and got['sets'].shape == (B, 4)
            assert np.array_equal(got['sets'].cpu().numpy(), want), (score, alpha)
            assert torch.equal(got['set_size'], got['sets'].sum(dim=1))
    got = cp.predict(out, score='aps')
    q_kan, q_mu = float(np.float32(cp.thresholds['kan_abs'][0.1][0])), float(np.float32(cp.thresholds['mu_scaled'][0.1][0]))
    kan, mu, sigma = out['kan_severity'].reshape(-1), out['mu'].reshape(-1), torch.exp(0.5 * out['log_var'].reshape(-1))
    assert torch.equal(got['kan_interval'], torch.stack([kan - q_kan, kan + q_kan], dim=1))
    assert torch.equal(got['mu_interval'], torch.stack([mu - q_mu * sigma, mu + q_mu * sigma], dim=1))


class _Copied(Exception):
    pass


def test_conformal_and_evaluate_copy_once_and_predict_never(monkeypatch):
    from rovit_hip import native as N
    from rovit_hip.evaluation import EvalAccumulator
    n = 1500
    d = {k: v.to(dev()) for k, v in make_data(n, 4, seed=2).items()}
    out = {'cls_logits': d['logits'], 'kan_severity': d['sev_pred'].reshape(-1, 1), 'mu': d['mu'].reshape(-1, 1), 'log_var': d['log_var'].reshape(-1, 1)}
    warm = _acc(d, 4).conformal(class_conditional=True)          # warm: allocator pools, code objects
    warm.evaluate(_acc(d, 4))
    warm.predict(out)
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
            acc.conformal(class_conditional=True)
        with pytest.raises(_Copied):
            acc.conformal(alphas=(0.1, 0.2), return_scores=True)
        with pytest.raises(_Copied):
            warm.evaluate(acc)
        sets = warm.predict(out, score='raps', row_offset=5)          # no copy at all: .cpu() would raise
    finally:
        torch.cuda.set_sync_debug_mode('default')
        monkeypatch.undo()
    assert sets['sets'].shape == (n, 4) and 'kan_interval' in sets and 'mu_interval' in sets
    copies = []
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (copies.append(tuple(self.shape)), real(self, *a, **k))[1])
    fresh = feed(EvalAccumulator(4), d, sizes=(700,), extra=('mu',))
    cp = fresh.conformal(class_conditional=True)
    cp2 = fresh.conformal(alphas=(0.1, 0.2), return_scores=True)
    cp.evaluate(fresh)
    cp.predict(out)
    monkeypatch.undo()
    assert copies == [(N.eval_conformal_words(6, 5, 1),), (N.eval_conformal_words(6, 1, 2) + (7 * n + 1) // 2,),
                      (N.eval_conformal_apply_words(6, 1),)], copies
    assert cp2.score_columns.shape == (6, n)


def test_descriptor_errors_are_refused_before_any_launch():
    from rovit_hip import native as N
    from rovit_hip.evaluation import RovitHipError
    n, C, M, A = 64, 4, 3, 2
    acc = _acc(make_data(n, C, seed=1), C)
    lib = N.load()
    ws_bytes = lib.rovit_eval_conformal_workspace_bytes(n, M, 1, A)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    assert lib.rovit_eval_conformal_workspace_bytes(n, 9, 1, A) == 0 and lib.rovit_eval_conformal_workspace_bytes(n, M, 1, 9) == 0
    assert lib.rovit_eval_conformal_workspace_bytes(0, M, 1, A) == 0 and lib.rovit_eval_conformal_apply_workspace_bytes(n, 9) == 0
    workspace = torch.zeros(ws_bytes + 16, dtype=torch.uint8, device=dev())
    result = torch.zeros(max(N.eval_conformal_words(M, 1, A), N.eval_conformal_apply_words(M, A)) + 1, dtype=torch.int64, device=dev())
    thresholds = torch.full((M * A,), 0.5, dtype=torch.float32, device=dev())
    member = torch.zeros(n * A, dtype=torch.uint8, device=dev())
    column = acc._extra['mu']

    def descriptor(kw=None):
        d = N.EvalConf()
        d.n, d.num_classes, d.num_scores, d.num_levels, d.randomized, d.raps_k, d.raps_lambda = n, C, M, A, 1, 1, 0.01
        d.score_kind[0], d.score_kind[1], d.score_kind[2] = N.EVAL_CONF_APS, N.EVAL_CONF_MU_SCALED, N.EVAL_CONF_COLUMN
        d.score_column[2] = N.ptr(column)
        d.alpha_num[0], d.alpha_den[0], d.alpha_num[1], d.alpha_den[1] = 1, 10, 1, 4
        for k in ('probs', 'label', 'sev_pred', 'sev_true', 'uncertainty'):
            setattr(d, k, N.ptr(acc._rec[k]))
        d.mu, d.thresholds = N.ptr(column), N.ptr(thresholds)
        d.workspace, d.workspace_bytes, d.result = N.ptr(workspace), ws_bytes, N.ptr(result)
        for k, v in (kw or {}).items():
            if isinstance(k, tuple):
                getattr(d, k[0])[k[1]] = v
            else:
                setattr(d, k, v)
        return d

    for entry in ('rovit_eval_conformal', 'rovit_eval_conformal_apply'):          # the descriptor itself is sound
        N.call(entry, ctypes.byref(descriptor()), N.stream_ptr())
        torch.cuda.synchronize()
        assert int(result[N.EVAL_CONF_N]) == n
    both = (({'n': 0}, 'rows'), ({'n': N.EVAL_MAX_ROWS + 1}, 'rows'), ({'num_classes': 9}, 'classes'), ({'num_classes': 1}, 'classes'),
            ({'num_scores': 0}, 'scores'), ({'num_scores': 9}, 'scores'), ({'num_levels': 0}, 'levels'), ({'num_levels': 9}, 'levels'),
            ({'max_workgroups': -1}, 'max_workgroups'), ({'raps_k': -1}, 'raps_k'), ({'raps_lambda': float('nan')}, 'raps_lambda'),
            ({'row_offset': 0xFFFFFFFF}, 'row_offset'), ({('score_kind', 0): 7}, 'unknown kind'), ({('score_kind', 1): -1}, 'unknown kind'),
            ({('score_column', 2): None}, 'null'), ({'probs': None}, 'null'), ({'sev_true': None}, 'null'), ({'mu': None}, 'null'),
            ({'uncertainty': None}, 'null'), ({'result': None}, 'null'), ({'workspace': None}, 'null'),
            ({('score_column', 2): N.ptr(column) + 2}, 'aligned'), ({'probs': N.ptr(acc._rec['probs']) + 4}, 'aligned'),
            ({'label': N.ptr(acc._rec['label']) + 2}, 'aligned'), ({'mu': N.ptr(column) + 1}, 'aligned'),
            ({'result': N.ptr(result) + 4}, 'aligned'), ({'workspace': N.ptr(workspace) + 8}, 'aligned'),
            ({'workspace_bytes': 0}, 'workspace holds'))
    fit_only = (({'label': None}, 'null'), ({('alpha_num', 0): 0}, 'level 0'), ({('alpha_num', 1): 4}, 'level 1'), ({('alpha_num', 1): 5}, 'level 1'),
                ({('alpha_den', 0): (1 << 20) + 1}, 'level 0'), ({'workspace_bytes': ws_bytes - 16}, 'workspace holds'),
                ({'scores_out': N.ptr(column) + 2}, 'aligned'), ({'u_out': N.ptr(column) + 1}, 'aligned'))
    apply_only = (({'thresholds': None}, 'null'), ({'thresholds': N.ptr(thresholds) + 2}, 'aligned'),
                  ({'label': None}, 'needs the labels'), ({'label': None, 'num_scores': 1}, 'nothing to do'))
    before = result.clone()
    for entry, cases in (('rovit_eval_conformal', both + fit_only), ('rovit_eval_conformal_apply', both + apply_only)):
        for kw, text in cases:
            with pytest.raises(RovitHipError, match=text):
                N.call(entry, ctypes.byref(descriptor(kw)), N.stream_ptr())
        with pytest.raises(RovitHipError, match='null'):
            N.call(entry, None, N.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(result, before), 'a refused descriptor touched the result block'
    # the deployment form of the application: no labels, class scores only, a membership matrix
    N.call('rovit_eval_conformal_apply', ctypes.byref(descriptor({'label': None, 'num_scores': 1, 'member_out': N.ptr(member), 'result': None,
                                                                     'workspace': None, 'workspace_bytes': 0})), N.stream_ptr())
    torch.cuda.synchronize()
    assert int(member.max()) < 16


def test_evaluator_with_conformal_on_the_depth2_model(tmp_path):
    from data.dataset import create_dataloaders
    from data.transforms import original_transforms
    from evaluation.evaluator import Evaluator
    from models.backbone import DeiTTiny
    from models.rovit_kan import RoViTKAN
    from rovit_hip.evaluation import Conformal
    model = RoViTKAN(pretrained=False)
    model.backbone.model = DeiTTiny(depth=2)
    model.load_state_dict(ref_cpu.init_rovit_state(depth=2, seed=23), strict=True)
    model = model.to(dev()).eval()
    _, val_loader, test_loader = create_dataloaders('data/Augmented Image', 'data/Original Image', CLASS_NAMES, SEVERITY,
                                                    original_transform=original_transforms(), batch_size=8, synthetic=96, seed=7, device=dev())
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=CLASS_NAMES, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    model.backbone.model.precision = 'fp32'
    try:
        plain = Evaluator(model, test_loader, cfg, dev()).evaluate()
        plain_text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
        ev = Evaluator(model, test_loader, cfg, dev())
        cp = ev.fit_conformal(test_loader, alphas=(0.1, 0.2))
        with_cp = ev.evaluate(conformal=cp)
        text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
        again = Evaluator(model, test_loader, cfg, dev()).evaluate()
        again_text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    finally:
        model.backbone.model.precision = 'bf16'
    assert isinstance(cp, Conformal) and ev.conformal is cp and cp.scores == ['lac', 'aps', 'raps', 'kan_abs', 'mu_abs', 'mu_scaled']
    assert set(with_cp) == set(plain) | {'conformal'} and set(again) == set(plain)
    strip = lambda t: '\n'.join(l for l in t.splitlines() if not l.startswith('FPS:'))          # a measured time
    assert strip(again_text) == strip(plain_text)
    for k in plain:
        if k != 'fps':
            assert with_cp[k] == plain[k] == again[k] or (with_cp[k] != with_cp[k] and plain[k] != plain[k]), k
    card = with_cp['conformal']
    n = sum(c['support'] for c in plain['per_class'].values())
    assert card['n'] == n and card['bad_labels'] == 0 and list(card['scores']) == cp.scores
    for s in cp.scores:
        for alpha in (0.1, 0.2):
            lv = card['scores'][s]['levels'][alpha]
            assert 0.0 <= lv['coverage'] <= 1.0
            if s not in ('aps', 'raps'):
                # fitted and evaluated on the same rows here, with no u drawn: the share of rows with s <= q is at least k / n
                assert lv['coverage'] >= min(1.0, cp.k[s][alpha] / cp.n[s]) - 1e-12, (s, alpha)
    assert 'Conformal prediction' in text and 'Conformal prediction' not in plain_text and 'mu_scaled' in text
