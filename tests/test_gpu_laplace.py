"""GPU tests of csrc/laplace.hip through rovit_hip.laplace: the weights, gram and predict kernels against the numpy fp64 statements on the
kernels' own inputs, their determinism, and the model / Evaluator entry points end to end.

Tolerances: four times the error of an fp32 numpy evaluation of the same formulas against fp64, maximum over each matrix
(laplace_cases.tolerance; the rule of tests/test_gpu_corrupt.py), computed from the references alone.  The tests print the ratio
error / tolerance before they assert.

Measured on the MI355X over the cases below:
  gram      max error / tolerance = 0.520 (n = 33, E = hid = 32, C = 8; 0.04 .. 0.52 over the 40 cases)
  predict   max error / tolerance = 0.250 (B = 300, E = hid = 32, C = 1; 0.017 .. 0.25 over the 32 cases)
With the hidden rows formed by an fp32 chain on the matrix instruction the gram ratio reached 1.22 (n = 1, E = hid = 32, C = 4), and 1.06 /
1.09 with four interleaved chains (n = 1, E = 192, hid = 128, C = 8; n = 31, E = hid = 32, C = 8): csrc/laplace.hip accumulates fc1 in fp64.
"""
import ctypes
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import laplace_cases as cases  # noqa: E402
from oracle import ref_cpu  # noqa: E402  (checker only)

from rovit_hip import laplace as L  # noqa: E402
from rovit_hip import native  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (192, 128)]
CLASSES = [1, 2, 4, 8]                     # 1: the Gaussian head, K = 1
GRAM_ROWS = [1, 31, 33, 257, 600]
PREDICT_ROWS = [1, 63, 65, 300]


def dev():
    return torch.device('cuda:0')


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@functools.lru_cache(maxsize=None)
def head_case(E, hid, C):
    arrays = cases.head(E, hid, C, seed=E + hid + C)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def gram_case(n, E, hid, C):
    """Feature rows, logits with a few non-finite rows (n >= 4) and the reference weights (the kernel's own inputs), the reference Grams
    and the tolerance per matrix."""
    w1, b1, w2, b2 = head_case(E, hid, C)
    x = cases.features(n, E, seed=n + C)
    out = cases.outputs(x, w1, b1, w2, b2, scale=3.0 if C > 1 else 1.0)
    if n >= 31:
        x, out = cases.with_bad_rows(x, out, seed=n)
    wr = L.weights_reference(out) if C > 1 else L.weights_reference(log_var=out[:, 0])
    w = wr['cls_weights'] if C > 1 else wr['mu_weights'][:, None]
    ref = L.gram_reference(x, w1, b1, w)
    tol = cases.tolerance(cases.gram_fp32(x, w1, b1, w), ref['gram'], (1, 2)) if ref['n_valid'] else np.zeros((w.shape[1], 1, 1))
    return x, out, wr, w, ref, tol


def device_weights(out, C, max_workgroups=0):
    n = out.shape[0]
    K = C * (C + 1) // 2
    w = torch.empty((n, K) if C > 1 else (n,), dtype=torch.float32, device=dev())
    counts = torch.empty(native.LAPLACE_COUNT_WORDS, dtype=torch.int64, device=dev())
    lg = up(out if C > 1 else out[:, 0])
    d = native.LaplaceWeightArgs()
    d.n, d.num_classes, d.max_workgroups = n, C, max_workgroups
    if C > 1:
        d.cls_logits, d.cls_weights = native.ptr(lg), native.ptr(w)
    else:
        d.log_var, d.mu_weights = native.ptr(lg), native.ptr(w)
    d.counts = native.ptr(counts)
    native.call('rovit_laplace_weights', ctypes.byref(d), native.stream_ptr())
    return w.cpu().numpy().reshape(n, -1), counts.cpu().numpy()


def device_gram(x, w1, b1, w, max_workgroups=0):
    n, E = x.shape
    hid, K = w1.shape[0], w.shape[1]
    lib = native.load()
    nbytes = lib.rovit_laplace_workspace_bytes(n, E, hid, K)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    result = torch.empty(native.laplace_words(hid, K), dtype=torch.int64, device=dev())
    tx, tw1, tb1, tw = up(x), up(w1), up(b1), up(w)
    d = native.LaplaceFit()
    d.n, d.embed, d.hid, d.num_weights, d.max_workgroups = n, E, hid, K, max_workgroups
    d.features, d.fc1_weight, d.fc1_bias, d.weights = native.ptr(tx), native.ptr(tw1), native.ptr(tb1), native.ptr(tw)
    d.workspace, d.workspace_bytes, d.result = native.ptr(ws), nbytes, native.ptr(result)
    native.call('rovit_laplace_gram', ctypes.byref(d), native.stream_ptr())
    return result.cpu().numpy()


@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('E,hid', SHAPES)
@pytest.mark.parametrize('n', GRAM_ROWS)
def test_weights_and_gram_against_the_fp64_reference(n, E, hid, C):
    """The weight table within one fp32 unit of the reference's (fp64 exp on either side, rounded once: |d| <= 2^-23 |w| + 2^-149),
    zeros in the bad rows, exact counts; every Gram matrix within four times the fp32 numpy evaluation's error, the header exact, every
    matrix exactly symmetric."""
    x, out, wr, w, ref, tol = gram_case(n, E, hid, C)
    w1, b1, _, _ = head_case(E, hid, C)
    got_w, counts = device_weights(out, C)
    assert counts[native.LAPLACE_BAD_LOGITS] == (wr['bad_logits'] if C > 1 else 0)
    assert counts[native.LAPLACE_BAD_LOG_VAR] == (wr['bad_log_var'] if C == 1 else 0)
    assert (np.abs(got_w.astype(np.float64) - w) <= 2.0 ** -23 * np.abs(w) + 2.0 ** -149).all()
    assert np.array_equal(got_w == 0, w == 0)
    blk = device_gram(x, w1, b1, w)
    g = L.gram_from_block(blk, hid, w.shape[1])
    assert (g['n'], g['n_valid'], g['bad_rows']) == (n, ref['n_valid'], ref['bad_rows'])
    assert (blk[native.LAPLACE_BAD_ROWS + 1:native.LAPLACE_HEADER] == 0).all()
    if n >= 31:
        assert g['bad_rows'] >= 1
    assert np.array_equal(g['gram'], g['gram'].transpose(0, 2, 1))
    err = np.abs(g['gram'] - ref['gram']).max(axis=(1, 2), keepdims=True)
    if ref['n_valid'] == 0:
        assert not g['gram'].any()
        return
    print(f'gram n={n} E={E} hid={hid} C={C}: max error / tolerance = {float((err / tol).max()):.3f} (tolerance {float(tol.min()):.3e} .. {float(tol.max()):.3e})')
    assert (err <= tol).all()


@functools.lru_cache(maxsize=None)
def fitted_case(E, hid, C):
    """A reference fit on 257 clean rows: the fp32 whitening table both sides read."""
    w1, b1, w2, b2 = head_case(E, hid, C)
    x = cases.features(257, E, seed=C)
    out = cases.outputs(x, w1, b1, w2, b2, scale=3.0 if C > 1 else 1.0)
    theta = np.concatenate([w2.ravel(), b2])
    ref = L.laplace_reference(x, out, w1, b1, theta, device_weights=True) if C > 1 else \
        L.laplace_reference(x, None, w1, b1, theta, log_var=out[:, 0], device_weights=True)
    return ref['whitening']


@functools.lru_cache(maxsize=None)
def query_case(E, hid, C):
    """The 300 query rows of a shape (every batch size reads their first B), the reference's outputs and ONE tolerance for the shape:
    four times the largest error of the fp32 numpy evaluation over the 300 rows (a lone row's own fp32 error can be anything down to
    zero, so it bounds nothing)."""
    w1, b1, w2, b2 = head_case(E, hid, C)
    W = fitted_case(E, hid, C)
    x = 1.5 * cases.features(max(PREDICT_ROWS), E, seed=100 + C)    # a little outside the fitted rows
    lg = cases.outputs(x, w1, b1, w2, b2) if C > 1 else None
    ref = L.predict_reference(x, w1, b1, W, C, lg)
    tol = float(cases.tolerance(cases.predict_fp32(x, w1, b1, W, C), ref['logit_cov'], (0, 1, 2)).max())
    return W, x, lg, ref, tol


def device_predict(x, w1, b1, W, C, logits=None, max_workgroups=0):
    B, E = x.shape
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev())
    out = {'logit_cov': f32(B, C, C), 'logit_var': f32(B, C)}
    if logits is not None:
        out['probs'], out['confidence_score'], out['mean_logit_var'] = f32(B, C), f32(B), f32(B)
    keep = [up(x), up(w1), up(b1), up(W), None if logits is None else up(logits)]
    d = native.LaplaceQuery()
    d.batch, d.embed, d.hid, d.num_classes, d.max_workgroups = B, E, w1.shape[0], C, max_workgroups
    d.features, d.fc1_weight, d.fc1_bias, d.whitening, d.cls_logits = (native.ptr(t) for t in keep)
    for k, v in out.items():
        setattr(d, k, native.ptr(v))
    native.call('rovit_laplace_predict', ctypes.byref(d), native.stream_ptr())
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('E,hid', SHAPES)
@pytest.mark.parametrize('B', PREDICT_ROWS)
def test_predict_against_the_fp64_reference(B, E, hid, C):
    """logit_cov (mu_var at C = 1) within four times the fp32 numpy evaluation's error (maximum over the shape's 300 rows), exactly symmetric, the
    diagonal in logit_var; the probit probabilities within the propagated tolerance, their argmax equal wherever the reference's
    top-two margin exceeds it."""
    w1, b1, w2, b2 = head_case(E, hid, C)
    W, xq, lq, full, tol = query_case(E, hid, C)
    x, lg = xq[:B], None if lq is None else lq[:B]
    ref = {k: v[:B] for k, v in full.items()}
    got = device_predict(x, w1, b1, W, C, lg)
    S = got['logit_cov']
    err = float(np.abs(S - ref['logit_cov']).max())
    print(f'predict B={B} E={E} hid={hid} C={C}: max error / tolerance = {err / tol:.3f} (tolerance {tol:.3e}, largest S {float(ref["logit_cov"].max()):.3e})')
    assert err <= tol
    assert np.array_equal(S, S.transpose(0, 2, 1)) and np.array_equal(got['logit_var'], np.einsum('bcc->bc', S))
    if C > 1:
        # d p / d S_cc is bounded by |l_c| (pi / 16) p (1 - p) <= |l| pi / 64, summed over the classes; then one fp32 rounding
        ptol = np.abs(lg).max() * np.pi / 64.0 * C * tol + 2.0 ** -24
        assert np.abs(got['probs'] - ref['probs']).max() <= ptol
        top = np.sort(ref['probs'], axis=1)
        clear = top[:, -1] - top[:, -2] > 2.0 * ptol
        assert np.array_equal(got['probs'].argmax(axis=1)[clear], ref['probs'].argmax(axis=1)[clear]) and clear.any()
        assert np.abs(got['confidence_score'] - ref['confidence_score']).max() <= ptol
        assert np.abs(got['mean_logit_var'] - ref['mean_logit_var']).max() <= tol + 2.0 ** -24 * ref['mean_logit_var'].max()


def _record(model_like, x, lg, lv, edges, max_workgroups):
    la = L.HeadLaplace(model_like, capacity=64)
    la.max_workgroups = max_workgroups
    for r0, r1 in zip(edges[:-1], edges[1:]):
        la.update(up(x[r0:r1]), up(lg[r0:r1]), up(lv[r0:r1]))
    return la


def test_bit_identity_across_runs_splits_and_grids():
    """The block ``fit`` copies and every output of ``predict``: identical across two runs, three splits of the rows into ``update``
    calls, and max_workgroups in {1, 3, default}."""
    E, hid, C, n = 192, 128, 4, 600
    w1, b1, w2, b2 = head_case(E, hid, C)
    u1, c1, u2, c2 = head_case(E, hid, 1)

    def lin(i, o, w, b):
        m = torch.nn.Linear(i, o)
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(w.reshape(o, i)))
            m.bias.copy_(torch.from_numpy(b))
        return m.to(dev())
    heads = (SimpleNamespace(fc1=lin(E, hid, w1, b1), fc2=lin(hid, C, w2, b2)), SimpleNamespace(fc1=lin(E, hid, u1, c1), fc_mu=lin(hid, 1, u2, c2)))
    x = cases.features(n, E, seed=1)
    lg = cases.outputs(x, w1, b1, w2, b2)
    lv = cases.outputs(x, u1, c1, u2, c2, scale=1.0)
    x, lg = cases.with_bad_rows(x, lg, seed=2)
    first = _record(heads, x, lg, lv, [0, n], 0)
    blk = first.result_block()
    for edges, cap in (([0, n], 0), (cases.splits_of(n, 3, 1), 0), (cases.splits_of(n, 7, 2), 0), ([0, 1, n], 0), ([0, n], 1), ([0, n], 3),
                       (cases.splits_of(n, 5, 3), 3)):
        assert np.array_equal(_record(heads, x, lg, lv, edges, cap).result_block(), blk), (edges, cap)
    first.fit()
    assert first.bad_logits == 2 and first.bad_rows == 3 and first.n_valid == n - 3 and first.bad_rows_mu == 3
    xq = cases.features(300, E, seed=3)
    q, ql, qv = up(xq), up(cases.outputs(xq, w1, b1, w2, b2)), up(cases.outputs(xq, u1, c1, u2, c2, scale=1.0))
    base = first.predict(q, ql, log_var=qv)
    for cap in (0, 1, 3):
        first.max_workgroups = cap
        again = first.predict(q, ql, log_var=qv)
        assert set(again) == set(base) and all(torch.equal(base[k], again[k]) for k in base), cap


CLASS_NAMES = ['Healthy Leaf', 'Leaf Holes', 'Black Spot', 'Dry Leaf']


def test_model_and_evaluator_end_to_end(tmp_path):
    """Batch 8 on the oracle-initialised RoViTKAN: fit_laplace / predict_laplace against the reference run on the model's own features
    and logits, within the bounds above; Evaluator.evaluate(laplace=...) produces the card; the default evaluate() keeps its keys."""
    from evaluation.evaluator import Evaluator
    from models.rovit_kan import RoViTKAN
    model = RoViTKAN(pretrained=False)
    model.load_state_dict(ref_cpu.init_rovit_state(seed=0))
    model = model.to(dev()).eval()
    g = torch.Generator().manual_seed(0)
    images = torch.nn.functional.interpolate(torch.randn(8, 3, 7, 7, generator=g), size=224, mode='bilinear', align_corners=False)
    labels = torch.arange(8) % 4
    la = model.fit_laplace(images.to(dev()))
    with torch.no_grad():
        out = model(images.to(dev()))
    f, lg, lv = out['features'].cpu().numpy(), out['cls_logits'].cpu().numpy(), out['log_var'].cpu().numpy().reshape(-1)
    assert la.n == 8 and la.n_valid == 8 and la.has_gaussian and la.status in L.STATUS and la.status_mu in L.STATUS
    c, u = model.classification_head, model.uncertainty_head
    P = lambda t: t.detach().cpu().numpy()
    lay = la._layout()
    blk = la.result_block()
    for params, last, hid, C, off, end, kw in ((c, c.fc2, la.hid, 4, lay['cls'], lay['mu'], {}), (u, u.fc_mu, la.hid_mu, 1, lay['mu'], lay['words'], {'log_var': lv})):
        w1, b1 = P(params.fc1.weight), P(params.fc1.bias)
        ref = L.laplace_reference(f, lg, w1, b1, np.concatenate([P(last.weight).ravel(), P(last.bias)]), device_weights=True, **kw)
        got = L.gram_from_block(blk[off:end], hid, C * (C + 1) // 2)
        tol = cases.tolerance(cases.gram_fp32(f, w1, b1, ref['weights']), ref['gram'], (1, 2))
        # the device's weights may differ from the reference's by one fp32 unit: 2^-23 of sum_i |w| |a_a a_b| at most
        a = L.augmented_hidden(f, w1, b1)
        slack = 2.0 ** -23 * np.einsum('ik,ia,ib->kab', np.abs(ref['weights']).astype(np.float64), np.abs(a), np.abs(a)).max(axis=(1, 2), keepdims=True)
        assert (np.abs(got['gram'] - ref['gram']).max(axis=(1, 2), keepdims=True) <= tol + slack).all()
        tau = la.prior_precision if C > 1 else la.prior_precision_mu
        assert tau == pytest.approx(ref['prior_precision'], rel=1e-3) and (la.status if C > 1 else la.status_mu) == ref['status']
    pred = model.predict_laplace(images.to(dev()), la)
    assert set(pred) == {'logit_cov', 'logit_var', 'probs', 'confidence_score', 'mean_logit_var', 'mu_var', 'total_std', 'class'}
    t = la.tables
    want = L.predict_reference(f, P(t['fc1_weight']), P(t['fc1_bias']), P(t['whitening']), 4, lg)
    tol = float(cases.tolerance(cases.predict_fp32(f, P(t['fc1_weight']), P(t['fc1_bias']), P(t['whitening']), 4), want['logit_cov'], (0, 1, 2)).max())
    assert np.abs(P(pred['logit_cov']) - want['logit_cov']).max() <= tol
    want_mu = L.predict_reference(f, P(t['fc1_weight_mu']), P(t['fc1_bias_mu']), P(t['whitening_mu']), 1)
    tol_mu = float(cases.tolerance(cases.predict_fp32(f, P(t['fc1_weight_mu']), P(t['fc1_bias_mu']), P(t['whitening_mu']), 1), want_mu['logit_cov'], (0, 1, 2)).max())
    assert np.abs(P(pred['mu_var']) - want_mu['logit_var'][:, 0]).max() <= tol_mu
    assert torch.allclose(pred['total_std'], torch.sqrt(torch.exp(out['log_var'].reshape(-1)) + pred['mu_var']))
    # a head parameter changes: the tables are stale
    with torch.no_grad():
        c.fc2.bias.add_(0.0)
    with pytest.raises(L.RovitHipError, match='has changed since fit'):
        model.predict_laplace(images.to(dev()), la)
    loader = [(images[i:i + 4], labels[i:i + 4], labels[i:i + 4]) for i in range(0, 8, 4)]
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=CLASS_NAMES, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    plain = Evaluator(model, loader, cfg, dev()).evaluate(selective=True)
    assert set(plain) == {'accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece', 'fps', 'params',
                          'params_m', 'per_class', 'selective'}
    assert list(plain['selective']['scores']) == ['confidence', 'entropy', 'sigma']
    assert 'Laplace' not in (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    ev = Evaluator(model, loader, cfg, dev())
    assert ev.fit_laplace(loader) is ev.laplace and ev.laplace.n == 8
    with_la = ev.evaluate(selective=True, laplace=ev.laplace)
    assert set(with_la) == set(plain) | {'laplace'}
    assert list(with_la['selective']['scores']) == ['confidence', 'entropy', 'sigma', 'laplace_logit_var', 'laplace_mu_std']
    card = with_la['laplace']
    assert card['n'] == 8 and card['before']['ece'] == with_la['ece'] and set(card['after']) == {'nll', 'ece', 'brier_score', 'accuracy'}
    assert 'Laplace approximation (n = 8' in (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    cards = ev.evaluate_ood([torch.randn(4, 3, 224, 224, generator=g) for _ in range(2)], laplace=ev.laplace)
    assert list(cards) == ['max_prob', 'entropy', 'energy', 'sigma', 'laplace'] and cards['laplace']['n_in'] == 8
