"""CPU tests of rovit_hip.laplace: the fp64 reference statements against brute-force autograd Jacobians, the marginal-likelihood rule for
the prior precision, the predictive's limits, the state dict and every refusal, and the Evaluator's defaults and new card on CPU tensors."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import laplace_cases as cases  # noqa: E402

from rovit_hip import laplace as L  # noqa: E402
from rovit_hip import native  # noqa: E402
from rovit_hip.native import RovitHipError  # noqa: E402

E, HID, N = 32, 32, 64


class Head(torch.nn.Module):
    """fc1 -> ReLU -> last layer(s) with the attribute names of models/heads.py, in plain torch (the product heads have no CPU path)."""

    def __init__(self, E, hid, outs, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.fc1 = torch.nn.Linear(E, hid)
        for name, o in outs.items():
            setattr(self, name, torch.nn.Linear(hid, o))

    def hidden(self, f):
        return torch.relu(self.fc1(f))


class Tiny(torch.nn.Module):
    def __init__(self, C=4, seed=3):
        super().__init__()
        self.classification_head = Head(E, HID, {'fc2': C}, seed)
        self.uncertainty_head = Head(E, HID, {'fc_mu': 1, 'fc_logvar': 1}, seed + 1)
        torch.manual_seed(seed + 2)
        self.sev = torch.nn.Linear(E, 1)

    def forward(self, x):
        f = x.flatten(1)[:, :E].contiguous()
        c, u = self.classification_head, self.uncertainty_head
        return {'cls_logits': c.fc2(c.hidden(f)), 'features': f, 'kan_severity': self.sev(f), 'mu': u.fc_mu(u.hidden(f)),
                'log_var': u.fc_logvar(u.hidden(f))}


def brute_force(a, theta_shape, lam_of_row, tau):
    """H = sum_i J_i^T Lambda_i J_i and S_i = J_i (H + tau I)^-1 J_i^T with J_i the autograd Jacobian of the last layer's outputs with
    respect to theta = [weight, bias] in the class-major order, everything in fp64."""
    C, D = theta_shape
    theta = torch.zeros(C * D, dtype=torch.float64)
    Js = [torch.autograd.functional.jacobian(lambda t, ai=ai: t.view(C, D) @ ai, theta) for ai in torch.from_numpy(a)]
    H = sum(J.T @ lam_of_row(i) @ J for i, J in enumerate(Js))
    Pinv = torch.linalg.inv(H + tau * torch.eye(C * D, dtype=torch.float64))
    return H.numpy(), np.stack([(J @ Pinv @ J.T).numpy() for J in Js])


@pytest.mark.parametrize('C', [2, 3, 4])
def test_classification_bookkeeping_against_autograd_jacobians(C):
    """H and every row's S of the reference agree with the brute force to 1e-9 relative (of the matrix's largest entry)."""
    w1, b1, w2, b2 = cases.head(E, HID, C, seed=C)
    x = cases.features(N, E, seed=10 + C)
    lg = cases.outputs(x, w1, b1, w2, b2)
    ref = L.laplace_reference(x, lg, w1, b1, np.concatenate([w2.ravel(), b2]), prior_precision=0.7)
    a = L.augmented_hidden(x, w1, b1)
    p = torch.softmax(torch.from_numpy(lg).double(), dim=1)
    H, S = brute_force(a, (C, HID + 1), lambda i: torch.diag(p[i]) - torch.outer(p[i], p[i]), 0.7)
    assert np.abs(ref['hessian'] - H).max() <= 1e-9 * np.abs(H).max()
    got = L.predict_reference(x, w1, b1, ref['whitening64'], C)['logit_cov']
    assert np.abs(got - S).max() <= 1e-9 * np.abs(S).max()


def test_gaussian_bookkeeping_against_autograd_jacobians():
    w1, b1, w2, b2 = cases.head(E, HID, 1, seed=7)
    x = cases.features(N, E, seed=17)
    lv = cases.outputs(x, w1, b1, w2, b2, scale=1.0)[:, 0]
    ref = L.laplace_reference(x, None, w1, b1, np.concatenate([w2.ravel(), b2]), prior_precision=2.5, log_var=lv)
    a = L.augmented_hidden(x, w1, b1)
    prec = torch.exp(-torch.from_numpy(lv).double())
    H, S = brute_force(a, (1, HID + 1), lambda i: prec[i].reshape(1, 1), 2.5)
    assert np.abs(ref['hessian'] - H).max() <= 1e-9 * np.abs(H).max()
    got = L.predict_reference(x, w1, b1, ref['whitening64'], 1)['logit_var'][:, 0]
    assert np.abs(got - S[:, 0, 0]).max() <= 1e-9 * np.abs(S).max()


def test_marginal_likelihood_root_argmax_and_the_two_ends():
    g = np.random.default_rng(0)
    eig = np.concatenate([np.exp(g.uniform(-6, 6, size=100)), np.zeros(29)])
    theta_sq = 3.7
    tau, status = L.marglik_prior_precision(eig, theta_sq)
    assert status == 'interior' and L.TAU_MIN < tau < L.TAU_MAX
    assert abs(L.stationarity(tau, eig, theta_sq)) <= 1e-8 * theta_sq
    grid = np.exp(np.linspace(math.log(L.TAU_MIN), math.log(L.TAU_MAX), 20001))
    best = grid[int(np.argmax([L.evidence(t, eig, theta_sq) for t in grid]))]
    step = grid[1] / grid[0]
    assert best / step <= tau <= best * step
    assert L.evidence(tau, eig, theta_sq) >= max(L.evidence(t, eig, theta_sq) for t in grid) - 1e-12
    assert L.marglik_prior_precision(np.zeros(129), theta_sq) == (L.TAU_MIN, 'at_min')          # H = 0: the evidence falls with tau
    assert L.marglik_prior_precision(eig, 1e-12) == (L.TAU_MAX, 'at_max')                      # |theta| tiny: it rises with tau
    # through the fit: the same rule, the status on the result
    w1, b1, w2, b2 = cases.head(E, HID, 3, seed=1)
    x = cases.features(N, E, seed=2)
    lg = cases.outputs(x, w1, b1, w2, b2)
    ref = L.laplace_reference(x, lg, w1, b1, np.concatenate([w2.ravel(), b2]))
    assert ref['status'] == 'interior' and abs(L.stationarity(ref['prior_precision'], ref['eigenvalues'], ref['theta_sq'])) <= 1e-8 * ref['theta_sq']
    assert L.laplace_reference(x, lg, w1, b1, 1e-7 * w2.ravel())['status'] == 'at_max'
    assert L.fit_from_gram(np.zeros((3, HID + 1, HID + 1)), 2, w2[:2].ravel())['status'] == 'at_min'


def test_predictive_limits():
    C = 3
    w1, b1, w2, b2 = cases.head(E, HID, C, seed=4)
    x = cases.features(N, E, seed=5)
    lg = cases.outputs(x, w1, b1, w2, b2)
    theta = np.concatenate([w2.ravel(), b2])
    P = HID + 32
    zero = L.predict_reference(x, w1, b1, np.zeros((C * P, C * P), dtype=np.float32), C, lg)
    soft = torch.softmax(torch.from_numpy(lg).double(), dim=1).numpy()
    assert np.array_equal(zero['logit_cov'], np.zeros((N, C, C))) and np.abs(zero['probs'] - soft).max() <= 4e-16
    ref = L.laplace_reference(x, lg, w1, b1, theta, prior_precision=1.0)
    out = L.predict_reference(x, w1, b1, ref['whitening'], C, lg)
    S = out['logit_cov']
    assert np.array_equal(S, S.transpose(0, 2, 1)) and np.linalg.eigvalsh(S).min() >= -1e-12 * np.abs(S).max()
    assert np.allclose(out['probs'].sum(axis=1), 1.0, atol=1e-12) and (out['probs'].max(axis=1) <= soft.max(axis=1) + 1e-12).all()
    assert np.allclose(out['confidence_score'], 1.0 - out['probs'].max(axis=1), atol=1e-12)
    var = [L.predict_reference(x, w1, b1, L.laplace_reference(x, lg, w1, b1, theta, prior_precision=t)['whitening'], C)['logit_var'].max()
           for t in (1.0, 1e2, 1e4, 1e6)]
    assert var[0] > var[1] > var[2] > var[3] and var[3] < 1e-3                       # S <= |a|^2 / tau -> 0
    far = L.predict_reference(50.0 * x[:1], w1, b1, ref['whitening'], C, 50.0 * lg[:1])
    assert far['mean_logit_var'][0] > out['mean_logit_var'].max()


def recorded(model, batches):
    la = L.HeadLaplace(model)
    with torch.no_grad():
        for x in batches:
            o = model(x)
            la.update(o['features'], o['cls_logits'], o['log_var'])
    return la


def test_head_laplace_on_cpu_tensors_state_dict_and_stale_tables():
    model = Tiny()
    torch.manual_seed(0)
    xs = [torch.randn(b, 3, 4, 4) for b in (16, 16, 9)]
    la = recorded(model, xs).fit()
    assert la.n == 41 and la.n_valid == 41 and la.bad_rows == 0 and la.status in L.STATUS and la.status_mu in L.STATUS
    assert L.TAU_MIN <= la.prior_precision <= L.TAU_MAX and math.isfinite(la.log_marginal_likelihood) and la.has_gaussian
    # the same block whichever way the rows arrived
    assert np.array_equal(recorded(model, [torch.cat(xs)]).result_block(), la.result_block())
    with torch.no_grad():
        o = model(xs[2])
    out = la.predict(o['features'], o['cls_logits'], o['mu'], o['log_var'])
    assert set(out) == {'logit_cov', 'logit_var', 'probs', 'confidence_score', 'mean_logit_var', 'mu_var', 'total_std'}
    assert tuple(out['logit_cov'].shape) == (9, 4, 4) and tuple(out['mu_var'].shape) == (9,) and (out['mu_var'] > 0).all()
    assert torch.allclose(out['total_std'], torch.sqrt(torch.exp(o['log_var'].reshape(-1)) + out['mu_var']))
    # against the reference fit of the classification head, rounded weights as the device has them
    c = model.classification_head
    ref = L.laplace_reference(torch.cat([model(x)['features'] for x in xs]).detach(), torch.cat([model(x)['cls_logits'] for x in xs]).detach(),
                              c.fc1.weight, c.fc1.bias, torch.cat([c.fc2.weight.reshape(-1), c.fc2.bias]).detach().numpy(), device_weights=True)
    assert ref['prior_precision'] == pytest.approx(la.prior_precision, rel=1e-9) and ref['status'] == la.status
    assert np.array_equal(ref['whitening'], la.tables['whitening'].numpy())
    # a given prior precision; stage < 3: no Gaussian part
    fixed = recorded(model, xs).fit(prior_precision=3.0)
    assert fixed.prior_precision == 3.0 and fixed.prior_precision_mu == 3.0
    plain = L.HeadLaplace(model)
    plain.update(o['features'], o['cls_logits'])
    assert not plain.fit().has_gaussian and 'mu_var' not in plain.predict(o['features'], o['cls_logits'])
    # state dict round trip
    sd = la.state_dict()
    back = L.HeadLaplace(model).load_state_dict(sd)
    again = back.predict(o['features'], o['cls_logits'], o['mu'], o['log_var'])
    assert all(torch.equal(out[k], again[k]) for k in out) and back.prior_precision == la.prior_precision and back.status_mu == la.status_mu
    with pytest.raises(RovitHipError, match='differs from the one the fit was made with'):
        L.HeadLaplace(Tiny(seed=9)).load_state_dict(sd)
    # stale tables are refused
    with torch.no_grad():
        model.classification_head.fc2.bias.add_(1.0)
    with pytest.raises(RovitHipError, match='has changed since fit'):
        la.predict(o['features'], o['cls_logits'])
    with torch.no_grad():
        model.uncertainty_head.fc1.weight.mul_(1.0)
    with pytest.raises(RovitHipError, match='has changed since fit'):
        back.predict(o['features'], o['cls_logits'])


def test_every_refusal():
    model = Tiny()
    la = L.HeadLaplace(model)
    f, lg, lv = torch.randn(5, E), torch.randn(5, 4), torch.randn(5, 1)
    for bad in ((torch.randn(5, E + 1), lg, lv), (f, torch.randn(5, 3), lv), (f, lg, torch.randn(4)), (torch.randn(0, E), torch.randn(0, 4), None),
                (f.reshape(5, E, 1), lg, lv)):
        with pytest.raises(RovitHipError, match='HeadLaplace.update'):
            la.update(*bad)
    with pytest.raises(RovitHipError, match='nothing recorded'):
        la.fit()
    with pytest.raises(RovitHipError, match='fit\\(\\) first'):
        la.state_dict()
    la.update(f, lg, lv)
    with pytest.raises(RovitHipError, match='every batch carries log_var or none'):
        la.update(f, lg)
    with pytest.raises(RovitHipError, match='fit\\(\\) \\(or load_state_dict\\) first'):
        la.predict(f, lg)
    for pp in (0.0, -1.0, float('nan'), 'auto'):
        with pytest.raises(RovitHipError, match='prior_precision'):
            la.fit(prior_precision=pp)
    la.fit()
    for bad in ((torch.randn(5, E + 1), lg), (f, torch.randn(5, 3)), (f, None), (f, lg, torch.randn(4)), (f, lg, None, torch.randn(6))):
        with pytest.raises(RovitHipError, match='HeadLaplace.predict'):
            la.predict(*bad)
    nan_rows = f.clone()
    nan_rows[:] = float('nan')
    la2 = L.HeadLaplace(model)
    la2.update(nan_rows, lg, lv)
    with pytest.raises(RovitHipError, match='no valid row among 5'):
        la2.fit()
    with pytest.raises(RovitHipError, match='capacity'):
        L.HeadLaplace(model, capacity=0)
    with pytest.raises(RovitHipError, match='hidden width'):
        L.HeadLaplace((Head(E, 48, {'fc2': 4}, 0), None))
    with pytest.raises(RovitHipError, match='num_classes'):
        L.HeadLaplace((Head(E, HID, {'fc2': 9}, 0), None))
    with pytest.raises(RovitHipError, match='needs a Linear fc1'):
        L.HeadLaplace(torch.nn.Linear(4, 4))
    with pytest.raises(RovitHipError, match='log_var without an uncertainty head'):
        L.HeadLaplace((Head(E, HID, {'fc2': 4}, 0), None)).update(f, lg, lv)


def test_bad_rows_are_left_out_and_counted():
    w1, b1, w2, b2 = cases.head(E, HID, 3, seed=1)
    x = cases.features(N, E, seed=2)
    lg = cases.outputs(x, w1, b1, w2, b2)
    xb, lb = cases.with_bad_rows(x, lg, seed=3)
    wr = L.weights_reference(lb, lb[:, 0])
    assert wr['bad_logits'] == 2 and wr['bad_log_var'] == int((~np.isfinite(lb[:, 0])).sum())
    assert (wr['cls_weights'][~np.isfinite(lb).all(axis=1)] == 0).all() and np.isfinite(wr['cls_weights']).all()
    g = L.gram_reference(xb, w1, b1, wr['cls_weights'])
    keep = np.isfinite(xb).all(axis=1)
    assert g['bad_rows'] == 3 and g['n_valid'] == N - 3
    clean = L.gram_reference(xb[keep], w1, b1, wr['cls_weights'][keep])
    assert np.allclose(g['gram'], clean['gram'], rtol=0, atol=1e-12 * np.abs(clean['gram']).max())
    # the weights: K columns in the order of pair_index, every row's Lambda rows summing to zero
    K = wr['cls_weights'].shape[1]
    assert K == 6 and L.pair_index(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    w64 = L.weights_reference(lg, dtype=np.float64)['cls_weights']
    assert np.abs(w64[:, 0] + w64[:, 1] + w64[:, 2]).max() < 1e-15


def test_binding_matches_the_header():
    import ctypes
    lib = native.load()
    assert lib.rovit_laplace_workspace_bytes(0, 192, 128, 10) == 0 and lib.rovit_laplace_workspace_bytes(10, 48, 128, 10) == 0
    assert lib.rovit_laplace_workspace_bytes(10, 192, 100, 10) == 0 and lib.rovit_laplace_workspace_bytes(10, 192, 128, 37) == 0
    assert lib.rovit_laplace_workspace_bytes(10, 192, 288, 1) == 0 and lib.rovit_laplace_workspace_bytes((1 << 22) + 1, 192, 128, 1) == 0
    small, large = lib.rovit_laplace_workspace_bytes(256, 192, 128, 10), lib.rovit_laplace_workspace_bytes(257, 192, 128, 10)
    assert large - small >= 10 * 15 * 1024 * 4                     # one more chunk: K x 15 tiles of partials
    assert native.laplace_words(128, 10) == 8 + 10 * 129 * 129
    for d, name in ((native.LaplaceWeightArgs(), 'rovit_laplace_weights'), (native.LaplaceFit(), 'rovit_laplace_gram'),
                    (native.LaplaceQuery(), 'rovit_laplace_predict')):
        assert getattr(lib, name)(ctypes.byref(d), None) != 0       # a bad descriptor is refused before any launch
        assert getattr(lib, name)(None, None) != 0


def test_cpu_evaluator_defaults_are_unchanged_and_laplace_adds_its_card(tmp_path, capsys):
    from evaluation.evaluator import Evaluator
    torch.manual_seed(5)
    data = [(torch.randn(b, 3, 224, 224), torch.randint(0, 4, (b,)), torch.randint(0, 4, (b,))) for b in (16, 16, 9)]
    names = ['Healthy Leaf', 'Leaf Holes', 'Black Spot', 'Dry Leaf']
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=names, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    fps_free = lambda t: [line for line in t.splitlines() if not line.startswith('FPS:')]
    ev = Evaluator(Tiny(), data, cfg, torch.device('cpu'))
    assert ev.laplace is None
    m = ev.evaluate()
    assert set(m) == {'accuracy', 'macro_f1', 'weighted_f1', 'mae', 'spearman_rho', 'spearman', 'brier_score', 'ece', 'fps', 'params',
                      'params_m', 'per_class'}
    text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    assert 'Laplace' not in text and 'Laplace' not in capsys.readouterr().out
    plain_sel = Evaluator(Tiny(), data, cfg, torch.device('cpu')).evaluate(selective=True)
    assert list(plain_sel['selective']['scores']) == ['confidence', 'entropy', 'sigma']
    model = Tiny()
    la = recorded(model, [b[0] for b in data]).fit()
    ev = Evaluator(model, data, cfg, torch.device('cpu'))
    with_la = ev.evaluate(laplace=la)
    assert set(with_la) == set(m) | {'laplace'}
    assert all(with_la[k] == m[k] for k in ('accuracy', 'macro_f1', 'mae', 'brier_score', 'ece', 'per_class'))
    card = with_la['laplace']
    assert set(card) == {'prior_precision', 'status', 'prior_precision_mu', 'status_mu', 'n', 'before', 'after'}
    assert card['prior_precision'] == la.prior_precision and card['status_mu'] == la.status_mu and card['n'] == 41
    assert all(set(card[s]) == {'nll', 'ece', 'brier_score', 'accuracy'} and all(math.isfinite(v) for v in card[s].values()) for s in ('before', 'after'))
    assert card['before']['ece'] == m['ece'] and card['before']['brier_score'] == m['brier_score'] and card['before']['accuracy'] == m['accuracy']
    new_text = (tmp_path / 'evaluation_results.txt').read_text(encoding='utf-8')
    at = new_text.index('Laplace approximation (n = 41')
    assert fps_free(new_text[:at]) == fps_free(text) and 'before' in new_text[at:] and 'after' in new_text[at:]
    assert 'Laplace approximation' in capsys.readouterr().out
    s = Evaluator(model, data, cfg, torch.device('cpu')).evaluate(selective=True, laplace=la)
    assert list(s['selective']['scores']) == ['confidence', 'entropy', 'sigma', 'laplace_logit_var', 'laplace_mu_std']
    ood = [torch.randn(b, 3, 224, 224) * 4.0 for b in (16, 5)]
    cards = Evaluator(model, data, cfg, torch.device('cpu')).evaluate_ood(ood, laplace=la)
    assert list(cards) == ['max_prob', 'entropy', 'energy', 'sigma', 'laplace']
    assert cards['laplace']['n_in'] == 41 and cards['laplace']['n_out'] == 21 and cards['laplace']['auroc'] > 0.9      # four times the spread
    assert list(Evaluator(model, data, cfg, torch.device('cpu')).evaluate_ood(ood)) == ['max_prob', 'entropy', 'energy', 'sigma']
