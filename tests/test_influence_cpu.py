"""CPU tests of the training-data influence (rovit_hip/influence.py): the numpy fp64 statements against a brute force with autograd
gradients and an explicit inverse, the leave-one-out identity that pins sign and scale, the relative self-match, the label audit on
planted label noise, the tie rule, the refusals, the model / Evaluator wrappers on CPU tensors and the C entry points' refusals."""
import ctypes
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import influence_cases as ic  # noqa: E402
import laplace_cases as cases  # noqa: E402

from rovit_hip import influence as I  # noqa: E402
from rovit_hip import laplace as L  # noqa: E402
from rovit_hip import native  # noqa: E402
from rovit_hip.native import RovitHipError  # noqa: E402

CPU = torch.device('cpu')
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize('C', [1, 2, 4])
@pytest.mark.parametrize('target', ['loss', 'output'])
def test_scores_against_the_brute_force(C, target):
    """u_t . u_j from ``embed_reference`` (fp64 residual, fp64 table) equals g_t^T (H + tau I)^-1 g_j with autograd gradients of the
    cross-entropy / the Gaussian NLL and an explicit inverse, to 1e-9 relative; ``search_reference`` returns those scores in order."""
    E = hid = 32
    n, B, tau = 40, 6, 0.7
    head = 'cls' if C > 1 else 'mu'
    target = {'loss': 'loss', 'output': 'logit' if C > 1 else 'mu'}[target]
    w1, b1, w2, b2 = cases.head(E, hid, C, seed=3 + C)
    x, xq = cases.features(n, E, seed=1), cases.features(B, E, seed=2)
    out, outq = (cases.outputs(z, w1, b1, w2, b2, scale=2.0 if C > 1 else 1.0).astype(np.float64) for z in (x, xq))
    g = np.random.default_rng(C)
    if C > 1:
        y, yq = g.integers(0, C, size=n), g.integers(0, C, size=B)
        fit = L.laplace_reference(x, out.astype(np.float32), w1, b1, np.concatenate([w2.ravel(), b2]), tau)
        kw = {'cls_logits': out, 'labels': y}
        kwq = {'cls_logits': outq, 'labels': yq}
        brute = {'out_train': out, 'out_query': outq, 'labels_train': y, 'labels_query': yq}
    else:
        lv, lvq = 0.3 * g.standard_normal(n), 0.3 * g.standard_normal(B)
        sev, sevq = g.integers(0, 4, size=n).astype(np.float64), g.integers(0, 4, size=B).astype(np.float64)
        fit = L.laplace_reference(x, None, w1, b1, np.concatenate([w2.ravel(), b2]), tau, log_var=lv.astype(np.float32))
        # the fit's weights are exp(-log_var) of the fp32 log_var: give the gradients the same values
        lv = lv.astype(np.float32).astype(np.float64)
        kw = {'mu': out[:, 0], 'log_var': lv, 'severity': sev}
        kwq = {'mu': outq[:, 0], 'log_var': lvq, 'severity': sevq} if target == 'loss' else {}
        brute = {'out_train': out[:, 0], 'out_query': outq[:, 0], 'log_var_train': lv, 'log_var_query': lvq, 'severity_train': sev, 'severity_query': sevq}
    W = fit['whitening64']
    rt = I.embed_reference(x, w1, b1, W, C, head, 'loss', dtype=np.float64, **kw)
    rq = I.embed_reference(xq, w1, b1, W, C, head, target, dtype=np.float64, **kwq)
    assert rt['valid'].all() and rq['valid'].all()
    theta = np.concatenate([w2.astype(np.float64), b2.astype(np.float64)[:, None]], axis=1)
    want = I.influence_reference(L.augmented_hidden(xq, w1, b1), L.augmented_hidden(x, w1, b1), theta, fit['hessian'], tau, head, target, **brute)
    got = rq['rows'] @ rt['rows'].T
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-9 * scale
    assert np.abs((rt['rows'] ** 2).sum(axis=1) - rt['norm2']).max() == 0.0
    s = I.search_reference(rq['rows'], rt['rows'], rt['norm2'], rt['valid'], k=5)
    order = np.argsort(-want, axis=1, kind='stable')[:, :5]
    assert np.abs(s['pro_scores'] - np.take_along_axis(want, order, axis=1)).max() <= 1e-9 * scale
    assert np.abs(s['opp_scores'] - np.sort(want, axis=1)[:, :5]).max() <= 1e-9 * scale
    assert (s['pro_scores'][:, 0] > 0).all() and (s['opp_scores'][:, 0] < 0).all()
    # padding entries are exactly zero
    P, D = hid + 32, hid + 1
    assert not rt['rows'].reshape(n, C, P)[:, :, D:].any()


def test_leave_one_out_identity_pins_sign_and_scale():
    """A ridge problem whose fc_mu parameters are the exact minimiser (log_var = 0, tau given): s(t, j) / (1 - h_j) equals the refitted
    change of mu_t when row j is removed, to 1e-9."""
    E = hid = 32
    n, B, tau = 50, 5, 0.5
    w1, b1, _, _ = cases.head(E, hid, 1, seed=4)
    x, xq = cases.features(n, E, seed=5), cases.features(B, E, seed=6)
    a, aq = L.augmented_hidden(x, w1, b1), L.augmented_hidden(xq, w1, b1)
    y = np.random.default_rng(0).standard_normal(n)
    Pm = a.T @ a + tau * np.eye(a.shape[1])
    theta = np.linalg.solve(Pm, a.T @ y)
    mu = a @ theta
    W = L.pad_whitening(L.whitening_of(a.T @ a, tau), 1, hid)
    zeros = np.zeros(n)
    rt = I.embed_reference(x, w1, b1, W, 1, 'mu', 'loss', mu=mu, log_var=zeros, severity=y, dtype=np.float64)
    rq = I.embed_reference(xq, w1, b1, W, 1, 'mu', 'mu', dtype=np.float64)
    s = rq['rows'] @ rt['rows'].T
    h = np.einsum('ia,ab,ib->i', a, np.linalg.inv(Pm), a)
    worst = 0.0
    for j in range(n):
        keep = np.arange(n) != j
        refit = np.linalg.solve(a[keep].T @ a[keep] + tau * np.eye(a.shape[1]), a[keep].T @ y[keep])
        change = aq @ (refit - theta)
        worst = max(worst, float(np.abs(s[:, j] / (1.0 - h[j]) - change).max() / np.abs(aq @ theta).max()))
    assert worst <= 1e-9
    # the sign in words: a row whose removal raises mu_t has s > 0
    j = int(np.argmax(np.abs(s[0])))
    keep = np.arange(n) != j
    refit = np.linalg.solve(a[keep].T @ a[keep] + tau * np.eye(a.shape[1]), a[keep].T @ y[keep])
    assert np.sign(aq[0] @ (refit - theta)) == np.sign(s[0, j])


def _cpu_index(E=32, hid=32, C=4, n=120, gaussian=True, seed=1, bad=True):
    la = ic.fitted_laplace(E, hid, C, CPU, gaussian)
    x, c = ic.recorded(n, E, hid, C, seed=seed, bad=bad)
    _, m = ic.recorded(n, E, hid, 1, seed=seed + 1, bad=bad)
    inf = I.HeadInfluence(la, capacity=16)
    for r0, r1 in zip([0, 7, 64], [7, 64, n]):
        inf.update(T(x[r0:r1]), T(c['cls_logits'][r0:r1]), T(c['labels'][r0:r1]),
                   *((T(m[k][r0:r1]) for k in ('mu', 'log_var', 'severity')) if gaussian else ()))
    return inf, x, c, m


def test_relative_self_match_and_exclude():
    """With relative=True, target 'loss' and its own label every valid training row's first proponent is itself (Cauchy-Schwarz); with
    exclude = arange(n) it never appears.  Invalid rows are never returned and, as queries, return -1 / NaN."""
    inf, x, c, m = _cpu_index()
    n = inf.n
    for head, kw in (('cls', {}), ('mu', {k: T(m[k]) for k in ('mu', 'log_var', 'severity')})):
        valid = inf._head_store(head)[3].numpy() != 0
        assert 0 < valid.sum() < n
        out = inf.search(T(x), T(c['cls_logits']), T(c['labels']), head=head, k=4, relative=True, **kw)
        first = out['pro_indices'][:, 0].numpy()
        assert np.array_equal(first[valid], np.arange(n)[valid]) and (first[~valid] == -1).all()
        assert np.isnan(out['pro_scores'].numpy()[~valid]).all() and np.isnan(out['query_self_influence'].numpy()[~valid]).all()
        si = inf.self_influence(head).numpy()
        assert np.allclose(out['pro_scores'][:, 0].numpy()[valid] ** 2, si[valid], rtol=1e-5) and np.isnan(si[~valid]).all()
        ex = inf.search(T(x), T(c['cls_logits']), T(c['labels']), head=head, k=4, relative=True, exclude=torch.arange(n), **kw)
        for end in ('pro', 'opp'):
            idx = ex[end + '_indices'].numpy()
            assert not (idx == np.arange(n)[:, None]).any() and valid[idx[idx >= 0]].all()
            assert np.array_equal(ex[end + '_labels'].numpy(), np.where(idx >= 0, c['labels'][np.maximum(idx, 0)], -1))
            assert np.array_equal(ex[end + '_severities'].numpy(), np.where(idx >= 0, m['severity'][np.maximum(idx, 0)], np.nan), equal_nan=True)
    counts = inf.counts()
    assert counts['n'] == n and counts['bad_rows'] >= 3 and counts['bad_labels'] >= 1 and counts['bad_rows_mu'] >= 3
    assert counts['n_valid'] == int((inf._store['valid'][:n] != 0).sum())
    assert set(out) == {'pro_scores', 'pro_indices', 'opp_scores', 'opp_indices', 'pro_labels', 'opp_labels', 'pro_severities', 'opp_severities',
                        'query_self_influence', 'residual'}


def test_label_audit_finds_planted_label_noise():
    """600 rows of a confident 4-class head, 30 labels moved to another class: the AUROC of self-influence for the planted rows against
    the rest is >= 0.99 (the numpy statement gives 0.9997 for this case, 0.997 .. 0.9998 over head seeds 7, 8, 9)."""
    E = hid = 32
    C, n = 4, 600
    w1, b1, w2, b2 = cases.head(E, hid, C, seed=7)
    x = cases.features(n, E, seed=1)
    lg = cases.outputs(x, w1, b1, w2, b2, scale=10)
    y = lg.argmax(axis=1).astype(np.int64)
    g = np.random.default_rng(0)
    planted = g.choice(n, size=30, replace=False)
    y[planted] = (y[planted] + 1 + g.integers(C - 1, size=30)) % C
    heads = (SimpleNamespace(fc1=ic.lin(E, hid, w1, b1, CPU), fc2=ic.lin(hid, C, w2, b2, CPU)), None)
    la = L.HeadLaplace(heads)
    la.update(T(x), T(lg))
    la.fit()
    inf = I.HeadInfluence(la)
    inf.update(T(x), T(lg), T(y))
    is_planted = np.zeros(n, dtype=bool)
    is_planted[planted] = True
    si = inf.self_influence().numpy()
    assert np.isfinite(si).all()
    area = ic.auroc(si, is_planted)
    print(f'label audit AUROC {area:.4f}')
    assert area >= 0.99
    audit = inf.label_audit(top=30)
    idx = audit['indices'].numpy()
    assert is_planted[idx].mean() >= 0.8 and np.array_equal(audit['labels'].numpy(), y[idx])
    assert np.array_equal(audit['predicted'].numpy(), lg[idx].argmax(axis=1)) and (np.diff(audit['scores'].numpy()) <= 0).all()
    p = torch.softmax(T(lg[idx]).double(), dim=1).numpy()
    assert np.allclose(audit['label_prob'].numpy(), p[np.arange(30), y[idx]], rtol=1e-6)


def test_tie_rule_on_integer_rows():
    """Integer-valued rows: equal scores go to the lower index at BOTH ends, -0 ties with +0, the two lists overlap when fewer than 2 k
    valid rows exist, empty slots hold -1 / NaN, an excluded or invalid row is never returned."""
    rows = np.zeros((8, 32), dtype=np.float32)
    rows[:, 0] = [1, 1, -1, -1, 0, 2, 1, 1]
    rows[4, 1] = 1                                                                       # score 0 against the query, but not a zero row
    valid = np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    norm2 = (rows.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    q = np.zeros((2, 32), dtype=np.float32)
    q[0, 0], q[1, 0] = 1, -1
    s = I.search_reference(q, rows, norm2, valid, k=4)
    assert s['pro_indices'][0].tolist() == [5, 0, 1, 7] and s['pro_scores'][0].tolist() == [2, 1, 1, 1]
    assert s['opp_indices'][0].tolist() == [2, 3, 4, 0] and s['opp_scores'][0].tolist() == [-1, -1, 0, 1]
    assert s['pro_indices'][1].tolist() == [2, 3, 4, 0] and s['opp_indices'][1].tolist() == [5, 0, 1, 7]
    assert not np.signbit(s['pro_scores'][1][2])                                         # -1 * 0 = -0 is reported as +0
    r = I.search_reference(q, rows, norm2, valid, k=4, relative=True, exclude=np.array([5, 2]))
    assert r['pro_indices'][0].tolist() == [0, 1, 7, 4] and r['opp_indices'][1].tolist() == [0, 1, 5, 7]
    many = I.search_reference(q, rows, norm2, valid, k=10, query_valid=np.array([1, 0]))
    assert many['pro_indices'][0].tolist() == [5, 0, 1, 7, 4, 2, 3, -1, -1, -1] and many['opp_indices'][0].tolist() == [2, 3, 4, 0, 1, 7, 5, -1, -1, -1]
    assert np.isnan(many['pro_scores'][0][7:]).all() and (many['pro_indices'][1] == -1).all() and np.isnan(many['opp_scores'][1]).all()


def test_refusals_before_any_launch():
    la = ic.fitted_laplace(32, 32, 4, CPU, gaussian=True)
    x, c = ic.recorded(20, 32, 32, 4, seed=1, bad=False)
    _, m = ic.recorded(20, 32, 32, 1, seed=2, bad=False)
    fx, lg, y = T(x), T(c['cls_logits']), T(c['labels'])
    with pytest.raises(RovitHipError, match='not fitted'):
        I.HeadInfluence(L.HeadLaplace((la.cls_head, la.unc_head)))
    with pytest.raises(RovitHipError, match='HeadLaplace is needed'):
        I.HeadInfluence(object())
    with pytest.raises(RovitHipError, match='capacity'):
        I.HeadInfluence(la, capacity=0)
    inf = I.HeadInfluence(la)
    with pytest.raises(RovitHipError, match='nothing recorded'):
        inf.self_influence()
    for bad in ((fx[:, :16], lg, y), (fx, lg[:, :2], y), (fx, lg, y[:5]), (fx, lg, y.float()), (fx, lg, None)):
        with pytest.raises(RovitHipError):
            inf.update(*bad)
    with pytest.raises(RovitHipError, match='missing'):
        inf.update(fx, lg, y, mu=T(m['mu']), log_var=T(m['log_var']))                  # a missing severity column
    inf.update(fx, lg, y)
    with pytest.raises(RovitHipError, match='columns of the first'):
        inf.update(fx, lg, y, T(m['mu']), T(m['log_var']), T(m['severity']))
    with pytest.raises(RovitHipError, match="'mu' head was not recorded"):
        inf.search(fx, lg, head='mu', target='mu')
    for k in (0, 33, 2.0, True):
        with pytest.raises(RovitHipError, match='k must be'):
            inf.search(fx, lg, k=k)
    for kw in ({'head': 'kan'}, {'target': 'mu'}, {'head': 'mu', 'target': 'logit'}, {'exclude': torch.zeros(3, dtype=torch.int64)},
               {'exclude': torch.zeros(20)}, {'labels': y[:3]}):
        with pytest.raises(RovitHipError):
            inf.search(fx, lg, **kw)
    with pytest.raises(RovitHipError):
        inf.search(fx[:, :16], lg)
    with pytest.raises(RovitHipError, match='top must be'):
        inf.label_audit(top=0)
    # without a Gaussian part the 'mu' head does not exist
    plain = I.HeadInfluence(ic.fitted_laplace(32, 32, 4, CPU, gaussian=False))
    plain.update(fx, lg, y, T(m['mu']), T(m['log_var']), T(m['severity']))                # the columns are not kept
    assert plain.has_mu is False
    with pytest.raises(RovitHipError, match='Gaussian part'):
        plain.search(fx, lg, head='mu', target='mu')
    # the loss of the 'mu' head needs its three columns
    full = I.HeadInfluence(la)
    full.update(fx, lg, y, T(m['mu']), T(m['log_var']), T(m['severity']))
    with pytest.raises(RovitHipError, match='needs mu, log_var and severity'):
        full.search(fx, lg, head='mu', target='loss', mu=T(m['mu']))
    assert full.search(fx, lg, head='mu', target='mu', k=3)['pro_indices'].shape == (20, 3)
    assert full.search(fx, lg, target='logit', class_index=2, k=3)['residual'][:, 2].eq(1).all()
    # a head parameter changes: the tables are stale
    with torch.no_grad():
        la.cls_head.fc2.bias.add_(0.0)
    with pytest.raises(RovitHipError, match='has changed since fit'):
        full.search(fx, lg)
    with pytest.raises(RovitHipError, match='has changed since fit'):
        full.update(fx, lg, y, T(m['mu']), T(m['log_var']), T(m['severity']))
    if torch.cuda.is_available():
        with pytest.raises(RovitHipError, match='the index on'):
            inf.search(fx.cuda(), lg.cuda())


class _Stub(torch.nn.Module):
    """The heads of a RoViTKAN behind a linear "backbone" that runs on CPU tensors, with the model's own influence entry points."""

    def __init__(self, E=32, hid=32, C=4):
        super().__init__()
        from models.rovit_kan import RoViTKAN
        w1, b1, w2, b2 = cases.head(E, hid, C, seed=21)
        u1, c1, u2, c2 = cases.head(E, hid, 1, seed=22)
        self.proj = torch.nn.Linear(48, E)
        self.classification_head = torch.nn.Module()
        self.classification_head.fc1, self.classification_head.fc2 = ic.lin(E, hid, w1, b1, CPU), ic.lin(hid, C, w2, b2, CPU)
        self.uncertainty_head = torch.nn.Module()
        self.uncertainty_head.fc1, self.uncertainty_head.fc_mu = ic.lin(E, hid, u1, c1, CPU), ic.lin(hid, 1, u2, c2, CPU)
        self.uncertainty_head.fc_logvar = ic.lin(hid, 1, 0.1 * u2, c2, CPU)
        self.fit_influence = RoViTKAN.fit_influence.__get__(self)
        self.influential_examples = RoViTKAN.influential_examples.__get__(self)

    def forward(self, x):
        f = self.proj(x.flatten(1))
        h, g = torch.relu(self.classification_head.fc1(f)), torch.relu(self.uncertainty_head.fc1(f))
        return {'features': f, 'cls_logits': 3 * self.classification_head.fc2(h), 'mu': self.uncertainty_head.fc_mu(g),
                'log_var': self.uncertainty_head.fc_logvar(g)}


def test_model_and_evaluator_wrappers_on_cpu_tensors(tmp_path, capsys):
    from evaluation.evaluator import Evaluator
    from explainability import TrainingInfluence
    torch.manual_seed(0)
    model = _Stub().eval()
    images = torch.randn(40, 3, 4, 4)
    labels = torch.arange(40) % 4
    loader = [(images[i:i + 16], labels[i:i + 16], labels[i:i + 16]) for i in range(0, 40, 16)]
    inf = model.fit_influence(loader, chunk=8)
    assert isinstance(inf, I.HeadInfluence) and inf.n == 40 and inf.has_mu and inf.laplace.n == 40 and inf.laplace.has_gaussian
    assert inf.counts() == {'n': 40, 'n_valid': 40, 'bad_rows': 0, 'bad_labels': 0, 'n_valid_mu': 40, 'bad_rows_mu': 0}
    out = model.influential_examples(images, inf, k=3, labels=labels)
    assert out['pro_indices'][:, 0].tolist() == list(range(40)) and out['pro_scores'].shape == (40, 3)
    with torch.no_grad():
        assert torch.equal(out['head_class'], model(images)['cls_logits'].argmax(dim=1))
    expl = TrainingInfluence(model, inf).explain(images[5:6], k=3, labels=labels[5:6])
    assert expl['proponents'][0]['index'] == 5 and expl['proponents'][0]['label'] == 1 and len(expl['opponents']) == 3
    # a fitted HeadLaplace is reused, and one pass records into it otherwise
    again = model.fit_influence(loader, laplace=inf.laplace)
    assert again.laplace is inf.laplace and torch.equal(again.rows(), inf.rows()) and torch.equal(again.rows('mu'), inf.rows('mu'))
    with pytest.raises(RovitHipError, match='needs the training labels'):
        model.fit_influence(images)
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=['a', 'b', 'c', 'd'], num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    ev = Evaluator(model, loader, cfg, 'cpu')
    assert ev.influence is None
    with pytest.raises(RovitHipError, match='fit_influence'):
        ev.audit_labels()
    assert ev.fit_influence(loader) is ev.influence
    capsys.readouterr()
    audit = ev.audit_labels(top=7)
    text = capsys.readouterr().out
    assert 'Label audit (top 7 of 40 valid training rows by self-influence):' in text
    assert len(audit['rows']) == 7 and audit['counts']['n'] == 40
    si = ev.influence.self_influence().numpy()
    assert [r['index'] for r in audit['rows']] == np.argsort(-si, kind='stable')[:7].tolist()
    assert (tmp_path / 'label_audit.txt').read_text(encoding='utf-8').splitlines()[0] == text.strip().splitlines()[0]
    assert json.loads((tmp_path / 'label_audit.json').read_text(encoding='utf-8')) == audit
    assert not (tmp_path / 'evaluation_results.txt').exists()


def test_c_entry_points_refuse_bad_descriptors_without_a_gpu():
    """Every check comes before the first launch, so the refusals can be seen on a machine without a device."""
    lib = native.load()
    assert lib.rovit_influence_workspace_bytes(65, 1000, 640, 10) > 0
    for bad in ((0, 10, 64, 1), (1, 0, 64, 1), (1, 10, 48, 1), (1, 10, 2336, 1), (1, 10, 64, 0), (1, 10, 64, 33), (1, native.KAN_STATS_MAX_ROWS + 1, 64, 1)):
        assert lib.rovit_influence_workspace_bytes(*bad) == 0, bad
    # the workspace of the default plan serves every cap on the splits: it only ever needs fewer lists
    assert lib.rovit_influence_workspace_bytes(65, 5000, 64, 32) == 65 * 2 * 40 * 32 * 8          # 79 tiles in 40 splits of 2
    assert lib.rovit_influence_embed(None, None) != 0 and b'null descriptor' in lib.rovit_last_error_string()
    assert lib.rovit_influence_search(None, None) != 0 and b'null descriptor' in lib.rovit_last_error_string()
    buf = (ctypes.c_char * 4096)()
    at = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16                            # never dereferenced: every call is refused
    d = native.InfluenceRows()
    d.n, d.embed, d.hid, d.num_classes, d.head, d.target = 8, 32, 32, 4, native.INFLUENCE_CLS, native.INFLUENCE_LOSS
    for name in ('features', 'fc1_weight', 'fc1_bias', 'whitening', 'cls_logits', 'rows', 'residual', 'norm2', 'valid', 'counts'):
        setattr(d, name, at)
    for field, value, word in (('n', 0, b'rows'), ('embed', 48, b'embed'), ('hid', 288, b'hid'), ('num_classes', 9, b'classes'), ('head', 2, b'head'),
                               ('target', 5, b'target'), ('max_workgroups', -1, b'max_workgroups'), ('whitening', None, b'null pointer'),
                               ('cls_logits', None, b'cls_logits'), ('counts', None, b'null pointer'), ('rows', at + 4, b'aligned')):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert lib.rovit_influence_embed(ctypes.byref(d), None) != 0 and word in lib.rovit_last_error_string(), field
        setattr(d, field, keep)
    d.head = native.INFLUENCE_MU
    assert lib.rovit_influence_embed(ctypes.byref(d), None) != 0 and b'one output' in lib.rovit_last_error_string()
    d.num_classes = 1
    assert lib.rovit_influence_embed(ctypes.byref(d), None) != 0 and b'mu, log_var and severity' in lib.rovit_last_error_string()
    q = native.InfluenceQuery()
    q.batch, q.n, q.dim, q.k, q.workspace_bytes = 4, 100, 64, 5, 4096
    for name in ('queries', 'rows', 'norm2', 'valid', 'workspace', 'pro_scores', 'pro_indices', 'opp_scores', 'opp_indices'):
        setattr(q, name, at)
    for field, value, word in (('batch', 0, b'batch'), ('n', 0, b'rows'), ('dim', 2336, b'dim'), ('dim', 48, b'dim'), ('k', 33, b'k 33'),
                               ('relative', 2, b'relative'), ('max_splits', -1, b'max_splits'), ('norm2', None, b'null pointer'),
                               ('opp_indices', None, b'output is missing'), ('ref_labels', at, b'go with ref_labels'),
                               ('pro_severities', at, b'go with ref_severity'), ('queries', at + 8, b'16-byte'), ('workspace_bytes', 64, b'are needed')):
        keep = getattr(q, field)
        setattr(q, field, value)
        assert lib.rovit_influence_search(ctypes.byref(q), None) != 0 and word in lib.rovit_last_error_string(), field
        setattr(q, field, keep)
    assert native.ABI_VERSION == 440 and lib.rovit_version() == 440
