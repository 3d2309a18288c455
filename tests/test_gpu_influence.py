"""GPU tests of csrc/influence.hip through rovit_hip.influence: the embed kernel against ``embed_reference``, the signed top-k search
against ``search_reference`` (exactly, on integer-valued rows, and by its properties on real-valued ones), their determinism, and the
model / Evaluator entry points end to end.

Tolerances: four times the error of an fp32 numpy evaluation of the same formulas against fp64, maximum over the case
(laplace_cases.tolerance), computed from the references alone.  The tests print error / tolerance before they assert.

Measured on the MI355X over the cases below:
  embed     max error / tolerance = 0.809 (n = 1, E = 192, hid = 128, C = 2; 0.055 .. 0.81 over the 32 cases; a single row has the
            smallest tolerance, the maximum of the fp32 error being taken over one row only)
  search    real-valued rows, max |score - its own fp64 score| / tolerance: 0.803 (dim 512) and 0.608 (dim 640); with relative 0.613 and
            0.214.  The kernel's score is ONE fp32 fma chain over the dim, numpy's fp32 product a blocked sum: the ratio is higher than
            the embed's, and stays below 1.
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
import influence_cases as ic  # noqa: E402
import laplace_cases as cases  # noqa: E402
from oracle import ref_cpu  # noqa: E402  (checker only)

from rovit_hip import influence as I  # noqa: E402
from rovit_hip import native  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (192, 128)]
CLASSES = [1, 2, 4, 8]                     # 1: the Gaussian head
EMBED_ROWS = [1, 63, 65, 300]
REL = 2.0 ** -22


def dev():
    return torch.device('cuda:0')


def up(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev())


def device_embed(x, cols, w1, b1, W, C, head, target, max_workgroups=0, edges=None):
    """rovit_influence_embed over the row ranges ``edges`` into one set of outputs: (rows, residual, norm2, valid, counts) as numpy."""
    n, E = x.shape
    hid, N = w1.shape[0], W.shape[0]
    t = {k: up(np.asarray(v)) for k, v in cols.items()}
    tx, tw1, tb1, tW = up(x), up(w1), up(b1), up(W)
    rows = torch.full((n, N), 7.0, dtype=torch.float32, device=dev())
    residual = torch.full((n, C), 7.0, dtype=torch.float32, device=dev())
    norm2 = torch.full((n,), 7.0, dtype=torch.float32, device=dev())
    valid = torch.full((n,), 7, dtype=torch.int32, device=dev())
    counts = torch.zeros(native.INFLUENCE_COUNT_WORDS, dtype=torch.int64, device=dev())
    edges = edges or [0, n]
    for r0, r1 in zip(edges[:-1], edges[1:]):
        d = native.InfluenceRows()
        d.n, d.embed, d.hid, d.num_classes, d.max_workgroups = r1 - r0, E, hid, C, max_workgroups
        d.head, d.target = I.HEADS[head], I.TARGETS[head][target]
        d.features, d.fc1_weight, d.fc1_bias, d.whitening = native.ptr(tx[r0:r1]), native.ptr(tw1), native.ptr(tb1), native.ptr(tW)
        for name, field in (('cls_logits', 'cls_logits'), ('labels', 'labels'), ('mu', 'mu'), ('log_var', 'log_var'), ('severity', 'severity')):
            if name in t:
                setattr(d, field, native.ptr(t[name][r0:r1]))
        d.rows, d.residual, d.norm2, d.valid, d.counts = (native.ptr(v) for v in (rows[r0:r1], residual[r0:r1], norm2[r0:r1], valid[r0:r1], counts))
        native.call('rovit_influence_embed', ctypes.byref(d), native.stream_ptr())
    return tuple(v.cpu().numpy() for v in (rows, residual, norm2, valid, counts))


def device_search(q, rows, norm2, valid, k, relative=False, exclude=None, query_valid=None, labels=None, severity=None, max_workgroups=0,
                  max_splits=0):
    B, N = q.shape
    n = rows.shape[0]
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev())
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev())
    out = {'pro_scores': f32(B, k), 'pro_indices': i32(B, k), 'opp_scores': f32(B, k), 'opp_indices': i32(B, k)}
    if labels is not None:
        out['pro_labels'], out['opp_labels'] = i32(B, k), i32(B, k)
    if severity is not None:
        out['pro_severities'], out['opp_severities'] = f32(B, k), f32(B, k)
    nbytes = native.load().rovit_influence_workspace_bytes(B, n, N, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    keep = [up(v) for v in (q, query_valid, rows, norm2, valid, exclude, labels, severity)]
    d = native.InfluenceQuery()
    d.batch, d.n, d.dim, d.k, d.relative, d.max_workgroups, d.max_splits = B, n, N, k, int(relative), max_workgroups, max_splits
    d.queries, d.query_valid, d.rows, d.norm2, d.valid, d.exclude, d.ref_labels, d.ref_severity = (native.ptr(v) for v in keep)
    d.workspace, d.workspace_bytes = native.ptr(ws), nbytes
    for name, v in out.items():
        setattr(d, name, native.ptr(v))
    native.call('rovit_influence_search', ctypes.byref(d), native.stream_ptr())
    return {name: v.cpu().numpy() for name, v in out.items()}


# ---- embed -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('E,hid', SHAPES)
@pytest.mark.parametrize('n', EMBED_ROWS)
def test_embed_against_the_fp64_reference(n, E, hid, C):
    """Rows within the tolerance of the case; padding columns and invalid rows exactly zero; norm2 within 2 ulp of the fp32 rounding of
    the fp64 sum of squares of the stored row; flags and counts exact."""
    w1, b1, _, _, fit = ic.fitted_head(E, hid, C)
    head = 'cls' if C > 1 else 'mu'
    x, cols, ref, tol = ic.embed_case(n, E, hid, C)
    rows, residual, norm2, valid, counts = device_embed(x, cols, w1, b1, fit['whitening'], C, head, 'loss')
    err = float(np.abs(rows - ref['rows']).max())
    print(f'embed n={n} E={E} hid={hid} C={C}: error {err:.3e} tolerance {tol:.3e} ratio {err / tol if tol else 0.0:.3f}')
    assert np.array_equal(valid, ref['valid'].astype(np.int32))
    assert counts.tolist() == [ref['n'], ref['n_valid'], ref['bad_rows'], ref['bad_labels']]
    if n >= 4:
        assert ref['bad_rows'] >= 3 and (C == 1 or ref['bad_labels'] == 2)
    assert err <= tol
    P, D = hid + 32, hid + 1
    assert not rows.reshape(n, C, P)[:, :, D:].any() and not rows[valid == 0].any()
    want = (rows.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    assert (np.abs(norm2 - want) <= 2 * np.spacing(want)).all() and not norm2[valid == 0].any()
    assert np.abs(norm2 - ref['norm2']).max() <= 2 * tol * np.sqrt(ref['norm2'].max() * rows.shape[1]) + 2 * np.spacing(want).max()
    assert np.array_equal(np.isnan(residual), np.isnan(ref['residual']))
    assert np.allclose(residual, ref['residual'], rtol=REL, atol=2.0 ** -50, equal_nan=True)


@pytest.mark.parametrize('C,head,target', [(4, 'cls', 'logit'), (1, 'mu', 'mu'), (4, 'cls', 'loss')])
def test_embed_query_targets(C, head, target):
    """The targets a query can have: a logit (of the first argmax), mu (r = 1, no columns read), and the loss of the prediction made."""
    E, hid, n = 32, 32, 65
    w1, b1, _, _, fit = ic.fitted_head(E, hid, C)
    x, cols = ic.recorded(n, E, hid, C, seed=5, bad=False)
    cols = {'cls_logits': cols['cls_logits']} if head == 'cls' else {}
    ref = I.embed_reference(x, w1, b1, fit['whitening'], C, head, target, **cols)
    u32 = ic.embed_fp32(x, w1, b1, fit['whitening'], C, ref['residual'])
    tol = float(cases.tolerance(u32, ref['rows'], (0, 1)).max())
    rows, residual, _, valid, counts = device_embed(x, cols, w1, b1, fit['whitening'], C, head, target)
    assert np.abs(rows - ref['rows']).max() <= tol and valid.all() and counts.tolist() == [n, n, 0, 0]
    assert np.allclose(residual, ref['residual'], rtol=REL, atol=2.0 ** -50)


# ---- search ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [1, 65])
@pytest.mark.parametrize('n', [1, 63, 65, 1000, 5000])
@pytest.mark.parametrize('dim', [64, 160, 640, 2304])
def test_search_exact_on_integer_rows(dim, n, B):
    """Every dot product is exact in fp32 and ties abound: without ``relative`` indices and scores equal the reference's at both ends;
    with it, indices wherever the reference's adjacent scores differ by more than 2^-22 relative, and scores within that."""
    q, rows, norm2, valid = ic.integer_rows(n, B, dim, seed=dim + n + B)
    g = np.random.default_rng(n)
    labels, severity = g.integers(0, 4, size=n).astype(np.int32), g.random(n).astype(np.float32)
    qv = np.ones(B, dtype=np.int32)
    if B > 3:
        qv[3] = 0
    exclude = g.integers(0, n, size=B).astype(np.int32)
    for relative in (False, True):
        for ex in (None, exclude):
            ref = I.search_reference(q, rows, norm2, valid, 32, relative, ex, qv, labels, severity)
            for k in (1, 10, 32):
                got = device_search(q, rows, norm2, valid, k, relative, ex, qv, labels, severity)
                for end in ('pro', 'opp'):
                    rs, ri = ref[end + '_scores'], ref[end + '_indices']
                    gs, gi = got[end + '_scores'], got[end + '_indices']
                    assert np.array_equal(np.isnan(gs), np.isnan(rs[:, :k])) and np.array_equal(gi < 0, ri[:, :k] < 0), (end, k, relative)
                    if not relative:
                        assert np.array_equal(gi, ri[:, :k]) and np.array_equal(gs, rs[:, :k].astype(np.float32), equal_nan=True), (end, k)
                    else:
                        gap = np.abs(np.diff(rs, axis=1))                                # NaN beside an empty slot: never "close"
                        close = gap <= REL * np.abs(rs[:, :-1])
                        tied = np.zeros(rs.shape, dtype=bool)
                        tied[:, :-1] |= close
                        tied[:, 1:] |= close
                        tied[:, -1] = True                                               # slot 31's right neighbour is not known
                        clear = ~tied[:, :k]
                        assert np.array_equal(gi[clear], ri[:, :k][clear]), (end, k)
                        real = ~np.isnan(gs)
                        assert (np.abs(gs[real] - rs[:, :k][real]) <= REL * np.abs(rs[:, :k][real])).all(), (end, k)
                    safe = np.maximum(gi, 0)
                    assert np.array_equal(got[end + '_labels'], np.where(gi >= 0, labels[safe], -1))
                    assert np.array_equal(got[end + '_severities'], np.where(gi >= 0, severity[safe], np.nan), equal_nan=True)
                    assert valid[safe][gi >= 0].all() and (ex is None or not (gi == ex[:, None]).any())
                if B > 3:
                    assert (got['pro_indices'][3] == -1).all() and np.isnan(got['opp_scores'][3]).all()


@functools.lru_cache(maxsize=None)
def embedded(E, hid, C, n, seed):
    """Device-embedded rows of a recorded case: (rows, norm2, valid)."""
    w1, b1, _, _, fit = ic.fitted_head(E, hid, C)
    x, cols = ic.recorded(n, E, hid, C, seed=seed)
    rows, _, norm2, valid, _ = device_embed(x, cols, w1, b1, fit['whitening'], C, 'cls', 'loss')
    return rows, norm2, valid


@pytest.mark.parametrize('E,hid,C', [(32, 32, 8), (192, 128, 4)])
@pytest.mark.parametrize('relative', [False, True])
def test_search_on_embedded_rows(E, hid, C, relative):
    """Real-valued rows (dim 512 and 640): the indices returned are distinct, valid and not excluded; each score is within tol of its own
    index's fp64 score; in every slot the fp64 score of the index returned is within 2 tol of the reference's score of that slot.  tol:
    four times the error of the fp32 numpy product against fp64, maximum over the case.  Every query is compared."""
    n, B, k = 300, 65, 10
    rows, norm2, valid = embedded(E, hid, C, n, 3)
    q, _, qvalid = embedded(E, hid, C, B, 4)
    exclude = np.arange(B, dtype=np.int32)
    r64, q64 = rows.astype(np.float64), q.astype(np.float64)
    div = np.sqrt(np.where(norm2 > 0, norm2, 1).astype(np.float64)) if relative else np.ones(n)
    s64 = (q64 @ r64.T) / div[None]
    s32 = (q @ rows.T) / div.astype(np.float32)[None] if relative else q @ rows.T
    tol = float(cases.tolerance(s32, s64, (0, 1)).max())
    ref = I.search_reference(q, rows, norm2, valid, k, relative, exclude, qvalid)
    got = device_search(q, rows, norm2, valid, k, relative, exclude, qvalid)
    worst = 0.0
    for end in ('pro', 'opp'):
        gi, gs, rs = got[end + '_indices'], got[end + '_scores'], ref[end + '_scores']
        assert np.array_equal(gi < 0, ref[end + '_indices'] < 0) and (gi >= 0).any()
        for b in range(B):
            real = gi[b][gi[b] >= 0]
            assert len(set(real.tolist())) == len(real) and valid[real].all() and exclude[b] not in real
            own = s64[b, real]
            worst = max(worst, float(np.abs(gs[b, :len(real)] - own).max(initial=0.0)))
            assert (np.abs(gs[b, :len(real)] - own) <= tol).all() and (np.abs(own - rs[b, :len(real)]) <= 2 * tol).all(), (end, b)
    print(f'search E={E} hid={hid} C={C} relative={relative}: worst |score - own fp64 score| {worst:.3e} tolerance {tol:.3e} ratio {worst / tol:.3f}')


# ---- determinism -------------------------------------------------------------------------------------------------------------------------

def _record(la, x, c, m, edges, max_workgroups):
    inf = I.HeadInfluence(la, capacity=64)
    inf.max_workgroups = max_workgroups
    for r0, r1 in zip(edges[:-1], edges[1:]):
        inf.update(up(x[r0:r1]), up(c['cls_logits'][r0:r1]), up(c['labels'][r0:r1]), up(m['mu'][r0:r1]), up(m['log_var'][r0:r1]), up(m['severity'][r0:r1]))
    return inf


def test_bit_identity_across_runs_splits_grids_and_reference_splits():
    """Both heads' rows, residuals, norms, flags and counts: identical across two runs, splits of the rows into ``update`` calls
    ([0, n], uneven splits, [0, 1, n]) and max_workgroups in {1, 3, default}.  Every output of ``search``, for both heads: identical
    across two runs, the same grids, and one reference split against five (n = 300 is five tiles of 64 rows)."""
    E, hid, C, n, B = 192, 128, 4, 300, 65
    la = ic.fitted_laplace(E, hid, C, dev())
    x, c = ic.recorded(n, E, hid, C, seed=1)
    _, m = ic.recorded(n, E, hid, 1, seed=2)
    first = _record(la, x, c, m, [0, n], 0)
    names = ('rows', 'residual', 'norm2', 'valid', 'rows_mu', 'residual_mu', 'norm2_mu', 'valid_mu')
    snap = lambda inf: {k: inf._store[k][:n].clone() for k in names}
    base, base_counts = snap(first), first.counts()
    w1, b1, _, _, fit = ic.fitted_head(E, hid, C)
    u1, c1, _, _, fit_mu = ic.fitted_head(E, hid, 1)
    rc, rm = I.embed_reference(x, w1, b1, fit['whitening'], C, 'cls', 'loss', **c), I.embed_reference(x, u1, c1, fit_mu['whitening'], 1, 'mu', 'loss', **m)
    assert base_counts == {'n': n, 'n_valid': rc['n_valid'], 'bad_rows': rc['bad_rows'], 'bad_labels': rc['bad_labels'],
                           'n_valid_mu': rm['n_valid'], 'bad_rows_mu': rm['bad_rows']} and rc['bad_rows'] >= 3 and rm['bad_rows'] >= 3
    for edges, cap in (([0, n], 0), (cases.splits_of(n, 3, 1), 0), (cases.splits_of(n, 7, 2), 0), ([0, 1, n], 0), ([0, n], 1), ([0, n], 3),
                       (cases.splits_of(n, 5, 3), 3)):
        other = _record(la, x, c, m, edges, cap)
        got = snap(other)
        assert all(torch.equal(base[k], got[k]) or (torch.equal(torch.isnan(base[k]), torch.isnan(got[k])) and
                                                    torch.equal(torch.nan_to_num(base[k]), torch.nan_to_num(got[k]))) for k in names), (edges, cap)
        assert other.counts() == base_counts, (edges, cap)
    xq, cq = ic.recorded(B, E, hid, C, seed=9, bad=False)
    _, mq = ic.recorded(B, E, hid, 1, seed=10, bad=False)
    same = lambda a, b: set(a) == set(b) and all(torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)) for k in a)
    for head, kw in (('cls', {}), ('mu', {'mu': up(mq['mu']), 'log_var': up(mq['log_var']), 'severity': up(mq['severity'])})):
        for relative in (False, True):
            first.max_workgroups = first.max_splits = 0
            want = first.search(up(xq), up(cq['cls_logits']), head=head, k=10, relative=relative, **kw)
            assert (want['pro_indices'] >= 0).all() and (want['opp_indices'] >= 0).all()
            for cap, splits in ((0, 0), (1, 0), (3, 0), (0, 1), (0, 2), (3, 1)):
                first.max_workgroups, first.max_splits = cap, splits
                assert same(want, first.search(up(xq), up(cq['cls_logits']), head=head, k=10, relative=relative, **kw)), (head, relative, cap, splits)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

CLASS_NAMES = ['Healthy Leaf', 'Leaf Holes', 'Black Spot', 'Dry Leaf']


def test_model_and_evaluator_end_to_end(tmp_path):
    """A depth-2 RoViTKAN at stage 4 on 12 random images: fit_influence, influential_examples with the relative self-match on the
    training images themselves, Evaluator.fit_influence / audit_labels, and the device results against the CPU entry points on the same
    recorded rows."""
    from evaluation.evaluator import Evaluator
    from explainability import TrainingInfluence
    from models.backbone import DeiTTiny
    from models.rovit_kan import RoViTKAN
    model = RoViTKAN(pretrained=False)
    model.backbone.model = DeiTTiny(depth=2)
    model.load_state_dict(ref_cpu.init_rovit_state(depth=2, seed=31), strict=True)
    model = model.to(dev()).eval()
    model.curriculum_stage = 4
    g = torch.Generator().manual_seed(0)
    images = torch.nn.functional.interpolate(torch.randn(12, 3, 7, 7, generator=g), size=224, mode='bilinear', align_corners=False)
    labels = torch.arange(12) % 4
    loader = [(images[i:i + 4], labels[i:i + 4], labels[i:i + 4]) for i in range(0, 12, 4)]
    inf = model.fit_influence(loader)
    assert inf.n == 12 and inf.has_mu and inf.counts() == {'n': 12, 'n_valid': 12, 'bad_rows': 0, 'bad_labels': 0, 'n_valid_mu': 12, 'bad_rows_mu': 0}
    out = model.influential_examples(images.to(dev()), inf, k=5, labels=labels.to(dev()), relative=True)
    assert set(out) == {'pro_scores', 'pro_indices', 'opp_scores', 'opp_indices', 'pro_labels', 'opp_labels', 'pro_severities', 'opp_severities',
                        'query_self_influence', 'residual', 'head_class'}
    assert out['pro_indices'][:, 0].cpu().tolist() == list(range(12))                   # Cauchy-Schwarz: a row is its own first proponent
    with torch.no_grad():
        fwd = model(images.to(dev()))
    excl = inf.search(fwd['features'], fwd['cls_logits'], labels.to(dev()), k=5, relative=True, exclude=torch.arange(12, device=dev()))
    assert not (excl['pro_indices'].cpu() == torch.arange(12)[:, None]).any() and not (excl['opp_indices'].cpu() == torch.arange(12)[:, None]).any()
    # the CPU entry points on the same recorded rows, with the same fitted tables
    P = lambda t: t.detach().cpu().numpy()
    t = inf.laplace.tables
    f, lg = P(fwd['features']), P(fwd['cls_logits'])
    for head, sfx, C, kw in (('cls', '', 4, {'cls_logits': lg, 'labels': labels.numpy()}),
                             ('mu', '_mu', 1, {'mu': P(fwd['mu']).ravel(), 'log_var': P(fwd['log_var']).ravel(), 'severity': labels.numpy().astype(np.float32)})):
        w1, b1, W = P(t['fc1_weight' + sfx]), P(t['fc1_bias' + sfx]), P(t['whitening' + sfx])
        ref = I.embed_reference(f, w1, b1, W, C, head, 'loss', **kw)
        tol = float(cases.tolerance(ic.embed_fp32(f, w1, b1, W, C, ref['residual']), ref['rows'], (0, 1)).max())
        err = float(np.abs(P(inf.rows(head)) - ref['rows']).max())
        print(f'end to end {head}: error {err:.3e} tolerance {tol:.3e}')
        assert err <= tol and np.array_equal(P(inf._head_store(head)[3]) != 0, ref['valid'])
        si = P(inf.self_influence(head))
        assert np.abs(si - ref['norm2']).max() <= 4 * tol * np.sqrt(ref['norm2'].max() * ref['rows'].shape[1])
    # search: the queries are the training rows themselves (the same bits); each score against its own index's fp64 score
    r32 = P(inf.rows('cls'))
    rows = r32.astype(np.float64)
    div = np.sqrt(P(inf._head_store('cls')[2]).astype(np.float64))
    s64 = (rows @ rows.T) / div[None]
    stol = float(cases.tolerance((r32 @ r32.T) / div.astype(np.float32)[None], s64, (0, 1)).max())
    for end in ('pro', 'opp'):
        gi, gs = P(out[end + '_indices']), P(out[end + '_scores'])
        assert (gi >= 0).all() and (np.abs(gs - np.take_along_axis(s64, gi.astype(np.int64), axis=1)) <= stol).all()
    assert torch.equal(out['head_class'], fwd['cls_logits'].argmax(dim=1))
    expl = TrainingInfluence(model, inf).explain(images[:1], k=3, labels=labels[:1].to(dev()))
    assert [len(expl[k]) for k in ('proponents', 'opponents')] == [3, 3] and expl['proponents'][0]['index'] == 0
    cfg = SimpleNamespace(data=SimpleNamespace(class_names=CLASS_NAMES, num_classes=4), paths=SimpleNamespace(results_dir=tmp_path))
    ev = Evaluator(model, loader, cfg, dev())
    assert ev.influence is None
    assert ev.fit_influence(loader) is ev.influence and ev.influence.n == 12
    audit = ev.audit_labels(top=5)
    assert len(audit['rows']) == 5 and audit['counts']['n_valid'] == 12
    scores = [r['self_influence'] for r in audit['rows']]
    assert scores == sorted(scores, reverse=True) and scores[0] == pytest.approx(float(np.nanmax(P(ev.influence.self_influence()))))
    assert 'Label audit (top 5 of 12' in (tmp_path / 'label_audit.txt').read_text(encoding='utf-8')
    import json
    assert json.loads((tmp_path / 'label_audit.json').read_text(encoding='utf-8'))['rows'][0]['index'] == audit['rows'][0]['index']
    # a head parameter changes: the tables are stale, and the index refuses to go on
    with torch.no_grad():
        model.classification_head.fc2.bias.add_(0.0)
    with pytest.raises(I.RovitHipError, match='has changed since fit'):
        model.influential_examples(images.to(dev()), inf)
