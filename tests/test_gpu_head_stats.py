"""GPU tests of the per-head attention statistics (csrc/head_stats.hip, rovit_hip/head_stats.py, explainability/attention_heads.py).

Every statistic is compared with ``head_stats_reference`` (numpy fp64) fed with ``get_attention_probabilities`` AT THE SAME BATCH, and
the features with that call's features bit for bit.  Errors are relative to the statistic's scale (ln 197 for entropies, 16 sqrt(338) =
294.2 px for distances, 1 for masses); every test prints its largest error per class of statistic before it asserts
min(4 x MEASURED, 8 x 197 x 2^-24 = 9.4e-5).

Measured on the MI355X (largest over every case of this file, relative to the scale):
  entropy  1.83e-07      distance  1.13e-07      mass  1.59e-07      (finalise vs the fp64 restatement: 4.68e-16 relative)
Every case's figures are in profiles/head_stats_error.jsonl.
"""
import json

import numpy as np
import pytest
import torch

import head_stats_cases as cases

pytestmark = pytest.mark.gpu

from oracle import ref_cpu  # noqa: E402  (weights only)

MEASURED = {'entropy': 1.83e-07, 'distance': 1.13e-07, 'mass': 1.59e-07}


def dev():
    return torch.device('cuda:0')


def _vit(depth, seed):
    from models.backbone import DeiTTiny
    m = DeiTTiny(depth)
    m.load_state_dict(ref_cpu.init_vit_state(depth, torch.Generator().manual_seed(seed)))
    return m.to(dev()).eval()


def _images(B, seed):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed)).to(dev())


_CASES = {}


def _case(name):
    """One run per named case, shared by the tests: the fused statistics (per_token included), the taps' probabilities and features at
    the same batch, and the fp64 oracle on those probabilities."""
    if name in _CASES:
        return _CASES[name]
    from rovit_hip import head_stats as hs
    from rovit_hip import native, taps
    depth, B, seed, edit = {'b1': (2, 1, 11, None), 'b3': (2, 3, 12, None), 'd12': (12, 2, 13, None), 'uniform': (2, 2, 14, 'zero'),
                            'peaked': (2, 2, 15, 'x30')}[name]
    m = _vit(depth, seed)
    with torch.no_grad():
        if edit == 'zero':                       # q = k = 0 in block 0: every probability is 1/197 (the engine re-prepares on _version)
            m.blocks[0].attn.qkv.weight.zero_()
            m.blocks[0].attn.qkv.bias.zero_()
        elif edit == 'x30':                      # scores x 900 in block 1: most probabilities underflow
            m.blocks[1].attn.qkv.weight.mul_(30.0)
    x = _images(B, seed)
    out = hs.attention_head_stats(m, x, per_token=True)
    probs = taps.attention_probabilities(m, x)
    # the features of the probability taps' own forward, at the same batch
    params = m.ordered_parameters()
    eng = m.engine
    ws = eng.take_ws(B, False, x.device)
    feats = torch.empty(B, 192, device=x.device, dtype=torch.float32)
    keep = [torch.empty(B, 3, 197, 197, device=x.device, dtype=torch.float32) for _ in range(depth)]
    native.call('rovit_vit_forward_taps', native.ptr(x), native.ptr_array(params), native.ptr(eng.prep), native.ptr(ws), native.ptr(feats),
                None, native.ptr_array(keep), B, depth, native.stream_ptr())
    eng.give_ws(B, False, ws)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(probs, keep))
    c = {'model': m, 'x': x, 'out': {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()},
         'probs': [p.cpu().numpy() for p in probs], 'tap_features': feats.cpu().numpy(), 'depth': depth, 'B': B}
    c['ref'] = hs.head_stats_reference(c['probs'])
    _CASES[name] = c
    return c


def _errors(name, got, ref, classes):
    """Largest |got - ref| / scale per class of statistic over the last axis' entries; printed, then returned."""
    err = {}
    for k, cl in enumerate(classes):
        e = float(np.abs(got[..., k].astype(np.float64) - ref[..., k]).max() / cases.SCALES[cl])
        err[cl] = max(err.get(cl, 0.0), e)
    print('HEAD_STATS_ERROR ' + json.dumps({'case': name, **err}))
    return err


def _assert_errors(err):
    for cl, e in err.items():
        assert e <= cases.tolerance(MEASURED[cl]), (cl, e, cases.tolerance(MEASURED[cl]))


@pytest.mark.parametrize('name', ['b1', 'b3', 'd12'])
def test_statistics_match_the_oracle_on_the_taps_probabilities(name):
    c = _case(name)
    out, ref = c['out'], c['ref']
    L, B = c['depth'], c['B']
    assert out['summary'].shape == (B, L, 3, 8) and out['cls_attention'].shape == (B, L, 3, 196) and out['per_token'].shape == (B, L, 3, 197, 4)
    assert out['summary'].dtype == np.float32 and np.isfinite(out['summary']).all() and np.isfinite(out['per_token']).all()
    assert np.array_equal(out['features'], c['tap_features'])                    # bit for bit
    err = _errors(name + ':summary', out['summary'], ref['summary'], cases.STAT_CLASS)
    _assert_errors(err)
    _assert_errors(_errors(name + ':per_token', out['per_token'], ref['per_token'], cases.TOKEN_CLASS))
    # the masses that are single probabilities are the taps' own bits
    P = np.stack(c['probs'], 1)                                                  # (B, L, 3, 197, 197) fp32
    assert np.array_equal(out['cls_attention'], P[:, :, :, 0, 1:])
    assert np.array_equal(out['per_token'][..., 2], P[..., 0]) and np.array_equal(out['per_token'][..., 3], P.max(-1))
    assert np.array_equal(out['summary'][..., 5], P[..., 0, 0])


def test_uniform_block_gives_the_analytic_values():
    c = _case('uniform')
    exp = cases.uniform_expected()
    got = c['out']['summary'][:, 0]                                              # block 0: (B, 3, 8)
    err = _errors('uniform:analytic', got, np.broadcast_to(exp['summary'], got.shape), cases.STAT_CLASS)
    _assert_errors(err)
    tok = c['out']['per_token'][:, 0]
    ref_tok = np.zeros((197, 4))
    ref_tok[:, 0], ref_tok[1:, 1], ref_tok[:, 2], ref_tok[:, 3] = cases.LN197, exp['distance_per_query'], 1 / 197, 1 / 197
    _assert_errors(_errors('uniform:per_token', tok, np.broadcast_to(ref_tok, tok.shape), cases.TOKEN_CLASS))
    assert np.all(c['out']['cls_attention'][:, 0] == np.float32(1.0) / np.float32(197.0))
    _assert_errors(_errors('uniform:oracle', c['out']['summary'], c['ref']['summary'], cases.STAT_CLASS))
    assert np.array_equal(c['out']['features'], c['tap_features'])


def test_peaked_block_stays_finite():
    c = _case('peaked')
    out = c['out']
    P1 = c['probs'][1]
    assert (P1 == 0).mean() > 0.5                                                # the case is what it says: most probabilities underflowed
    for k in ('summary', 'cls_attention', 'per_token', 'features'):
        assert np.isfinite(out[k]).all(), k
    assert (out['per_token'][..., 0] >= 0).all() and (out['summary'][..., 0] >= 0).all() and (out['summary'][..., 4] >= 0).all()
    assert (out['per_token'][..., 1] >= 0).all() and (out['per_token'][..., 1] <= 294.3).all()
    _assert_errors(_errors('peaked:summary', out['summary'], c['ref']['summary'], cases.STAT_CLASS))
    _assert_errors(_errors('peaked:per_token', out['per_token'], c['ref']['per_token'], cases.TOKEN_CLASS))
    assert np.array_equal(out['features'], c['tap_features'])


@pytest.mark.parametrize('name', ['b3', 'd12', 'peaked'])
def test_per_token_means_reproduce_the_summary_in_the_stated_order(name):
    """The fp32 sums of csrc/head_stats.hip's header, redone on the host from per_token: 4 rows per wave in row order, the 4 waves in
    order, the 13 slices in order, times 1/197 or 1/196.  Bit for bit, so the padded query rows 197..207 added nothing."""
    c = _case(name)
    tok, s = c['out']['per_token'], c['out']['summary']
    assert np.array_equal(cases.stated_order_mean(tok[..., 0], False), s[..., 0])
    assert np.array_equal(cases.stated_order_mean(tok[..., 1], True), s[..., 1])
    assert np.array_equal(cases.stated_order_mean(tok[..., 2], True), s[..., 2])
    assert np.array_equal(cases.stated_order_mean(tok[..., 3], False), s[..., 6])
    assert np.array_equal(tok[..., 0, 0], s[..., 4]) and np.array_equal(tok[..., 0, 2], s[..., 5])
    assert np.all(tok[..., 0, 1] == 0)                                           # D_0 = 0


def test_padded_query_rows_leave_no_trace_and_the_last_key_slot_counts():
    from rovit_hip import head_stats as hs
    c = _case('b3')
    m, x, B, L = c['model'], c['x'], c['B'], c['depth']
    # per_token with a guard behind it: rows 197..207 of the last 16-row group would land there
    n = B * L * 3 * 197 * 4
    buf = torch.full((n + 11 * 4 * 4,), -7.0, device=dev(), dtype=torch.float32)
    summary = torch.empty(B, L, 3, 8, device=dev(), dtype=torch.float32)
    cls = torch.empty(B, L, 3, 196, device=dev(), dtype=torch.float32)
    hs._forward(m, x, summary, cls, buf[:n].view(B, L, 3, 197, 4))
    assert torch.all(buf[n:] == -7.0)
    assert np.array_equal(buf[:n].view(B, L, 3, 197, 4).cpu().numpy(), c['out']['per_token'])
    assert np.array_equal(summary.cpu().numpy(), c['out']['summary'])
    # keys 192..196 sit in the fourth 64-key slot, lanes 0..4: the class-token row puts visible mass there, and it arrives
    P = np.stack(c['probs'], 1)
    tail = c['out']['cls_attention'][..., 191:196]
    assert (tail > 1e-4).all()
    assert np.array_equal(tail, P[:, :, :, 0, 192:197])
    # ... and enters the sums: without those keys the entropy of the class-token row would miss their share
    part = -(P[..., 0, :192].astype(np.float64) * np.log(P[..., 0, :192].astype(np.float64))).sum(-1)
    assert (c['ref']['summary'][..., 4] - part > 10 * cases.CAP * cases.LN197).all()


def test_two_runs_are_bit_identical():
    from rovit_hip import head_stats as hs
    c = _case('b3')
    again = hs.attention_head_stats(c['model'], c['x'], per_token=True)
    for k in ('summary', 'cls_attention', 'per_token', 'features'):
        assert np.array_equal(again[k].cpu().numpy(), c['out'][k]), k
    lean = hs.attention_head_stats(c['model'], c['x'])
    assert 'per_token' not in lean and np.array_equal(lean['summary'].cpu().numpy(), c['out']['summary'])
    assert lean['STAT_NAMES'] == hs.STAT_NAMES


@pytest.mark.parametrize('n', cases.FINALIZE_N)
def test_finalize_is_split_invariant_and_matches_the_reference(n):
    from rovit_hip import head_stats as hs
    C = cases.FINALIZE_CLASSES
    summary, cls, labels = cases.finalize_rows(n)
    ref = hs.finalize_reference((summary, cls), labels, C)
    ts, tc, tl = (torch.from_numpy(a).to(dev()) for a in (summary, cls, labels))
    blocks = []
    for split in cases.finalize_splits(n):
        acc = hs.AttentionHeadStats(2, 3, C, capacity=4)                         # small: the buffers grow on the way
        at = 0
        for k in split:
            acc.update_rows(ts[at:at + k], tc[at:at + k], tl[at:at + k])
            at += k
        res = acc.compute()
        assert acc.n == n and res['count'][0] == n
        blocks.append(res['block'])
    for b in blocks[1:]:
        assert np.array_equal(blocks[0], b)                                      # bit-identical over the splits
    got = blocks[0]
    assert np.isfinite(got).all()
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), np.finfo(np.float64).tiny)
    rel[ref == got] = 0.0
    print('HEAD_STATS_ERROR ' + json.dumps({'case': f'finalize:n{n}', 'fp64_rel': float(rel.max())}))
    assert rel.max() <= n * 2.0 ** -52
    res = hs.result_from_block(got, 2, 3, C)
    e = 1 + cases.FINALIZE_EMPTY_CLASS
    assert res['count'][e] == 0 and not res['mean'][e].any() and not res['var'][e].any() and not res['cls_attention_mean'][e].any()
    if n == 1:
        assert not res['var'].any()


def test_model_surface():
    from explainability import AttentionHeadAnalysis
    from models.rovit_kan import RoViTKAN
    from rovit_hip import head_stats as hs
    from rovit_hip.native import RovitHipError
    m = RoViTKAN(pretrained=False)
    m.load_state_dict(ref_cpu.init_rovit_state(seed=3), strict=True)
    m = m.to(dev()).eval()
    x = _images(6, 21)
    labels = torch.tensor([0, 1, 1, 3, 0, 1])
    out = m.attention_head_stats(x[:2], per_token=True)
    assert out['summary'].shape == (2, 12, 3, 8) and out['cls_attention'].shape == (2, 12, 3, 196) and out['per_token'].shape == (2, 12, 3, 197, 4)
    assert torch.equal(out['summary'], m.backbone.attention_head_stats(x[:2])['summary'])
    # a three-batch loader of (images, class_labels, severity_labels), host batches
    loader = [(x[k:k + 2].cpu(), labels[k:k + 2], labels[k:k + 2]) for k in range(0, 6, 2)]
    res = m.attention_head_stats(loader)
    assert res['groups'] == ['all', 0, 1, 2, 3] and res['count'].tolist() == [6, 2, 3, 0, 1]
    assert res['mean'].shape == (5, 12, 3, 8) and res['var'].shape == (5, 12, 3, 8) and res['cls_attention_mean'].shape == (5, 12, 3, 196)
    rows = [m.attention_head_stats(x[k:k + 2]) for k in range(0, 6, 2)]
    ref = hs.finalize_reference((torch.cat([r['summary'] for r in rows]), torch.cat([r['cls_attention'] for r in rows])), labels, 4)
    rel = np.abs(res['block'] - ref) / np.maximum(np.abs(ref), np.finfo(np.float64).tiny)
    rel[ref == res['block']] = 0.0
    assert rel.max() <= 6 * 2.0 ** -52
    assert not res['var'][4].any() and not res['mean'][3].any()                  # one row; no row
    # the class token's maps
    ana = AttentionHeadAnalysis(m, dev())
    maps = ana.cls_maps(x[:2])
    assert maps.shape == (2, 12, 3, 224, 224) and float(maps.min()) >= 0.0 and float(maps.max()) <= 1.0
    assert torch.all(maps.flatten(3).max(-1)[0] > 0.999)
    raw = ana.cls_maps(x[:2], upsample=False)
    assert raw.shape == (2, 12, 3, 14, 14) and torch.equal(raw.reshape(2, 12, 3, 196), out['cls_attention'])
    assert torch.equal(ana.compute(x[:2])['summary'], out['summary'])
    # refusals
    with pytest.raises(RovitHipError):
        m.attention_head_stats(x[:1].cpu())
    with pytest.raises(RovitHipError):
        m.attention_head_stats(loader, per_token=True)
    with pytest.raises(RovitHipError):
        hs.AttentionHeadStats(12, num_classes=4).update_rows(out['summary'].cpu(), out['cls_attention'].cpu(), labels[:2])
