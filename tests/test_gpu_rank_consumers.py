"""GPU tests of the three score cards behind the sorted rank (rovit_eval_finalize_ex, rovit_eval_selective_ex, rovit_ood_metrics_ex):
``rank_method='sort'`` against ``'count'`` on the same rows.  Only the rank step differs and it fills the same integer words, so every
comparison is byte for byte; the old entry points, called directly through ctypes, still give the block they gave before."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rank_cases import WIDE, add_wide_columns, column  # noqa: E402
from selective_cases import feed, make_data  # noqa: E402

pytestmark = pytest.mark.gpu

FINAL_SIZES = (1, 257, 1025, 5000)


def dev():
    return torch.device('cuda:0')


def _acc(d, method, extra=('mu',), sizes=(1 << 30,)):
    from rovit_hip.evaluation import EvalAccumulator
    acc = EvalAccumulator(4)
    acc.rank_method = method
    return feed(acc, d, sizes=sizes, device=dev(), extra=extra)


def _nonfinite_data(n):
    d = make_data(n, 4, seed=77, ties=True)
    d['sev_true'] = d['sev_true'].float()
    d['sev_true'][5], d['sev_true'][n - 1] = float('nan'), float('inf')
    d['sev_pred'][0], d['sev_pred'][7], d['sev_pred'][n // 2] = float('-inf'), float('nan'), -0.0
    return d


@pytest.mark.parametrize('n', FINAL_SIZES)
def test_finalise_block_rank_counts_and_bootstrap_are_byte_identical(n):
    d = make_data(n, 4, seed=100 + n, ties=True)
    a, b = _acc(d, 'count'), _acc(d, 'sort', sizes=(97, 31))
    assert np.array_equal(a.result_block(), b.result_block())
    assert torch.equal(a._rank_counts, b._rank_counts)
    ta = a.bootstrap(num_resamples=16, seed=3, return_table=True, return_blocks=True)
    tb = b.bootstrap(num_resamples=16, seed=3, return_table=True, return_blocks=True)
    assert np.array_equal(ta['table'].view(np.int64), tb['table'].view(np.int64)) and np.array_equal(ta['blocks'], tb['blocks'])
    from rovit_hip import native
    from rovit_hip.evaluation import rank_sums
    arr = a.arrays()
    want = rank_sums(arr['severity_true'], arr['severity_pred'])[:3]
    assert [int(v) for v in b.result_block()[native.EVAL_RANK:native.EVAL_RANK + 3]] == list(want)


def test_finalise_with_nan_and_infinite_severities_is_byte_identical():
    from rovit_hip import native
    d = _nonfinite_data(1025)
    a, b = _acc(d, 'count'), _acc(d, 'sort')
    ba, bb = a.result_block(), b.result_block()
    assert np.array_equal(ba, bb) and torch.equal(a._rank_counts, b._rank_counts)
    assert list(ba[native.EVAL_NONFINITE:native.EVAL_NONFINITE + 2]) == [2, 2]
    cnt = b._rank_counts.cpu().numpy().reshape(4, 1025)
    assert cnt[0, 5] == 0 and cnt[1, 5] == 0 and cnt[2, 7] == 0 and cnt[3, 7] == 0          # a NaN row counts nothing
    assert cnt[0, 1024] == 1023 and cnt[2, 0] == 0 and cnt[3, 0] == 1                       # +inf above every number, -inf below


def _selective_pair(d, scores, risks, P, extra):
    blocks = []
    for method in ('count', 'sort'):
        res = _acc(d, method, extra=extra).selective(scores, risks, coverages=P, return_keys=True)
        blocks.append((res['block'], res['keys'], res['risk_values']))
    return blocks


@pytest.mark.parametrize('n', (1, 2, 257, 1025, 2051))
def test_selective_block_of_the_builtin_scores_is_byte_identical(n):
    d = make_data(n, 4, seed=300 + n, ties=True)
    (b0, k0, r0), (b1, k1, r1) = _selective_pair(d, ['confidence', 'entropy', 'sigma'], ['error', 'abs_err'], 20, ('mu',))
    assert np.array_equal(b0, b1) and np.array_equal(k0.view(np.uint32), k1.view(np.uint32)) and np.array_equal(r0, r1)


def test_selective_block_of_the_wide_case_is_byte_identical_for_every_grid():
    n = 257
    d = make_data(n, 4, seed=300 + n, ties=True)
    extra = add_wide_columns(d, n)
    (b0, k0, _), (b1, k1, _) = _selective_pair(d, WIDE[0], WIDE[1], 256, extra)
    assert np.array_equal(b0, b1) and np.array_equal(k0.view(np.uint32), k1.view(np.uint32))
    assert (k0 < 0).any() and (k0.view(np.uint32) == 0x80000000).any()                       # negative keys and -0 are in the case
    acc = _acc(d, 'sort', extra=extra)
    for mw in (1, 7):
        assert np.array_equal(acc.selective(WIDE[0], WIDE[1], coverages=256, return_keys=True, _max_workgroups=mw)['block'], b0)


def test_selective_counters_agree_with_a_nan_key():
    from rovit_hip import RovitHipError, native
    n = 300
    d = make_data(n, 4, seed=9, ties=True)
    d['c1'] = torch.randn(n, generator=torch.Generator().manual_seed(1)).round()
    d['c1'][17] = float('nan')
    messages = []
    for method in ('count', 'sort'):
        acc = _acc(d, method, extra=('c1', 'mu'))
        with pytest.raises(RovitHipError) as err:
            acc.selective(['c1'], ['error'])
        messages.append(str(err.value))
    assert messages[0] == messages[1] and '1' in messages[0] and native.EVAL_SEL_NONFINITE_KEYS == 0


def _ood_cases():
    a = column('two_decimals', 300, seed=1)
    b = (column('two_decimals', 1025, seed=2) + np.float32(0.5)).round(2).astype(np.float32)          # ties across the two sides
    a[3], a[4], b[5], b[6] = 0.0, -0.0, -0.0, 0.0
    yield 'n1_n300', a[:1].copy(), b[:300].copy()
    yield 'n300_n1', a.copy(), b[:1].copy()
    yield 'n257_n1025', a[:257].copy(), b.copy()
    yield 'n1025_n257', b.copy(), a[:257].copy()
    yield 'all_tied', np.full(257, 0.25, np.float32), np.full(300, 0.25, np.float32)
    an, bn = a.copy(), b.copy()
    an[11] = np.float32('nan')
    yield 'nan_in', an, b.copy()
    bn[0], bn[1024] = np.float32('nan'), -np.float32('nan')
    yield 'nan_out', a.copy(), bn
    yield 'inf_both', np.concatenate([a, np.float32([np.inf, -np.inf])]), np.concatenate([b, np.float32([np.inf])])


@pytest.mark.parametrize('name,a,b', list(_ood_cases()), ids=[c[0] for c in _ood_cases()])
def test_ood_block_is_byte_identical(name, a, b):
    from rovit_hip import native
    from rovit_hip.density import ood_block, ood_block_reference
    ta, tb = torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev())
    levels = (0.5, 0.95)
    counted = ood_block(ta, tb, levels, rank='count')
    for mw in (0, 1, 7):
        assert np.array_equal(ood_block(ta, tb, levels, max_workgroups=mw, rank='sort'), counted), f'{name} max_workgroups={mw}'
    if not counted[native.OOD_BAD]:
        ref = ood_block_reference(a, b, levels)
        assert np.array_equal(counted[:native.OOD_AP_OUT_SUM], ref[:native.OOD_AP_OUT_SUM])          # the integer words and the thresholds
    else:
        assert counted[native.OOD_BAD] == int(np.isnan(a).sum() + np.isnan(b).sum() + np.isinf(a).sum() + np.isinf(b).sum())


def test_auto_equals_both_methods_on_each_side_of_the_threshold():
    """Below ROVIT_RANK_SORT_ROWS 'auto' counts, from it on 'auto' sorts: the blocks cannot tell, so all three are compared.  The upper
    side exists only when the threshold is inside the row limit."""
    from rovit_hip import native
    from rovit_hip.density import ood_block
    sizes = [min(native.RANK_SORT_ROWS - 1, 3000)]
    if native.RANK_SORT_ROWS <= native.EVAL_MAX_ROWS:
        sizes.append(native.RANK_SORT_ROWS)
    for n in sizes:
        d = make_data(n, 4, seed=n, ties=True)
        accs = {m: _acc(d, m) for m in ('auto', 'count', 'sort')}
        blocks = {m: acc.result_block() for m, acc in accs.items()}
        sels = {m: acc.selective(return_keys=True)['block'] for m, acc in accs.items()}
        assert np.array_equal(blocks['auto'], blocks['count']) and np.array_equal(blocks['auto'], blocks['sort'])
        assert np.array_equal(sels['auto'], sels['count']) and np.array_equal(sels['auto'], sels['sort'])
        a = torch.from_numpy(column('two_decimals', n // 2, seed=1)).to(dev())
        b = torch.from_numpy(column('two_decimals', n - n // 2, seed=2)).to(dev())
        oods = {m: ood_block(a, b, rank=m) for m in ('auto', 'count', 'sort')}
        assert np.array_equal(oods['auto'], oods['count']) and np.array_equal(oods['auto'], oods['sort'])


def test_old_entry_points_called_directly_give_the_counted_blocks():
    """rovit_eval_finalize, rovit_eval_selective and rovit_ood_metrics still exist with their argument lists; through ctypes, with the
    descriptors the Python layer builds, they give the blocks of the 'count' method."""
    from rovit_hip import native
    from rovit_hip.density import ood_block
    from rovit_hip.evaluation import SELECTIVE_RISKS, SELECTIVE_SCORES, bin_edges
    lib = native.load()
    n = 1025
    d = make_data(n, 4, seed=41, ties=True)
    acc = _acc(d, 'count')
    want = acc.result_block()
    edges = torch.from_numpy(bin_edges(10)).to(dev())
    counts = torch.empty(4 * n, dtype=torch.int32, device=dev())
    partials = torch.empty(lib.rovit_eval_partials_doubles(n), dtype=torch.float64, device=dev())
    result = torch.empty(native.EVAL_RESULT_WORDS, dtype=torch.int64, device=dev())
    f = native.EvalFinal()
    f.n, f.num_classes, f.n_bins, f.n_loss_rows = n, 4, 10, 0
    for k in ('probs', 'pred', 'label', 'sev_pred', 'sev_true'):
        setattr(f, k, native.ptr(acc._rec[k]))
    f.bin_edges, f.rank_counts, f.partials, f.result = (native.ptr(t) for t in (edges, counts, partials, result))
    native.call('rovit_eval_finalize', ctypes.byref(f), native.stream_ptr())
    assert np.array_equal(result.cpu().numpy(), want) and torch.equal(counts, acc._rank_counts)

    scores, risks, P = ['confidence', 'entropy', 'sigma'], ['error', 'abs_err'], 20
    want_sel = acc.selective(scores, risks, coverages=P, return_keys=True)['block']
    W = native.eval_selective_offsets(3, 2, P)['words']
    out = torch.empty(W, dtype=torch.int64, device=dev())
    nbytes = lib.rovit_eval_selective_workspace_bytes(n, 3, 2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    s = native.EvalSel()
    s.n, s.num_classes, s.num_scores, s.num_risks, s.num_coverages, s.max_workgroups = n, 4, 3, 2, P, 0
    for i, name in enumerate(scores):
        s.score_kind[i] = SELECTIVE_SCORES[name]
    for i, name in enumerate(risks):
        s.risk_kind[i] = SELECTIVE_RISKS[name]
    for k, _ in acc._FIELDS:
        setattr(s, k, native.ptr(acc._rec[k]))
    s.workspace, s.workspace_bytes, s.result = native.ptr(ws), nbytes, native.ptr(out)
    native.call('rovit_eval_selective', ctypes.byref(s), native.stream_ptr())
    assert np.array_equal(out.cpu().numpy(), want_sel)

    a = torch.from_numpy(column('two_decimals', 257, seed=1)).to(dev())
    b = torch.from_numpy(column('two_decimals', 1025, seed=2)).to(dev())
    want_ood = ood_block(a, b, (0.5, 0.95), rank='count')
    nbytes = lib.rovit_ood_metrics_workspace_bytes(257, 1025)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    res = torch.empty(native.OOD_WORDS, dtype=torch.int64, device=dev())
    o = native.Ood()
    o.n_in, o.n_out, o.num_levels, o.max_workgroups = 257, 1025, 2, 0
    o.tpr_levels[0], o.tpr_levels[1] = 0.5, 0.95
    o.scores_in, o.scores_out, o.workspace, o.workspace_bytes, o.result = native.ptr(a), native.ptr(b), native.ptr(ws), nbytes, native.ptr(res)
    native.call('rovit_ood_metrics', ctypes.byref(o), native.stream_ptr())
    assert np.array_equal(res.cpu().numpy(), want_ood)


def test_ex_entry_points_refuse_a_bad_method_or_rank_workspace():
    from rovit_hip import native
    lib = native.load()
    n = 300
    assert lib.rovit_eval_finalize_rank_workspace_bytes(0) == 0 and lib.rovit_eval_finalize_rank_workspace_bytes(n) > 0
    assert lib.rovit_eval_selective_rank_workspace_bytes(n, 9, 2) == 0 and lib.rovit_eval_selective_rank_workspace_bytes(n, 3, 2) > 0
    assert lib.rovit_ood_metrics_rank_workspace_bytes(0, 5) == 0 and lib.rovit_ood_metrics_rank_workspace_bytes(n, 5) > 0
    a = torch.from_numpy(column('two_decimals', n)).to(dev())
    nbytes = lib.rovit_ood_metrics_workspace_bytes(n, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    rbytes = lib.rovit_ood_metrics_rank_workspace_bytes(n, n)
    rws = torch.empty(rbytes + 16, dtype=torch.uint8, device=dev())
    res = torch.empty(native.OOD_WORDS, dtype=torch.int64, device=dev())
    o = native.Ood()
    o.n_in, o.n_out, o.num_levels, o.max_workgroups = n, n, 0, 0
    o.scores_in, o.scores_out, o.workspace, o.workspace_bytes, o.result = native.ptr(a), native.ptr(a), native.ptr(ws), nbytes, native.ptr(res)
    call = lambda method, p, size: lib.rovit_ood_metrics_ex(ctypes.byref(o), method, p, size, native.stream_ptr())
    assert call(3, rws.data_ptr(), rbytes) != 0 and call(-1, rws.data_ptr(), rbytes) != 0
    assert call(native.RANK_SORT, None, rbytes) != 0
    assert call(native.RANK_SORT, rws.data_ptr() + 4, rbytes) != 0
    assert call(native.RANK_SORT, rws.data_ptr(), rbytes - 1) != 0
    assert call(native.RANK_COUNT, None, 0) == 0 and call(native.RANK_SORT, rws.data_ptr(), rbytes) == 0
    torch.cuda.synchronize()
