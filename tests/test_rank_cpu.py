"""CPU tests of rovit_hip/rank.py: the numpy statements of the sort and of the ranks against the O(n^2) definitions the counting kernels
implement, the CPU path of the public functions, and the accumulator's ``rank_method`` attribute on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rank_cases import CONTENTS, CPU_SIZES, NEG_NAN, TILE, brute_force_ranks, column, u32  # noqa: E402
from selective_cases import feed, make_data  # noqa: E402


def test_constants_mirror_the_header():
    from rovit_hip import native
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rovit_hip.h')).read()
    assert f'#define ROVIT_SORT_TILE {native.SORT_TILE}\n' in txt and native.SORT_TILE == TILE
    assert f'#define ROVIT_SORT_MAX_COLUMNS {native.SORT_MAX_COLUMNS}\n' in txt
    assert 'enum { ROVIT_RANK_AUTO = 0, ROVIT_RANK_COUNT = 1, ROVIT_RANK_SORT = 2 };' in txt
    assert (native.RANK_AUTO, native.RANK_COUNT, native.RANK_SORT) == (0, 1, 2)
    value = txt.split('#define ROVIT_RANK_SORT_ROWS ')[1].split('/*')[0].strip()
    assert eval(value, {}) == native.RANK_SORT_ROWS          # an integer expression of the header
    assert native.rank_method('auto', native.RANK_SORT_ROWS - 1) == native.RANK_COUNT
    assert native.rank_method('auto', native.RANK_SORT_ROWS) == native.RANK_SORT
    assert native.rank_method('sort', 1) == native.RANK_SORT and native.rank_method('count', 1 << 20) == native.RANK_COUNT
    with pytest.raises(native.RovitHipError):
        native.rank_method('fast', 10)


def test_keys_order_the_numbers_and_put_every_nan_last():
    from rovit_hip.rank import sort_keys
    vals = np.array([-np.inf, -3.4e38, -1.5, -1e-45, -0.0, 0.0, 1e-45, 1.5, 3.4e38, np.inf], dtype=np.float32)
    k = sort_keys(vals)
    assert k[4] == k[5] == 0x80000000
    assert np.all(np.diff(np.delete(k, 4).astype(np.int64)) > 0)
    nans = np.array([0x7FC00000, NEG_NAN, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    assert np.all(sort_keys(nans) == 0xFFFFFFFF) and k.max() < 0xFFFFFFFF


@pytest.mark.parametrize('content', sorted(CONTENTS))
def test_rank_reference_equals_the_quadratic_definitions(content):
    from rovit_hip.rank import rank_reference, sort_keys, sort_reference
    for n in CPU_SIZES:
        x = column(content, n)
        less, eq, before, perm = rank_reference(x)
        bl, be, bb = brute_force_ranks(x)
        what = f'{content} n={n}'
        assert np.array_equal(less, bl) and np.array_equal(eq, be) and np.array_equal(before, bb), what
        assert sorted(perm.tolist()) == list(range(n)), what
        num = ~np.isnan(x)
        assert np.array_equal(perm[(bl + bb)[num]], np.arange(n)[num]), what          # row i sits in slot less + before
        assert np.array_equal(perm[num.sum():], np.arange(n)[~num]), what              # NaN rows last, in row order
        ks, p2 = sort_reference(x)
        assert np.array_equal(p2, perm) and np.array_equal(ks, sort_keys(x)[perm]) and np.all(np.diff(ks.astype(np.int64)) >= 0), what


def test_public_functions_on_cpu_tensors_run_the_reference():
    from rovit_hip.rank import argsort, rank_columns, rank_reference, sort_columns, sort_keys
    cols = [column(c, n) for c, n in (('nans', 257), ('two_decimals', 300), ('specials', 255))]
    for x in cols:
        t = torch.from_numpy(x)
        assert np.array_equal(argsort(t).numpy(), np.argsort(sort_keys(x), kind='stable'))
        for method in ('auto', 'count', 'sort'):
            out = rank_columns(t, method=method)
            for got, want in zip(out, rank_reference(x)):
                assert got.dtype == torch.int32 and np.array_equal(u32(got), want)
    m = torch.from_numpy(np.stack([column('two_decimals', 300, seed=s) for s in range(3)]))
    less, eq, before, perm = rank_columns(m)
    assert less.shape == perm.shape == (3, 300)
    assert np.array_equal(u32(perm[2]), rank_reference(m[2].numpy())[3])
    assert np.array_equal(argsort(m).numpy(), np.argsort(sort_keys(m.numpy()), axis=1, kind='stable'))
    outs = sort_columns([torch.from_numpy(x) for x in cols])
    assert [o[0].shape[0] for o in outs] == [257, 300, 255]
    from rovit_hip import RovitHipError
    with pytest.raises(RovitHipError):
        rank_columns(m, method='radix')
    with pytest.raises(RovitHipError):
        rank_columns(torch.zeros(2, 3, 4))


def test_eval_accumulator_on_the_cpu_is_unchanged_by_rank_method():
    from rovit_hip.evaluation import EvalAccumulator, result_block_from_arrays
    d = make_data(300, 4, seed=5, ties=True)
    blocks, sels = [], []
    for method in ('auto', 'count', 'sort'):
        acc = EvalAccumulator(4)
        assert acc.rank_method == 'auto'
        acc.rank_method = method
        feed(acc, d, sizes=(64, 7))
        blocks.append(acc.result_block())
        sels.append(acc.selective(return_keys=True)['block'])
    a = acc._cpu_arrays()
    want = result_block_from_arrays(a['label'], a['pred'], a['probs'], a['sev_true'], a['sev_pred'], 4, 10, None)
    for b, s in zip(blocks, sels):
        assert np.array_equal(b, want) and np.array_equal(s, sels[0])


def test_ood_reference_on_cpu_tensors_takes_the_rank_argument():
    from rovit_hip import RovitHipError
    from rovit_hip.density import ood_block, ood_block_reference, ood_metrics
    a, b = torch.from_numpy(column('two_decimals', 257)), torch.from_numpy(column('two_decimals', 300, seed=1) + 0.5)
    for rank in ('auto', 'count', 'sort'):
        assert np.array_equal(ood_block(a, b, (0.5, 0.95), rank=rank), ood_block_reference(a, b, (0.5, 0.95)))
    assert ood_metrics(a, b, rank='sort') == ood_metrics(a, b)
    with pytest.raises(RovitHipError):
        ood_block(a, b, rank='quick')
