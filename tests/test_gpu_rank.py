"""GPU tests of the device radix sort and the rank entry points (csrc/sort_rank.hip, rovit_hip/rank.py).  Every comparison is exact:
``np.array_equal`` on the integer words, against the numpy statements ``sort_reference`` / ``rank_reference`` and between the methods.

The order of the (key, row) pairs is unique, so there is no tolerance anywhere.  Ties dominate the contents because an LSD pass that is
not stable is wrong only with ties."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rank_cases import CONTENTS, SIZES, TILE, column, u32  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def _check_sort(got, x, what):
    from rovit_hip.rank import sort_reference
    keys, perm = sort_reference(x)
    assert np.array_equal(u32(got[0]), keys), f'{what}: keys_sorted'
    assert np.array_equal(u32(got[1]), perm), f'{what}: perm'


def _check_rank(got, x, what, with_perm=True):
    from rovit_hip.rank import rank_reference
    for name, g, want in zip(('less', 'eq', 'before', 'perm'), got, rank_reference(x)):
        if name != 'perm' or with_perm:
            assert np.array_equal(u32(g), want), f'{what}: {name}'


@pytest.mark.parametrize('content', sorted(CONTENTS))
def test_sort_and_ranks_equal_the_reference_at_every_size(content):
    """All sizes of one content as ONE batched call per entry point (ten columns of different lengths), sort and both rank methods."""
    from rovit_hip import native
    from rovit_hip.rank import rank_columns, sort_columns
    assert native.SORT_TILE == TILE
    xs = [column(content, n) for n in SIZES]
    ts = [torch.from_numpy(x).to(dev()) for x in xs]
    sorts = sort_columns(ts)
    by_sort = rank_columns(ts, method='sort')
    by_count = rank_columns(ts, method='count')
    for x, s, rs, rc in zip(xs, sorts, by_sort, by_count):
        what = f'{content} n={len(x)}'
        _check_sort(s, x, what)
        _check_rank(rs, x, what + ' (sort)')
        _check_rank(rc, x, what + ' (count)')
        for a, b in zip(rs, rc):
            assert np.array_equal(u32(a), u32(b)), what + ': sort against count'


def test_single_columns_grids_and_reruns_give_the_same_bytes():
    """max_workgroups in {0, 1, 7}, a second run, and a (cols, n) matrix against its rows one by one."""
    from rovit_hip.rank import rank_columns, sort_columns
    for content, n in (('two_decimals', 2 * TILE + 1), ('nans', TILE + 1), ('two_values', 257), ('byte3', 3 * TILE + 5)):
        x = column(content, n, seed=3)
        t = torch.from_numpy(x).to(dev())
        base_sort, base_rank = sort_columns(t), rank_columns(t, method='sort')
        _check_sort(base_sort, x, f'{content} n={n}')
        _check_rank(base_rank, x, f'{content} n={n}')
        for mw in (0, 1, 7):
            what = f'{content} n={n} max_workgroups={mw}'
            for a, b in zip(sort_columns(t, max_workgroups=mw), base_sort):
                assert np.array_equal(u32(a), u32(b)), what
            for a, b in zip(rank_columns(t, method='sort', max_workgroups=mw), base_rank):
                assert np.array_equal(u32(a), u32(b)), what
            for a, b in zip(rank_columns(t, method='count', max_workgroups=mw), base_rank):
                assert np.array_equal(u32(a), u32(b)), what + ' (count)'
    m = torch.from_numpy(np.stack([column('two_decimals', 1000, seed=s) for s in range(3)])).to(dev())
    whole = rank_columns(m, method='sort')
    for r in range(3):
        for a, b in zip(whole, rank_columns(m[r], method='sort')):
            assert np.array_equal(u32(a[r]), u32(b))


def test_a_batch_of_twelve_columns_equals_the_columns_one_by_one():
    from rovit_hip.rank import rank_columns, sort_columns
    names = sorted(CONTENTS)
    sizes = (1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5000, 3, 12345)
    xs = [column(names[k % len(names)], n, seed=9) for k, n in enumerate(sizes)]
    ts = [torch.from_numpy(x).to(dev()) for x in xs]
    batch_sort, batch_rank = sort_columns(ts), rank_columns(ts, method='sort')
    for t, x, bs, br in zip(ts, xs, batch_sort, batch_rank):
        what = f'n={len(x)}'
        _check_sort(bs, x, what)
        for a, b in zip(sort_columns(t), bs):
            assert np.array_equal(u32(a), u32(b)), what
        for a, b in zip(rank_columns(t, method='sort'), br):
            assert np.array_equal(u32(a), u32(b)), what


def test_a_million_rows_against_numpy():
    """Once at the row limit, the sort only: 512 tiles, the scan's two tiles per thread, every digit of every pass in use."""
    from rovit_hip.rank import argsort, sort_columns
    rng = np.random.default_rng(20)
    x = (rng.standard_normal(1 << 20) * 100).round(1).astype(np.float32)
    x[::4099] = np.float32('nan')
    x[1::5003] = -np.float32(0.0)
    t = torch.from_numpy(x).to(dev())
    _check_sort(sort_columns(t), x, 'n=2^20')
    assert argsort(t).dtype == torch.int64


def test_argsort_is_stable_with_nans_last():
    from rovit_hip.rank import argsort, sort_keys
    x = column('nans', 4097, seed=1)
    got = argsort(torch.from_numpy(x).to(dev())).cpu().numpy()
    assert np.array_equal(got, np.argsort(sort_keys(x), kind='stable'))
    nan_rows = np.flatnonzero(np.isnan(x))
    assert np.array_equal(got[-len(nan_rows):], nan_rows)


def test_bad_descriptors_are_refused_before_any_launch():
    from rovit_hip import native
    lib = native.load()
    n = 300
    x = torch.zeros(n, device=dev())
    outs = [torch.empty(n, dtype=torch.int32, device=dev()) for _ in range(4)]
    ns = (ctypes.c_int * 1)(n)
    nbytes = lib.rovit_sort_workspace_bytes(ns, 1)
    assert nbytes > 0 and lib.rovit_sort_workspace_bytes(ns, 0) == 0 and lib.rovit_sort_workspace_bytes(ns, 17) == 0
    assert lib.rovit_sort_workspace_bytes((ctypes.c_int * 1)(0), 1) == 0 and lib.rovit_sort_workspace_bytes((ctypes.c_int * 1)((1 << 20) + 1), 1) == 0
    assert lib.rovit_rank_workspace_bytes(ns, 1, native.RANK_COUNT) == 0 and lib.rovit_rank_workspace_bytes(ns, 1, native.RANK_SORT) > nbytes
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev())

    def sort_desc():
        d = native.Sort()
        d.num_columns, d.max_workgroups, d.workspace, d.workspace_bytes = 1, 0, ws.data_ptr(), nbytes
        d.n[0], d.x[0], d.keys_sorted[0], d.perm[0] = n, x.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr()
        return d

    def refused(d, fn=lib.rovit_sort_f32):
        rc = fn(ctypes.byref(d), native.stream_ptr())
        assert rc != 0 and lib.rovit_last_error_string()
        return rc

    d = sort_desc(); d.num_columns = 0; refused(d)
    d = sort_desc(); d.num_columns = 17; refused(d)
    d = sort_desc(); d.n[0] = 0; refused(d)
    d = sort_desc(); d.n[0] = (1 << 20) + 1; refused(d)
    d = sort_desc(); d.x[0] = None; refused(d)
    d = sort_desc(); d.perm[0] = None; refused(d)
    d = sort_desc(); d.keys_sorted[0] = outs[0].data_ptr() + 2; refused(d)
    d = sort_desc(); d.workspace = None; refused(d)
    d = sort_desc(); d.workspace = ws.data_ptr() + 4; refused(d)
    d = sort_desc(); d.workspace_bytes = nbytes - 1; refused(d)
    d = sort_desc(); d.max_workgroups = -1; refused(d)
    assert lib.rovit_sort_f32(None, native.stream_ptr()) != 0

    def rank_desc(method):
        d = native.Rank()
        d.num_columns, d.method, d.max_workgroups = 1, method, 0
        d.n[0], d.x[0] = n, x.data_ptr()
        d.less[0], d.eq[0], d.before[0], d.perm[0] = (t.data_ptr() for t in outs)
        return d

    d = rank_desc(3); refused(d, lib.rovit_rank_f32)
    d = rank_desc(native.RANK_SORT); refused(d, lib.rovit_rank_f32)                      # no workspace
    d = rank_desc(native.RANK_COUNT); d.before[0] = None; refused(d, lib.rovit_rank_f32)
    d = rank_desc(native.RANK_COUNT); d.n[0] = 0; refused(d, lib.rovit_rank_f32)
    torch.cuda.synchronize()
    native.call('rovit_sort_f32', ctypes.byref(sort_desc()), native.stream_ptr())          # the good descriptor goes through
    native.call('rovit_rank_f32', ctypes.byref(rank_desc(native.RANK_COUNT)), native.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(u32(outs[3]), np.arange(n, dtype=np.uint32))                    # all equal: the stable order is the row order
