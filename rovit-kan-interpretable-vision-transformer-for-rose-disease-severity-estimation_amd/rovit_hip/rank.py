"""Stable sort and ranks of fp32 columns on the device (``rovit_sort_f32`` / ``rovit_rank_f32``, csrc/sort_rank.hip).

The evaluation score cards rank their columns internally (``EvalAccumulator.rank_method``, ``ood_metrics(..., rank=...)``); this module
gives the same primitive to the user.

Key of a value: the order-preserving uint32 of ``v + 0.0`` (so -0 shares +0's key); every NaN, of either sign and any payload, has the
key 0xFFFFFFFF and sorts behind +inf.  The sorted element is the pair (key, row): (key << 32) | row has no duplicates, so the ascending
order is unique and every correct algorithm, grid and run gives the same bytes.  That is the whole determinism argument.

``rank_columns`` returns, per row i with key k: ``less`` = #{keys < k}, ``eq`` = #{keys == k}, ``before`` = #{j < i : key_j == k} and
``perm``, the row in every sorted slot (row i sits in slot less + before).  A NaN row has less = eq = before = 0 and is counted for no
other row: the values of the counting kernels, where a NaN compares false.  ``method='count'`` counts in O(n^2), ``'sort'`` sorts,
``'auto'`` sorts from ``native.RANK_SORT_ROWS`` rows on; all three give the same words.

Integer outputs are int32 tensors (torch has no general uint32): counts and rows are below 2^20; ``keys_sorted`` holds the uint32 key
bits (``.view(np.uint32)`` on the host).  CPU tensors run the numpy statements below (``sort_reference`` / ``rank_reference``), the
kernels' oracle, as every other module here does.
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch

from . import native
from .native import RovitHipError


# ---- host restatement (exact integers) ---------------------------------------------------------------------------------------------

def sort_keys(x) -> np.ndarray:
    """The uint32 sort key of every fp32 value: see the module docstring."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    b = np.where(b == np.uint32(0x80000000), np.uint32(0), b)                                  # v + 0.0: -0 becomes +0
    k = np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(0x80000000))
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(native.SORT_NAN_KEY), k).astype(np.uint32)


def sort_reference(x) -> Tuple[np.ndarray, np.ndarray]:
    """``(keys_sorted, perm)`` of one column, both uint32: the stable argsort of the keys."""
    k = sort_keys(np.asarray(x).reshape(-1))
    perm = np.argsort(k, kind='stable')
    return k[perm], perm.astype(np.uint32)


def rank_reference(x) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``(less, eq, before, perm)`` of one column, all uint32, by the stable argsort and two searches."""
    k = sort_keys(np.asarray(x).reshape(-1))
    ks, perm = sort_reference(x)
    less = np.searchsorted(ks, k, 'left').astype(np.int64)
    eq = np.searchsorted(ks, k, 'right').astype(np.int64) - less
    slot = np.empty(k.shape[0], dtype=np.int64)
    slot[perm.astype(np.int64)] = np.arange(k.shape[0], dtype=np.int64)
    before = slot - less
    nan = k == np.uint32(native.SORT_NAN_KEY)
    less[nan], eq[nan], before[nan] = 0, 0, 0
    return less.astype(np.uint32), eq.astype(np.uint32), before.astype(np.uint32), perm


# ---- device entry points -------------------------------------------------------------------------------------------------------------

Columns = Union[torch.Tensor, Sequence[torch.Tensor]]


def _columns(x: Columns, what: str) -> Tuple[List[torch.Tensor], object]:
    """The columns as a list of contiguous 1-D fp32 tensors, and the shape to give the outputs (None for a sequence)."""
    if isinstance(x, torch.Tensor):
        if x.dim() not in (1, 2) or x.numel() < 1:
            raise RovitHipError(f'{what}: x must be (n,) or (cols, n) with n >= 1, got {tuple(x.shape)}')
        t = x.detach().float().contiguous()
        cols, shape = ([t] if t.dim() == 1 else list(t.unbind(0))), tuple(t.shape)
    else:
        cols, shape = [c.detach().float().reshape(-1).contiguous() for c in x], None
        if not cols:
            raise RovitHipError(f'{what}: no columns')
    for c in cols:
        if not 1 <= c.shape[0] <= native.EVAL_MAX_ROWS:
            raise RovitHipError(f'{what}: a column has {c.shape[0]} rows (1..{native.EVAL_MAX_ROWS})')
        if c.device != cols[0].device:
            raise RovitHipError(f'{what}: columns on {c.device} and {cols[0].device}')
    return cols, shape


def _shaped(outs: List[Tuple[torch.Tensor, ...]], shape):
    if shape is None:
        return outs
    if len(shape) == 1:
        return outs[0]
    return tuple(torch.stack([o[k] for o in outs]) for k in range(len(outs[0])))


def _from_numpy(arrays) -> Tuple[torch.Tensor, ...]:
    return tuple(torch.from_numpy(a.view(np.int32).copy()) for a in arrays)


def sort_columns(x: Columns, max_workgroups: int = 0):
    """``(keys_sorted, perm)`` int32 tensors shaped like ``x`` ((n,) or (cols, n)); for a sequence of 1-D tensors of individual lengths,
    a list of such pairs.  Up to 16 columns share one call of ``rovit_sort_f32``."""
    cols, shape = _columns(x, 'sort_columns')
    if not cols[0].is_cuda:
        return _shaped([_from_numpy(sort_reference(c.numpy())) for c in cols], shape)
    lib, outs = native.load(), []
    for g in range(0, len(cols), native.SORT_MAX_COLUMNS):
        grp = cols[g:g + native.SORT_MAX_COLUMNS]
        ns = (ctypes.c_int * len(grp))(*[c.shape[0] for c in grp])
        nbytes = lib.rovit_sort_workspace_bytes(ns, len(grp))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=grp[0].device)
        d = native.Sort()
        d.num_columns, d.max_workgroups, d.workspace, d.workspace_bytes = len(grp), max_workgroups, native.ptr(ws), nbytes
        res = []
        for k, c in enumerate(grp):
            keys, perm = torch.empty_like(c, dtype=torch.int32), torch.empty_like(c, dtype=torch.int32)
            d.n[k], d.x[k], d.keys_sorted[k], d.perm[k] = c.shape[0], native.ptr(c), native.ptr(keys), native.ptr(perm)
            res.append((keys, perm))
        native.call('rovit_sort_f32', ctypes.byref(d), native.stream_ptr())
        outs += res
    return _shaped(outs, shape)


def rank_columns(x: Columns, method: str = 'auto', max_workgroups: int = 0):
    """``(less, eq, before, perm)`` int32 tensors shaped like ``x`` ((n,) or (cols, n)); for a sequence of 1-D tensors of individual
    lengths, a list of such tuples.  ``method``: ``'count'``, ``'sort'`` or ``'auto'`` (by the longest column of a call); the outputs do
    not depend on it.  Up to 16 columns share one call of ``rovit_rank_f32``."""
    if method not in native.RANK_METHODS:
        raise RovitHipError(f"rank_columns: method must be one of {sorted(native.RANK_METHODS)}, got {method!r}")
    cols, shape = _columns(x, 'rank_columns')
    if not cols[0].is_cuda:
        return _shaped([_from_numpy(rank_reference(c.numpy())) for c in cols], shape)
    lib, outs = native.load(), []
    for g in range(0, len(cols), native.SORT_MAX_COLUMNS):
        grp = cols[g:g + native.SORT_MAX_COLUMNS]
        ns = (ctypes.c_int * len(grp))(*[c.shape[0] for c in grp])
        nbytes = lib.rovit_rank_workspace_bytes(ns, len(grp), native.RANK_METHODS[method])
        ws = torch.empty(nbytes, dtype=torch.uint8, device=grp[0].device) if nbytes else None
        d = native.Rank()
        d.num_columns, d.method, d.max_workgroups, d.workspace, d.workspace_bytes = len(grp), native.RANK_METHODS[method], max_workgroups, native.ptr(ws), nbytes
        res = []
        for k, c in enumerate(grp):
            o = tuple(torch.empty_like(c, dtype=torch.int32) for _ in range(4))
            d.n[k], d.x[k] = c.shape[0], native.ptr(c)
            d.less[k], d.eq[k], d.before[k], d.perm[k] = (native.ptr(t) for t in o)
            res.append(o)
        native.call('rovit_rank_f32', ctypes.byref(d), native.stream_ptr())
        outs += res
    return _shaped(outs, shape)


def argsort(x: torch.Tensor) -> torch.Tensor:
    """Stable ascending argsort of an (n,) or (cols, n) fp32 tensor along its last dimension as int64, -0 equal to +0 and NaNs last."""
    if not isinstance(x, torch.Tensor):
        raise RovitHipError('argsort: x must be a tensor')
    return sort_columns(x)[1].long()
