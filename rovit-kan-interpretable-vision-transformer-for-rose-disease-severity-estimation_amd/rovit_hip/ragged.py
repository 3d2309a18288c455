"""Ragged batches of the token-gather forward: sequences of different lengths in one backbone call (rovit_vit_forward_ragged).

``perturbation='drop'`` removes tokens, so the sequences of one explanation come in up to 197 lengths.  rovit_vit_forward_tokens takes one
length per call; here the sequences of a call are packed back to back in one row space, longest first (the attention grid is issued in
that order, so the long items start first), and a call holds as many as fit ``max_rows`` rows.  The lengths are known on the host in
both callers (perturbation.step_counts, shap._drop_layout): nothing is read back from the device."""
import numpy as np
import torch

from .native import RovitHipError, call, load, ptr, stream_ptr

MAX_TOKENS = 197


def ragged_layout(lengths, max_rows: int):
    """The calls that evaluate sequences of ``lengths`` (host array of ints in [1, 197]) within ``max_rows`` rows each.

    The sequences are taken longest first (ties in the caller's order) and a call is closed when the next sequence would pass
    ``max_rows``.  Returns ``(calls, perm)``: ``calls`` a list of ``(seq, offsets)`` -- ``seq`` (n,) int64 the caller's indices of the
    call's sequences in packed order, ``offsets`` (n + 1,) int32 their row offsets from 0 -- and ``perm`` (N,) int64 with
    ``concat(features of the calls)[perm]`` in the caller's order."""
    what = 'ragged_layout'
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda:
            raise RovitHipError(f'{what}: lengths must be a host array (nothing is read back from the device)')
        lengths = lengths.numpy()
    arr = np.asarray(lengths)
    if arr.ndim != 1 or arr.size == 0 or arr.dtype.kind not in 'iu':
        raise RovitHipError(f'{what}: lengths must be a non-empty 1-D integer array, got shape {arr.shape} of {arr.dtype}')
    arr = arr.astype(np.int64)
    if arr.min() < 1 or arr.max() > MAX_TOKENS:
        raise RovitHipError(f'{what}: every length must be in [1, {MAX_TOKENS}], got [{int(arr.min())}, {int(arr.max())}]')
    if isinstance(max_rows, bool) or not isinstance(max_rows, (int, np.integer)) or max_rows < MAX_TOKENS:
        raise RovitHipError(f'{what}: max_rows must be an int >= {MAX_TOKENS} (one full sequence), got {max_rows!r}')
    order = np.argsort(-arr, kind='stable')
    ends = np.cumsum(arr[order])
    calls, i0, base = [], 0, 0
    while i0 < len(order):
        i1 = int(np.searchsorted(ends, base + int(max_rows), side='right'))          # the first sequence that would pass max_rows
        seq = order[i0:i1]
        off = np.concatenate([[0], ends[i0:i1] - base]).astype(np.int32)
        calls.append((seq, off))
        base, i0 = int(ends[i1 - 1]), i1
    perm = np.empty(len(order), dtype=np.int64)
    perm[order] = np.arange(len(order))
    return calls, perm


def packed_rows(offsets: np.ndarray, dev):
    """Device index tensors of one call: ``(offsets (n + 1,) int32, seq_of_row (rows,) int64, pos_in_seq (rows,) int64)``; sizes from the
    host copy, so no device value is read."""
    off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int32)).pin_memory().to(dev, non_blocking=True)
    total = int(offsets[-1])
    lens = (off[1:] - off[:-1]).long()
    seq_of_row = torch.repeat_interleave(torch.arange(len(offsets) - 1, device=dev), lens, output_size=total)
    pos = torch.arange(total, device=dev) - off[:-1].long()[seq_of_row]
    return off, seq_of_row, pos


def take_ws(eng, max_rows: int, dev) -> torch.Tensor:
    """An inference workspace of ``max_rows`` rows from the engine's pool (give it back with ``eng.give_ws(max_rows, 'ragged', ws)``)."""
    pool = eng._ws_pool.setdefault((max_rows, 'ragged', str(dev)), [])
    if pool:
        return pool.pop()
    nbytes = load().rovit_vit_ragged_workspace_bytes(max_rows, eng.depth)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def forward_ragged(bb, img_tokens, base_tokens, base_shared, seq_img, src, offsets_dev, offsets_host, ws, mlp_path):
    """Inference features (n,192) of the n packed sequences (``_Backbone.forward_ragged``).  seq_img (n,) int32 and src (rows,) int32 on
    the device; offsets_dev (n + 1,) int32 on the device and offsets_host the same numbers as a host int32 array; ws: a workspace of
    at least offsets_host[-1] rows (take_ws)."""
    host = np.ascontiguousarray(offsets_host, dtype=np.int32)
    n = len(host) - 1
    if n < 1 or offsets_dev.numel() != n + 1 or seq_img.numel() != n or offsets_dev.dtype != torch.int32:
        raise RovitHipError(f'forward_ragged: {n} sequences need n + 1 int32 offsets on the device and n image indices')
    total = int(host[-1])
    if src.numel() != total or src.dtype != torch.int32 or seq_img.dtype != torch.int32:
        raise RovitHipError(f'forward_ragged: src must hold one int32 per packed row ({total}), got {src.numel()} of {src.dtype}')
    need = load().rovit_vit_ragged_workspace_bytes(max(total, 1), bb.vit.depth)
    if ws.numel() * ws.element_size() < need:
        raise RovitHipError(f'forward_ragged: {total} rows are beyond the workspace ({ws.numel() * ws.element_size()} bytes, {need} needed)')
    feats = torch.empty(n, 192, device=bb.dev, dtype=torch.float32)
    call('rovit_vit_forward_ragged', ptr(img_tokens), ptr(base_tokens), img_tokens.shape[0], int(base_shared), ptr(seq_img), ptr(src),
         ptr(offsets_dev), host.ctypes.data, bb.pa, ptr(bb.eng.prep), ptr(ws), ptr(feats), n, bb.vit.depth, int(mlp_path), stream_ptr())
    return feats
