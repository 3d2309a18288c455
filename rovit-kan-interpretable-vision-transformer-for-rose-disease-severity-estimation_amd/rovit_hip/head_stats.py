"""Per-head attention statistics on the GPU (csrc/head_stats.hip): entropy, mean attention distance, class-token mass, self mass, row
maximum and 3x3 locality of every (image, block, head), and the class token's own attention row, reduced inside the fused forward
without storing a 197x197 matrix.

Definitions.  P is the 197x197 softmax of one (image, block, head); token 0 is the class token; patch t >= 1 sits at grid cell
(r, c) = divmod(t - 1, 14); dist(i, j) = 16 sqrt((r_i - r_j)^2 + (c_i - c_j)^2) pixels; 0 ln 0 = 0.  Per query row i (``per_token[..., i, :]``):

  H_i = -sum_j P_ij ln P_ij (nats)       D_i = sum_{j>=1} P_ij dist(i, j) / sum_{j>=1} P_ij for i >= 1, D_0 = 0
  C_i = P_i0                             M_i = max_j P_ij

(D_i is also 0 where the patch keys' mass underflowed to 0: the ratio has no value there.)  ``summary[..., k]``, k as in ``STAT_NAMES``:
mean H_i over the 197 queries; mean D_i, mean C_i over the 196 patch queries; mean P_ii over the 197 queries; H_0; P_00; mean M_i over
the 197 queries; mean over the patch queries of sum P_ij over the patch keys within Chebyshev grid distance 1 of i (self included, not
renormalised).  ``cls_attention[..., j - 1]`` = P_0j, j = 1..196.

``head_stats_reference`` and ``finalize_reference`` are the numpy fp64 statements of the kernels; they need no GPU.  Out of scope: masking
or pruning heads, and the fp32 engine (the statistics describe the bf16 engine's probabilities, as ``get_attention_probabilities`` does).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import native
from .native import RovitHipError, call, ptr, ptr_array, stream_ptr

STAT_NAMES = ('entropy', 'distance', 'cls_mass', 'self_mass', 'cls_entropy', 'cls_self_mass', 'max_prob', 'locality')
TOKEN_STAT_NAMES = ('entropy', 'distance', 'cls_mass', 'max_prob')
TOKENS, PATCHES, GRID, HEADS, NSTAT = 197, 196, 14, 3, 8
# scales of the statistics (what an error is measured against): ln 197 for entropies, the grid's diagonal in pixels for distances, 1 for masses
ENTROPY_SCALE, DISTANCE_SCALE = float(np.log(197.0)), float(16.0 * np.sqrt(338.0))
STAT_SCALES = (ENTROPY_SCALE, DISTANCE_SCALE, 1.0, 1.0, ENTROPY_SCALE, 1.0, 1.0, 1.0)
TOKEN_STAT_SCALES = (ENTROPY_SCALE, DISTANCE_SCALE, 1.0, 1.0)


# ---- host restatement (fp64) ---------------------------------------------------------------------------------------------------------

def patch_distances() -> np.ndarray:
    """(196, 196) fp64 pixel distances between patch centres."""
    r, c = np.divmod(np.arange(PATCHES), GRID)
    return 16.0 * np.sqrt((r[:, None] - r[None, :]) ** 2.0 + (c[:, None] - c[None, :]) ** 2.0)


def patch_neighbours() -> np.ndarray:
    """(196, 196) bool: Chebyshev grid distance <= 1, self included."""
    r, c = np.divmod(np.arange(PATCHES), GRID)
    return (np.abs(r[:, None] - r[None, :]) <= 1) & (np.abs(c[:, None] - c[None, :]) <= 1)


def head_stats_reference(probs: Sequence) -> Dict[str, np.ndarray]:
    """``summary`` (B, L, 3, 8), ``cls_attention`` (B, L, 3, 196) and ``per_token`` (B, L, 3, 197, 4) in fp64 from a list of L
    (B, heads, 197, 197) probability arrays or tensors (``get_attention_probabilities``)."""
    dist, near = patch_distances(), patch_neighbours().astype(np.float64)
    summ, cls, tok = [], [], []
    for p in probs:
        P = np.asarray(p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p, dtype=np.float64)
        if P.ndim != 4 or P.shape[2:] != (TOKENS, TOKENS):
            raise RovitHipError(f'head_stats_reference: probabilities must be (B, heads, 197, 197), got {P.shape}')
        with np.errstate(divide='ignore', invalid='ignore'):
            ent = -np.where(P > 0, P * np.log(np.where(P > 0, P, 1.0)), 0.0).sum(-1)                     # (B, h, 197)
            pp = P[:, :, 1:, 1:]
            mass = pp.sum(-1)
            d = np.where(mass > 0, (pp * dist).sum(-1) / np.where(mass > 0, mass, 1.0), 0.0)
        D = np.concatenate([np.zeros_like(ent[..., :1]), d], axis=-1)
        C, M = P[..., 0], P.max(-1)
        diag = np.diagonal(P, axis1=-2, axis2=-1)
        s = np.stack([ent.mean(-1), d.mean(-1), C[..., 1:].mean(-1), diag.mean(-1), ent[..., 0], P[..., 0, 0], M.mean(-1),
                      (pp * near).sum(-1).mean(-1)], axis=-1)
        summ.append(s)
        cls.append(P[:, :, 0, 1:])
        tok.append(np.stack([ent, D, C, M], axis=-1))
    return {'summary': np.stack(summ, 1), 'cls_attention': np.stack(cls, 1), 'per_token': np.stack(tok, 1)}


def _as_rows(a, n: Optional[int] = None) -> np.ndarray:
    a = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.reshape(a.shape[0] if n is None else n, -1)


def block_layout(depth: int, heads: int, num_classes: int):
    R, Q = depth * heads * NSTAT, depth * heads * PATCHES
    return R, Q, 1 + 2 * R + Q, num_classes + 1


def result_from_block(block: np.ndarray, depth: int, heads: int, num_classes: int) -> Dict:
    """The finalise kernel's block as arrays per group: group 0 is every row, group 1 + c the rows labelled c."""
    R, Q, stride, G = block_layout(depth, heads, num_classes)
    b = np.asarray(block, dtype=np.float64).reshape(G, stride)
    return {'groups': ['all'] + list(range(num_classes)), 'count': b[:, 0].astype(np.int64),
            'mean': b[:, 1:1 + R].reshape(G, depth, heads, NSTAT), 'var': b[:, 1 + R:1 + 2 * R].reshape(G, depth, heads, NSTAT),
            'cls_attention_mean': b[:, 1 + 2 * R:].reshape(G, depth, heads, PATCHES), 'stat_names': STAT_NAMES, 'block': b.reshape(-1)}


def finalize_reference(rows, labels, C: Optional[int]) -> np.ndarray:
    """The block ``rovit_head_stats_finalize`` writes, in fp64 on the host: ``rows`` = (summary (n, ...), cls_attention (n, ...)) fp32,
    ``labels`` (n) integers or None, ``C`` classes (None or 0: the group of every row alone).  Per group [count, mean, unbiased variance,
    mean cls_attention]; sums walk the rows in storage order, two passes (mean, then squared deviations); an empty group gives zeros,
    a group of one row variance 0."""
    summary, cls = rows
    summary = _as_rows(summary)
    n = summary.shape[0]
    x = np.concatenate([summary, _as_rows(cls, n)], axis=1).astype(np.float64)
    R, C = summary.shape[1], int(C or 0)
    lab = None if labels is None else _as_rows(labels, n)[:, 0].astype(np.int64)
    if C and lab is None:
        raise RovitHipError('finalize_reference: classes without labels')
    out = []
    for g in range(C + 1):
        xs = x if g == 0 else x[lab == g - 1]
        cnt = xs.shape[0]
        s = np.zeros(x.shape[1])
        for row in xs:
            s = s + row
        mean = s / cnt if cnt else s
        ss = np.zeros(R)
        for row in xs:
            d = row[:R] - mean[:R]
            ss = ss + d * d
        var = ss / (cnt - 1) if cnt > 1 else np.zeros(R)
        out.append(np.concatenate([[float(cnt)], mean[:R], var, mean[R:]]))
    return np.concatenate(out)


# ---- the device path -----------------------------------------------------------------------------------------------------------------

def _container(model):
    """The DeiTTiny parameter container behind a RoViTKAN, a DeiTTinyBackbone or itself."""
    if hasattr(model, 'backbone'):
        model = model.backbone
    if not hasattr(model, 'engine') and hasattr(model, 'model'):
        model = model.model
    if not hasattr(model, 'engine'):
        raise RovitHipError('attention_head_stats: needs a RoViTKAN, a DeiTTinyBackbone or its DeiTTiny container')
    return model


def _forward(model, x: torch.Tensor, summary: torch.Tensor, cls: torch.Tensor, per_token: Optional[torch.Tensor]) -> torch.Tensor:
    params = model.ordered_parameters()
    eng = model.engine
    eng.prepare(params)
    B = x.shape[0]
    ws = eng.take_ws(B, False, x.device)
    feats = torch.empty(B, 192, device=x.device, dtype=torch.float32)
    with torch.no_grad():
        call('rovit_vit_forward_head_stats', ptr(x), ptr_array(params), ptr(eng.prep), ptr(ws), ptr(feats), ptr(summary), ptr(cls),
             ptr(per_token), B, eng.depth, stream_ptr())
    eng.give_ws(B, False, ws)
    return feats


def _check_images(what: str, x: torch.Tensor) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RovitHipError(f'{what}: the images must be on the GPU (there is no CPU fallback)')
    if x.dim() != 4 or tuple(x.shape[1:]) != (3, 224, 224) or x.shape[0] < 1:
        raise RovitHipError(f'{what}: images must be (B >= 1, 3, 224, 224), got {tuple(x.shape)}')
    return x.float().contiguous()


def attention_head_stats(model, x: torch.Tensor, per_token: bool = False) -> Dict:
    """``summary`` (B, L, 3, 8), ``cls_attention`` (B, L, 3, 196) and, with ``per_token``, ``per_token`` (B, L, 3, 197, 4) fp32 on the
    device, plus ``features`` (B, 192) (the bits ``get_attention_probabilities``' forward gives at the same batch), ``STAT_NAMES`` and
    ``TOKEN_STAT_NAMES``.  One fused forward on the bf16 engine; see the module docstring for the definitions."""
    model = _container(model)
    x = _check_images('attention_head_stats', x)
    B, L = x.shape[0], model.engine.depth
    summary = torch.empty(B, L, HEADS, NSTAT, device=x.device, dtype=torch.float32)
    cls = torch.empty(B, L, HEADS, PATCHES, device=x.device, dtype=torch.float32)
    tok = torch.empty(B, L, HEADS, TOKENS, 4, device=x.device, dtype=torch.float32) if per_token else None
    feats = _forward(model, x, summary, cls, tok)
    out = {'summary': summary, 'cls_attention': cls, 'features': feats, 'STAT_NAMES': STAT_NAMES, 'TOKEN_STAT_NAMES': TOKEN_STAT_NAMES}
    if per_token:
        out['per_token'] = tok
    return out


class AttentionHeadStats:
    """Per-head statistics over a data set: ``update`` runs the fused forward straight into the row offset the host already knows (no
    synchronisation; the device buffers grow geometrically), ``compute`` runs one finalise launch and copies one block to the host.
    Groups: every row, and with ``num_classes`` the rows of each class label."""

    def __init__(self, depth: int, heads: int = HEADS, num_classes: Optional[int] = None, capacity: int = 1024):
        if not (isinstance(depth, int) and 1 <= depth <= 64):
            raise RovitHipError(f'AttentionHeadStats: depth must be in 1..64, got {depth!r}')
        if heads != HEADS:
            raise RovitHipError(f'AttentionHeadStats: the kernels are built for {HEADS} heads, got {heads!r}')
        if num_classes is not None and not (isinstance(num_classes, int) and 1 <= num_classes <= 4096):
            raise RovitHipError(f'AttentionHeadStats: num_classes must be None or in 1..4096, got {num_classes!r}')
        if not (isinstance(capacity, int) and capacity >= 1):
            raise RovitHipError(f'AttentionHeadStats: capacity must be a positive integer, got {capacity!r}')
        self.depth, self.heads, self.num_classes, self._capacity0 = depth, heads, num_classes, capacity
        self.reset()

    def reset(self) -> None:
        self.n = 0
        self.device: Optional[torch.device] = None
        self._summary = self._cls = self._labels = None
        self._result: Optional[Dict] = None

    def _reserve(self, rows: int, device: torch.device) -> None:
        if self.device is None:
            self.device = device
        elif device != self.device:
            raise RovitHipError(f'AttentionHeadStats: batch on {device}, earlier batches on {self.device}; reset() first')
        cap = self._summary.shape[0] if self._summary is not None else 0
        if rows <= cap:
            return
        new_cap = max(rows, 2 * cap, self._capacity0)
        new = (torch.empty(new_cap, self.depth, self.heads, NSTAT, dtype=torch.float32, device=device),
               torch.empty(new_cap, self.depth, self.heads, PATCHES, dtype=torch.float32, device=device),
               torch.empty(new_cap, dtype=torch.int32, device=device))
        for dst, src in zip(new, (self._summary, self._cls, self._labels)):
            if src is not None:
                dst[:self.n].copy_(src[:self.n])                 # device-to-device, stream-ordered: no synchronisation
        self._summary, self._cls, self._labels = new

    def _take_labels(self, what: str, labels, B: int, device: torch.device) -> Optional[torch.Tensor]:
        if self.num_classes is None:
            return None
        if labels is None:
            raise RovitHipError(f'{what}: num_classes = {self.num_classes} needs a label per row')
        labels = torch.as_tensor(labels)
        if labels.numel() != B:
            raise RovitHipError(f'{what}: {labels.numel()} labels for {B} rows')
        return labels.reshape(B).to(device=device, dtype=torch.int32, non_blocking=True)

    def update(self, model, x: torch.Tensor, labels=None) -> torch.Tensor:
        """Record a batch of images; returns the forward's features (B, 192)."""
        model = _container(model)
        x = _check_images('AttentionHeadStats.update', x)
        if model.engine.depth != self.depth:
            raise RovitHipError(f'AttentionHeadStats.update: a depth-{model.engine.depth} backbone, the accumulator was built for {self.depth}')
        B = x.shape[0]
        lab = self._take_labels('AttentionHeadStats.update', labels, B, x.device)
        self._reserve(self.n + B, x.device)
        self._result = None
        feats = _forward(model, x, self._summary[self.n:self.n + B], self._cls[self.n:self.n + B], None)
        if lab is not None:
            self._labels[self.n:self.n + B].copy_(lab)
        self.n += B
        return feats

    def update_rows(self, summary: torch.Tensor, cls_attention: torch.Tensor, labels=None) -> None:
        """Record rows computed elsewhere: ``summary`` (B, L, 3, 8) and ``cls_attention`` (B, L, 3, 196) on the GPU."""
        for name, t, w in (('summary', summary, NSTAT), ('cls_attention', cls_attention, PATCHES)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RovitHipError(f'AttentionHeadStats.update_rows: {name} must be on the GPU (there is no CPU fallback)')
            if t.dim() < 1 or t.shape[0] < 1 or t[0].numel() != self.depth * self.heads * w:
                raise RovitHipError(f'AttentionHeadStats.update_rows: {name} must be (B >= 1, {self.depth}, {self.heads}, {w}), got {tuple(t.shape)}')
        B = summary.shape[0]
        if cls_attention.shape[0] != B:
            raise RovitHipError(f'AttentionHeadStats.update_rows: {B} summary rows, {cls_attention.shape[0]} cls_attention rows')
        lab = self._take_labels('AttentionHeadStats.update_rows', labels, B, summary.device)
        self._reserve(self.n + B, summary.device)
        self._result = None
        self._summary[self.n:self.n + B].copy_(summary.detach().reshape(B, self.depth, self.heads, NSTAT))
        self._cls[self.n:self.n + B].copy_(cls_attention.detach().reshape(B, self.depth, self.heads, PATCHES))
        if lab is not None:
            self._labels[self.n:self.n + B].copy_(lab)
        self.n += B

    def compute(self) -> Dict:
        """numpy fp64 ``count`` (G), ``mean`` and ``var`` (G, L, 3, 8), ``cls_attention_mean`` (G, L, 3, 196) per group of ``groups``
        ('all', then the classes), and ``block``, the buffer as the kernel wrote it.  One launch, one device-to-host copy."""
        if self._result is not None:
            return self._result
        if self.n < 1:
            raise RovitHipError('AttentionHeadStats: nothing recorded yet')
        C = self.num_classes or 0
        words = native.load().rovit_head_stats_block_words(self.depth, self.heads, C)
        with torch.cuda.device(self.device):
            block = torch.empty(words, dtype=torch.float64, device=self.device)
            call('rovit_head_stats_finalize', ptr(self._summary), ptr(self._cls), ptr(self._labels) if C else None, ptr(block), self.n,
                 self.depth, self.heads, C, stream_ptr())
            host = block.cpu().numpy()                           # the single device-to-host copy
        self._result = result_from_block(host, self.depth, self.heads, C)
        return self._result


def model_head_stats(model, x_or_loader, per_token: bool = False, chunk: int = 256):
    """``RoViTKAN.attention_head_stats``: a tensor gives ``attention_head_stats`` of the batch; an iterable of (images, class_labels, ...)
    batches gives ``AttentionHeadStats.compute()`` grouped by class label (host batches are copied to the model's device)."""
    if isinstance(x_or_loader, torch.Tensor):
        return attention_head_stats(model, x_or_loader, per_token)
    if per_token:
        raise RovitHipError('attention_head_stats: per_token needs an image tensor (a data set\'s per-token values are not accumulated)')
    if not (isinstance(chunk, int) and chunk >= 1):
        raise RovitHipError(f'attention_head_stats: chunk must be a positive integer, got {chunk!r}')
    dev = next(model.parameters()).device
    num_classes = model.classification_head.fc2.out_features if hasattr(model, 'classification_head') else None
    acc = AttentionHeadStats(_container(model).engine.depth, HEADS, num_classes)
    for batch in x_or_loader:
        if not isinstance(batch, (tuple, list)) or len(batch) < 2:
            raise RovitHipError('attention_head_stats: a loader must yield (images, class_labels, ...) batches')
        images, labels = batch[0].to(dev, non_blocking=True), batch[1]
        for r0 in range(0, images.shape[0], chunk):
            acc.update(model, images[r0:r0 + chunk], labels[r0:r0 + chunk] if num_classes is not None else None)
    return acc.compute()
