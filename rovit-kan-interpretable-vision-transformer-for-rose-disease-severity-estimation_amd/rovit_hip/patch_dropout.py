"""PatchDropout (Liu et al., "PatchDropout: Economizing Vision Transformers Using Patch Dropout", WACV 2023) for the training step.

During fine-tuning every image keeps a random subset of k of its 196 patches plus the class token; evaluation sees all patches.  The
backbone's forward AND backward then run on B * (1 + k) token rows instead of B * 197 (rovit_vit_forward_train_tokens /
rovit_vit_backward_tokens, csrc/vit.hip), and only the two ends stay at 197 tokens: the patch embedding in front of the gather, and its
weight, position and class-token gradients behind the scatter (csrc/patch_dropout.hip), where a dropped patch contributes exact zeros.

* ``draw(seed, step, B, k, device)``: one launch, no host read; ``draw_reference`` is the same rule in numpy.
* ``forward_kept(backbone, images, keep)``: the token path with explicit (B, k) patch indices.
* ``VitTokensFn``: the autograd Function both go through; ``DeiTTinyBackbone.set_patch_dropout`` switches it on for ``train()`` mode.

Out of scope here, refused with a ``RovitHipError`` rather than run densely: hook / tap paths, images that require grad, and the
data-parallel wrapper (``rovit_hip.parallel.GradSync``).  A frozen backbone (or ``torch.no_grad()``) runs the forward alone."""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np
import torch

from . import native
from .functions import VitEngine, _f32c
from .native import RovitHipError, call, ptr, ptr_array, stream_ptr

PATCHES, TOKENS, EMBED = 196, 197, 192
STREAM = 0x50447200          # ROVIT_PATCH_DROPOUT_STREAM: Philox counter word 1 is STREAM + patch // 4


def kept_patches(keep: float) -> int:
    """k = max(1, round(keep * 196)), halves rounded up."""
    return max(1, min(PATCHES, int(math.floor(float(keep) * PATCHES + 0.5))))


def check_keep_seed(keep, seed) -> Tuple[float, int]:
    if isinstance(keep, bool) or not isinstance(keep, (int, float)) or not (0.0 < float(keep) <= 1.0):
        raise ValueError(f'patch dropout: keep must be a number in (0, 1], got {keep!r}')
    if isinstance(seed, bool) or not isinstance(seed, int) or not (0 <= seed < 1 << 64):
        raise ValueError(f'patch dropout: seed must be an integer in [0, 2^64), got {seed!r}')
    return float(keep), int(seed)


def _check_draw_args(seed, step, B, k) -> None:
    for name, v in (('seed', seed), ('step', step)):
        if isinstance(v, bool) or not isinstance(v, int) or not (0 <= v < 1 << 64):
            raise ValueError(f'patch dropout: {name} must be an integer in [0, 2^64), got {v!r}')
    if not (isinstance(B, int) and B >= 1):
        raise ValueError(f'patch dropout: B must be a positive integer, got {B!r}')
    if not (isinstance(k, int) and 1 <= k <= PATCHES):
        raise ValueError(f'patch dropout: k must be an integer in [1, {PATCHES}], got {k!r}')


def draw_reference(seed: int, step: int, B: int, k: int) -> np.ndarray:
    """The kept patches (B, k) int32, ascending, as rovit_patch_dropout_draw writes them.  Patch p of sample b gets key word p % 4 of
    Philox4x32-10(key = seed, counter = (b, STREAM + p // 4, step lo, step hi)); the patches are ranked by the pair (key, p) and those of
    rank < k are kept."""
    from oracle import philox          # the numpy generator (test infrastructure at the repository root)
    _check_draw_args(seed, step, B, k)
    b = np.repeat(np.arange(B, dtype=np.uint64), PATCHES // 4)
    g = np.tile(np.arange(PATCHES // 4, dtype=np.uint64), B) + np.uint64(STREAM)
    n = b.size
    out = philox.philox4x32_10([b, g, np.full(n, step & 0xFFFFFFFF, np.uint64), np.full(n, step >> 32, np.uint64)],
                               [seed & 0xFFFFFFFF, seed >> 32])
    words = np.stack(out, axis=1).reshape(B, PATCHES)                  # word q of group g is patch 4 g + q
    order = np.argsort(words, axis=1, kind='stable')                   # stable: equal keys in patch order = the pair (key, p)
    return np.sort(order[:, :k], axis=1).astype(np.int32)


def maps_reference(keep: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """src (B, 1 + k) and inv (B, 197) of kept patches (B, k), as the draw kernel writes them."""
    keep = np.asarray(keep, dtype=np.int64)
    B, k = keep.shape
    src = np.concatenate([np.zeros((B, 1), np.int64), 1 + keep], axis=1)
    inv = np.full((B, TOKENS), -1, np.int64)
    np.put_along_axis(inv, src, np.broadcast_to(np.arange(1 + k), (B, 1 + k)), axis=1)
    return src.astype(np.int32), inv.astype(np.int32)


def draw(seed: int, step: int, B: int, k: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(keep (B, k), src (B, 1 + k), inv (B, 197)), int32 on `device`: one launch on the current stream, nothing read back."""
    _check_draw_args(seed, step, B, k)
    keep = torch.empty(B, k, dtype=torch.int32, device=device)
    src = torch.empty(B, 1 + k, dtype=torch.int32, device=device)
    inv = torch.empty(B, TOKENS, dtype=torch.int32, device=device)
    call('rovit_patch_dropout_draw', seed, step, ptr(keep), ptr(src), ptr(inv), B, k, stream_ptr())
    return keep, src, inv


def refuse_unsupported(model, x, hooked: bool) -> None:
    """The combinations patch dropout does not cover; checked before anything touches the device."""
    if hooked:
        raise RovitHipError('patch dropout is active and a hook / tap on blocks[i].attn or blocks[i].norm1 is registered: the taps read '
                            '197-token buffers.  Remove the hooks, or switch patch dropout off (set_patch_dropout(1.0) or eval())')
    if torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad:
        raise RovitHipError('patch dropout is active and the images require grad: the image gradient of the token path is not '
                            'implemented.  Detach the images, or switch patch dropout off (set_patch_dropout(1.0) or eval())')
    eng = model._engine
    if eng is not None and (eng.range_hook is not None or eng.backward_ranges is not None or eng.notify_stream is not None):
        raise RovitHipError('patch dropout is active and the data-parallel wrapper (rovit_hip.parallel.GradSync) is attached to this '
                            'backbone: the token backward is one block range without the reduction hooks.  Train on one device, or '
                            'switch patch dropout off')


class VitTokensFn(torch.autograd.Function):
    """features = backbone(images) on the token rows `src` keeps.  Parameter gradients are installed like VitFn's (the engine's flat
    buffer; grad += new when a grad exists).  No image gradient; one backward per forward.  Unlike VitFn the training forward leaves
    no ``engine.last_ws``: its workspace holds 1 + k token rows per image, not the 197 the readers of ``last_ws`` (rovit_hip.taps)
    index, so it is cleared and those readers report that no dense training forward is pending instead of reading stale rows."""

    @staticmethod
    def forward(ctx, images, engine: VitEngine, training: bool, src, inv, *params):
        if ctx.needs_input_grad[0]:
            raise RovitHipError('the token path gives no gradient with respect to the images')
        images = _f32c(images)
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, 224, 224):
            raise RovitHipError(f'backbone expects (B,3,224,224) images, got {tuple(images.shape)}')
        B, dev = images.shape[0], images.device
        if src.dtype != torch.int32 or inv.dtype != torch.int32 or src.dim() != 2 or src.shape[0] != B or tuple(inv.shape) != (B, TOKENS):
            raise RovitHipError(f'token path: src must be int32 (B, 1 + k) and inv int32 (B, {TOKENS})')
        tokens = int(src.shape[1])
        if not (2 <= tokens <= TOKENS):
            raise RovitHipError(f'token path: 1 + k must be in [2, {TOKENS}], got {tokens}')
        need_bwd = bool(training) and any(p.requires_grad for p in params)
        mlp_path = int(engine.mlp_path if engine.mlp_path is not None else VitEngine.default_mlp_path)
        seq = engine.seq_img
        if seq is None or seq.numel() < B or seq.device != dev:
            seq = engine.seq_img = torch.arange(max(B, 256), dtype=torch.int32, device=dev)
        feats = torch.empty(B, EMBED, device=dev, dtype=torch.float32)
        table = torch.empty(B, TOKENS, EMBED, device=dev, dtype=torch.float32)
        parr = ptr_array(params)
        ctx.engine, ctx.need_bwd = engine, need_bwd
        if not need_bwd:       # frozen backbone / no_grad: embed, then the inference forward of the kept rows
            engine.prepare(params)
            ws = engine.take_ws(B, False, dev)
            call('rovit_vit_embed', ptr(images), parr, ptr(engine.prep), ptr(table), B, engine.depth, stream_ptr())
            call('rovit_vit_forward_tokens', ptr(table), ptr(table), B, 0, ptr(seq), ptr(src), tokens, parr, ptr(engine.prep), ptr(ws),
                 ptr(feats), B, engine.depth, mlp_path, stream_ptr())
            engine.give_ws(B, False, ws)
            return feats
        prep_mode = engine.prepare(params, defer=True)
        ws = engine.take_ws(B, True, dev)
        try:
            call('rovit_vit_forward_train_tokens', ptr(images), ptr(seq), ptr(src), tokens, parr, ptr(engine.prep), ptr(ws), ptr(table),
                 ptr(feats), B, engine.depth, mlp_path, int(prep_mode), stream_ptr())
        except Exception:
            if prep_mode:
                engine._prep_key, engine._tables_written = None, False       # nothing can be assumed about the weight images
            raise
        engine.last_ws = None
        ctx.ws, ctx.batch, ctx.tokens, ctx.mlp_path = ws, B, tokens, mlp_path
        ctx.save_for_backward(images, inv)
        ctx.params = params
        ctx.prep_key = engine._prep_key
        return feats

    @staticmethod
    def backward(ctx, dfeat):
        engine: VitEngine = ctx.engine
        n_out = 5 + engine.n_params
        if not ctx.need_bwd:
            return (None,) * n_out
        params = ctx.params
        if ctx.ws is None:
            raise RovitHipError('backbone backward called twice on the same graph: the activation workspace is recycled after the '
                                'first backward (run the forward again instead of retain_graph=True)')
        if engine._prep_key != ctx.prep_key:
            raise RovitHipError('backbone parameters changed between forward and backward (optimizer step or in-place update): the '
                                'prepared bf16 weights no longer match the saved activations')
        if engine.range_hook is not None:
            raise RovitHipError('the token backward cannot feed the data-parallel reduction hooks (rovit_hip.parallel.GradSync)')
        dfeat = _f32c(dfeat)
        images, inv = ctx.saved_tensors
        engine.ensure_grads(params)
        fresh = all(p.grad is None for p in params)
        owned = (not fresh) and all(p.grad is not None and p.grad.data_ptr() == v.data_ptr() for p, v in zip(params, engine.grad_views))
        targets = engine.grad_views if fresh else engine.stage_views
        dense = torch.empty(ctx.batch * TOKENS, EMBED, device=dfeat.device, dtype=torch.bfloat16)
        call('rovit_vit_backward_tokens', ptr(images), ptr(dfeat), ptr(inv), ctx.tokens, ptr_array(params), ptr(engine.prep), ptr(ctx.ws),
             ptr(dense), ptr_array(targets), ctx.batch, engine.depth, ctx.mlp_path, stream_ptr())
        if fresh:
            for p, v in zip(params, engine.grad_views):
                if p.requires_grad:
                    p.grad = v
        elif owned:
            engine.grad_flat.add_(engine.grad_stage)
        else:
            for p, v in zip(params, engine.stage_views):
                if p.requires_grad:
                    p.grad = v.clone() if p.grad is None else p.grad.add_(v)
        engine.give_ws(ctx.batch, True, ctx.ws)
        ctx.ws = None
        return (None,) * n_out


def _vit(backbone):
    return getattr(backbone, 'model', backbone)          # DeiTTinyBackbone or its DeiTTiny


def forward_kept(backbone, images: torch.Tensor, keep) -> torch.Tensor:
    """Features (B, 192) of `images` with patches keep (B, k) kept: int indices in [0, 196), strictly ascending per row.  The token
    path whatever k is (k = 196 included); gradients flow to the backbone parameters when grad is enabled.  The indices are checked on
    the host (one copy when `keep` is a device tensor): this is the explicit entry, the module's own draws never leave the device."""
    vit = _vit(backbone)
    hooked = any(b.attn._forward_hooks or b.norm1._forward_hooks or b.norm1._backward_hooks for b in vit.blocks)
    refuse_unsupported(vit, images, hooked)
    kn = keep.detach().cpu().numpy() if isinstance(keep, torch.Tensor) else np.asarray(keep)
    B = images.shape[0]
    if kn.ndim != 2 or kn.shape[0] != B or not (1 <= kn.shape[1] <= PATCHES) or kn.dtype.kind not in 'iu':
        raise ValueError(f'forward_kept: keep must be an integer array of shape (B = {B}, k in [1, {PATCHES}]), got '
                         f'{kn.dtype} {tuple(kn.shape)}')
    kn = kn.astype(np.int64)
    if kn.min() < 0 or kn.max() >= PATCHES or (np.diff(kn, axis=1) <= 0).any():
        raise ValueError(f'forward_kept: every row of keep must be strictly ascending patch indices in [0, {PATCHES})')
    src, inv = maps_reference(kn)
    dev = images.device
    return VitTokensFn.apply(images, vit.engine, torch.is_grad_enabled(), torch.from_numpy(src).to(dev), torch.from_numpy(inv).to(dev),
                             *vit.ordered_parameters())


def forward_dropped(vit, x: torch.Tensor, hooked: bool) -> torch.Tensor:
    """DeiTTiny.forward in train() mode with keep < 1: a new subset per call from (seed, step), the step counter advanced."""
    refuse_unsupported(vit, x, hooked)
    if x.dim() != 4 or tuple(x.shape[1:]) != (3, 224, 224):
        raise RovitHipError(f'backbone expects (B,3,224,224) images, got {tuple(x.shape)}')
    k = kept_patches(vit.patch_keep)
    keep, src, inv = draw(vit.patch_dropout_seed, vit.patch_dropout_step, int(x.shape[0]), k, x.device)
    vit.patch_dropout_step += 1
    vit.last_patch_keep = keep
    return VitTokensFn.apply(x, vit.engine, torch.is_grad_enabled(), src, inv, *vit.ordered_parameters())
