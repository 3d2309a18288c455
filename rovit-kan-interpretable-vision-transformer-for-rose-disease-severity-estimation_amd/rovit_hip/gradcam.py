"""Grad-CAM++ on the GPU (csrc/gradcam.hip, rovit_vit_gradcam in csrc/vit.hip): what the reference's GradCAMPlusPlus.compute
(explainability/gradcam.py:34-104) computes with a forward and a full-backward hook on ``blocks[-1].norm1``, for a whole batch, from
a forward that keeps only the last block and a backward that stops at the last block's dqkv."""
from typing import NamedTuple

import torch

from .native import RovitHipError, call, ptr, ptr_array, stream_ptr


class GradCAMTaps(NamedTuple):
    act: torch.Tensor        # (B,197,192) fp32: the output of blocks[-1].norm1
    grad: torch.Tensor       # (B,197,192) fp32: d cls_logits[b, target[b]] / d act
    logits: torch.Tensor     # (B,classes) fp32: the classification head's logits (eval semantics)
    target: torch.Tensor     # (B,) int64: the class each map explains


def _targets(class_idx, batch: int, classes: int, device):
    """None -> None (the kernel takes the first argmax); an int or a (B,) integer tensor -> int32 on the device.  Raises before any launch."""
    if class_idx is None:
        return None
    if isinstance(class_idx, torch.Tensor):
        if class_idx.dtype.is_floating_point or class_idx.dtype.is_complex or class_idx.dtype == torch.bool:
            raise RovitHipError(f'grad_cam_pp: class_idx must be an integer tensor, got {class_idx.dtype}')
        if tuple(class_idx.shape) != (batch,):
            raise RovitHipError(f'grad_cam_pp: class_idx tensor must have shape ({batch},), got {tuple(class_idx.shape)}')
        lo, hi = int(class_idx.min()), int(class_idx.max())          # the one host synchronisation
        if lo < 0 or hi >= classes:
            raise RovitHipError(f'grad_cam_pp: class_idx values must be in [0, {classes}), got [{lo}, {hi}]')
        return class_idx.to(device=device, dtype=torch.int32).contiguous()
    if isinstance(class_idx, bool) or not isinstance(class_idx, int):
        raise RovitHipError(f'grad_cam_pp: class_idx must be None, an int or a (B,) integer tensor, got {type(class_idx).__name__}')
    if not 0 <= class_idx < classes:
        raise RovitHipError(f'grad_cam_pp: class_idx must be in [0, {classes}), got {class_idx}')
    return torch.full((batch,), class_idx, dtype=torch.int32, device=device)


def grad_cam_pp(model, x: torch.Tensor, class_idx=None, upsample: bool = True, return_taps: bool = False):
    """Grad-CAM++ of ``cls_logits`` at ``backbone.model.blocks[-1].norm1`` for every image of the batch.

    ``model``: a RoViTKAN (the classification head seeds the backward).  ``class_idx``: None (each image's first argmax), an int for
    every image, or a (B,) integer tensor.  Returns the reference's maps (B,224,224) fp32 -- bilinear resize (cv2.resize INTER_LINEAR)
    and min-max when the map's max is > 0 (gradcam.py:89-101; an all-equal positive map comes out NaN, as the reference's 0/0) -- or
    the raw relu'd (B,14,14) cam when ``upsample=False``.  ``return_taps=True``: ``(maps, GradCAMTaps(act, grad, logits, target))``.

    Always the bf16 engine and eval semantics (no dropout), whatever ``model.precision`` / ``model.training`` say.  Writes no ``.grad``
    and leaves the training workspace, the flat gradient buffers and the backward's stream state alone, so it may run between a
    training forward and its backward, under torch.no_grad(), with a frozen backbone and beside GradSync."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (3, 224, 224):
        raise RovitHipError(f'grad_cam_pp: expects (B,3,224,224) images, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}')
    B = x.shape[0]
    if B < 1:
        raise RovitHipError('grad_cam_pp: empty batch')
    head = model.classification_head
    classes, hidden = head.fc2.out_features, head.fc1.out_features
    if head.fc1.in_features != 192:
        raise RovitHipError(f'grad_cam_pp: the classification head must read the 192 backbone features, got {head.fc1.in_features}')
    targets = _targets(class_idx, B, classes, x.device)
    if not x.is_cuda:
        raise RovitHipError('grad_cam_pp: the images must be on the GPU (there is no CPU fallback)')
    vit = model.backbone.model
    dev = x.device
    with torch.no_grad():
        x = x.detach().float().contiguous()
        params = vit.ordered_parameters()
        eng = vit.engine
        eng.prepare(params)
        hp = [t.detach().float().contiguous() for t in (head.fc1.weight, head.fc1.bias, head.fc2.weight, head.fc2.bias)]
        ws = eng.take_gradcam_ws(B, dev)
        feats = torch.empty(B, 192, device=dev, dtype=torch.float32)
        logits = torch.empty(B, classes, device=dev, dtype=torch.float32)
        chosen = torch.empty(B, device=dev, dtype=torch.int32)
        cam = torch.empty(B, 14, 14, device=dev, dtype=torch.float32)
        act = torch.empty(B, 197, 192, device=dev, dtype=torch.float32) if return_taps else None
        grad = torch.empty(B, 197, 192, device=dev, dtype=torch.float32) if return_taps else None
        pa = ptr_array(params)
        call('rovit_vit_forward_gradcam', ptr(x), pa, ptr(eng.prep), ptr(ws), ptr(feats), B, vit.depth, stream_ptr())
        call('rovit_vit_gradcam', pa, ptr(eng.prep), ptr(ws), ptr(feats), *[ptr(t) for t in hp], hidden, classes, ptr(targets), ptr(logits),
             ptr(chosen), ptr(cam), ptr(act), ptr(grad), B, vit.depth, stream_ptr())
        eng.give_ws(B, 'gradcam', ws)
        out = cam
        if upsample:
            out = torch.empty(B, 224, 224, device=dev, dtype=torch.float32)
            call('rovit_gradcam_map', ptr(cam), ptr(out), B, stream_ptr())
    if return_taps:
        return out, GradCAMTaps(act, grad, logits, chosen.long())
    return out
