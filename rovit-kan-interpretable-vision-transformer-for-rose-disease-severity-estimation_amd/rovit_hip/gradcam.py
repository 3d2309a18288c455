"""Grad-CAM++ on the GPU (csrc/gradcam.hip, csrc/explain.hip, rovit_vit_gradcam(_seeded) in csrc/vit.hip): what the reference's
GradCAMPlusPlus.compute (explainability/gradcam.py:34-104) computes with a forward and a full-backward hook on ``blocks[-1].norm1``, for a
whole batch, from a forward that keeps only the last block and a backward that stops at the last block's dqkv -- of a class logit, or of
the severity and uncertainty outputs (``target=``), several of them from one forward."""
import ctypes as C
from typing import NamedTuple

import torch

from .native import RovitHipError, call, ptr, ptr_array, stream_ptr

# target name -> (ROVIT_TARGET_* kind, the curriculum stage from which forward() returns it)
TARGETS = {'class': (0, 1), 'ordinal_severity': (1, 2), 'mu': (2, 3), 'log_var': (3, 3), 'kan_severity': (4, 4)}
_HOOK_RECIPE = ('use the hook recipe instead: a forward hook and a full-backward hook on backbone.model.blocks[-1].norm1, then '
                'backward() of the target')


class GradCAMTaps(NamedTuple):
    act: torch.Tensor        # (B,197,192) fp32: the output of blocks[-1].norm1
    grad: torch.Tensor       # (B,197,192) fp32: d cls_logits[b, target[b]] / d act
    logits: torch.Tensor     # (B,classes) fp32: the classification head's logits (eval semantics)
    target: torch.Tensor     # (B,) int64: the class each map explains


class TargetCAMTaps(NamedTuple):
    act: torch.Tensor            # (B,197,192) fp32: the output of blocks[-1].norm1
    grad: torch.Tensor           # (B,197,192) fp32: d target[b] / d act
    value: torch.Tensor          # (B,) fp32: the target's value (eval semantics)
    features: torch.Tensor       # (B,192) fp32: the backbone features the heads read
    feature_grad: torch.Tensor   # (B,192) fp32: d target[b] / d features (feature_grad * features: per-feature attribution)


def _target_names(target, class_idx, stage: int):
    """(names, several) from a name or a list / tuple of names.  Raises before any launch."""
    several = isinstance(target, (list, tuple))
    names = list(target) if several else [target]
    if not names or not all(isinstance(n, str) for n in names):
        raise RovitHipError(f'grad_cam_pp: target must be a name or a non-empty list / tuple of names out of {list(TARGETS)}, got {target!r}')
    for n in names:
        if n not in TARGETS:
            raise RovitHipError(f'grad_cam_pp: unknown target {n!r}; the targets are {list(TARGETS)}')
    if len(set(names)) != len(names):
        raise RovitHipError(f'grad_cam_pp: target {names!r} names an output more than once')
    for n in names:
        if stage < TARGETS[n][1]:
            raise RovitHipError(f'grad_cam_pp: target {n!r} needs curriculum stage {TARGETS[n][1]}; at stage {stage} forward() returns '
                                'None for it')
    if class_idx is not None and 'class' not in names:
        raise RovitHipError(f"grad_cam_pp: class_idx is given but target {target!r} does not contain 'class'")
    return names, several


def _check_coverage(model, names):
    """The head / KAN shapes rovit_explain_seed covers (those of the head phase, 192 features, a one-output KAN stack)."""
    c, o, u, k = model.classification_head, model.ordinal_head, model.uncertainty_head, model.kan_module
    hid = c.fc1.out_features
    heads = []
    if 'ordinal_severity' in names:
        heads.append(o)
    if 'mu' in names or 'log_var' in names:
        heads.append(u)
    bad = None
    if heads:
        C_ = c.fc2.out_features
        if not (all(h.fc1.in_features == 192 and h.fc1.out_features == hid for h in heads) and hid % 4 == 0 and 4 <= hid <= 256
                and 2 <= C_ <= 8 and (o not in heads or o.fc2.out_features == C_ - 1)):
            bad = f'heads of hidden width {[h.fc1.out_features for h in heads]} (4..256, a multiple of 4, equal to the classification ' \
                  f"head's {hid}) / {C_} classes (2..8) / 192 input features"
    if bad is None and 'kan_severity' in names:
        d = list(k.layers_dims)
        if not (k.degree == 3 and 1 <= len(k.kan_layers) <= 4 and d[0] == 192 and all(1 <= w <= 64 for w in d[1:]) and d[-1] == 1
                and all(8 <= l.knots.numel() <= 64 for l in k.kan_layers)):
            bad = f'a KAN stack {d} of degree {k.degree} (degree 3, 1..4 layers behind the 192 features, widths <= 64, one output, ' \
                  '8..64 knots per layer)'
    if bad is not None:
        raise RovitHipError(f'grad_cam_pp: {bad} is outside what the fused seed covers; {_HOOK_RECIPE}')


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


def grad_cam_pp(model, x: torch.Tensor, class_idx=None, upsample: bool = True, return_taps: bool = False, target='class'):
    """Grad-CAM++ of one model output at ``backbone.model.blocks[-1].norm1`` for every image of the batch.

    ``model``: a RoViTKAN.  ``target`` names the scalar per image whose gradient seeds the backward, with eval semantics (no dropout):
    ``'class'`` -- ``cls_logits[b, c_b]`` (the default; ``class_idx``: None for each image's first argmax, an int for every image, or a
    (B,) integer tensor), ``'ordinal_severity'`` -- predict()'s sum_k k P(y = k) (stage >= 2), ``'mu'`` and ``'log_var'`` -- the
    uncertainty head's outputs, log_var clamped to +-10 with no gradient outside (stage >= 3), ``'kan_severity'`` -- the KAN module's
    output (stage 4).  Grad-CAM++ keeps relu(g): a map shows where the image RAISES its target (e.g. the KAN severity), not what lowers
    it.  A list or tuple of names explains each of them from ONE backbone forward and returns a dict name -> result in the order given.

    Returns the reference's maps (B,224,224) fp32 -- bilinear resize (cv2.resize INTER_LINEAR) and min-max when the map's max is > 0
    (gradcam.py:89-101; an all-equal positive map comes out NaN, as the reference's 0/0) -- or the raw relu'd (B,14,14) cam when
    ``upsample=False``.  ``return_taps=True``: ``(maps, taps)``, with ``GradCAMTaps(act, grad, logits, target)`` for ``'class'`` and
    ``TargetCAMTaps(act, grad, value, features, feature_grad)`` for the other targets (feature_grad * features is the per-feature
    attribution of the target).

    Always the bf16 engine and eval semantics (no dropout), whatever ``model.precision`` / ``model.training`` / the Dropout flags say.
    Writes no ``.grad`` and leaves the training workspace, the flat gradient buffers and the backward's stream state alone, so it may run
    between a training forward and its backward, under torch.no_grad(), with a frozen backbone and beside GradSync.  Targets or shapes
    the fused path does not cover are refused (RovitHipError) before anything runs."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (3, 224, 224):
        raise RovitHipError(f'grad_cam_pp: expects (B,3,224,224) images, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}')
    B = x.shape[0]
    if B < 1:
        raise RovitHipError('grad_cam_pp: empty batch')
    names, several = _target_names(target, class_idx, model.curriculum_stage)
    others = [n for n in names if n != 'class']
    head = model.classification_head
    classes, hidden = head.fc2.out_features, head.fc1.out_features
    if head.fc1.in_features != 192:
        raise RovitHipError(f'grad_cam_pp: the classification head must read the 192 backbone features, got {head.fc1.in_features}')
    targets = _targets(class_idx, B, classes, x.device) if 'class' in names else None
    _check_coverage(model, others)
    if not x.is_cuda:
        raise RovitHipError('grad_cam_pp: the images must be on the GPU (there is no CPU fallback)')
    vit = model.backbone.model
    dev = x.device
    res = {}
    f32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
    with torch.no_grad():
        x = x.detach().float().contiguous()
        params = vit.ordered_parameters()
        eng = vit.engine
        eng.prepare(params)
        ws = eng.take_gradcam_ws(B, dev)
        feats = f32(B, 192)
        pa = ptr_array(params)
        call('rovit_vit_forward_gradcam', ptr(x), pa, ptr(eng.prep), ptr(ws), ptr(feats), B, vit.depth, stream_ptr())
        if 'class' in names:
            hp = [t.detach().float().contiguous() for t in (head.fc1.weight, head.fc1.bias, head.fc2.weight, head.fc2.bias)]
            logits = f32(B, classes)
            chosen = torch.empty(B, device=dev, dtype=torch.int32)
            cam = f32(B, 14, 14)
            act = f32(B, 197, 192) if return_taps else None
            grad = f32(B, 197, 192) if return_taps else None
            call('rovit_vit_gradcam', pa, ptr(eng.prep), ptr(ws), ptr(feats), *[ptr(t) for t in hp], hidden, classes, ptr(targets),
                 ptr(logits), ptr(chosen), ptr(cam), ptr(act), ptr(grad), B, vit.depth, stream_ptr())
            res['class'] = (cam, GradCAMTaps(act, grad, logits, chosen.long()) if return_taps else None)
        if others:
            values, seeds = f32(len(others), B), f32(len(others), B, 192)
            _explain_seed(model, feats, others, values, seeds)
            for t, n in enumerate(others):
                cam = f32(B, 14, 14)
                act = f32(B, 197, 192) if return_taps else None
                grad = f32(B, 197, 192) if return_taps else None
                call('rovit_vit_gradcam_seeded', pa, ptr(eng.prep), ptr(ws), ptr(seeds[t]), ptr(cam), ptr(act), ptr(grad), B, vit.depth,
                     stream_ptr())
                res[n] = (cam, TargetCAMTaps(act, grad, values[t], feats, seeds[t]) if return_taps else None)
        eng.give_ws(B, 'gradcam', ws)
        out = {}
        for n in names:
            cam, taps = res[n]
            m = cam
            if upsample:
                m = f32(B, 224, 224)
                call('rovit_gradcam_map', ptr(cam), ptr(m), B, stream_ptr())
            out[n] = (m, taps) if return_taps else m
    return out if several else out[names[0]]


def _explain_seed(model, feats, names, values, seeds):
    """rovit_explain_seed on the backbone features: values (T,B) and d target / d features (T,B,192) of the named targets."""
    from .functions import ACT_RELU, ACT_SIGMOID3, HeadPhaseFn
    k = model.kan_module
    kan = 'kan_severity' in names
    nl = len(k.kan_layers)
    hp = [t.detach().float().contiguous() for t in model._head_params()]
    kp = [t.detach().float().contiguous() for t in model._kan_params()] if kan else []
    knots = [l.knots.detach().float().contiguous() for l in k.kan_layers] if kan else []
    cfg = {'stage': model.curriculum_stage, 'kan_dims': list(k.layers_dims) if kan else [], 'kan_knots': knots,
           'kan_acts': [ACT_SIGMOID3 if i == nl - 1 else ACT_RELU for i in range(nl)]}
    d = HeadPhaseFn._desc(feats, cfg, hp, kp)
    kinds = (C.c_int * len(names))(*[TARGETS[n][0] for n in names])
    call('rovit_explain_seed', C.byref(d), C.cast(kinds, C.c_void_p), len(names), ptr(values), ptr(seeds), stream_ptr())
