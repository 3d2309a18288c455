"""Gradients of a RoViTKAN output with respect to the input pixels, and integrated gradients, on the GPU.

One call runs the fused backbone forward that keeps the training activations, the head phase on the features (csrc/head_phase.hip:
its own backward gives d target / d features), and the backbone's dgrad chain alone down to the pixels (rovit_vit_backward_input with
no weight gradients; the patch embedding's data gradient is csrc/input_grad.hip).  Integrated gradients stack several interpolants of
each image in one backbone call; the pixel kernel sums them in its accumulators and adds the scaled sum into one buffer across calls,
so each image's attribution is written once per call and never kept per step."""
import torch

from .gradcam import TARGETS, _check_coverage, _target_names, _targets
from .native import RovitHipError, call, ptr, ptr_array, stream_ptr


def _check_phase(model, what='input_gradients'):
    """The head / KAN shapes of the fused head phase (the seeds come from its backward).  Raises before any launch."""
    c, o, u, k = model.classification_head, model.ordinal_head, model.uncertainty_head, model.kan_module
    hid, C_ = c.fc1.out_features, c.fc2.out_features
    ok = (c.fc1.in_features == o.fc1.in_features == u.fc1.in_features == 192 and o.fc1.out_features == hid == u.fc1.out_features
          and hid % 4 == 0 and 4 <= hid <= 256 and 2 <= C_ <= 8 and o.fc2.out_features == C_ - 1)
    if ok and model.curriculum_stage >= 4:
        d = list(k.layers_dims)
        ok = (k.degree == 3 and 1 <= len(k.kan_layers) <= 4 and d[0] == 192 and all(1 <= w <= 64 for w in d[1:])
              and all(8 <= l.knots.numel() <= 64 for l in k.kan_layers))
    if not ok:
        raise RovitHipError(f'{what}: the heads / KAN stack are outside the shapes of the fused head phase (192 features, '
                            'equal hidden widths 4..256 in multiples of 4, 2..8 classes, a degree-3 KAN of 1..4 layers of width <= 64); '
                            'use autograd through the model with images that require grad instead')


def _check_args(model, x, target, class_idx, steps, baseline, chunk, what='input_gradients'):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or tuple(x.shape[1:]) != (3, 224, 224):
        raise RovitHipError(f'{what}: expects (B,3,224,224) images, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}')
    if x.shape[0] < 1:
        raise RovitHipError(f'{what}: empty batch')
    if not x.dtype.is_floating_point:
        raise RovitHipError(f'{what}: the images must be floating point, got {x.dtype}')
    if isinstance(target, (list, tuple)):
        raise RovitHipError(f'{what}: one target per call, got {target!r}')
    names, _ = _target_names(target, class_idx, model.curriculum_stage)
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
        raise RovitHipError(f'{what}: steps must be an int >= 0 (0: the plain gradient), got {steps!r}')
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise RovitHipError(f'{what}: chunk must be an int >= 1, got {chunk!r}')
    if baseline is not None:
        if steps == 0:
            raise RovitHipError(f'{what}: a baseline is only used by integrated gradients (steps >= 1)')
        if not isinstance(baseline, torch.Tensor) or not baseline.dtype.is_floating_point:
            raise RovitHipError(f'{what}: baseline must be a floating-point tensor, got {type(baseline).__name__}')
        try:
            shape = torch.broadcast_shapes(baseline.shape, x.shape)
        except RuntimeError:
            shape = None
        if shape != x.shape:
            raise RovitHipError(f'{what}: baseline of shape {tuple(baseline.shape)} does not broadcast to the images '
                                f'{tuple(x.shape)}')
        if baseline.device != x.device:
            raise RovitHipError(f'{what}: baseline on {baseline.device}, images on {x.device}')
    head = model.classification_head
    targets = _targets(class_idx, x.shape[0], head.fc2.out_features, x.device) if target == 'class' else None
    _check_coverage(model, [n for n in names if n != 'class'])
    _check_phase(model, what)
    if not x.is_cuda:
        raise RovitHipError(f'{what}: the images must be on the GPU (there is no CPU fallback)')
    return targets


def _head_outputs(model, feats):
    """HeadPhaseFn on features that require grad, eval semantics (no dropout), detached parameters: autograd through it gives
    d target / d features from the head phase's own backward and writes no parameter gradient."""
    from .functions import ACT_RELU, ACT_SIGMOID3, HeadPhaseFn
    stage = model.curriculum_stage
    k = model.kan_module
    nl = len(k.kan_layers)
    cfg = {'stage': stage, 'masks': None, 'drop_p': 0.0, 'seed': 0, 'offset': 0,
           'kan_dims': list(k.layers_dims) if stage >= 4 else [],
           'kan_knots': [l.knots for l in k.kan_layers] if stage >= 4 else [],
           'kan_acts': [ACT_SIGMOID3 if i == nl - 1 else ACT_RELU for i in range(nl)], 'grad_views': None}
    hp = [p.detach() for p in model._head_params()]
    kp = [p.detach() for p in model._kan_params()] if stage >= 4 else []
    return HeadPhaseFn.apply(feats, cfg, *hp, *kp)


def _target_value(name, outs, cls_idx):
    """(B,) value of the target, as RoViTKAN.forward / predict() define it."""
    cls, ordl, mu, lv, kan = outs
    if name == 'class':
        return cls.gather(1, cls_idx.view(-1, 1)).squeeze(1)
    if name == 'ordinal_severity':
        from models.heads import OrdinalHead
        p = OrdinalHead.probabilities_from_logits(ordl)
        levels = torch.arange(p.shape[1], dtype=torch.float32, device=p.device)
        return (p * levels).sum(dim=1)
    return {'mu': mu, 'log_var': lv, 'kan_severity': kan}[name][:, 0]


def _seed(model, feats, name, cls_idx):
    """(value (B,), d value / d features (B,192), logits (B,C)) with argmax classes when cls_idx is None."""
    with torch.enable_grad():
        f = feats.detach().requires_grad_(True)
        outs = _head_outputs(model, f)
        if name == 'class' and cls_idx is None:
            cls_idx = outs[0].detach().argmax(dim=1)
        v = _target_value(name, outs, cls_idx)
        g, = torch.autograd.grad(v.sum(), f)
    return v.detach(), g.contiguous()


class _Backbone:
    """The backbone calls of one input_gradients call: the engine's prepared weights, workspaces from its pool (never the one a
    pending training backward holds; engine.last_ws untouched), the training-mode forward and the dgrad-only backward."""

    def __init__(self, model, dev):
        from .functions import VitEngine
        self.vit = model.backbone.model
        self.eng = self.vit.engine
        self.params = self.vit.ordered_parameters()
        self.eng.prepare(self.params)
        self.pa = ptr_array(self.params)
        self.mlp = int(self.eng.mlp_path if self.eng.mlp_path is not None else VitEngine.default_mlp_path)
        self.dev = dev

    def features(self, imgs, training):
        n = imgs.shape[0]
        ws = self.eng.take_ws(n, training, self.dev)
        feats = torch.empty(n, 192, device=self.dev, dtype=torch.float32)
        call('rovit_vit_forward', ptr(imgs), self.pa, ptr(self.eng.prep), ptr(ws), ptr(feats), n, self.vit.depth, int(training), self.mlp,
             stream_ptr())
        if not training:
            self.eng.give_ws(n, False, ws)
            return feats, None
        return feats, ws

    def pixels(self, imgs, ws, seed, out, copies, scale, accumulate):
        n = imgs.shape[0]
        call('rovit_vit_backward_input', ptr(imgs), ptr(seed), self.pa, ptr(self.eng.prep), ptr(ws), None, n, self.vit.depth,
             self.vit.depth - 1, 0, self.mlp, stream_ptr(), ptr(out), copies, float(scale), int(accumulate))
        self.eng.give_ws(n, True, ws)

    def embed(self, imgs, out):
        """The token rows the forward starts from (rovit_vit_embed): out (n,197,192) fp32."""
        call('rovit_vit_embed', ptr(imgs), self.pa, ptr(self.eng.prep), ptr(out), imgs.shape[0], self.vit.depth, stream_ptr())

    def forward_tokens(self, img_tokens, base_tokens, base_shared, seq_img, src, ws, mlp_path):
        """Inference features (n,192) of the n sequences of src (n, tokens) gathered from the token tables (rovit_vit_forward_tokens);
        ws: an inference workspace of at least n sequences (a shorter sequence uses a prefix of it)."""
        n, tokens = src.shape
        feats = torch.empty(n, 192, device=self.dev, dtype=torch.float32)
        call('rovit_vit_forward_tokens', ptr(img_tokens), ptr(base_tokens), img_tokens.shape[0], int(base_shared), ptr(seq_img), ptr(src),
             tokens, self.pa, ptr(self.eng.prep), ptr(ws), ptr(feats), n, self.vit.depth, int(mlp_path), stream_ptr())
        return feats

    def forward_ragged(self, img_tokens, base_tokens, base_shared, seq_img, src, offsets_dev, offsets_host, ws, mlp_path):
        """The same for n sequences of different lengths packed back to back (rovit_vit_forward_ragged; rovit_hip.ragged): src one
        entry per packed row, the (n + 1,) row offsets on the device and as a host array; ws from ragged.take_ws."""
        from .ragged import forward_ragged
        return forward_ragged(self, img_tokens, base_tokens, base_shared, seq_img, src, offsets_dev, offsets_host, ws, mlp_path)

    def relevance(self, ws, seed, out, scratch):
        """The dgrad chain alone with one relevance step per block (rovit_vit_backward_relevance): out (n,197) = row 0 of R_L."""
        n = out.shape[0]
        call('rovit_vit_backward_relevance', ptr(seed), self.pa, ptr(self.eng.prep), ptr(ws), n, self.vit.depth, self.mlp, ptr(out),
             ptr(scratch), stream_ptr())
        self.eng.give_ws(n, True, ws)


def input_gradients(model, x: torch.Tensor, target='class', class_idx=None, steps: int = 0, baseline=None, chunk: int = 256,
                    return_values: bool = False):
    """d target / d images of one RoViTKAN output for every image of the batch, or its integrated gradients.

    ``target``: ``'class'`` -- ``cls_logits[b, c_b]`` (``class_idx``: None for each image's argmax at ``x``, an int, or a (B,) integer
    tensor), ``'ordinal_severity'`` (stage >= 2; predict()'s sum_k k P(y = k)), ``'mu'``, ``'log_var'`` (stage >= 3) or
    ``'kan_severity'`` (stage 4), as in grad_cam_pp.
    ``steps == 0``: the gradient, (B,3,224,224) fp32.
    ``steps == m >= 1``: integrated gradients with the right Riemann rule, (x - x') * (1/m) sum_{s=1..m} grad f(x' + (s/m)(x - x')),
    x' = ``baseline`` (default zeros; any tensor broadcastable to x).  Each backbone call holds at most ``chunk`` images: as many
    interpolants of each image as fit (up to m), for as many images as then fit.
    ``return_values=True``: also the target's value at x, (B,) fp32, and for steps >= 1 at x' too: (grads, f(x)) or (attr, f(x), f(x')).

    Eval semantics, as grad_cam_pp: the bf16 engine whatever ``precision`` says, no dropout whatever the flags say; no ``.grad`` is
    written, ``requires_grad`` and training flags are left as they are.  The call uses workspaces of its own and leaves the engine's
    saved training activations, its flat gradient buffers and the backward's stream state alone, so it may run between a training forward
    and its backward.  Every bad argument is refused (RovitHipError) before anything is launched."""
    targets = _check_args(model, x, target, class_idx, steps, baseline, chunk)
    dev = x.device
    B = x.shape[0]
    with torch.no_grad():
        x32 = x.detach().float().contiguous()
        bb = _Backbone(model, dev)
        out = torch.empty(B, 3, 224, 224, device=dev, dtype=torch.float32)
        fx = torch.empty(B, device=dev, dtype=torch.float32)
        cls = targets.long() if targets is not None else None
        if steps == 0:
            for b0 in range(0, B, chunk):
                b1 = min(B, b0 + chunk)
                feats, ws = bb.features(x32[b0:b1], True)
                v, g = _seed(model, feats, target, cls[b0:b1] if cls is not None else None)
                fx[b0:b1] = v
                bb.pixels(x32[b0:b1], ws, g, out[b0:b1], 1, 1.0, 0)
            return (out, fx) if return_values else out
        xb = torch.zeros_like(x32) if baseline is None else baseline.detach().float().expand_as(x32).contiguous()
        diff = x32 - xb
        fxb = torch.empty(B, device=dev, dtype=torch.float32)
        if (target == 'class' and cls is None) or return_values:
            want_cls = target == 'class' and cls is None
            if want_cls:
                cls = torch.empty(B, device=dev, dtype=torch.long)
            for b0 in range(0, B, chunk):
                b1 = min(B, b0 + chunk)
                feats, _ = bb.features(x32[b0:b1], False)
                outs = _head_outputs(model, feats)
                if want_cls:
                    cls[b0:b1] = outs[0].argmax(dim=1)
                fx[b0:b1] = _target_value(target, outs, cls[b0:b1] if cls is not None else None)
                if return_values:
                    feats, _ = bb.features(xb[b0:b1], False)
                    fxb[b0:b1] = _target_value(target, _head_outputs(model, feats), cls[b0:b1] if cls is not None else None)
        m = steps
        k = min(m, chunk)                       # interpolants of one image per call
        nb = max(1, min(B, chunk // k))         # images per call
        for b0 in range(0, B, nb):
            b1 = min(B, b0 + nb)
            n = b1 - b0
            for s0 in range(1, m + 1, k):
                kk = min(k, m + 1 - s0)
                alpha = torch.tensor([s / m for s in range(s0, s0 + kk)], dtype=torch.float32, device=dev).view(kk, 1, 1, 1, 1)
                imgs = (xb[b0:b1].unsqueeze(0) + alpha * diff[b0:b1].unsqueeze(0)).reshape(kk * n, 3, 224, 224)   # rows s * n + b
                feats, ws = bb.features(imgs, True)
                _, g = _seed(model, feats, target, cls[b0:b1].repeat(kk) if cls is not None else None)
                bb.pixels(imgs, ws, g, out[b0:b1], kk, 1.0 / m, s0 > 1)
        attr = out.mul_(diff)
        return (attr, fx, fxb) if return_values else attr


def ig_reference(f, x: torch.Tensor, baseline: torch.Tensor, steps: int) -> torch.Tensor:
    """Integrated gradients of a scalar-per-sample function with autograd, the same right Riemann rule as input_gradients: the oracle
    the tests run in float64 on the CPU.  f maps (N,...) -> (N,)."""
    diff = x - baseline
    total = torch.zeros_like(x)
    for s in range(1, steps + 1):
        xi = (baseline + (s / steps) * diff).detach().requires_grad_(True)
        g, = torch.autograd.grad(f(xi).sum(), xi)
        total += g
    return diff * total / steps
