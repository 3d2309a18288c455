"""Gradient-weighted attention relevance (Chefer, Gur & Wolf, "Generic Attention-model Explainability for Interpreting Bi-Modal and
Encoder-Decoder Transformers", ICCV 2021) of a RoViTKAN output, on the GPU, and its fp64 reference.

For block l with per-head softmax probabilities P_{l,h} and G_{l,h} = d y / d P_{l,h} of one scalar y per image,

    A_l = mean_h relu(G_{l,h} * P_{l,h}),   R_0 = I,   R_l = R_{l-1} + A_l R_{l-1}   (l = 1..L, forward order),

and the relevance of the tokens is row 0 of R_L (avg_heads, apply_self_attention_rules and R[0, 1:] of the paper's reference code).
Since R_L = (I + A_L) ... (I + A_1), row 0 is also a vector recursion in backward order (u = e_0, u <- u + u A_l for l = L..1), the
order in which the backbone's dgrad chain visits the blocks.  One GPU call runs, per chunk of images, the fused training-mode forward,
the head phase on the features (its own backward gives d target / d features, as for input_gradients) and the dgrad chain alone with
one relevance step behind every block's attention-output gradient (rovit_vit_backward_relevance; csrc/relevance.hip), so no 197x197
matrix is stored.  relevance_reference keeps the matrix form so that it stays an independent statement of the method."""
import torch

from .input_grad import _Backbone, _check_args, _seed
from .native import call, ptr, stream_ptr


def relevance_vectors(model, x: torch.Tensor, target='class', class_idx=None, chunk: int = 256):
    """(relevance (B,197) fp32 = row 0 of R_L with the class token's entry, the target's value (B,) fp32): what attention_relevance
    maps, with its arguments and semantics."""
    targets = _check_args(model, x, target, class_idx, 0, None, chunk, 'attention_relevance')
    dev = x.device
    B = x.shape[0]
    with torch.no_grad():
        x32 = x.detach().float().contiguous()
        bb = _Backbone(model, dev)
        rel = torch.empty(B, 197, device=dev, dtype=torch.float32)
        fx = torch.empty(B, device=dev, dtype=torch.float32)
        scratch = torch.empty(min(B, chunk) * 3 * 197, device=dev, dtype=torch.float32)
        cls = targets.long() if targets is not None else None
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            feats, ws = bb.features(x32[b0:b1], True)
            v, g = _seed(model, feats, target, cls[b0:b1] if cls is not None else None)
            fx[b0:b1] = v
            bb.relevance(ws, g, rel[b0:b1], scratch)
    return rel, fx


def attention_relevance(model, x: torch.Tensor, target='class', class_idx=None, upsample: bool = True, chunk: int = 256,
                        return_values: bool = False):
    """Gradient-weighted attention relevance of one RoViTKAN output for every image of the batch, through every block.

    ``target``: ``'class'`` -- ``cls_logits[b, c_b]`` (``class_idx``: None for each image's argmax, an int, or a (B,) integer tensor),
    ``'ordinal_severity'`` (stage >= 2), ``'mu'``, ``'log_var'`` (stage >= 3) or ``'kan_severity'`` (stage 4), as in input_gradients;
    one target per call.  ``upsample=True``: (B,224,224) fp32, row 0 of R_L without the class token as 14x14, resized bilinearly and
    min-max normalised per image (rovit_rollout_map, the map of attention_rollout).  ``upsample=False``: the raw (B,14,14).
    ``return_values=True``: also the target's value at x, (B,) fp32.  At most ``chunk`` images per backbone call.

    Eval semantics, as input_gradients: the bf16 engine whatever ``precision`` says, no dropout; no ``.grad`` is written and
    ``requires_grad`` / training flags are left as they are; workspaces come from the engine's pool, so the call may run between a
    training forward and its backward.  Every bad argument is refused (RovitHipError) before anything is launched."""
    rel, fx = relevance_vectors(model, x, target, class_idx, chunk)
    B = rel.shape[0]
    if upsample:
        out = torch.empty(B, 224, 224, device=rel.device, dtype=torch.float32)
        call('rovit_rollout_map', ptr(rel), ptr(out), B, stream_ptr())
    else:
        out = rel[:, 1:].reshape(B, 14, 14)
    return (out, fx) if return_values else out


def relevance_reference(attn_probs, value: torch.Tensor) -> torch.Tensor:
    """Row 0 of R_L, (B,N), by the forward-order matrix recursion.

    ``attn_probs``: the blocks' (B,H,N,N) softmax probabilities in forward order, in the autograd graph of ``value`` (B,), one scalar per
    image -- e.g. collected with ``oracle.ref_cpu.vit_forward(..., attn_probs=list)``.  The images must not interact (as in a ViT), so
    that the gradient of ``value.sum()`` is each image's own.  The graph is kept, so several targets may share one forward.  The oracle
    the tests run in float64 on the CPU, in the pattern of ``input_grad.ig_reference``."""
    probs = list(attn_probs)
    grads = torch.autograd.grad(value.sum(), probs, retain_graph=True)
    with torch.no_grad():
        B, _, N, _ = probs[0].shape
        R = torch.eye(N, dtype=probs[0].dtype, device=probs[0].device).expand(B, N, N)
        for P, G in zip(probs, grads):
            A = (G * P).clamp(min=0).mean(dim=1)
            R = R + A @ R
        return R[:, 0, :].clone()
