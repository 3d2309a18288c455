"""Attention rollout on the GPU (csrc/rollout.hip): what the reference's ViTAttentionRollout.generate
(explainability/attention_maps.py:40-105) computes from hooked attention probabilities, for a whole batch, without ever
storing a 197x197 matrix."""
import torch

from .native import RovitHipError, call, ptr, ptr_array, stream_ptr

HEAD_FUSION = {'mean': 0, 'max': 1, 'min': 2}


def attention_rollout(model, x: torch.Tensor, head_fusion: str = 'mean', upsample: bool = True) -> torch.Tensor:
    """Row 0 of  A^_1 ... A^_depth  without the class-token entry, A^_l = rownorm(fuse_heads(P_l) + I).

    ``upsample=True``: the reference's map, (B,224,224) fp32 -- bilinear resize of the 14x14 grid (cv2.resize INTER_LINEAR)
    and per-image min-max normalisation (attention_maps.py:96-103).  ``upsample=False``: the raw (B,14,14) rollout.
    ``head_fusion``: 'mean', 'max' or 'min' over the three heads (attention_maps.py:63-70).  Runs on the bf16 engine, as
    ``attention_probabilities`` does, whatever ``model.precision`` says.  ``model`` is the DeiTTiny parameter container
    (``backbone.model``)."""
    if head_fusion not in HEAD_FUSION:
        raise RovitHipError(f"attention_rollout: head_fusion must be one of {sorted(HEAD_FUSION)}, got {head_fusion!r}")
    if not x.is_cuda:
        raise RovitHipError('attention_rollout: the images must be on the GPU (there is no CPU fallback)')
    x = x.float().contiguous()
    params = model.ordered_parameters()
    eng = model.engine
    eng.prepare(params)
    B = x.shape[0]
    ws = eng.take_ws(B, False, x.device)
    feats = torch.empty(B, 192, device=x.device, dtype=torch.float32)
    v = torch.empty(B, 197, device=x.device, dtype=torch.float32)
    with torch.no_grad():
        call('rovit_vit_forward_rollout', ptr(x), ptr_array(params), ptr(eng.prep), ptr(ws), ptr(feats), ptr(v),
             HEAD_FUSION[head_fusion], B, eng.depth, stream_ptr())
        eng.give_ws(B, False, ws)
        if not upsample:
            return v[:, 1:].reshape(B, 14, 14)
        out = torch.empty(B, 224, 224, device=x.device, dtype=torch.float32)
        call('rovit_rollout_map', ptr(v), ptr(out), B, stream_ptr())
    return out
