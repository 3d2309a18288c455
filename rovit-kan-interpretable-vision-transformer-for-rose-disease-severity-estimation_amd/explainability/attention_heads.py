"""Per-head attention analysis (no counterpart in the reference's explainability package): the statistics of
rovit_hip.head_stats -- entropy, mean attention distance, class-token mass, locality per (image, block, head) -- and the class
token's attention map of every head and block, computed inside the fused backbone forward (csrc/head_stats.hip).  No plotting."""
import torch

from rovit_hip.head_stats import STAT_NAMES, TOKEN_STAT_NAMES  # noqa: F401
from rovit_hip.native import call, ptr, stream_ptr


class AttentionHeadAnalysis:
    """``model``: a RoViTKAN or a DeiTTinyBackbone (anything with ``attention_head_stats``)."""

    def __init__(self, model, device='cuda'):
        self.model = model
        self.device = device

    def compute(self, image_tensor: torch.Tensor, per_token: bool = False):
        """The dict of ``attention_head_stats`` for the batch: ``summary`` (B, L, 3, 8), ``cls_attention`` (B, L, 3, 196), ..."""
        self.model.eval()
        return self.model.attention_head_stats(image_tensor.to(self.device), per_token=per_token)

    def cls_maps(self, image_tensor: torch.Tensor, upsample: bool = True) -> torch.Tensor:
        """The class token's attention over the patches, per head and block: (B, L, 3, 224, 224) fp32 maps in [0, 1] -- bilinear resize
        of the 14x14 grid and min-max normalisation per map, the map of the attention rollout (rovit_rollout_map) -- or with
        ``upsample=False`` the raw (B, L, 3, 14, 14) probabilities.  The upsampled maps are materialised at once: 224 x 224 fp32 per
        (image, block, head), 7.2 MB per image at depth 12 and 1.8 GB at batch 256 -- pass the images a few at a time, or take
        ``upsample=False`` (0.6 KB per map) and resize the maps that are drawn."""
        out = self.compute(image_tensor)
        cls = out['cls_attention']
        B, L, H = cls.shape[:3]
        if not upsample:
            return cls.reshape(B, L, H, 14, 14)
        rows = torch.empty(B * L * H, 197, device=cls.device, dtype=torch.float32)
        rows[:, 0] = out['summary'][..., 5].reshape(-1)          # the class entry in slot 0 (the map kernel skips it)
        rows[:, 1:] = cls.reshape(B * L * H, 196)
        maps = torch.empty(B * L * H, 224, 224, device=cls.device, dtype=torch.float32)
        call('rovit_rollout_map', ptr(rows), ptr(maps), B * L * H, stream_ptr())
        return maps.view(B, L, H, 224, 224)
