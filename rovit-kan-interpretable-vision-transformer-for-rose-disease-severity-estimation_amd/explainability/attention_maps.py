"""Drop-in for the reference's explainability/attention_maps.py (ViTAttentionRollout, :10-160).

The reference hooks ``blocks[i].attn`` to collect attention probabilities; on current timm that hook sees the module's
output (B,197,192), so its rollout is computed from the wrong tensor.  This class keeps the interface and
computes what the reference means to: the rollout runs inside the fused backbone forward (csrc/rollout.hip) for every
image of the batch, from the bf16 engine's attention probabilities."""
import numpy as np
import torch

from rovit_hip.rollout import HEAD_FUSION

_PLOTS = 'ViTAttentionRollout.{}: needs cv2 and matplotlib, which this package does not depend on (plots are out of scope); ' \
         'use generate() / generate_batch() and draw the map with your own plotting code'


class ViTAttentionRollout:
    """``model``: a RoViTKAN or a DeiTTinyBackbone (anything with ``attention_rollout``).

    ``discard_ratio`` is stored and never used, as in the reference (attention_maps.py:12-15): no low-attention entries are
    discarded."""

    def __init__(self, model, device='cuda', discard_ratio=0.9):
        self.model = model
        self.device = device
        self.discard_ratio = discard_ratio

    def generate_batch(self, images: torch.Tensor, head_fusion: str = 'mean') -> torch.Tensor:
        """(B,224,224) fp32 maps on the device, one per image; an unknown ``head_fusion`` means 'mean' (attention_maps.py:63-70)."""
        self.model.eval()
        fusion = head_fusion if head_fusion in HEAD_FUSION else 'mean'
        return self.model.attention_rollout(images.to(self.device), head_fusion=fusion, upsample=True)

    def generate(self, image_tensor: torch.Tensor, head_fusion: str = 'mean') -> np.ndarray:
        """The reference's contract (attention_maps.py:40-105): the whole batch runs, the (224,224) map of item 0 is returned as numpy."""
        return self.generate_batch(image_tensor, head_fusion)[0].cpu().numpy()

    def overlay_on_image(self, image, attention_map, alpha=0.5, colormap=None):
        raise NotImplementedError(_PLOTS.format('overlay_on_image'))

    def visualize(self, image_tensor, original_image, save_path=None):
        raise NotImplementedError(_PLOTS.format('visualize'))
