"""Drop-in for the reference's explainability/gradcam.py (GradCAMPlusPlus, :10-160).

The reference hooks ``backbone.model.blocks[-1].norm1`` and back-propagates one class logit through the whole model.  This class
keeps the interface and computes the same map with the fused Grad-CAM++ path (rovit_hip.gradcam, csrc/gradcam.hip): a forward that
keeps only the last block and a backward that stops at that block's qkv gradient, for every image of the batch, with no parameter
gradient written -- so it also works on a frozen backbone."""
import numpy as np
import torch

from rovit_hip.gradcam import grad_cam_pp

_PLOTS = 'GradCAMPlusPlus.{}: needs cv2 and matplotlib, which this package does not depend on (plots are out of scope); ' \
         'use compute() / compute_batch() and draw the map with your own plotting code'


class GradCAMPlusPlus:
    """``model``: a RoViTKAN."""

    def __init__(self, model, device='cuda'):
        self.model = model
        self.device = device

    def compute_batch(self, images: torch.Tensor, class_idx=None, target='class'):
        """(B,224,224) fp32 maps on the device, one per image; ``class_idx``: None (each image's argmax), an int or a (B,) tensor.
        ``target`` (extension): the output explained -- 'class', 'ordinal_severity', 'mu', 'log_var' or 'kan_severity' -- or a list of
        them, which gives a dict name -> maps from one forward (rovit_hip.gradcam.grad_cam_pp)."""
        self.model.eval()
        return grad_cam_pp(self.model, images.to(self.device), class_idx, upsample=True, target=target)

    def compute(self, image_tensor: torch.Tensor, class_idx: int = None, target='class'):
        """The reference's contract (gradcam.py:34-104): the (224,224) map of item 0 as numpy, for ``class_idx`` or item 0's argmax
        (a dict name -> map for a list of targets).  The caller's tensor is not modified (the reference sets its requires_grad; nothing
        here needs it)."""
        maps = self.compute_batch(image_tensor, class_idx, target)
        if isinstance(maps, dict):
            return {n: m[0].cpu().numpy() for n, m in maps.items()}
        return maps[0].cpu().numpy()

    def overlay_on_image(self, image, cam, alpha=0.5, colormap=None):
        raise NotImplementedError(_PLOTS.format('overlay_on_image'))

    def visualize(self, image_tensor, original_image, class_idx=None, save_path=None):
        raise NotImplementedError(_PLOTS.format('visualize'))
