"""Patch Shapley values in the interface of this package's explainers (GradCAMPlusPlus, ViTAttentionRollout).

The reference has no Shapley explainer: its maps read gradients or attention weights of the network.  PatchSHAP is black-box -- it only
evaluates the model on images with patches removed -- and its values sum to f(image) - f(nothing).  The work is rovit_hip.shap.patch_shap
(csrc/shap.hip and the token-gather forwards of csrc/perturb.hip)."""
import torch

from rovit_hip.shap import patch_shap


class PatchSHAP:
    """``model``: a RoViTKAN."""

    def __init__(self, model, device='cuda'):
        self.model = model
        self.device = device

    def explain_batch(self, images: torch.Tensor, class_idx=None, target='class', **kwargs):
        """patch_shap's result dict for every image (a dict name -> result for a list of targets), tensors on the device.  ``kwargs``:
        num_samples, players, perturbation, baseline, seed, chunk, upsample, return_values, ragged (rovit_hip.shap.patch_shap)."""
        self.model.eval()
        return patch_shap(self.model, images.to(self.device), target, class_idx, **kwargs)

    def explain(self, image_tensor: torch.Tensor, class_idx: int = None, target='class', **kwargs):
        """The (224,224) map of item 0 as numpy (a dict name -> map for a list of targets), for ``class_idx`` or item 0's argmax."""
        res = self.explain_batch(image_tensor, class_idx, target, **kwargs)
        if isinstance(target, (list, tuple)):
            return {n: r['shap'][0].cpu().numpy() for n, r in res.items()}
        return res['shap'][0].cpu().numpy()
