"""Explanation by training example in the interface of this package's explainers (PatchSHAP, GradCAMPlusPlus).

The reference has none: its explanations are maps over the image.  TrainingInfluence names the recorded training rows whose removal would
raise the loss of the prediction made (proponents) and the ones whose removal would lower it (opponents), through the last layer of the
classification head.  The work is rovit_hip.influence.HeadInfluence (csrc/influence.hip)."""
import torch


class TrainingInfluence:
    """``model``: a RoViTKAN; ``influence``: the ``HeadInfluence`` of ``model.fit_influence(train_loader)``."""

    def __init__(self, model, influence, device=None):
        self.model = model
        self.influence = influence
        self.device = device if device is not None else influence.device

    def explain_batch(self, images: torch.Tensor, k: int = 5, labels=None, relative: bool = True):
        """``RoViTKAN.influential_examples``' result dict for every image, tensors on the device."""
        self.model.eval()
        return self.model.influential_examples(images.to(self.device), self.influence, k=k, labels=labels, relative=relative)

    def explain(self, image_tensor: torch.Tensor, k: int = 5, labels=None, relative: bool = True):
        """Item 0's proponents and opponents as a list of k dicts each, best first: ``{'index', 'score', 'label'}`` (slots beyond the valid
        rows are left out)."""
        res = {name: v[0].cpu() for name, v in self.explain_batch(image_tensor, k, labels, relative).items() if v.dim() == 2}
        out = {}
        for end in ('pro', 'opp'):
            out['proponents' if end == 'pro' else 'opponents'] = [
                {'index': int(i), 'score': float(s), 'label': int(y)}
                for i, s, y in zip(res[end + '_indices'], res[end + '_scores'], res[end + '_labels']) if int(i) >= 0]
        return out
