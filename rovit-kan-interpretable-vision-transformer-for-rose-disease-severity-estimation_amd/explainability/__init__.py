"""Drop-in for the reference's ``explainability`` package: attention rollout and Grad-CAM++ computed on the GPU."""
from .attention_maps import ViTAttentionRollout  # noqa: F401
from .gradcam import GradCAMPlusPlus  # noqa: F401
