"""Drop-in for the reference's ``explainability`` package: attention rollout, Grad-CAM++ and the KAN head's edge statistics computed on the GPU."""
from .attention_maps import ViTAttentionRollout  # noqa: F401
from .attention_heads import AttentionHeadAnalysis  # noqa: F401
from .gradcam import GradCAMPlusPlus  # noqa: F401
from .kan_viz import KANVisualizer  # noqa: F401
from .shap import PatchSHAP  # noqa: F401
from .influence import TrainingInfluence  # noqa: F401
