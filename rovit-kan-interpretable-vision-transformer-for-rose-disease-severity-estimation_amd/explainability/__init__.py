"""Drop-in for the reference's ``explainability`` package: attention rollout computed on the GPU."""
from .attention_maps import ViTAttentionRollout  # noqa: F401
