"""``training.optimizer`` of the reference (training/optimizer.py:7-49) on the HIP path: ``build_optimizer`` returns a ``RoViTAdamW``
(the reference's two parameter groups; the gradient clip of training/trainer.py:123-126 is inside its ``step()``), ``build_scheduler`` the
same ``CosineAnnealingLR``, ``get_lr`` the first group's rate."""
from rovit_hip.optim import RoViTAdamW, build_optimizer, build_scheduler, get_lr  # noqa: F401
