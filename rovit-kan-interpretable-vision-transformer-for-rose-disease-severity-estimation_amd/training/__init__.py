"""Drop-in ``training`` package: the reference's import paths (``training.trainer.Trainer``, ``training.losses.JointLoss``,
``training.optimizer.build_optimizer``) on the HIP path.  See INTEGRATION.md section C."""
from .losses import JointLoss  # noqa: F401
from .optimizer import build_optimizer, build_scheduler, get_lr  # noqa: F401
from .trainer import Trainer  # noqa: F401
