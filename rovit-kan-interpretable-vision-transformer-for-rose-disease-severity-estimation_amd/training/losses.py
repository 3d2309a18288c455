"""``training.losses`` of the reference (training/losses.py:117-181) on the HIP path: ``JointLoss`` is ``rovit_hip.losses.JointLoss``,
same constructor, call signature and returned dict, one launch for the loss and its gradient; ``JointLoss.mixed`` is the CutMix / MixUp
form the Trainer uses."""
from rovit_hip.losses import JointLoss  # noqa: F401
