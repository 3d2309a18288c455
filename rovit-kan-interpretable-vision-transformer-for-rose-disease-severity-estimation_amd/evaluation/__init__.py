"""Drop-in for the reference's ``evaluation`` package: the same names and signatures, computed by ``rovit_hip.evaluation`` (one device
synchronisation per epoch; fp64 on the host; neither sklearn nor scipy)."""
from .evaluator import Evaluator, load_model_for_evaluation  # noqa: F401
