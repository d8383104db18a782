"""Training: the step (`InstanceSegmentation`), the loop around it (`TrainLoop`, `fit`) and the export post-processing."""
from .loop import TrainLoop, fit  # noqa: F401
from .trainer import InstanceSegmentation, StepsInFlight, prepare_steady_state  # noqa: F401
