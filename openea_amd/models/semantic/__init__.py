"""The semantic-matching ModelFamily members (openea/models/semantic/__init__.py) that the reference ships run configs for:
HolE (circular correlation) and SimplE (two entity and two relation tables), on one fused device step
(csrc/semantic_step.hip).  (DistMult -- no shipped args file, a labelled-batch epoch loop -- and the plain RotatE are not
built.)"""
from .hole import HolE  # noqa: F401
from .simple import SimplE  # noqa: F401
