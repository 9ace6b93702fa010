"""The semantic-matching ModelFamily members (openea/models/semantic/__init__.py): DistMult (trilinear product), HolE
(circular correlation) and SimplE (two entity and two relation tables) on one fused device step (csrc/semantic_step.hip), and
RotatE (rotations in the complex plane, fp64) on the step it shares with BootEA_RotatE (csrc/rotate_step.hip)."""
from .distmult import DistMult  # noqa: F401
from .hole import HolE  # noqa: F401
from .rotate import RotatE  # noqa: F401
from .simple import SimplE  # noqa: F401
