"""The neural ModelFamily members (openea/models/neural/__init__.py) that need relation triples only: ProjE, on the fused
sampled-softmax step of csrc/proje_step.hip, and ConvE -- conv2d, three more batch norms, dropout in front of the same NCE output
half -- on csrc/conve_step.hip."""
from .conve import ConvE  # noqa: F401
from .proje import ProjE  # noqa: F401
