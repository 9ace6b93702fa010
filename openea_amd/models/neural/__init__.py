"""The neural ModelFamily members (openea/models/neural/__init__.py) that need relation triples only: ProjE, on the fused
sampled-softmax step of csrc/proje_step.hip.  (ConvE -- conv2d, three more batch norms, dropout in front of the same NCE output
half -- is not built.)"""
from .proje import ProjE  # noqa: F401
