"""Kernels of the reference's `src.kernels` package, backed by the HIP library."""
from ._kernels import BaseKernel, GaussianKernel, IMQKernel, ScaledGaussianKernel, ScaledIMQKernel
from ._traj_kernels import (BatchGaussianKernel, BatchIMQKernel, BatchRationalQuadraticKernel, PathSigKernel,
                            SignatureKernel, TrajectoryKernel)

__all__ = sorted(
    ["BaseKernel", "BatchGaussianKernel", "BatchIMQKernel", "BatchRationalQuadraticKernel", "GaussianKernel", "IMQKernel",
     "PathSigKernel", "ScaledGaussianKernel", "ScaledIMQKernel", "SignatureKernel", "TrajectoryKernel"]
)
