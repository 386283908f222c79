from .math import bw_from_median, bw_median
from .scheduler import CosineScheduler, FactorScheduler, SquareRootScheduler
from .spline import NaturalCubicSpline, create_spline_trajectory, natural_cubic_spline_coeffs

__all__ = ["bw_median", "bw_from_median", "SquareRootScheduler", "FactorScheduler", "CosineScheduler",
           "NaturalCubicSpline", "natural_cubic_spline_coeffs", "create_spline_trajectory"]
