"""Homotopy value schedule of the reference (src/utils/homotopy.jl:22-73): the sharpness of a smooth approximation (a sigmoid
here) as a function of a sweep variable x in [0, 1], chosen so that the transition width of the sigmoid shrinks geometrically from
delta_max to delta_min."""
import math


class Homotopy:
    """`Homotopy(delta_min; delta_max = 1.0, eps = 1e-2)`.  A sigmoid 1 / (1 + exp(-kappa d)) is within eps of its limits outside
    |d| <= delta when kappa = log(1 / eps - 1) / delta; the sweep takes delta = delta_max rho^x with rho = delta_min / delta_max."""

    def __init__(self, delta_min, delta_max=1.0, eps=1e-2):
        self.delta_min, self.delta_max, self.eps = float(delta_min), float(delta_max), float(eps)
        self.rho = self.delta_min / self.delta_max

    def __call__(self, x):
        return math.log(1.0 / self.eps - 1.0) / (self.rho ** float(x) * self.delta_max)
