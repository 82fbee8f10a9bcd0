"""Rigid analytic obstacles for T10 meshes: half-spaces and solid spheres in implicit penalty contact with
the surface nodes.  Hand a list of them to GPU_FEAT10_Data.SetRigidObstacles; UpdateRigidObstacle moves one between
steps.  Every value is checked here, before the C-ABI (which checks them again)."""
import math

import numpy as np

from .binding import ObstacleC

MAX_OBSTACLES = 16  # per element object (include/tlfea_c.h)


def _vec3(v, what):
    a = np.broadcast_to(np.asarray(v, dtype=np.float64), (3,)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)
    if a.shape != (3,):
        raise ValueError(f"{what} must be a 3-vector, got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what} must be finite")
    return a.copy()


def _common(stiffness, friction, eps_v):
    for name, v in (("stiffness", stiffness), ("friction", friction), ("eps_v", eps_v)):
        if not math.isfinite(float(v)):
            raise ValueError(f"{name} must be finite")
    if not stiffness > 0:
        raise ValueError(f"stiffness must be > 0 (Pa/m), got {stiffness}")
    if not friction >= 0:
        raise ValueError(f"friction must be >= 0, got {friction}")
    if not eps_v > 0:
        raise ValueError(f"eps_v must be > 0 (m/s), got {eps_v}")
    return float(stiffness), float(friction), float(eps_v)


class RigidPlane:
    """Half-space {x : normal . (x - point) < 0} behind the plane through `point`; `normal` is the outward unit normal.
    stiffness: Pa/m (pressure per metre of penetration); friction: Coulomb coefficient; eps_v: slip velocity below which
    friction is regularised; velocity: the plane's velocity (friction only)."""
    kind = 0

    def __init__(self, point, normal, stiffness, friction=0.0, eps_v=1e-3, velocity=0.0):
        self.point = _vec3(point, "point")
        self.normal = _vec3(normal, "normal")
        if not abs(float(np.linalg.norm(self.normal)) - 1.0) <= 1e-12:
            raise ValueError(f"normal must have unit length (to 1e-12), got |n| = {np.linalg.norm(self.normal)!r}")
        self.stiffness, self.friction, self.eps_v = _common(stiffness, friction, eps_v)
        self.velocity = _vec3(velocity, "velocity")

    def to_c(self):
        return ObstacleC(self.kind, tuple(self.point), tuple(self.normal), 0.0, tuple(self.velocity), self.stiffness,
                         self.friction, self.eps_v)


class RigidSphere:
    """Solid sphere of centre `center` and radius `radius`; the other arguments as RigidPlane's."""
    kind = 1

    def __init__(self, center, radius, stiffness, friction=0.0, eps_v=1e-3, velocity=0.0):
        self.center = _vec3(center, "center")
        if not (math.isfinite(float(radius)) and radius > 0):
            raise ValueError(f"radius must be > 0, got {radius}")
        self.radius = float(radius)
        self.stiffness, self.friction, self.eps_v = _common(stiffness, friction, eps_v)
        self.velocity = _vec3(velocity, "velocity")

    def to_c(self):
        return ObstacleC(self.kind, tuple(self.center), (0.0, 0.0, 0.0), self.radius, tuple(self.velocity),
                         self.stiffness, self.friction, self.eps_v)


def as_c(obstacle):
    if not isinstance(obstacle, (RigidPlane, RigidSphere)):
        raise ValueError(f"expected a RigidPlane or RigidSphere, got {type(obstacle).__name__}")
    return obstacle.to_c()
