"""Rigid analytic obstacles for T10 meshes: half-spaces and solid spheres in implicit penalty contact with
the surface nodes.  Hand a list of them to GPU_FEAT10_Data.SetRigidObstacles; UpdateRigidObstacle moves one between
steps.  Every value is checked here, before the C-ABI (which checks them again).

RigidField (DESIGN 3e'') is a rigid obstacle of any closed shape, given as a regular grid of signed-distance samples with a
rigid pose; it goes to SetFieldObstacles / UpdateFieldObstacle of the three data classes, beside the analytic list."""
import ctypes as C
import math

import numpy as np

from .binding import FieldObstacleC, ObstacleC, check, dp, ip, load_library

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


MAX_FIELD_SAMPLES = 1 << 27


def check_closed_surface(V, T):
    """V (n, 3) float, T (m, 3) int: raises ValueError unless the triangles form a closed, consistently oriented surface
    without degenerate triangles (every directed edge occurs once and its reverse once).  Returns (V, T) as contiguous
    float64 / int32 arrays."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    Ti = np.asarray(T)
    if V.ndim != 2 or V.shape[1] != 3 or Ti.ndim != 2 or Ti.shape[1] != 3:
        raise ValueError(f"vertices must be (n, 3) and triangles (m, 3), got {V.shape} and {Ti.shape}")
    if not np.issubdtype(Ti.dtype, np.integer):
        raise ValueError("triangle indices must be integers")
    if V.shape[0] < 4 or Ti.shape[0] < 4:
        raise ValueError("a closed surface needs at least 4 vertices and 4 triangles")
    if not np.all(np.isfinite(V)):
        raise ValueError("vertices must be finite")
    if Ti.min() < 0 or Ti.max() >= V.shape[0]:
        raise ValueError(f"triangle indices must lie in 0..{V.shape[0] - 1}")
    Ti = np.ascontiguousarray(Ti, dtype=np.int32)
    a, b, c = V[Ti[:, 0]], V[Ti[:, 1]], V[Ti[:, 2]]
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    if not np.all(area2 > 0):
        raise ValueError(f"triangle {int(np.argmin(area2 > 0))} has zero area")
    e = np.concatenate([Ti[:, [0, 1]], Ti[:, [1, 2]], Ti[:, [2, 0]]]).astype(np.int64)
    fwd = e[:, 0] * V.shape[0] + e[:, 1]
    if np.unique(fwd).size != fwd.size:
        raise ValueError("the surface is not consistently oriented (a directed edge occurs twice)")
    if not np.all(np.isin(e[:, 1] * V.shape[0] + e[:, 0], fwd)):
        raise ValueError("the surface is open (an edge has no opposite)")
    return V, Ti


def sdf_from_triangles(V, T, shape, origin, spacing):
    """Signed distance (negative inside) of the closed surface (V, T) at the grid points origin + spacing * (ix, iy, iz),
    computed on the device; shape = (nx, ny, nz), the result is indexed [iz, iy, ix]."""
    V, T = check_closed_surface(V, T)
    nx, ny, nz = (int(n) for n in shape)
    if min(nx, ny, nz) < 1 or nx * ny * nz > MAX_FIELD_SAMPLES:
        raise ValueError(f"the grid needs 1..2^27 samples, got {nx} x {ny} x {nz}")
    origin = _vec3(origin, "origin")
    if not (math.isfinite(float(spacing)) and spacing > 0):
        raise ValueError(f"spacing must be > 0, got {spacing}")
    out = np.zeros((nz, ny, nx))
    check(load_library().tlfea_sdf_from_triangles(dp(V), V.shape[0], ip(T), T.shape[0], nx, ny, nz, dp(origin),
                                                  C.c_double(float(spacing)), dp(out)))
    return out


class RigidField:
    """Rigid obstacle given as signed-distance samples (negative inside the body) on a regular grid: values[iz, iy, ix] at
    origin + spacing * (ix, iy, iz) in the obstacle's frame, which `position` and `rotation` (3 x 3, frame -> world) place
    in the world.  The gap is the quadratic B-spline interpolant of the samples; the obstacle acts only inside its grid
    (half a spacing in from the outermost samples).  Every sample must be finite and the two outermost layers of each axis
    positive: a closed body well inside its grid.  The other arguments as RigidPlane's."""
    kind = 2

    def __init__(self, values, origin, spacing, stiffness, friction=0.0, eps_v=1e-3, position=0.0, rotation=None,
                 velocity=0.0):
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim != 3:
            raise ValueError(f"values must be a 3-d array indexed [iz, iy, ix], got shape {v.shape}")
        if min(v.shape) < 5:
            raise ValueError(f"every axis needs at least 5 samples, got {v.shape[2]} x {v.shape[1]} x {v.shape[0]}")
        if v.size > MAX_FIELD_SAMPLES:
            raise ValueError(f"at most 2^27 samples, got {v.size}")
        if not np.all(np.isfinite(v)):
            raise ValueError("every sample must be finite")
        rim = np.ones(v.shape, dtype=bool)
        rim[2:-2, 2:-2, 2:-2] = False
        if not np.all(v[rim] > 0):
            raise ValueError("every sample of the two outermost layers must be > 0 (the body must lie well inside its grid)")
        self.values = v
        self.origin = _vec3(origin, "origin")
        if not (math.isfinite(float(spacing)) and spacing > 0):
            raise ValueError(f"spacing must be > 0, got {spacing}")
        self.spacing = float(spacing)
        self.stiffness, self.friction, self.eps_v = _common(stiffness, friction, eps_v)
        self.velocity = _vec3(velocity, "velocity")
        self._set_pose(position, rotation)

    def _set_pose(self, position, rotation):
        position = _vec3(position, "position")
        R = np.eye(3) if rotation is None else np.array(rotation, dtype=np.float64)
        if R.shape != (3, 3) or not np.all(np.isfinite(R)):
            raise ValueError("rotation must be a finite 3 x 3 matrix")
        if not (np.max(np.abs(R @ R.T - np.eye(3))) <= 1e-12 and np.linalg.det(R) > 0):
            raise ValueError("rotation must be orthonormal (to 1e-12) with determinant +1")
        self.position, self.rotation = position, R

    def moved(self, position=None, rotation=None, velocity=None):
        """A field of the same samples (shared, not copied) at another pose: the argument of UpdateFieldObstacle."""
        other = object.__new__(RigidField)
        other.__dict__.update(self.__dict__)
        other._set_pose(self.position if position is None else position, self.rotation if rotation is None else rotation)
        if velocity is not None:
            other.velocity = _vec3(velocity, "velocity")
        return other

    @property
    def shape(self):
        """(nx, ny, nz)"""
        return self.values.shape[::-1]

    def to_c(self):
        nx, ny, nz = self.shape
        return FieldObstacleC(nx, ny, nz, tuple(self.origin), self.spacing, tuple(self.position),
                              tuple(self.rotation.reshape(-1)), tuple(self.velocity), self.stiffness, self.friction,
                              self.eps_v)

    @classmethod
    def from_function(cls, f, lo, hi, spacing, stiffness, **kw):
        """Samples f (points (..., 3) -> signed distance) on the grid lo, lo + spacing, ... that reaches hi on every axis."""
        lo, hi = _vec3(lo, "lo"), _vec3(hi, "hi")
        if not (math.isfinite(float(spacing)) and spacing > 0):
            raise ValueError(f"spacing must be > 0, got {spacing}")
        if not np.all(hi > lo):
            raise ValueError("hi must exceed lo on every axis")
        n = np.ceil((hi - lo) / spacing - 1e-9).astype(int) + 1
        if int(np.prod(n.astype(np.int64))) > MAX_FIELD_SAMPLES:
            raise ValueError(f"at most 2^27 samples, got {n[0]} x {n[1]} x {n[2]}")
        iz, iy, ix = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
        pts = lo + spacing * np.stack([ix, iy, iz], axis=-1)
        return cls(np.asarray(f(pts), dtype=np.float64).reshape(n[2], n[1], n[0]), lo, spacing, stiffness, **kw)

    @classmethod
    def from_triangles(cls, V, T, spacing, stiffness, margin=3.0, **kw):
        """The signed distance of the closed triangle surface (V, T), built on the device, on a grid that extends `margin`
        spacings (at least 2.5) beyond the surface's bounding box."""
        V, T = check_closed_surface(V, T)
        if not (math.isfinite(float(margin)) and margin >= 2.5):
            raise ValueError(f"margin must be at least 2.5 spacings, got {margin}")
        if not (math.isfinite(float(spacing)) and spacing > 0):
            raise ValueError(f"spacing must be > 0, got {spacing}")
        lo = V.min(axis=0) - margin * spacing
        n = np.ceil((V.max(axis=0) + margin * spacing - lo) / spacing - 1e-9).astype(int) + 1
        if int(np.prod(n.astype(np.int64))) > MAX_FIELD_SAMPLES:
            raise ValueError(f"at most 2^27 samples, got {n[0]} x {n[1]} x {n[2]}")
        return cls(sdf_from_triangles(V, T, n, lo, spacing), lo, spacing, stiffness, **kw)

    @classmethod
    def from_t10_surface(cls, data, spacing, stiffness, current=False, **kw):
        """The boundary of a T10 mesh (GPU_FEAT10_Data.GetBoundaryTriangles) as a rigid obstacle."""
        V, T = data.GetBoundaryTriangles(current=current)
        return cls.from_triangles(V, T, spacing, stiffness, **kw)


def fields_as_c(fields):
    """(FieldObstacleC array, array of sample pointers, n) of a list of RigidField; the fields keep the samples alive."""
    fields = list(fields)
    for f in fields:
        if not isinstance(f, RigidField):
            raise ValueError(f"expected a RigidField, got {type(f).__name__}")
    if len(fields) > MAX_OBSTACLES:
        raise ValueError(f"at most {MAX_OBSTACLES} obstacles per object, got {len(fields)}")
    arr = (FieldObstacleC * max(1, len(fields)))(*[f.to_c() for f in fields])
    ptrs = (C.POINTER(C.c_double) * max(1, len(fields)))(*[dp(f.values) for f in fields])
    return arr, ptrs, len(fields)
