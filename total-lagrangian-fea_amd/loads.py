"""Distributed surface loads for ANCF beam and shell meshes: a dead traction (force per reference area, fixed
direction) and a follower pressure (normal to the deformed face), each on one face of a list of elements.  Hand them to
GPU_ANCF3243_Data / GPU_ANCF3443_Data.AddSurfaceTraction / AddFollowerPressure, or build the objects here and pass them
to AddSurfaceLoad; SetLoadScale ramps one between steps.  Faces: shell zeta = -1, +1 -> 0, 1; beam eta = -1, +1,
zeta = -1, +1 -> 0..3.  A T10 mesh takes the same two loads on a list of its boundary faces (DESIGN 3h',
GPU_FEAT10_Data.GetBoundaryFaces / AddFaceTraction / AddFacePressure): FaceLoad below.  Every value is checked here, before
the C-ABI (which checks them again)."""
import collections
import math

import numpy as np

from .binding import SurfaceLoadC, T10SurfaceLoadC, ip

MAX_LOADS = 16  # surface loads per element object (include/tlfea_c.h)
FACES = {8: 4, 16: 2}  # faces that can carry a load, by shape functions per element (beam, shell)


def _elements(elements):
    e = np.asarray(elements)
    if e.ndim != 1 or e.size == 0:
        raise ValueError("a surface load needs a non-empty 1-D list of element indices")
    if not np.issubdtype(e.dtype, np.integer):
        raise ValueError("element indices must be integers")
    if e.min() < 0:
        raise ValueError(f"element index {int(e.min())} is negative")
    if np.unique(e).size != e.size:
        raise ValueError("the same element is listed twice for one face")
    return np.ascontiguousarray(e, dtype=np.int32)


def _face(face):
    if int(face) != face or not 0 <= int(face) < max(FACES.values()):
        raise ValueError(f"face must be 0..1 (shell) or 0..3 (beam), got {face!r}")
    return int(face)


def _finite(v, what):
    if not math.isfinite(float(v)):
        raise ValueError(f"{what} must be finite")
    return float(v)


class _SurfaceLoad:
    kind = -1

    def __init__(self, face, elements, scale):
        self.face = _face(face)
        self.elements = _elements(elements)
        self.scale = _finite(scale, "scale")

    def check_against(self, S, n_elem):
        """the checks that need the object: the face range of the element kind and the element count"""
        if self.face >= FACES[S]:
            raise ValueError(f"face {self.face} outside 0..{FACES[S] - 1} of this element kind")
        if self.elements.max() >= n_elem:
            raise ValueError(f"element index {int(self.elements.max())} outside 0..{n_elem - 1}")

    def to_c(self):
        """(struct, the array it points into: keep it alive as long as the struct)"""
        return SurfaceLoadC(self.kind, self.face, tuple(self.value3()), self.scale, ip(self.elements),
                            int(self.elements.size)), self.elements


class SurfaceTraction(_SurfaceLoad):
    """Dead traction `traction` (3-vector, force per reference area) on face `face` of `elements`, times `scale`."""
    kind = 0

    def __init__(self, face, elements, traction, scale=1.0):
        super().__init__(face, elements, scale)
        t = np.asarray(traction, dtype=np.float64)
        if t.shape != (3,) or not np.all(np.isfinite(t)):
            raise ValueError("traction must be a finite 3-vector")
        self.traction = t.copy()

    def value3(self):
        return self.traction


class FollowerPressure(_SurfaceLoad):
    """Pressure `pressure` on face `face` of `elements`, times `scale`: positive pushes against the outward normal of the
    deformed face."""
    kind = 1

    def __init__(self, face, elements, pressure, scale=1.0):
        super().__init__(face, elements, scale)
        self.pressure = _finite(pressure, "pressure")

    def value3(self):
        return (self.pressure, 0.0, 0.0)


BoundaryFaces = collections.namedtuple("BoundaryFaces", "elem local_face nodes centroid normal area")


class FaceLoad:
    """A dead traction (kind 0, 3-vector) or a follower pressure (kind 1, scalar) on boundary faces of a T10 mesh."""

    def __init__(self, kind, faces, value, scale=1.0):
        f = np.asarray(faces)
        if f.ndim != 1 or f.size == 0:
            raise ValueError("a face load needs a non-empty 1-D list of boundary-face indices")
        if not np.issubdtype(f.dtype, np.integer):
            raise ValueError("boundary-face indices must be integers")
        if f.min() < 0:
            raise ValueError(f"boundary-face index {int(f.min())} is negative")
        if np.unique(f).size != f.size:
            raise ValueError("the same boundary face is listed twice in one load")
        self.kind, self.faces = int(kind), np.ascontiguousarray(f, dtype=np.int32)
        if self.kind == 0:
            t = np.asarray(value, dtype=np.float64)
            if t.shape != (3,) or not np.all(np.isfinite(t)):
                raise ValueError("traction must be a finite 3-vector")
            self.value = tuple(float(c) for c in t)
        elif self.kind == 1:
            self.value = (_finite(value, "pressure"), 0.0, 0.0)
        else:
            raise ValueError(f"kind must be 0 (traction) or 1 (pressure), got {kind!r}")
        self.scale = _finite(scale, "scale")

    def check_against(self, n_faces):
        if self.faces.max() >= n_faces:
            raise ValueError(f"boundary-face index {int(self.faces.max())} outside 0..{n_faces - 1}")

    def to_c(self):
        """(struct, the array it points into: keep it alive as long as the struct)"""
        return T10SurfaceLoadC(self.kind, self.value, self.scale, ip(self.faces), int(self.faces.size)), self.faces
