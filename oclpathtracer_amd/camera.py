"""The look-at camera of the fused renderer (include/pt_shim.h: pt_camera).

The reference keeps its camera as literals in ``generateRay`` (GenerateColors.cl:263-269): eye (0, 2.75, 4), looking
at eye + (0, 0, -1), up (0, 1, 0), 60 degrees of vertical field of view.  A :class:`Camera` carries the same four values;
the renderer derives the view basis and tan(fov / 2) from them once per render, on the host, with the reference's
arithmetic.  ``Camera.reference()`` renders exactly what the renderer renders without a camera.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import shim

Vec3 = Tuple[float, float, float]


def _vec3(v, what: str) -> Vec3:
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.shape != (3,):
        raise ValueError("camera: %s must have three components" % what)
    return tuple(float(np.float32(x)) for x in a)   # the values the renderer sees (binary32)


@dataclass(frozen=True)
class Camera:
    """``eye`` looks at ``center``; ``up`` fixes the roll; ``fov_y_deg`` is the vertical field of view in degrees, in (0, 180).
    ``lens_radius`` > 0 (world units) makes it a thin lens focused on the sphere of radius ``focus_distance`` about the eye
    (include/pt_shim.h: pt_camera); 0 is the pinhole.  The sample-by-sample renderers (``AORenderer``, ``DirectRenderer``,
    ``IndirectRenderer``) and ``RayCaster.camera_rays`` take a lens; the fused ones (``Renderer``, ``ProgressiveRenderer``,
    ``StripeImage``) refuse it.
    Invalid cameras (non-finite values, ``center == eye``, ``up`` parallel to the view direction, a negative lens radius or focus
    distance, a lens without a focus distance) raise ``ValueError`` here, before anything is enqueued."""

    eye: Vec3
    center: Vec3
    up: Vec3 = (0.0, 1.0, 0.0)
    fov_y_deg: float = 60.0
    lens_radius: float = 0.0
    focus_distance: float = 0.0

    def __post_init__(self):
        object.__setattr__(self, "eye", _vec3(self.eye, "eye"))
        object.__setattr__(self, "center", _vec3(self.center, "center"))
        object.__setattr__(self, "up", _vec3(self.up, "up"))
        object.__setattr__(self, "fov_y_deg", float(np.float32(self.fov_y_deg)))
        object.__setattr__(self, "lens_radius", float(np.float32(self.lens_radius)))
        object.__setattr__(self, "focus_distance", float(np.float32(self.focus_distance)))
        self.derive()   # validates

    @classmethod
    def reference(cls) -> "Camera":
        """The reference's camera (GenerateColors.cl:263-267)."""
        c = shim.Camera()
        shim.load().pt_camera_reference(ctypes.byref(c))
        return cls(tuple(c.eye), tuple(c.center), tuple(c.up), c.fov_y_deg)

    @classmethod
    def fit(cls, triangles: np.ndarray, view_dir: Sequence[float] = (0.0, 0.0, -1.0), up: Sequence[float] = (0.0, 1.0, 0.0),
            fov_y_deg: float = 60.0, margin: float = 1.05, aspect: float = 1.0) -> "Camera":
        """A camera looking along ``view_dir`` at the centre of the scene's bounding sphere, far enough back for its frustum
        to contain the sphere (times ``margin``) in an image of width / height >= ``aspect``."""
        pts = np.concatenate([np.asarray(triangles[f])[:, :3] for f in ("p1", "p2", "p3")]).astype(np.float64)
        if pts.size == 0 or not np.all(np.isfinite(pts)):
            raise ValueError("camera: the scene has no finite vertices to fit")
        if not (0.0 < fov_y_deg < 180.0) or not margin >= 1.0 or not aspect > 0.0:
            raise ValueError("camera: fov_y_deg must lie in (0, 180), margin >= 1, aspect > 0")
        c = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
        radius = max(float(np.sqrt(((pts - c) ** 2).sum(axis=1)).max()), 1e-6)
        v = np.asarray(view_dir, np.float64)
        n = float(np.linalg.norm(v))
        if not np.isfinite(n) or n == 0.0:
            raise ValueError("camera: view_dir must be a finite non-zero vector")
        v = v / n
        half_v = 0.5 * math.radians(fov_y_deg)
        half = min(half_v, math.atan(math.tan(half_v) * aspect))   # the narrower of the two half-angles
        dist = margin * radius / math.sin(half)
        return cls(tuple(c - dist * v), tuple(c), tuple(up), fov_y_deg)

    def with_lens(self, lens_radius: float, focus_distance: Optional[float] = None, focus_on: Optional[Sequence[float]] = None) -> "Camera":
        """This camera with a thin lens of ``lens_radius``, focused at ``focus_distance`` or on the point ``focus_on`` (the distance is
        |point - eye|): exactly one of the two, unless ``lens_radius`` is 0 (the pinhole, which needs neither)."""
        if (focus_distance is None) == (focus_on is None) and not (focus_on is None and float(lens_radius) == 0.0):
            raise ValueError("camera: give exactly one of focus_distance and focus_on")
        if focus_on is not None:
            p = np.asarray(_vec3(focus_on, "focus_on"), np.float64)
            focus_distance = float(np.sqrt(((p - np.asarray(self.eye, np.float64)) ** 2).sum()))
        return Camera(self.eye, self.center, self.up, self.fov_y_deg, lens_radius, 0.0 if focus_distance is None else focus_distance)

    def pinhole_ray(self, u: float = 0.5, v: float = 0.5, aspect: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
        """(origin, unit direction), float64, of the ray through image position (``u``, ``v``) in [0, 1]^2 -- (0, 0) the top left corner --
        of an image of width / height ``aspect``, without jitter and without a lens."""
        d = self.derive().astype(np.float64)
        eye, view, hol, up, angle = d[0:3], d[3:6], d[6:9], d[9:12], d[12]
        w = hol * ((2.0 * u - 1.0) * angle * aspect) + up * ((1.0 - 2.0 * v) * angle) + view
        return eye, w / np.sqrt((w * w).sum())

    def autofocus(self, caster, lens_radius: float, u: float = 0.5, v: float = 0.5, aspect: float = 1.0) -> "Camera":
        """This camera with a thin lens of ``lens_radius`` focused on what the pinhole ray of image position (``u``, ``v``) hits: one
        closest-hit query through ``caster`` (a ``RayCaster`` of the scene), the focus distance is the hit's ``t``.  Raises
        ``ValueError`` when the ray leaves the scene."""
        from .query import make_rays

        o, w = self.pinhole_ray(u, v, aspect)
        hit = caster.closest(make_rays(o[None, :], w[None, :]))[0]
        if int(hit["tri"]) < 0 or not np.isfinite(hit["t"]):
            raise ValueError("camera: nothing to focus on at image position (%g, %g)" % (u, v))
        return self.with_lens(lens_radius, focus_distance=float(hit["t"]))

    @classmethod
    def struct_of(cls, camera: Optional["Camera"]) -> Optional[shim.Camera]:
        """What every entry point that takes a camera hands to the library: None (the reference's camera) for None, else the
        ``pt_camera`` struct of a :class:`Camera`, derived once here so that a bad one is rejected before anything is enqueued."""
        if camera is None:
            return None
        if not isinstance(camera, cls):
            raise TypeError("camera must be an oclpathtracer_amd.camera.Camera or None")
        s = camera.to_struct()
        shim.check(shim.load().pt_camera_derive(ctypes.byref(s), (ctypes.c_float * 16)()))
        return s

    def to_struct(self) -> shim.Camera:
        s = shim.Camera()
        s.eye[:] = self.eye
        s.center[:] = self.center
        s.up[:] = self.up
        s.fov_y_deg = self.fov_y_deg
        s.lens_radius = self.lens_radius
        s.focus_distance = self.focus_distance
        return s

    def derive(self) -> np.ndarray:
        """The renderer's derived values (pt_camera_derive): float32[16] = eye xyz, viewDir xyz, holDir xyz, upDir xyz,
        angle = tan(fov / 2), lens_radius, focus_distance, 0."""
        out = np.zeros(16, np.float32)
        s = self.to_struct()
        rc = shim.load().pt_camera_derive(ctypes.byref(s), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        if rc != shim.PT_OK:
            raise ValueError(shim.load().pt_last_error().decode("utf-8", "replace"))
        return out
