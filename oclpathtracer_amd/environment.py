"""Environment lighting: an octahedral sky map that the lit renderers look up where a ray leaves the scene and sample at every vertex
(``pt_render_direct_env``, ``pt_render_indirect_env``; ``include/pt_shim.h`` states every expression).

The map is ``N`` x ``N`` texels, ``N`` a power of two in 1 .. 2048, y up.  A direction d maps to the square [-1, 1]^2 through
(a, b) = (d.x, d.z) / (|d.x| + |d.y| + |d.z|), the lower hemisphere folded outward over the square's diagonals; texel (row, col) covers
a in [2 col / N - 1, 2 (col + 1) / N - 1) and b likewise of row: the centre of the map looks straight up, its corners straight down.
``Environment.directions(N)`` gives the texel centres' directions, for filling a map from a function.

An ``Environment`` holds the texels on the host; the device map and its selection table (``pt_env_table``) are made the first time a
renderer uses it on a device and kept until ``release``.  All compute is HIP in libptshim.so.
"""
from __future__ import annotations

from typing import Callable

import numpy as np

from . import adl, shim

SIZE_MAX = 2048
ENV_SAMPLES_MAX = 256


def _check_size(size) -> int:
    if isinstance(size, bool) or int(size) != size:
        raise ValueError("the map's size must be an integer")
    n = int(size)
    if n < 1 or n > SIZE_MAX or n & (n - 1):
        raise ValueError("the map's size must be a power of two in 1..%d, not %d" % (SIZE_MAX, n))
    return n


def check_env_samples(env_samples) -> int:
    if isinstance(env_samples, bool) or int(env_samples) != env_samples or not 0 <= int(env_samples) <= ENV_SAMPLES_MAX:
        raise ValueError("env_samples must be an integer in 0..%d" % ENV_SAMPLES_MAX)
    return int(env_samples)


class Environment:
    """``texels``: an (N, N, 3) or (N, N, 4) array of linear radiance, row-major as the map is (a fourth channel is ignored).  Texels are
    used as they are: a negative or NaN texel is the caller's business."""

    def __init__(self, texels):
        t = np.asarray(texels, np.float32)
        if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] not in (3, 4):
            raise ValueError("texels must have the shape (N, N, 3) or (N, N, 4), not %s" % (t.shape,))
        self.size = _check_size(t.shape[0])
        self.texels = np.zeros((self.size, self.size, 4), np.float32)
        self.texels[..., :t.shape[2]] = t
        self.texels.setflags(write=False)
        self._on = {}   # device handle -> (map buffer, table buffer)

    # ---- makers -------------------------------------------------------------------------------------------------------------
    @classmethod
    def constant(cls, rgb, size: int = 1) -> "Environment":
        """every texel ``rgb`` (a scalar or three values)"""
        n = _check_size(size)
        c = np.broadcast_to(np.asarray(rgb, np.float32), (3,))
        return cls(np.broadcast_to(c, (n, n, 3)))

    @staticmethod
    def directions(size: int) -> np.ndarray:
        """float64 (N, N, 3): the unit direction of every texel's centre"""
        n = _check_size(size)
        c = (np.arange(n, dtype=np.float64) + 0.5) * (2.0 / n) - 1.0
        a, b = np.meshgrid(c, c, indexing="xy")   # a along the columns, b along the rows
        h = 1.0 - np.abs(a) - np.abs(b)
        sgn = lambda v: np.where(v < 0, -1.0, 1.0)
        x = np.where(h >= 0, a, (1.0 - np.abs(b)) * sgn(a))
        z = np.where(h >= 0, b, (1.0 - np.abs(a)) * sgn(b))
        p = np.stack([x, h, z], -1)
        return p / np.linalg.norm(p, axis=-1, keepdims=True)

    @classmethod
    def from_directions(cls, fn: Callable[[np.ndarray], np.ndarray], size: int) -> "Environment":
        """``fn`` maps the (N, N, 3) texel-centre directions to (N, N, 3) radiance"""
        d = cls.directions(size)
        v = np.asarray(fn(d), np.float32)
        if v.shape != d.shape:
            raise ValueError("fn must return an array of the shape %s, not %s" % (d.shape, v.shape))
        return cls(v)

    @classmethod
    def sun(cls, direction, angular_radius_deg: float, radiance, sky=0.45, size: int = 64) -> "Environment":
        """a sky of ``sky`` with a disc of ``radiance`` of ``angular_radius_deg`` around ``direction``: the texels whose centre lies in
        the disc, and always the one nearest to ``direction``"""
        d = np.asarray(direction, np.float64)
        if d.shape != (3,) or not np.all(np.isfinite(d)) or not np.linalg.norm(d) > 0:
            raise ValueError("direction must be three finite numbers, not all zero")
        r = float(angular_radius_deg)
        if not 0.0 < r <= 180.0:
            raise ValueError("angular_radius_deg must lie in (0, 180]")
        dirs = cls.directions(size)
        cosines = dirs @ (d / np.linalg.norm(d))
        inside = cosines >= np.cos(np.radians(r))
        inside.reshape(-1)[np.argmax(cosines)] = True
        t = np.empty(dirs.shape, np.float32)
        t[...] = np.broadcast_to(np.asarray(sky, np.float32), (3,))
        t[inside] = np.broadcast_to(np.asarray(radiance, np.float32), (3,))
        return cls(t)

    # ---- the device side ----------------------------------------------------------------------------------------------------
    def buffers(self, dev: adl.Device):
        """(map, table) on ``dev``: uploaded and built (``pt_env_table``) on first use, then kept"""
        key = dev._h.value if hasattr(dev._h, "value") else dev._h
        if key not in self._on:
            lib = shim.load()
            n = self.size * self.size
            env = adl.Buffer(dev, n, adl.float4)
            cdf = None
            try:
                env.write(np.ascontiguousarray(self.texels).reshape(n, 4), n)
                cdf = adl.Buffer(dev, lib.pt_env_table_bytes(self.size) // 8, np.uint64)
                shim.check(lib.pt_env_table(dev._h, env._h, self.size, cdf._h, None))
            except Exception:
                env.release()
                if cdf is not None:
                    cdf.release()
                raise
            self._on[key] = (env, cdf)
        return self._on[key]

    def block(self, env_samples: int) -> shim.Environment:
        return shim.Environment(self.size, check_env_samples(env_samples))

    def release(self) -> None:
        for env, cdf in self._on.values():
            env.release()
            cdf.release()
        self._on = {}
