"""Which rows of which image a device renders, from which camera, over which frames: what every renderer of an image decides the
same way.  Rows are dealt to the ranks in stripes of ``stripe_rows``, round-robin."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import shim
from .camera import Camera

LIMIT = 0x7fffffff   # pixels of an image and frame numbers: both are int32 on the device


def check_size(width, height, what: str = "image"):
    """``(width, height)`` as ints; ValueError unless the image has a pixel and fewer than 2^31 of them"""
    width, height = int(width), int(height)
    if width < 1 or height < 1 or width * height > LIMIT:
        raise ValueError("invalid %s size %dx%d" % (what, width, height))
    return width, height


def frame_range(frames, frame_begin, frames_done: int, *, resumes: bool = False, who: str = "a render"):
    """``(frames, frame_begin)`` as ints, ``frame_begin`` None meaning ``frames_done``: ValueError unless 0 <= frame_begin <=
    frame_begin + frames < 2^31.  ``resumes``: the caller counts every frame it renders, so a call of any frames starts at frame 0
    or at ``frames_done`` -- a frame rendered twice would be counted twice."""
    if frame_begin is None:
        frame_begin = frames_done
    frames, frame_begin = int(frames), int(frame_begin)
    if frames < 0 or frame_begin < 0 or frame_begin + frames > LIMIT:
        raise ValueError("invalid frame range [%d, %d)" % (frame_begin, frame_begin + frames))
    if resumes and frames > 0 and frame_begin not in (0, frames_done):
        raise ValueError("%s starts at frame 0 or at frames_done (%d), not at %d" % (who, frames_done, frame_begin))
    return frames, frame_begin


class ImageShare:
    """One device's rows of an image.  ``local_rows`` rows of ``width`` pixels, ``local_pixels`` in all; with the defaults the whole
    image.  Refused here, before any device call: an image size ``check_size`` refuses (``sized=False`` leaves the size to the
    library, as the fused renderer does) and a stripe geometry ``pt_local_rows`` refuses."""

    def __init__(self, width: int, height: int, stripe_rows: int = 16, n_ranks: int = 1, rank: int = 0, *, sized: bool = True):
        self.width, self.height = check_size(width, height) if sized else (int(width), int(height))
        self.stripe_rows, self.n_ranks, self.rank = int(stripe_rows), int(n_ranks), int(rank)
        self.local_rows = shim.load().pt_local_rows(self.height, self.stripe_rows, self.n_ranks, self.rank)
        if self.local_rows < 0:
            raise ValueError("invalid stripe geometry")
        self.local_pixels = self.local_rows * self.width

    def global_rows(self) -> np.ndarray:
        """Global row index of every local row (ascending)."""
        rows = np.arange(self.height)
        return rows[(rows // self.stripe_rows) % self.n_ranks == self.rank]

    def fill(self, p, frames: int, frame_begin: int):
        """``p`` (any of the render parameter blocks) with the image, the frames and the sharding set"""
        p.width, p.height = self.width, self.height
        p.frame_begin, p.frame_count = frame_begin, frames
        p.stripe_rows, p.n_ranks, p.rank = self.stripe_rows, self.n_ranks, self.rank
        return p


class ImageRenderer(ImageShare):
    """What the renderers of an image share: each is one device's share of it (a constructor calls ``ImageShare.__init__`` where it
    refuses its geometry), seen from a camera.  A subclass says in ``_restart`` what a new camera invalidates."""

    def _set_camera(self, camera: Optional[Camera]) -> None:
        self._cam = Camera.struct_of(camera)   # rejected here, before anything is enqueued
        self.camera = camera

    def _cam_ref(self):
        """the camera's struct by reference; None for the reference's camera"""
        return ctypes.byref(self._cam) if self._cam is not None else None

    def set_camera(self, camera: Optional[Camera]) -> None:
        """Render from ``camera``, its lens included, from now on (None: the reference's).  The image of another camera is another
        image: the next render starts again at frame 0.  Renders already enqueued keep the camera they were enqueued with."""
        self._set_camera(camera)
        self._restart()

    def _restart(self) -> None:
        self.frames_done = 0


def like(renderer, kw: dict):
    """``(width, height)`` for a renderer made beside ``renderer``, taken out of ``kw``; the image size, camera and sharding that
    ``kw`` does not name are ``renderer``'s"""
    for name in ("camera", "stripe_rows", "n_ranks", "rank"):
        kw.setdefault(name, getattr(renderer, name))
    return kw.pop("width", renderer.width), kw.pop("height", renderer.height)
