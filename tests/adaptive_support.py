"""What tests/test_gpu_adaptive.py and tests/test_gpu_lit_cells.py share beside roulette_support: the raw C-ABI harness of
pt_render_indirect_pixels (roulette_support.RouletteBuffers with a pixel list), scattered lists, what the restatement
(tests/roulette_oracle.c) says of one list render, and that render compared with it.  TEST INFRASTRUCTURE (an ordinary module: every
assert carries its message)."""
import ctypes

import numpy as np

import adaptive_oracle as ao
import direct_oracle as do
import ris_oracle as rs
import roulette_oracle as ro
from conftest import assert_fb_equal
from oclpathtracer_amd import adl, scene, shim
from oclpathtracer_amd.camera import Camera
from roulette_support import RouletteBuffers
from scenes import edge_scene

SENTINEL = np.float32(-7.25)


def _list_bytes(slots):
    s = np.ascontiguousarray(slots, ao.SLOT_DTYPE)
    return np.frombuffer(np.array([len(s), 0, 0, 0], np.uint32).tobytes() + s.tobytes(), np.uint8)


def _slots(pixels, frames):
    s = np.zeros(len(pixels), ao.SLOT_DTYPE)
    s["pixel"], s["frame"] = pixels, frames
    return s


def _scattered(rng, npix, listed, max_frame=6):
    """``listed`` distinct pixels in no order, each at a frame number of its own in [0, max_frame], some at frame 0"""
    s = _slots(rng.permutation(npix)[:listed], rng.integers(0, max_frame + 1, listed))
    s["frame"][::7] = 0
    return s


class PixelBuffers(RouletteBuffers):
    """The buffers of one raw call of pt_render_indirect_pixels: pt_render_indirect_rr's (the framebuffer a sentinel, four pixels
    longer than the image) and a list ``pl``; the workspace starts as the sentinel too."""

    def __init__(self, device, scene4, W, H, frames=1, **kw):
        tris, mats, lights, _ = scene4
        lights = scene.emitters(tris, mats) if lights is None else lights
        super().__init__(device, np.ascontiguousarray(tris), np.ascontiguousarray(mats), W, H, lights=tuple(int(i) for i in lights), frames=frames, **kw)
        self.nl = len(lights)
        self.pl = adl.Buffer(device, self.lib.pt_adaptive_list_bytes(W * H), np.uint8)
        self.ws_sentinel = np.full(3 * W * H * frames, SENTINEL, np.float32)
        self.sb.write(self.ws_sentinel, self.ws_sentinel.size)
        self.listed = 0

    def estimator(self, mis, power):
        self.mis, self.power = mis, power
        return self

    def set_list(self, slots):
        raw = _list_bytes(slots)
        self.pl.write(raw, raw.size)
        self.listed = len(slots)

    def full_list(self, npix, frame):
        self.set_list(_slots(np.arange(npix), np.full(npix, frame)))

    def rr(self, p, **kw):
        """the parent: pt_render_indirect_rr"""
        return super().call(p, **kw)

    def call(self, p, cam=None, rr="default", candidates=0, **over):
        """pt_render_indirect_pixels; with ``candidates`` pt_render_indirect_pixels_ris with that many"""
        h = {name: over.get(name, getattr(self, name)) for name in ("tb", "mb", "lb", "cb", "qb", "tq", "sb", "fb", "pl")}
        mis = int(over.get("mis", self.mis))
        if not mis and "cb" not in over:
            h["cb"] = None
        if not self.power:
            h["qb"], h["tq"] = over.get("qb"), over.get("tq")
        h = {k: (b._h if b is not None else None) for k, b in h.items()}
        if isinstance(rr, str):
            rr = self.roulette()
        head = (self.device._h, h["tb"], h["mb"], h["lb"], mis, h["cb"], h["qb"], h["tq"], h["sb"], h["fb"], h["pl"],
                over.get("num_listed", self.listed), ctypes.byref(p) if p is not None else None, ctypes.byref(rr) if rr is not None else None)
        if candidates:
            ris = shim.Ris(candidates)
            return self.lib.pt_render_indirect_pixels_ris(*head, ctypes.byref(ris), cam, None)
        return self.lib.pt_render_indirect_pixels(*head, cam, None)

    def workspace(self):
        return self.read(self.sb, like=self.ws_sentinel)

    def release(self):
        super().release()
        self.pl.release()


def _uniform(name, W, H, n, K, B, R, cap, mis, power, candidates=0, **stripes):
    tris, mats, lights, cam = edge_scene(name)[1]
    if n == 0:
        return (np.zeros((do.local_row_count(H, **stripes) * W, 4), np.float32),)
    if candidates:   # (resampling draws from the table: by power)
        return (rs.render(tris, mats, W, H, 0, n, K, candidates, B=B, R=R, cap=cap, mis=mis, lights=lights, cam=cam, **stripes),)
    return (ro.render(tris, mats, W, H, 0, n, K, B, R, cap, mis=mis, power=power, lights=lights, cam=cam, **stripes),)


def uniform(name, W, H, n, K, B, R, cap, mis, power, candidates=0, **stripes):
    """the restatement's framebuffer of frames [0, n) -- with ``candidates`` tests/ris_oracle.c's with that many --: computed once per
    case, shared, read-only"""
    return do.once(_uniform, name, W, H, int(n), K, B, R, cap, bool(mis), bool(power), int(candidates), **stripes)[0]


def _expect(name, W, H, slots, F, K, B, R, cap, mis, power, offset=0, candidates=0, **stripes):
    """(workspace [F, listed, 3], {pixel: its framebuffer record}, the framebuffer pixels to start from) of one list render -- with
    ``candidates`` of pt_render_indirect_pixels_ris with that many (``power`` is then implied)"""
    tris, mats, lights, cam = edge_scene(name)[1]
    gids = do.local_gids(W, H, **stripes)
    px, first = slots["pixel"].astype(np.int64), slots["frame"].astype(np.int64) + offset
    gid = np.tile(gids[px], F)
    frame = (first[None, :] + np.arange(F)[:, None]).reshape(-1)
    if candidates:
        assert power, "resampling draws its candidates from the table"
        ws = rs.samples(tris, mats, W, H, gid, frame, K, candidates, B=B, R=R, cap=cap, mis=mis, lights=lights, cam=cam)
    else:
        ws = ro.samples(tris, mats, W, H, gid, frame, K, B, R, cap, mis=mis, power=power, lights=lights, cam=cam)[0]
    ws = ws.reshape(F, len(px), 3)
    start = np.stack([uniform(name, W, H, z, K, B, R, cap, mis, power, candidates, **stripes)[p] for p, z in zip(px, first)])
    end = np.stack([uniform(name, W, H, z + F, K, B, R, cap, mis, power, candidates, **stripes)[p] for p, z in zip(px, first)])
    return ws, end, start


def _run_list(device, b, name, W, H, slots, F, K, B, R, cap, mis, power, what, offset=0, candidates=0, **stripes):
    """one list render on PixelBuffers ``b`` from the restatement's starting image, with the scene's own camera -- with ``candidates``
    through pt_render_indirect_pixels_ris --, compared with the restatement: the workspace's records, the listed pixels, and every other byte of both buffers unchanged"""
    want_ws, want_px, start = _expect(name, W, H, slots, F, K, B, R, cap, mis, power, offset, candidates, **stripes)
    fb0 = b.sentinel.copy()
    fb0[slots["pixel"]] = start
    b.fb.write(fb0, len(fb0))
    b.sb.write(b.ws_sentinel, b.ws_sentinel.size)
    b.estimator(mis, power).set_list(slots)
    p = b.params(b.nl, frame_begin=offset, frame_count=F, light_samples=K, max_bounces=B, **stripes)
    cam = Camera.struct_of(edge_scene(name)[1][3])
    assert b.call(p, cam=ctypes.byref(cam) if cam is not None else None, rr=b.roulette(R, cap), candidates=candidates) == shim.PT_OK, what
    ws, fb = b.workspace(), b.read()
    n = F * len(slots) * 3
    assert_fb_equal(ws[:n], want_ws, what + ": radiance before the fold")
    assert np.array_equal(ws[n:], b.ws_sentinel[n:]), what + ": the workspace behind the launch's records was written"
    assert_fb_equal(fb[slots["pixel"]], want_px, what + ": the listed pixels")
    fb[slots["pixel"]] = fb0[slots["pixel"]]
    assert fb.tobytes() == fb0.tobytes(), what + ": a pixel that is not listed was written"
