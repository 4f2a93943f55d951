"""What the GPU test modules share: device options for a block, one render through the fused entry point, one direct or indirect
render with its sample workspace, the comparison of hit records and the ray generators of the query tests.  TEST INFRASTRUCTURE (an ordinary module: every assert carries its message)."""
from contextlib import contextmanager

import numpy as np

from conftest import assert_fb_equal
from oclpathtracer_amd import shim

SEARCHES = [(q, a) for a in (1, 2) for q in (0, 1, 4)]   # (PT_OPT_QUAD_FILTER, PT_OPT_ACCEL)


@contextmanager
def options(device, **opts):
    """Set device options, named by what follows PT_OPT_, for a block and put back what they were.  The device is shared by the
    whole session: an option left behind would change what every later test exercises."""
    ids = {getattr(shim, "PT_OPT_" + k): int(v) for k, v in opts.items()}
    old = {k: int(shim.load().pt_device_get_option(device._h, k)) for k in ids}
    try:
        for k, v in ids.items():
            device.setOption(k, v)
        yield
    finally:
        for k, v in old.items():
            device.setOption(k, v)


def render(device, tris, mats, W, H, frames, *, depth=16, frame_begin=0, fb_init=None, camera=None, want_stats=False, **renderer_kw):
    """One Renderer, one render, released: the pixels, and with want_stats (pixels, the PT_STAT_* words)."""
    from oclpathtracer_amd.render import Renderer

    r = Renderer(device, tris, mats, W, H, camera=camera, want_stats=want_stats, **renderer_kw)
    try:
        if fb_init is not None:
            r.fb.write(np.ascontiguousarray(fb_init, np.float32), r.local_pixels)
        r.render(frames, frame_begin=frame_begin, max_bounces=depth)
        got = r.read()
        return (got, r.read_stats_raw()) if want_stats else got
    finally:
        r.release()


def lit_with_samples(device, scene4, W, H, frames, K, chunk_frames=None, max_bounces=None, **kw):
    """One DirectRenderer -- with max_bounces an IndirectRenderer -- on (tris, mats, lights, camera), whose workspace holds every
    frame of the call (chunk_frames >= frames unless given), one render from frame 0: the framebuffer [local pixels, 4] and the
    whole sample workspace [chunk_frames, local pixels, 3]."""
    from oclpathtracer_amd.direct import DirectRenderer
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats, lights, cam = scene4
    kw.setdefault("stripe_rows", 1)
    kw.update(light_samples=K, lights=lights, camera=cam, chunk_frames=max(frames, 1) if chunk_frames is None else chunk_frames)
    r = DirectRenderer(device, tris, mats, W, H, **kw) if max_bounces is None else \
        IndirectRenderer(device, tris, mats, W, H, max_bounces=max_bounces, **kw)
    try:
        r.render(frames, 0)
        fb = r.read()
        ws = np.zeros((r.chunk_frames, r.local_pixels, 3), np.float32)
        r.samples.read(ws, ws.size)
        device.waitForCompletion()
        return fb, ws
    finally:
        r.release()


def words(hits) -> np.ndarray:
    """pt_hit records (HIT_DTYPE or [N, 12] float32) as float32 [N, 12]."""
    h = np.asarray(hits)
    return np.ascontiguousarray(h).view(np.float32).reshape(-1, 12)


def assert_hits_equal(got, want, what=""):
    """t, tri, u, v, p, material, n bit-exact (NaN masks equal), the reserved word ignored."""
    g, w = words(got), words(want)
    assert g.shape == w.shape, what
    assert np.array_equal(g[:, 1].view(np.int32), w[:, 1].view(np.int32)), "%s: triangles differ at %s" % (
        what, np.flatnonzero(g[:, 1].view(np.int32) != w[:, 1].view(np.int32))[:8])
    assert_fb_equal(g[:, :11], w[:, :11], what)


def cornell_rays(rng, n, tris):
    """Origins inside the box, on its surfaces and outside it; directions random, axis-aligned, with +-0 components, of
    lengths 1e-3 .. 1e3."""
    pts = np.concatenate([tris["p1"][:, :3], tris["p2"][:, :3], tris["p3"][:, :3]])
    lo, hi = pts.min(0), pts.max(0)
    k = n // 3
    inside = rng.uniform(lo + 0.01, hi - 0.01, (k, 3))
    t = rng.integers(0, len(tris), k)
    a, b = rng.uniform(0, 1, (2, k, 1))
    swap = a + b > 1
    a, b = np.where(swap, 1 - a, a), np.where(swap, 1 - b, b)
    on = tris["p1"][t, :3] + a * (tris["p2"][t, :3] - tris["p1"][t, :3]) + b * (tris["p3"][t, :3] - tris["p1"][t, :3])
    outside = rng.uniform(lo - 6.0, hi + 6.0, (n - 2 * k, 3))
    o = np.concatenate([inside, on, outside]).astype(np.float32)
    d = rng.normal(size=(n, 3))
    axis = rng.uniform(size=n) < 0.25                       # axis-aligned, signed zeros in the other components
    ax = rng.integers(0, 3, n)
    sgn = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    d[axis] = 0.0
    d[axis, ax[axis]] = sgn[axis]
    zero = rng.uniform(size=(n, 3)) < 0.1                   # +-0 components elsewhere
    d[zero] = 0.0
    d = d.astype(np.float32)
    d[zero & (rng.uniform(size=(n, 3)) < 0.5)] = np.float32(-0.0)
    d *= (10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    r = np.zeros((n, 8), np.float32)
    r[:, :3], r[:, 3], r[:, 4:7] = o, np.float32(1e20), d
    return r


def refill_rays(n, seed):
    """n random rays through the 3 000-triangle soup, with long runs of rays that search nothing (tmax NaN, 0, -0, negative) and of
    live ones after them, in every phase of a 64-ray group -- more rays than the LBVH query kernel's persistent grid holds lanes"""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 8), np.float32)
    r[:, :3] = rng.uniform(-4, 4, (n, 3))
    r[:, 3] = rng.uniform(0.5, 12.0, n)                          # mostly finite reach: hits and misses both
    r[rng.uniform(size=n) < 0.3, 3] = 1e20
    r[:, 4:7] = rng.normal(size=(n, 3))
    dead = np.array([np.nan, 0.0, -0.0, -1.0, -np.inf], np.float32)
    pos = 0
    while pos < n:
        pos += int(rng.integers(1, 4000))                        # a live stretch
        run = int(rng.integers(1, 3000))                         # then a run of dead rays, often longer than a refill
        r[pos: pos + run, 3] = dead[int(rng.integers(0, len(dead)))] if rng.uniform() < 0.7 else \
            dead[rng.integers(0, len(dead), len(r[pos: pos + run]))]
        pos += run
    return r
