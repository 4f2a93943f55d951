"""What tests/test_gpu_env.py needs beside gpu_support and adaptive_support: the raw C-ABI harness of pt_env_table, pt_render_direct_env and
pt_render_indirect_env (adaptive_support.PixelBuffers -- the scene, the counts, the light table, sentinels in framebuffer and workspace --
with the map, its table and the pt_environment block), one case of tests/env_cases.py rendered through it and what the restatement
says of that case.  TEST INFRASTRUCTURE (an ordinary module: every assert carries its message)."""
import ctypes

import numpy as np

import direct_oracle as do
import env_oracle as eo
from adaptive_support import PixelBuffers
from env_scenes import env_map, env_scene
from gpu_support import options
from oclpathtracer_amd import adl, shim
from oclpathtracer_amd.camera import Camera


def device_env_table(device, texels):
    """One raw pt_env_table over fresh buffers filled with a sentinel: (return code, cdf uint64 [N * N + 1])"""
    lib = shim.load()
    t = eo.texels4(texels)
    N = eo.size_of(t)
    words = lib.pt_env_table_bytes(N) // 8
    eb = adl.Buffer(device, N * N, adl.float4)
    qb = adl.Buffer(device, words, np.uint64)
    try:
        eb.write(t, N * N)
        qb.write(np.full(words, 0xdeadbeefdeadbeef, np.uint64), words)
        rc = lib.pt_env_table(device._h, eb._h, N, qb._h, None)
        cdf = np.zeros(N * N + 1, np.uint64)
        qb.read(cdf, len(cdf))
        device.waitForCompletion()
        return rc, cdf
    finally:
        eb.release()
        qb.release()


class EnvBuffers(PixelBuffers):
    """The buffers of one raw call of pt_render_direct_env or pt_render_indirect_env over a scene of env_scenes.env_scene under a map of
    env_scenes.env_map: pt_render_indirect_pixels' (counts, light table; framebuffer and workspace start as sentinels), the map ``eb`` and
    its table ``ec`` made by pt_env_table."""

    def __init__(self, device, scene, map, W, H, frames=1, **kw):
        self.scene4 = env_scene(scene)
        tris, mats, lights, cam = self.scene4
        if len(tris) == 0:   # (an empty scene: the harness needs a record to allocate; num_triangles = 0 is passed)
            tris = np.zeros(1, tris.dtype)
            lights = np.zeros(0, np.int32)
        super().__init__(device, (tris, mats, lights, cam), W, H, frames=frames, **kw)
        self.ntri = len(self.scene4[0])
        cs = Camera.struct_of(cam)
        self.cam = ctypes.byref(cs) if cs is not None else None
        self._cam_struct = cs
        self.texels = eo.texels4(env_map(map))
        self.N = eo.size_of(self.texels)
        self.eb = adl.Buffer(device, self.N * self.N, adl.float4)
        self.ec = adl.Buffer(device, self.lib.pt_env_table_bytes(self.N) // 8, np.uint64)
        self.eb.write(self.texels, self.N * self.N)
        assert self.lib.pt_env_table(device._h, self.eb._h, self.N, self.ec._h, None) == shim.PT_OK

    def environment(self, Ke=1, size=None, reserved=None):
        e = shim.Environment(self.N if size is None else size, Ke)
        if reserved is not None:
            e.reserved[reserved] = 1
        return e

    def direct_params(self, nl, **kw):
        """pt_direct_params as LitBuffers.params fills pt_indirect_params"""
        p = shim.DirectParams()
        p.width, p.height, p.frame_begin, p.frame_count = self.W, self.H, 0, 1
        p.num_triangles, p.num_materials, p.num_lights, p.light_samples = self.ntri, self.nmat, nl, 2
        p.stripe_rows, p.n_ranks, p.rank = 1, 1, 0
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    def _handles(self, over, nl):
        h = {name: over.get(name, getattr(self, name)) for name in ("tb", "mb", "lb", "cb", "qb", "tq", "eb", "ec", "sb", "fb")}
        if nl == 0:   # every emitter buffer may be NULL
            for name in ("lb", "cb", "qb", "tq"):
                if name not in over:
                    h[name] = None
        return {k: (b._h if b is not None else None) for k, b in h.items()}

    @staticmethod
    def _ref(x):
        return ctypes.byref(x) if x is not None else None

    def direct(self, p, env="default", cam=None, **over):
        """pt_render_direct_env; env: a shim.Environment, None (NULL) or the default of one sample"""
        h = self._handles(over, p.num_lights if p is not None else 1)
        env = self.environment() if isinstance(env, str) else env
        return self.lib.pt_render_direct_env(self.device._h, h["tb"], h["mb"], h["lb"], h["qb"], h["tq"], h["eb"], h["ec"], h["sb"], h["fb"],
                                             self._ref(p), self._ref(env), cam, None)

    def indirect(self, p, rr="default", env="default", cam=None, **over):
        """pt_render_indirect_env"""
        h = self._handles(over, p.num_lights if p is not None else 1)
        rr = self.roulette() if isinstance(rr, str) else rr
        env = self.environment() if isinstance(env, str) else env
        return self.lib.pt_render_indirect_env(self.device._h, h["tb"], h["mb"], h["lb"], h["cb"], h["qb"], h["tq"], h["eb"], h["ec"], h["sb"],
                                               h["fb"], self._ref(p), self._ref(rr), self._ref(env), cam, None)

    def direct_power(self, p, cam=None):
        """the parent: pt_render_direct_power"""
        h = self._handles({}, p.num_lights)
        return self.lib.pt_render_direct_power(self.device._h, h["tb"], h["mb"], h["lb"], h["qb"], h["tq"], h["sb"], h["fb"], self._ref(p), cam, None)

    def indirect_rr(self, p, rr, cam=None):
        """the parent: pt_render_indirect_rr with mis = 1 and the table"""
        h = self._handles({}, p.num_lights)
        return self.lib.pt_render_indirect_rr(self.device._h, h["tb"], h["mb"], h["lb"], 1, h["cb"], h["qb"], h["tq"], h["sb"], h["fb"], self._ref(p),
                                              self._ref(rr), cam, None)

    def reset(self, fb_init=None):
        fb0 = self.sentinel if fb_init is None else fb_init
        self.fb.write(np.ascontiguousarray(fb0, np.float32), len(self.sentinel))
        self.sb.write(self.ws_sentinel, self.ws_sentinel.size)

    def render(self, c, Ke=None, parent=False, fb_init=None, **stripes):
        """one render of case ``c`` (env_cases.Case) from fresh sentinels (or the framebuffer ``fb_init``) through the _env entry point of
        its form -- with ``parent`` through pt_render_direct_power / pt_render_indirect_rr --, under the case's search options: (return
        code, framebuffer [W * H + pad, 4], workspace)"""
        assert (c.W, c.H) == (self.W, self.H), "the buffers are another image's"
        self.reset(fb_init)
        nl = 0 if c.nl0 else self.nl
        shared = dict(frame_begin=c.frame_begin, frame_count=c.frames, light_samples=c.K, **stripes)
        env = self.environment(c.Ke if Ke is None else Ke)
        with options(self.device, QUAD_FILTER=c.search[0], ACCEL=c.search[1]):
            if c.B is None:
                p = self.direct_params(nl, **shared)
                rc = self.direct_power(p, cam=self.cam) if parent else self.direct(p, env=env, cam=self.cam)
            else:
                p = self.params(nl, max_bounces=c.B, **shared)
                rr = self.roulette(c.R, c.cap)
                rc = self.indirect_rr(p, rr, cam=self.cam) if parent else self.indirect(p, rr=rr, env=env, cam=self.cam)
            fb, ws = self.read(), self.workspace()
        return rc, fb, ws

    def release(self):
        super().release()
        self.eb.release()
        self.ec.release()


def expect(c, **stripes):
    """what the restatement says of case ``c`` (one rank's share with ``stripes``): (workspace [frames, local pixels, 3] before the fold,
    framebuffer [local pixels, 4], the framebuffer the call resumes -- empty when it starts at frame 0) -- computed once per case and rank, shared, read-only"""
    return do.once(_expect, c, **stripes)


def _expect(c, **stripes):
    tris, mats, lights, cam = env_scene(c.scene)
    if c.nl0:
        lights = np.zeros(0, np.int32)
    t = env_map(c.map)
    gids = do.local_gids(c.W, c.H, **stripes)
    gid = np.tile(gids, c.frames)
    frame = np.repeat(np.arange(c.frame_begin, c.frame_begin + c.frames, dtype=np.int32), len(gids))
    ws = eo.samples(tris, mats, t, c.W, c.H, gid, frame, c.K, c.Ke, B=c.B, R=c.R, cap=c.cap, lights=lights, cam=cam)
    start = None
    if c.frame_begin > 0:   # the image the call resumes: the restatement's own of the frames before
        start = eo.render(tris, mats, t, c.W, c.H, 0, c.frame_begin, c.K, c.Ke, B=c.B, R=c.R, cap=c.cap, lights=lights, cam=cam, **stripes)
    fb = eo.render(tris, mats, t, c.W, c.H, c.frame_begin, c.frames, c.K, c.Ke, B=c.B, R=c.R, cap=c.cap, lights=lights, cam=cam, start=start, **stripes)
    return ws.reshape(c.frames, len(gids), 3), fb, (start if start is not None else np.zeros((0, 4), np.float32))
