"""What tests/test_gpu_ris.py needs beside gpu_support, roulette_support and adaptive_support: the raw C-ABI harness of the three _ris
entry points (adaptive_support.PixelBuffers with the pt_ris block and the new argument lists, and direct illumination's parameter
block) and one case of tests/ris_cases.py rendered through it.  TEST INFRASTRUCTURE (an ordinary module: every assert carries its
message)."""
import ctypes

import numpy as np

import direct_oracle as do
from adaptive_support import PixelBuffers
from oclpathtracer_amd import shim
from oclpathtracer_amd.camera import Camera
from ris_scenes import ris_scene


class RisBuffers(PixelBuffers):
    """The buffers of one raw call of pt_render_direct_ris, pt_render_indirect_ris or pt_render_indirect_pixels_ris over a scene of
    ris_scenes.ris_scene: pt_render_indirect_pixels' (counts, table, list; framebuffer and workspace start as sentinels)."""

    def __init__(self, device, name, W, H, frames=1, **kw):
        self.scene4 = ris_scene(name)
        super().__init__(device, self.scene4, W, H, frames=frames, **kw)
        cam = Camera.struct_of(self.scene4[3])
        self.cam = ctypes.byref(cam) if cam is not None else None
        self._cam_struct = cam

    def ris(self, candidates=8, reserved=None):
        r = shim.Ris(candidates)
        if reserved is not None:
            r.reserved[reserved] = 1
        return r

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

    def _handles(self, over):
        h = {name: over.get(name, getattr(self, name)) for name in ("tb", "mb", "lb", "cb", "qb", "tq", "sb", "fb", "pl")}
        return {k: (b._h if b is not None else None) for k, b in h.items()}

    @staticmethod
    def _ref(x):
        return ctypes.byref(x) if x is not None else None

    def direct(self, p, ris="default", cam=None, **over):
        """pt_render_direct_ris; ris: a shim.Ris, None (NULL) or the default of 8 candidates"""
        h = self._handles(over)
        ris = self.ris() if isinstance(ris, str) else ris
        return self.lib.pt_render_direct_ris(self.device._h, h["tb"], h["mb"], h["lb"], h["qb"], h["tq"], h["sb"], h["fb"], self._ref(p),
                                             self._ref(ris), cam, None)

    def direct_power(self, p, cam=None):
        """the parent: pt_render_direct_power"""
        h = self._handles({})
        return self.lib.pt_render_direct_power(self.device._h, h["tb"], h["mb"], h["lb"], h["qb"], h["tq"], h["sb"], h["fb"], self._ref(p), cam, None)

    def indirect(self, p, mis=True, rr="default", ris="default", cam=None, **over):
        """pt_render_indirect_ris"""
        h = self._handles(over)
        rr = self.roulette() if isinstance(rr, str) else rr
        ris = self.ris() if isinstance(ris, str) else ris
        return self.lib.pt_render_indirect_ris(self.device._h, h["tb"], h["mb"], h["lb"], int(mis), h["cb"] if mis or "cb" in over else None,
                                               h["qb"], h["tq"], h["sb"], h["fb"], self._ref(p), self._ref(rr), self._ref(ris), cam, None)

    def pixels(self, p, mis=True, rr="default", ris="default", cam=None, **over):
        """pt_render_indirect_pixels_ris over the list of ``set_list``"""
        h = self._handles(over)
        rr = self.roulette() if isinstance(rr, str) else rr
        ris = self.ris() if isinstance(ris, str) else ris
        return self.lib.pt_render_indirect_pixels_ris(self.device._h, h["tb"], h["mb"], h["lb"], int(mis), h["cb"] if mis or "cb" in over else None,
                                                      h["qb"], h["tq"], h["sb"], h["fb"], h["pl"], over.get("num_listed", self.listed),
                                                      self._ref(p), self._ref(rr), self._ref(ris), cam, None)

    def reset(self):
        self.fb.write(self.sentinel, len(self.sentinel))
        self.sb.write(self.ws_sentinel, self.ws_sentinel.size)

    def render_case(self, case, M=None, parent=False, nl=None, frame_begin=0, **stripes):
        """one render of ``case`` (ris_cases) from fresh sentinels, through the _ris entry point of its form -- with ``parent`` through
        pt_render_direct_power / pt_render_indirect_rr instead: (return code, framebuffer [W * H + pad, 4], workspace)"""
        name, W, H, frames, K, Mc, B, R, cap, mis = case
        assert (W, H) == (self.W, self.H), "the buffers are another image's"
        self.reset()
        nl = self.nl if nl is None else nl
        shared = dict(frame_begin=frame_begin, frame_count=frames, light_samples=K, **stripes)
        ris = self.ris(Mc if M is None else M)
        if B is None:
            p = self.direct_params(nl, **shared)
            rc = self.direct_power(p, cam=self.cam) if parent else self.direct(p, ris=ris, cam=self.cam)
        else:
            p = self.params(nl, max_bounces=B, **shared)
            if parent:
                rc = self.estimator(mis, True).rr(p, cam=self.cam, rr=self.roulette(R, cap))
            else:
                rc = self.indirect(p, mis=mis, rr=self.roulette(R, cap), ris=ris, cam=self.cam)
        return rc, self.read(), self.workspace()


def local_pixels(W, H, **stripes):
    return do.local_row_count(H, **stripes) * W if stripes else W * H
