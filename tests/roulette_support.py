"""What tests/test_gpu_roulette.py needs beside gpu_support and power_support: the raw C-ABI harness of pt_render_indirect_rr
(power_support.PowerBuffers with the roulette block and the new argument list) and one render through IndirectRenderer with
``roulette=``.  TEST INFRASTRUCTURE (an ordinary module: every assert carries its message)."""
import ctypes

import power_oracle as po
from gpu_support import lit_with_samples
from oclpathtracer_amd import shim
from oclpathtracer_amd.indirect import Roulette
from power_support import PowerBuffers


def roulette_with_samples(device, scene4, W, H, frames, K, B, R, cap, mis=False, power=False, **kw):
    """gpu_support.lit_with_samples for the estimator (mis, power) with the roulette (R, cap)"""
    return lit_with_samples(device, scene4, W, H, frames, K, max_bounces=B, mis=mis, light_choice="power" if power else "uniform",
                            roulette=Roulette(R, cap), **kw)


class RouletteBuffers(PowerBuffers):
    """The buffers of one raw call of pt_render_indirect_rr: pt_render_indirect_power's with mis = 1 (the counts and the table are
    there; ``call`` passes what the estimator (mis, power) takes, NULL otherwise) and the roulette block."""

    def __init__(self, device, tris, mats, W, H, mis=True, power=True, **kw):
        super().__init__(po.MIS, device, tris, mats, W, H, **kw)
        self.mis, self.power = mis, power

    def roulette(self, first_bounce=1, max_survival=0.5, reserved=None):
        r = shim.Roulette(first_bounce, max_survival)
        if reserved is not None:
            r.reserved[reserved] = 1
        return r

    def call(self, p, cam=None, rr="default", **over):
        h = {name: over.get(name, getattr(self, name)) for name in ("tb", "mb", "lb", "cb", "qb", "tq", "sb", "fb")}
        mis = int(over.get("mis", self.mis))
        if not mis and "cb" not in over:
            h["cb"] = None
        if not self.power:
            h["qb"], h["tq"] = over.get("qb"), over.get("tq")
        h = {k: (b._h if b is not None else None) for k, b in h.items()}
        if isinstance(rr, str):
            rr = self.roulette()
        return self.lib.pt_render_indirect_rr(self.device._h, h["tb"], h["mb"], h["lb"], mis, h["cb"], h["qb"], h["tq"], h["sb"], h["fb"],
                                              ctypes.byref(p) if p is not None else None, ctypes.byref(rr) if rr is not None else None, cam, None)
