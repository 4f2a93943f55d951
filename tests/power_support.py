"""What tests/test_gpu_power.py and tests/test_gpu_light_scale.py need beside gpu_support: the raw C-ABI harness of
pt_render_direct_power and pt_render_indirect_power (gpu_support.LitBuffers with the table's two buffers and the new argument lists), a
raw pt_light_table call with its comparison against the restatement, and one render through the Python renderers with
``light_choice="power"``.  TEST INFRASTRUCTURE (an ordinary module: every assert carries its message)."""
import ctypes

import numpy as np

import power_oracle as po
from gpu_support import LitBuffers, lit_with_samples
from oclpathtracer_amd import shim

_PARENT = {po.DIRECT: "pt_render_direct", po.INDIRECT: "pt_render_indirect", po.MIS: "pt_render_indirect_mis"}


def power_with_samples(device, mode, scene4, W, H, frames, K, B=1, **kw):
    """gpu_support.lit_with_samples for the estimator ``mode`` of power_oracle with the choice by power"""
    return lit_with_samples(device, scene4, W, H, frames, K, max_bounces=None if mode == po.DIRECT else B, mis=mode == po.MIS,
                            light_choice="power", **kw)


def device_table(device, tris, mats, lights, num_triangles=None, tables=None):
    """One raw pt_light_table over fresh scene buffers: (return code, cdf uint64 [nl + 1], tri_q uint32 [num_triangles]).  tables: a
    (cdf, tri_q) pair of adl.Buffers to build into (kept), otherwise fresh ones filled with a sentinel first."""
    from oclpathtracer_amd import adl, scene

    lib = shim.load()
    li = np.ascontiguousarray(lights, np.int32)
    ntri = len(tris) if num_triangles is None else num_triangles
    words = lib.pt_light_table_bytes(len(li)) // 8
    tb = adl.Buffer(device, max(len(tris), 1), scene.TRIANGLE_DTYPE)
    mb = adl.Buffer(device, len(mats), scene.MATERIAL_DTYPE)
    lb = adl.Buffer(device, max(len(li), 1), np.int32)
    qb, tq = tables if tables else (adl.Buffer(device, words, np.uint64), adl.Buffer(device, max(ntri, 1), np.uint32))
    try:
        if len(tris):
            tb.write(np.ascontiguousarray(tris), len(tris))
        mb.write(np.ascontiguousarray(mats), len(mats))
        if len(li):
            lb.write(li, len(li))
        if not tables:
            qb.write(np.full(words, 0xdeadbeefdeadbeef, np.uint64), words)
            tq.write(np.full(max(ntri, 1), 0xdeadbeef, np.uint32), max(ntri, 1))
        rc = lib.pt_light_table(device._h, tb._h, ntri, mb._h, len(mats), lb._h if len(li) else None, len(li), qb._h, tq._h, None)
        cdf, tri_q = np.zeros(len(li) + 1, np.uint64), np.zeros(max(ntri, 1), np.uint32)
        qb.read(cdf, len(cdf))
        tq.read(tri_q, len(tri_q))
        device.waitForCompletion()
        return rc, cdf, tri_q[:ntri]
    finally:
        for b in (tb, mb, lb) + (() if tables else (qb, tq)):
            b.release()


def assert_table(device, tris, mats, lights, what, want=None, **kw):
    """pt_light_table of the list (``device_table``) is the restatement's, cdf[0 .. nl] and tri_q bit for bit.  want: the restatement's
    (cdf, tri_q) where the caller has it already.  Returns the device's pair."""
    rc, cdf, tri_q = device_table(device, tris, mats, lights, **kw)
    assert rc == shim.PT_OK, what
    want_cdf, want_q = po.table(tris, mats, lights) if want is None else want
    assert np.array_equal(cdf, want_cdf), "%s: cdf differs first at %s" % (what, np.flatnonzero(cdf != want_cdf)[:4])
    assert np.array_equal(tri_q, want_q), "%s: tri_q differs at %s" % (what, np.flatnonzero(tri_q != want_q)[:4])
    return cdf, tri_q


class PowerBuffers(LitBuffers):
    """The buffers of one raw call of pt_render_direct_power (``mode`` DIRECT) or pt_render_indirect_power (INDIRECT: mis = 0, MIS:
    mis = 1 with the counts): the parent entry point's, and the table of the list (``qb``, ``tq``) made by pt_light_table."""

    def __init__(self, mode, device, tris, mats, W, H, lights=(10, 11), frames=1, pad=4):
        from oclpathtracer_amd import adl

        super().__init__(_PARENT[mode], device, tris, mats, W, H, lights=lights, frames=frames, pad=pad)
        self.mode = mode
        self.qb = adl.Buffer(device, self.lib.pt_light_table_bytes(len(lights)) // 8, np.uint64)
        self.tq = adl.Buffer(device, max(len(tris), 1), np.uint32)
        assert self.lib.pt_light_table(device._h, self.tb._h, len(tris), self.mb._h, len(mats), self.lb._h if len(lights) else None,
                                       len(lights), self.qb._h, self.tq._h, None) == shim.PT_OK

    def call(self, p, cam=None, **over):
        h = {name: over.get(name, getattr(self, name)) for name in ("tb", "mb", "lb", "cb", "qb", "tq", "sb", "fb")}
        h = {k: (b._h if b is not None else None) for k, b in h.items()}
        pp = ctypes.byref(p) if p is not None else None
        if self.mode == po.DIRECT:
            return self.lib.pt_render_direct_power(self.device._h, h["tb"], h["mb"], h["lb"], h["qb"], h["tq"], h["sb"], h["fb"], pp, cam, None)
        return self.lib.pt_render_indirect_power(self.device._h, h["tb"], h["mb"], h["lb"], int(over.get("mis", self.mode == po.MIS)), h["cb"],
                                                 h["qb"], h["tq"], h["sb"], h["fb"], pp, cam, None)

    def release(self):
        super().release()
        for b in (self.qb, self.tq):
            b.release()
