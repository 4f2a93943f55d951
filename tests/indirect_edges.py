"""The inputs of tests/test_gpu_indirect_edges.py and what the restatement (tests/indirect_oracle.c) says of them: one table, so that
tests/test_indirect_cpu.py proves its floors on exactly the scenes and sizes the device renders.  TEST INFRASTRUCTURE.

A case is (scene name of scenes.edge_scene, W, H, frames, K, B, stripes): ``stripes`` a dict of stripe_rows / n_ranks / rank."""
from __future__ import annotations

import numpy as np

import direct_oracle as do
import indirect_oracle as io
from scenes import FINITE_SHIFTS, MIXED_SCALE, edge_scene

FINITE_SIZE = (40, 24, 3)                 # W, H, frames of the finite glossy rooms
FINITE_KB = ((1, 4), (2, 6))              # (K, B)
SCALED_SIZE = (32, 32, 2, 2, 4)           # W, H, frames, K, B of the scaled scenes
SCALED = ["scaled:15,%d" % MIXED_SCALE, "scaled:15,-9", "scaled:10,%d" % MIXED_SCALE, "scaled:10,-9", "scaled:1,-9"]
NAMED_SIZE = (40, 24, 2, 4, 4)
NAMED = ["lights:list", "lights:36", "lights:10", "lights:all", "other_type", "from_behind"]
SMALL = [(5, 3, 4), (1, 1, 16), (13, 5, 4)]   # (W, H, B), 2 frames, K = 4: one partial wave; one sample; a full wave and one lane
SMALL_SCENES = ["cornell", "nested:15"]
STRIPED_SIZE = (40, 31, 2, 2, 4)          # 1 240 pixels: 19 waves and 24 lanes; rows of 5 over 3 ranks are 440, 400 and 400 pixels
STRIPE_ROWS, RANKS = 5, 3
CHUNKED_FRAMES = 5
LIMITS_SIZE = (16, 16, 1)
LIMITS_KB = ((1, 3), (256, 3), (1, 65535), (1, 64))
CLAMPED_SIZE = (40, 24, 1, 2, 3)


def clamped_raw(ntri):
    """the light list of the raw C-ABI call; the device clamps each index to [0, ntri) where it uses it"""
    return [-1, 10, ntri + 5, 11]


def clamped_scene():
    """the Cornell box with the light list the device makes of clamped_raw"""
    _, (tris, mats, _, _) = edge_scene("cornell")
    raw = clamped_raw(len(tris))
    return "cornell:clamped", (tris, mats, np.clip(raw, 0, len(tris) - 1).astype(np.int32), None)


def cases():
    """every (group, scene name, W, H, frames, K, B, stripes) the GPU module compares with the restatement"""
    out = []
    for shift in FINITE_SHIFTS:
        for K, B in FINITE_KB:
            out.append(("finite", "finite:%d" % shift) + FINITE_SIZE + (K, B, {}))
    out += [("scaled", name) + SCALED_SIZE + ({},) for name in SCALED]
    out += [("named", name) + NAMED_SIZE + ({},) for name in NAMED]
    out += [("small", name, W, H, 2, 4, B, {}) for name in SMALL_SCENES for W, H, B in SMALL]
    out.append(("stripes", "cornell") + STRIPED_SIZE + (dict(stripe_rows=STRIPE_ROWS),))
    out += [("stripes", "cornell") + STRIPED_SIZE + (dict(stripe_rows=STRIPE_ROWS, n_ranks=RANKS, rank=r),) for r in range(RANKS)]
    W, H, _, K, B = STRIPED_SIZE
    out.append(("chunks", "cornell", W, H, CHUNKED_FRAMES, K, B, {}))
    out += [("limits", "cornell") + LIMITS_SIZE + (K, B, {}) for K, B in LIMITS_KB]
    out.append(("clamped", "cornell:clamped") + CLAMPED_SIZE + ({},))
    return out


def scene_of(name):
    return clamped_scene() if name == "cornell:clamped" else edge_scene(name)


def _want(name, W, H, frames, K, B, **stripes):
    tris, mats, lights, cam = scene_of(name)[1]
    gid, frame = do.sample_ids(W, H, frames, **stripes)
    return (io.render(tris, mats, W, H, 0, frames, K, B, lights=lights, cam=cam, **stripes),
            io.samples(tris, mats, W, H, gid, frame, K, B, lights=lights, cam=cam)[0].reshape(frames, -1, 3))


def wanted(name, W, H, frames, K, B, **stripes):
    """the restatement's (framebuffer, radiance [frames, local pixels, 3]) of a case: computed once, shared, read-only"""
    return do.once(_want, name, W, H, frames, K, B, **stripes)


def details(name, W, H, frames, K, B, **stripes):
    """io.details of every local sample of a case"""
    tris, mats, lights, cam = scene_of(name)[1]
    gid, frame = do.sample_ids(W, H, frames, **stripes)
    return io.details(tris, mats, W, H, gid, frame, K, B, lights=lights, cam=cam)
