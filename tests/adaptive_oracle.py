"""The numpy restatement of adaptive sampling (include/pt_shim.h states every step): pt_adaptive_select's rule and list, and the loop
of IndirectRenderer.render_adaptive built on it.  The rule follows the header's operations one by one on moments_oracle's resolve (numpy
rounds each float64 operation on its own); the loop takes its samples from roulette_oracle.samples, counts them with
moments_oracle.accumulate and forms the image from roulette_oracle.render by the identity the feature rests on: a pixel that has received
n samples holds what the uniform render holds for it after n frames.  Nothing is compiled.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import collections

import numpy as np

import direct_oracle as do
import moments_oracle as mom
import roulette_oracle as ro

SLOT_DTYPE = np.dtype([("pixel", np.uint32), ("frame", np.uint32)])   # pt_pixel_slot
HEADER_BYTES = 16
Rule = collections.namedtuple("Rule", "tol2 floor2 min_samples max_samples")


def rule_of(tolerance, floor, min_samples, max_samples) -> Rule:
    """the rule render_adaptive hands to the device: the squares are formed in Python floats"""
    return Rule(float(tolerance) * float(tolerance), float(floor) * float(floor), int(min_samples), int(max_samples))


def terms(moments):
    """(b, c) float64 [pixels] of pt_adaptive_select's step 2 -- pt_moments_resolve's se2_sum and mean2_sum terms -- for every record,
    whatever its n (the rule looks at them only when n >= 2)"""
    m = np.asarray(moments)
    mean, v = mom.resolve(m)
    n = m["n"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        b = ((v[:, 0] / n) + (v[:, 1] / n)) + (v[:, 2] / n)
        c = ((mean[:, 0] * mean[:, 0]) + (mean[:, 1] * mean[:, 1])) + (mean[:, 2] * mean[:, 2])
    return b, c


def active(moments, rule: Rule):
    """(active bool [pixels], taken uint64 [pixels])"""
    m = np.asarray(moments)
    taken = m["n"].astype(np.uint64) + m["rejected"].astype(np.uint64)
    b, c = terms(m)
    with np.errstate(invalid="ignore", over="ignore"):
        noisy = (m["n"] >= 2) & (b > np.float64(rule.tol2) * (c + np.float64(rule.floor2)))   # (a comparison with a NaN is false)
    return (taken < np.uint64(rule.max_samples)) & ((m["n"] < np.uint32(min(rule.min_samples, 0xFFFFFFFF))) | noisy), taken


def select(moments, rule: Rule) -> np.ndarray:
    """the slots of the list, SLOT_DTYPE [count]: the active pixels ascending, frame = (uint32)taken"""
    a, taken = active(moments, rule)
    out = np.zeros(int(a.sum()), SLOT_DTYPE)
    out["pixel"] = np.flatnonzero(a)
    out["frame"] = (taken[a] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out


def list_bytes(moments, rule: Rule) -> bytes:
    """header and slots as the device writes them"""
    s = select(moments, rule)
    return np.array([len(s), 0, 0, 0], np.uint32).tobytes() + s.tobytes()


Loop = collections.namedtuple("Loop", "passes moments counts fb finite")


def loop(scene4, W, H, K, B, R, cap, *, mis, power=False, tolerance, min_samples, max_samples, frames_per_pass, floor=1e-2, **stripes) -> Loop:
    """render_adaptive from a fresh renderer: ``passes`` the list length of every pass, ``moments`` the records, ``counts`` uint32 n +
    rejected, ``fb`` float32 [local pixels, 4] the framebuffer, ``finite`` whether every sample taken was finite"""
    tris, mats, lights, cam = scene4
    gids = do.local_gids(W, H, **stripes)
    rule = rule_of(tolerance, floor, min_samples, max_samples)
    kw = dict(mis=mis, power=power, lights=lights, cam=cam)

    def radiance(pixels, first, frames):
        """float32 [frames, len(pixels), 3]: frames first[j] .. first[j] + frames - 1 of local pixel pixels[j]"""
        gid = np.tile(gids[pixels], frames)
        frame = (np.asarray(first, np.int64)[None, :] + np.arange(frames, dtype=np.int64)[:, None]).reshape(-1)
        return ro.samples(tris, mats, W, H, gid, frame, K, B, R, cap, **kw)[0].reshape(frames, len(pixels), 3)

    every = np.arange(len(gids))
    finite = True
    m = mom.zeros(len(gids))
    if min_samples > 0:
        rad = radiance(every, np.zeros(len(gids), np.int64), min_samples)
        finite &= bool(np.isfinite(rad).all())
        m = mom.accumulate(rad)
    passes = []
    while True:
        s = select(m, rule)
        if len(s) == 0:
            break
        passes.append(len(s))
        rad = radiance(s["pixel"], s["frame"], frames_per_pass)
        finite &= bool(np.isfinite(rad).all())
        m[s["pixel"]] = mom.accumulate(rad, m[s["pixel"]])
    counts = m["n"] + m["rejected"]
    fb = np.zeros((len(gids), 4), np.float32)
    for n in np.unique(counts):
        if n:
            fb[counts == n] = ro.render(tris, mats, W, H, 0, int(n), K, B, R, cap, **kw, **stripes)[counts == n]
    return Loop(tuple(passes), m, counts, fb, finite)
