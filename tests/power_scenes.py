"""Scenes and light lists of the light-choice-by-power tests (tests/test_power_cpu.py, tests/test_gpu_power.py,
tests/test_gpu_light_scale.py), beside those of scenes.py: the room of unequal lights with its short lists, lists over it of up to
2^24 - 1 entries whose table's total passes 2^32 (long_list, panel_heavy_list, panel_list), and a scene that is never rendered, made
for the numeric domain of the table's powers and quanta (power_sweep).  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from oclpathtracer_amd import scene as _scene

SMALL, TINY = 48, 8          # the dim emitters of unequal_lights: q of a few units; and the ones whose q is the floor, 1
WALL = 3                     # a triangle of the Cornell box that emits nothing
LONG = 256 * 2048 + 1        # the smallest list of 257 tiles: pt_light_tiles_kernel's threads own two tiles each
MAX = (1 << 24) - 1          # the longest list the ABI accepts
_UNEQUAL = []
_LONG = {}
_SWEEP = []


def unequal_lights():
    """(tris, mats): the Cornell room with its panel (triangles 10 and 11, emission 30) plus SMALL small dim emissive triangles
    (emission 1, a new material), TINY more whose power is below 1 / 65536 of a panel triangle's (emission 1e-4: q = 1), and one
    emissive triangle of no area (q = 0) -- 36 + 48 + 8 + 1 = 93 triangles, ``scene.emitters`` names the last 57 and the panel."""
    if not _UNEQUAL:
        tris, mats = _scene.load_model()
        rng = np.random.default_rng(7)
        n = SMALL + TINY + 1
        extra = np.zeros(n, _scene.TRIANGLE_DTYPE)
        c = rng.uniform([-2.3, 0.4, -5.0], [2.3, 4.9, -0.8], (n, 3)).astype(np.float32)
        extra["p1"][:, :3] = c
        extra["p2"][:, :3] = c + rng.uniform(-0.12, 0.12, (n, 3)).astype(np.float32)
        extra["p3"][:, :3] = c + rng.uniform(-0.12, 0.12, (n, 3)).astype(np.float32)
        extra["p2"][-1] = extra["p3"][-1] = extra["p1"][-1]                  # no area
        more = np.zeros(2, _scene.MATERIAL_DTYPE)
        more["albedo"][:, :3] = 0.5
        more["albedo"][:, 3] = more["emissive"][:, 3] = 1.0
        more["roughness"], more["type"] = 1.0, _scene.DIFFUSE
        more["emissive"][0, :3], more["emissive"][1, :3] = 1.0, 1e-4
        extra["id"] = len(mats)
        extra["id"][SMALL:SMALL + TINY] = len(mats) + 1
        _UNEQUAL.append((np.concatenate([tris, extra]), np.concatenate([mats, more])))
        for a in _UNEQUAL[0]:
            a.setflags(write=False)
    return _UNEQUAL[0]


def edge_list():
    """int32: a list over unequal_lights() made for the edges of the choice -- a panel triangle first and (again: its count is 2) last,
    a wall (q = 0) directly before the other panel triangle, every q = 1 triangle twenty times over, the small ones, the one of no
    area; unsorted, with duplicates and a non-emitter"""
    tiny = np.tile(np.arange(36 + SMALL, 36 + SMALL + TINY), 20)
    return np.concatenate([[10, WALL, 11], tiny, np.arange(36, 36 + SMALL)[::-1], [36 + SMALL + TINY, WALL, 10]]).astype(np.int32)


def zero_list():
    """int32: entries of unequal_lights() none of which has positive power: walls and the emitter of no area (total == 0)"""
    return np.array([WALL, 0, 36 + SMALL + TINY, WALL], np.int32)


def long_list(nl, seed=5):
    """int32 [nl]: ``nl`` entries of unequal_lights() drawn at random from edge_list() and as many copies of the panel triangles (40
    of each) that about a quarter of the entries have q = 65536 -- walls (q = 0), q = 1 entries, duplicates and the emitter of no area
    stay in it.  The total passes 2^32 from about 230 000 entries on.  Made once per (nl, seed), read-only."""
    k = (int(nl), int(seed))
    if k not in _LONG:
        pool = np.concatenate([np.tile([10, 11], 40), edge_list()])
        _LONG[k] = np.random.default_rng(seed).choice(pool, int(nl)).astype(np.int32)
        _LONG[k].setflags(write=False)
    return _LONG[k]


def panel_heavy_list(nl, seed=5):
    """int32 [nl]: the two panel triangles at random and one q = 1 entry among them: a total of 65536 (nl - 1) + 1, which passes 2^32
    at nl = 65 537, the shortest list whose total can"""
    rng = np.random.default_rng(seed)
    li = rng.choice(np.array([10, 11], np.int32), int(nl)).astype(np.int32)
    li[int(rng.integers(0, nl))] = 36 + SMALL
    return li


def panel_list():
    """int32 [MAX]: one panel triangle 2^24 - 1 times: the total (2^24 - 1) 65536 = 2^40 - 65536 is the largest the ABI admits.  Made
    once, read-only."""
    if "panels" not in _LONG:
        _LONG["panels"] = np.full(MAX, 10, np.int32)
        _LONG["panels"].setflags(write=False)
    return _LONG["panels"]


# ---- the numeric domain of pt_light_power and pt_light_quantum -------------------------------------------------------------------
SWEEP_TRIANGLES, SWEEP_RANDOM_MATERIALS, SWEEP_GREY = 4096, 44, 12
WINDOW_RATIO, WINDOW_ENTRIES = 2.0 ** 17, 512   # a window of the sorted powers ends at this ratio to its first, or at this many entries
# the fixed materials, behind the random and the grey ones: (name, emission)
SWEEP_FIXED = (("nan", (1.0, np.nan, 1.0)), ("inf", (np.inf, 0.0, 1.0)), ("negative_sum", (1.0, -3.0, 1.0)), ("zero", (0.0, 0.0, 0.0)),
               ("overflowed_sum", (3e38, 3e38, 0.0)), ("smallest_subnormal", (1e-45, 0.0, 0.0)), ("negative_channel", (4.0, -1.0, 0.5)),
               ("subnormal_channels", (3e-42, 5e-43, 1e-44)))


def _windows(order, pw):
    """``order`` (indices by ascending power ``pw``) cut into consecutive windows: each ends before the power WINDOW_RATIO times its
    first, and holds WINDOW_ENTRIES entries at the most"""
    out, start = [], 0
    for i in range(1, len(order) + 1):
        if i == len(order) or i - start == WINDOW_ENTRIES or pw[order[i]] > WINDOW_RATIO * pw[order[start]]:
            out.append(order[start:i])
            start = i
    return out


def sweep_power(tris, mats):
    """(float64 [ntri], float64 [ntri]): area x emission sum of every triangle and its dot(N, N), from the records as the device reads
    them (material indices clamped) but in float64 throughout -- no float32 rounding, underflow or overflow; NaN and infinities as the
    emission has them"""
    p1, p2, p3 = (tris[k][:, :3].astype(np.float64) for k in ("p1", "p2", "p3"))
    with np.errstate(all="ignore"):
        n2 = (np.cross(p3 - p1, p2 - p1) ** 2).sum(axis=1)
        em = mats["emissive"][np.clip(tris["id"], 0, len(mats) - 1), :3].astype(np.float64)
        return 0.5 * np.sqrt(n2) * em.sum(axis=1), n2


def power_sweep():
    """(tris, mats, lists): a scene for the table alone -- it is never rendered -- and the light lists over it, {name: int32}.

    Triangles: right triangles, the product of whose legs is log-uniform over 1e-26 .. 1e22 and their quotient over 1e-6 .. 1e6, so
    that dot(N, N) = (leg x leg)^2 runs from underflow to zero through the subnormals and both ends of pt_sqrt's window [1e-30, 1e30]
    to overflow.  Even triangles lie along the axes at the origin; odd ones are rotated and offset by about their shorter leg, so that
    every term of the cross product is a difference that cancels.  Every eighth has power-of-two legs and a grey power-of-two material: within a list of such triangles alone every
    quotient of two powers is a power of two.  Every 32nd has legs of 1 .. 2^11 and one of the two subnormal emissions: a subnormal power
    from a normal area.  The last 32 have no area.  Materials: SWEEP_RANDOM_MATERIALS with every channel
    log-uniform over 2^-60 .. 2^60, SWEEP_GREY grey powers of two over the same range, then SWEEP_FIXED.  A few material indices lie
    out of range at either end.

    Lists: "window<k>" -- the finite positive powers (float64) in ascending order, cut so that a window's ratios stay within 2^17;
    "grey<k>" -- the same of the power-of-two triangles alone; "subnormal" -- only entries whose float64 power lies below 2^-127 (pmax is
    subnormal); "floor" -- powers above 2^120 beside powers below 2^-10 (the quotient underflows: q = 1); "zeros" -- only entries
    without positive finite power, in float64 or because dot(N, N) is infinite or zero in binary32; "all" -- every triangle at random, then once more with indices out of range at either end."""
    if _SWEEP:
        return _SWEEP[0]
    rng = np.random.default_rng(11)
    n, nr, ng = SWEEP_TRIANGLES, SWEEP_RANDOM_MATERIALS, SWEEP_GREY
    grey = np.arange(n) % 8 == 3
    product, skew = rng.uniform(-26.0, 22.0, n), rng.uniform(-3.0, 3.0, n)
    a, b = 10.0 ** (product / 2 + skew), 10.0 ** (product / 2 - skew)
    a[grey], b[grey] = 2.0 ** rng.integers(-41, 36, (2, int(grey.sum())))
    a[np.arange(n) % 32 == 9], b[np.arange(n) % 32 == 9] = 2.0 ** rng.uniform(0.0, 11.0, (2, n // 32))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(u, rng.normal(size=(n, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    origin = rng.uniform(-1.0, 1.0, (n, 3)) * np.minimum(a, b)[:, None]
    flat = np.arange(n) % 2 == 0
    u[flat], v[flat], origin[flat] = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.0
    tris = np.zeros(n, _scene.TRIANGLE_DTYPE)
    tris["p1"][:, :3] = origin
    tris["p2"][:, :3] = origin + a[:, None] * u
    tris["p3"][:, :3] = origin + b[:, None] * v
    tris["p2"][-32:] = tris["p1"][-32:]                                        # no area
    mats = np.zeros(nr + ng + len(SWEEP_FIXED), _scene.MATERIAL_DTYPE)
    mats["albedo"][:, :3], mats["albedo"][:, 3], mats["emissive"][:, 3] = 0.5, 1.0, 1.0
    mats["roughness"], mats["type"] = 1.0, _scene.DIFFUSE
    mats["emissive"][:nr, :3] = 2.0 ** rng.uniform(-60.0, 60.0, (nr, 3))
    mats["emissive"][nr:nr + ng, :3] = (2.0 ** np.linspace(-60, 60, ng).round())[:, None]
    for k, (_, em) in enumerate(SWEEP_FIXED):
        mats["emissive"][nr + ng + k, :3] = em
    ids = rng.integers(0, len(mats), n)
    ids[grey] = nr + rng.integers(0, ng, int(grey.sum()))
    tiny = np.arange(n) % 32 == 9
    ids[tiny] = nr + ng + rng.choice([k for k, (name, _) in enumerate(SWEEP_FIXED) if "subnormal" in name], int(tiny.sum()))
    ids[5::64], ids[37::64] = -3, len(mats) + 5                               # clamped to the first and the last material
    tris["id"] = ids

    pw, n2 = sweep_power(tris, mats)
    good = np.isfinite(pw) & (pw > 0)
    order = np.flatnonzero(good)[np.argsort(pw[good], kind="stable")]
    lists = {"window%d" % k: w for k, w in enumerate(_windows(order, pw))}
    lists.update({"grey%d" % k: w for k, w in enumerate(_windows(order[grey[order]], pw))})
    lists["subnormal"] = order[pw[order] < 2.0 ** -127]
    lists["floor"] = rng.permutation(np.concatenate([order[pw[order] > 2.0 ** 120], order[pw[order] < 2.0 ** -10][::3]]))
    lists["zeros"] = np.flatnonzero(~good | (n2 > 2.0 ** 130) | (n2 < 2.0 ** -151))   # ... or dot(N, N) leaves binary32 at either end
    again = rng.permutation(n)
    again[::97], again[50::97] = -1 - again[::97], n + again[50::97]
    lists["all"] = np.concatenate([rng.permutation(n), again])
    lists = {k: np.ascontiguousarray(w, np.int32) for k, w in lists.items()}
    for x in (tris, mats) + tuple(lists.values()):
        x.setflags(write=False)
    _SWEEP.append((tris, mats, lists))
    return _SWEEP[0]
