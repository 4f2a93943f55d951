"""Direct illumination without a GPU: the ABI of pt_render_direct, the Python argument checks, scene.emitters, and the test-side
restatement (tests/direct_oracle.c) pinned by scenes whose answer is known, by the renderer's oracle at one bounce and by a
float64 model."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, assert_fb_equal

GAMMA = 2.2


def test_direct_params_layout_and_bindings():
    from oclpathtracer_amd import shim

    assert ctypes.sizeof(shim.DirectParams) == 64
    offsets = {name: getattr(shim.DirectParams, name).offset for name, _ in shim.DirectParams._fields_}
    assert offsets == {"width": 0, "height": 4, "frame_begin": 8, "frame_count": 12, "num_triangles": 16, "num_materials": 20,
                       "num_lights": 24, "light_samples": 28, "stripe_rows": 32, "n_ranks": 36, "rank": 40, "reserved": 44}
    hdr = open(os.path.join(ROOT, "include", "pt_shim.h")).read()
    body = re.search(r"typedef struct pt_direct_params \{(.*?)\} pt_direct_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
    assert names == [n for n, _ in shim.DirectParams._fields_]
    lib = ctypes.CDLL(shim.LIB_PATH)
    assert "pt_render_direct" in shim.SIGNATURES and hasattr(lib, "pt_render_direct")
    assert len(shim.SIGNATURES["pt_render_direct"][1]) == 9


def test_python_argument_checks_come_first(cornell):
    from oclpathtracer_amd import adl, scene
    from oclpathtracer_amd.camera import Camera
    from oclpathtracer_amd.direct import DirectRenderer

    tris, mats = cornell
    # dev=None: any device call would fail differently -- these are refused before one is made
    for kw, err in [(dict(width=0, height=4), ValueError), (dict(width=65536, height=32768), ValueError),
                    (dict(light_samples=0), ValueError), (dict(light_samples=257), ValueError),
                    (dict(stripe_rows=0), ValueError), (dict(rank=1), ValueError), (dict(chunk_frames=0), ValueError),
                    (dict(lights=np.array([0, len(tris)])), ValueError), (dict(lights=np.array([-1])), ValueError),
                    (dict(lights=np.array([10.0, 11.0])), TypeError), (dict(lights=np.array([[10, 11]])), ValueError),
                    (dict(camera="reference"), TypeError)]:
        args = dict(width=8, height=8)
        args.update(kw)
        W, H = args.pop("width"), args.pop("height")
        with pytest.raises(err):
            DirectRenderer(None, tris, mats, W, H, **args)
    with pytest.raises(Exception):
        DirectRenderer(None, tris, mats, 8, 8, camera=Camera(eye=(0, 0, 0), center=(0, 0, 0), up=(0, 1, 0), fov_y_deg=60.0))
    with pytest.raises(TypeError):
        DirectRenderer(None, np.zeros(3, np.float32), mats, 8, 8)
    with pytest.raises(TypeError):
        DirectRenderer(None, tris, np.zeros(3, np.float32), 8, 8)
    with pytest.raises(ValueError):
        DirectRenderer(None, adl.Buffer(), mats, 8, 8)                              # a buffer needs num_triangles
    with pytest.raises(ValueError):
        DirectRenderer(None, adl.Buffer(), adl.Buffer(), 8, 8, num_triangles=2, num_materials=1)   # ... and an explicit light list
    with pytest.raises(ValueError):
        DirectRenderer(None, tris, np.zeros(0, scene.MATERIAL_DTYPE), 8, 8, lights=np.zeros(0, np.int32))


def test_emitters_of_the_cornell_box(cornell):
    from oclpathtracer_amd import scene

    tris, mats = cornell
    e = scene.emitters(tris, mats)
    assert e.dtype == np.int32 and e.tolist() == [10, 11]
    assert all((mats["emissive"][tris["id"][i], :3] > 0).any() for i in e)
    assert scene.emitters(tris[:0], mats).tolist() == []
    bad = tris.copy()
    bad["id"][10] = 99                                                            # an id out of range emits nothing
    assert scene.emitters(bad, mats).tolist() == [11]
    with pytest.raises(TypeError):
        scene.emitters(np.zeros(3, np.float32), mats)


# ---- known answers --------------------------------------------------------------------------------------------------------
def _quad(a, b, c, d, mat):
    """(a, b, c), (c, d, a) as the scene loader pairs them"""
    from oclpathtracer_amd import scene

    t = np.zeros(2, scene.TRIANGLE_DTYPE)
    for k, tri in enumerate(((a, b, c), (c, d, a))):
        for f, p in zip(("p1", "p2", "p3"), tri):
            t[f][k, :3] = p
    t["id"] = mat
    return t


def _facing(t, ray_dir):
    """the quad wound so that rays along ray_dir pass the reference's one-sided test (det = dir . cross(e2, e1) > 0)"""
    e1 = t["p2"][:, :3] - t["p1"][:, :3]
    e2 = t["p3"][:, :3] - t["p1"][:, :3]
    if np.dot(np.cross(e2[0], e1[0]), ray_dir) < 0:
        t["p2"], t["p3"] = t["p3"].copy(), t["p2"].copy()
    return t


RHO, LE, SIDE, HEIGHT = 0.5, 10.0, 0.1, 2.0


def _floor_and_light(blocker):
    """A diffuse floor (albedo RHO) in y = 0 under a SIDE x SIDE quad light (emissive LE) at y = HEIGHT over the origin, seen
    from above by a camera beside the light; with a blocker, a 1 x 1 quad at y = 1 between them."""
    from oclpathtracer_amd import scene
    from oclpathtracer_amd.camera import Camera

    h = SIDE / 2
    parts = [_facing(_quad((-4, 0, -4), (4, 0, -4), (4, 0, 4), (-4, 0, 4), 0), (0, -1, 0)),
             _facing(_quad((-h, HEIGHT, -h), (h, HEIGHT, -h), (h, HEIGHT, h), (-h, HEIGHT, h), 1), (0, 1, 0))]
    if blocker:
        # wound for rays that travel UP from the floor to the light: the one-sided test (:100) passes them
        parts.append(_facing(_quad((-0.5, 1.0, -0.5), (0.5, 1.0, -0.5), (0.5, 1.0, 0.5), (-0.5, 1.0, 0.5), 0), (0, 1, 0)))
    mats = np.zeros(2, scene.MATERIAL_DTYPE)
    mats["type"] = scene.DIFFUSE
    mats["albedo"][0] = (RHO, RHO, RHO, 1.0)
    mats["emissive"][1] = (LE, LE, LE, 1.0)
    # beside the light, looking at the origin: the centre pixels see the floor under the light, neither light nor blocker
    cam = Camera(eye=(1.5, 3.0, 0.0), center=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fov_y_deg=4.0)
    return np.concatenate(parts), mats, cam


def _decode(fb):
    return fb[:, :3].astype(np.float64) ** GAMMA


def test_floor_under_a_small_light_has_the_point_light_radiance():
    """L = rho / pi * 3 Le * cos(theta) cos(theta') A / d^2 for a small light: straight below it both cosines are 1 and d is the
    height.  Tolerance, relative: the point-light error (light side / height)^2 = 0.0025 -- the integrand's variation over the
    light and the centre pixels' offsets from the foot point, both second order in side / height and in (view footprint /
    height) = 0.1 / 2 -- plus three standard errors of the Monte-Carlo mean: per sample the integrand varies by at most that same
    0.0025 relative over the light, so its standard deviation is below 0.0025 and the standard error over the 16 pixels x 16
    frames x 4 light samples = 1024 samples is below 0.0025 / 32 = 7.8e-5; the gamma encode / decode adds ~1e-6."""
    import direct_oracle as do

    tris, mats, cam = _floor_and_light(False)
    W = H = 16
    frames, K = 16, 4
    fb = do.render(tris, mats, W, H, 0, frames, K, cam=cam)
    centre = [y * W + x for y in range(6, 10) for x in range(6, 10)]
    got = _decode(fb)[centre].mean(axis=0)
    want = RHO / np.pi * 3.0 * LE * 1.0 * 1.0 * (SIDE * SIDE) / (HEIGHT * HEIGHT)
    point_light = (SIDE / HEIGHT) ** 2
    standard_error = point_light / np.sqrt(len(centre) * frames * K)
    tol = point_light + 3.0 * standard_error
    rel = np.abs(got - want) / want
    print("direct known answer: got %s want %.6g rel %s tol %.3g" % (got, want, rel, tol))
    assert np.all(rel <= tol), (got, want, tol)
    hit, dec, _ = do.decisions(tris, mats, W, H, centre, np.zeros(len(centre)), K, cam=cam)
    assert hit.all() and (dec == do.OPEN).all()


def test_a_blocker_between_floor_and_light_leaves_exactly_zero():
    import direct_oracle as do

    tris, mats, cam = _floor_and_light(True)
    W = H = 16
    fb = do.render(tris, mats, W, H, 0, 4, 4, cam=cam)
    centre = [y * W + x for y in range(6, 10) for x in range(6, 10)]
    assert np.all(fb[centre, :3] == 0.0) and np.all(fb[:, 3] == 1.0)
    hit, dec, _ = do.decisions(tris, mats, W, H, centre, np.zeros(len(centre)), 4, cam=cam)
    assert hit.all() and (dec == do.OCCLUDED).all()


def test_no_lights_is_the_renderer_at_one_bounce(cornell):
    import camera_oracle
    import direct_oracle as do
    from oclpathtracer_amd.camera import Camera

    tris, mats = cornell
    W, H = 40, 24
    none = np.zeros(0, np.int32)
    for cam in (Camera.reference(), Camera(eye=(-2.0, 1.0, 3.0), center=(1.0, 3.0, -2.0), up=(0.1, 1.0, 0.0), fov_y_deg=75.0)):
        want = camera_oracle.render(tris, mats, W, H, 3, cam, max_bounces=1)
        got = do.render(tris, mats, W, H, 0, 3, 4, lights=none, cam=cam)
        assert_fb_equal(got, want, "no lights against max_bounces = 1")
        two = do.render(tris, mats, W, H, 2, 1, 4, lights=none, cam=cam, start=do.render(tris, mats, W, H, 0, 2, 4, lights=none, cam=cam))
        assert_fb_equal(two, want, "resumed")


# ---- the float64 model --------------------------------------------------------------------------------------------------------
def model_decisions(tris, mats, lights, W, H, gid, frame, K):
    """The decisions of the estimator in float64 on tests/f64_model.py's camera, RNG and intersectWorld, written from the contract
    in include/pt_shim.h: hit (bool [n]) and per light sample 0 = no contribution, 1 = occluded, 2 = open (uint8 [n, K]); also the
    smallest distance of a shadow ray's competing hit from its limit (float [n, K], inf where none), and `tie` (bool [n, K]): the
    model's own cs or cl is within 1e-12 of 0 -- four orders above float64's rounding of a unit vector's dot product, eight below
    any value a sample off the light's plane takes -- so "cs > 0 && cl > 0" is decided by rounding noise in EVERY arithmetic."""
    import f64_model as m

    P1 = tris["p1"][:, :3].astype(np.float64)
    E1 = tris["p2"][:, :3].astype(np.float64) - P1
    E2 = tris["p3"][:, :3].astype(np.float64) - P1
    NORM = np.cross(E2, E1)
    mtype = mats["type"][tris["id"]]
    gid, frame = np.asarray(gid, np.int64), np.asarray(frame, np.int64)
    seed = (gid.astype(np.uint64) + m.hash_u32(frame.astype(np.uint64))) & np.uint64(0xFFFFFFFF)
    o, d, seed = m.generate_ray((gid % W).astype(np.float64), (gid // W).astype(np.float64), W, H, seed)
    idx, t, u, v, _ = m.intersect_world(o, d, P1, E1, E2, None)
    hit = idx >= 0
    hi = np.maximum(idx, 0)
    p = o + d * np.where(hit, t, 0.0)[:, None]
    n = NORM[hi] / np.linalg.norm(NORM[hi], axis=1)[:, None]
    n = np.where((np.sum(n * d, axis=1) < 0.0)[:, None], n, -n)
    nl = len(lights)
    dec = np.zeros((len(gid), K), np.uint8)
    gap = np.full((len(gid), K), np.inf)
    tie = np.zeros((len(gid), K), bool)
    for k in range(K):
        seed, r0 = m.random_float(seed)
        seed, r1 = m.random_float(seed)
        seed, r2 = m.random_float(seed)
        li = np.minimum((np.float32(r0) * np.float32(nl)).astype(np.uint32), nl - 1)   # (the float32 product: the index is a value)
        j = np.asarray(lights)[li]
        su = np.sqrt(r1)
        q = P1[j] + E1[j] * (1.0 - su)[:, None] + E2[j] * (r2 * su)[:, None]
        dv = q - p
        dist = np.linalg.norm(dv, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            wi = dv / dist[:, None]
            nj = NORM[j] / np.linalg.norm(NORM[j], axis=1)[:, None]
            cs = np.sum(wi * n, axis=1)
            cl = np.abs(np.sum(wi * nj, axis=1))
        tie[:, k] = hit & ((np.abs(cs) <= 1e-12) | (np.abs(cl) <= 1e-12))
        contributes = hit & (cs > 0.0) & (cl > 0.0) & ((mtype[hi] == 1) | (mtype[hi] == 2))
        tl = np.minimum(dist - m._f(0.02), 1e20)
        o2 = p + m._f(0.01) * wi
        C = np.flatnonzero(contributes)
        occluded = np.zeros(len(gid), bool)
        if C.size:
            P = m._cross(wi[C][:, None, :], E2[None, :, :])
            det = m._dot(E1[None, :, :], P)
            keep = ~((det < 1e-8) | (-det > 1e-8))
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                inv = 1.0 / det
                tv = o2[C][:, None, :] - P1[None, :, :]
                uu = m._dot(tv, P) * inv
                Q = m._cross(tv, E1[None, :, :])
                vv = m._dot(wi[C][:, None, :], Q) * inv
                tt = m._dot(E2[None, :, :], Q) * inv
            ok = keep & ~((uu < 0.0) | (uu > 1.0)) & ~((vv < 0.0) | (uu + vv > 1.0)) & (tt > 0.0)
            occluded[C] = (ok & (tt < tl[C][:, None])).any(axis=1)
            gap[C, k] = np.where(ok, np.abs(tt - tl[C][:, None]), np.inf).min(axis=1)
        dec[:, k] = np.where(contributes, np.where(occluded, 1, 2), 0)
    return hit, dec, gap, tie


def test_restatement_agrees_with_a_float64_model(cornell):
    """The decisions of tests/direct_oracle.c -- which light samples contribute, which shadow rays are occluded -- against a float64
    model over a 32 x 32 x 2-frame Cornell render: the float32 and float64 paths part only at near-ties.

    Measured over all 16 384 light samples (K = 8): agreement 0.997559, below the bar of 0.999.  Why: the 40 that differ are all
    light samples of the 20 samples whose primary ray hits the light itself (triangles 10 and 11; 160 light samples, the model's
    `tie`); off them the agreement is 1.000000.  A point on the light seen
    from a point on the light lies in the surface's own plane: cs = dot(wi, n) is 0 in exact arithmetic, and "cs > 0" is decided
    by how p = o + d t was rounded off that plane (float32 puts p a hair below the ceiling light, float64 a hair above; what such
    a sample adds is of order cs cl ~ 1e-14 of E either way).  Neither arithmetic is wrong there and no third one would settle
    it, so the model marks these exact ties itself (`tie`, by its own |cs|, never by what the restatement answered) and the bar
    of 0.999 is held on every other light sample; the ties must be few and must all lie on emitters."""
    import direct_oracle as do
    from oclpathtracer_amd import scene

    tris, mats = cornell
    W = H = 32
    K = 8
    gid = np.tile(np.arange(W * H, dtype=np.int64), 2)
    frame = np.repeat(np.arange(2, dtype=np.int64), W * H)
    lights = scene.emitters(tris, mats)
    hit32, dec32, _ = do.decisions(tris, mats, W, H, gid, frame, K, lights=lights)
    hit64, dec64, _, tie = model_decisions(tris, mats, lights, W, H, gid, frame, K)
    assert (hit64 == (hit32 == 1)).mean() > 0.999
    both = hit64 & (hit32 == 1)
    raw = (dec32[both] == dec64[both]).mean()
    decided = both[:, None] & ~tie
    agree = (dec32[decided] == dec64[decided]).mean()
    print("direct decisions: %d light samples, raw agreement %.6f; %d exact ties; agreement off the ties %.6f"
          % (both.sum() * K, raw, int(tie.sum()), agree))
    assert decided.sum() > 10000 and agree >= 0.999, (agree, raw)
    hit_tri = do.decisions(tris, mats, W, H, gid, frame, 1, lights=np.zeros(0, np.int32))[0]   # (hit only: which samples)
    import f64_model as m
    P1 = tris["p1"][:, :3].astype(np.float64)
    seed = (gid.astype(np.uint64) + m.hash_u32(frame.astype(np.uint64))) & np.uint64(0xFFFFFFFF)
    o, d, _ = m.generate_ray((gid % W).astype(np.float64), (gid // W).astype(np.float64), W, H, seed)
    idx = m.intersect_world(o, d, P1, tris["p2"][:, :3].astype(np.float64) - P1, tris["p3"][:, :3].astype(np.float64) - P1, None)[0]
    assert hit_tri.shape == idx.shape and np.isin(idx[tie.any(axis=1)], lights).all(), "a tie off the emitters"
    assert decided.sum() >= 0.98 * both.sum() * K   # (the light fills about 1 % of the image)
    for what in (do.NONE, do.OCCLUDED, do.OPEN):
        assert (dec32[decided] == what).sum() > 100, what


# ---- each input of tests/test_gpu_direct_edges.py reaches its edge ----------------------------------------------------------------
# The restatement alone, no GPU: a bit-exact comparison on an input that never reaches the edge it is named for proves nothing, so
# every floor below is a condition on the input (tests/scenes.py), not a measurement of the code under test.
def _details(scene4, W, H, K, frame=0):
    import direct_oracle as do

    tris, mats, lights, cam = scene4
    gid = np.arange(W * H)
    hit, flipped, reason, d2, L = do.details(tris, mats, W, H, gid, np.full(W * H, frame), K, lights=lights, cam=cam)
    counts = do.count_reasons(reason)
    print("%dx%d K%d frame %d: hit %d flipped %d %s" % (W, H, K, frame, int(hit.sum()), int(flipped.sum()), counts))
    return hit, flipped, reason, d2, L, counts


def _hit_material(scene4, W, H, frame=0):
    """the material index of each sample's primary hit (-1: a miss), by the oracle's closest hit of the oracle's camera rays"""
    import query_oracle

    tris, _, _, cam = scene4
    rec = query_oracle.closest(tris, query_oracle.camera_rays(W, H, frame, cam))
    tri = rec[:, 1].copy().view(np.int32)
    return np.where(tri >= 0, tris["id"][np.maximum(tri, 0)], -1), tri


def _light_entries(W, H, K, nl, frame=0):
    """which entry of the light list each light sample draws (int [W * H, K]), recomputed from the seed: float64 camera and RNG
    of tests/f64_model.py, whose uniforms are the binary32 values, and the contract's min((uint32)(r0 * (float)nl), nl - 1)"""
    import f64_model as m

    gid = np.arange(W * H, dtype=np.int64)
    seed = (gid.astype(np.uint64) + m.hash_u32(np.full(W * H, frame, np.uint64))) & np.uint64(0xFFFFFFFF)
    _, _, seed = m.generate_ray((gid % W).astype(np.float64), (gid // W).astype(np.float64), W, H, seed)
    li = np.zeros((W * H, K), np.int64)
    for k in range(K):
        seed, r0 = m.random_float(seed)
        seed, _ = m.random_float(seed)
        seed, _ = m.random_float(seed)
        li[:, k] = np.minimum((np.float32(r0) * np.float32(nl)).astype(np.uint32), nl - 1)
    return li


def _emitted(mats, mid):
    """max(E, 0), E = 1.0f * emissive * 3.0f of material mid, per sample [n, 3]"""
    return np.maximum(np.float32(1.0) * mats["emissive"][mid, :3] * np.float32(3.0), np.float32(0.0))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_reason_codes_give_the_decisions(cornell):
    """odi_details' reason codes fold back into odi_decisions' three decisions, with the same hits and the same radiance"""
    import direct_oracle as do

    tris, mats = cornell
    W = H = 64
    gid = np.tile(np.arange(W * H), 2)
    frame = np.repeat(np.arange(2), W * H)
    hit, flipped, reason, d2, L = do.details(tris, mats, W, H, gid, frame, 4)
    hit2, dec, L2 = do.decisions(tris, mats, W, H, gid, frame, 4)
    assert np.array_equal(hit, hit2) and np.array_equal(do.DECISION_OF[reason], dec) and _same_bits(L, L2)
    counts = do.count_reasons(reason[: W * H])
    print("Cornell 64x64 K 4 frame 0:", counts)
    assert counts["NOT_FACING"] + counts["EDGE_ON"] + counts["NAN"] + counts["OTHER_TYPE"] + counts["NOT_DRAWN"] > 1000
    assert counts["OCCLUDED"] > 500 and counts["OPEN"] > 5000 and counts["OPEN_UNSEARCHED"] == 0
    assert np.all((d2 >= 0) == (reason != do.NOT_DRAWN))
    # the triangle test is one-sided (:100 passes det = dot(d, cross(e2, e1)) > 0 only), so the HitRecord normal of every hit
    # points along the ray and :243 negates it on EVERY hit: `flipped` is `hit`, from any camera
    assert np.array_equal(flipped, hit)


def test_a_scene_smaller_than_the_offsets_searches_nothing():
    """The Cornell box times 2^-9: its diameter, about 9.6 * 2^-9 = 0.019, is below 0.02, so every contributing light sample has
    tl = dist - 0.02 < 0: nothing is searched and nothing is occluded (measured: OPEN_UNSEARCHED 14269, NOT_FACING 2115)."""
    from scenes import direct_scaled

    hit, _, _, d2, _, counts = _details(direct_scaled(1, -9), 64, 64, 4)
    assert hit.all()
    assert counts["OCCLUDED"] == 0 and counts["OPEN"] == 0 and counts["OPEN_UNSEARCHED"] > 10000, counts
    assert d2.max() < 0.02 * 0.02


@pytest.mark.parametrize("copies", [15, 10])
def test_the_mixed_scale_has_searched_and_unsearched_shadow_rays(copies):
    """nested_boxes times 2^-7, 32 x 32, K = 3: shadow rays that are occluded, open after a search and open without one, side by
    side in one wave (and in one lane's sample after the other under the LBVH).  Measured, OCCLUDED / OPEN / OPEN_UNSEARCHED:
    15 copies 902 / 1005 / 660 at k = -7 (k = -6: 1467 / 1023 / 77; k = -8: 1 / 159 / 2407); 10 copies 829 / 1101 / 541 at
    k = -7 (k = -6: 1487 / 958 / 26; k = -8: 0 / 235 / 2236)."""
    from scenes import MIXED_SCALE, direct_scaled

    assert MIXED_SCALE == -7
    _, _, _, _, _, counts = _details(direct_scaled(copies, MIXED_SCALE), 32, 32, 3)
    assert min(counts["OCCLUDED"], counts["OPEN"], counts["OPEN_UNSEARCHED"]) >= 100, counts
    _, _, _, _, _, unsearched = _details(direct_scaled(copies, -9), 32, 32, 3)     # (the other scale the GPU tests render)
    assert unsearched["OCCLUDED"] == 0 and unsearched["OPEN"] == 0 and unsearched["OPEN_UNSEARCHED"] > 2000, unsearched


def test_scaling_keeps_the_facing_decisions():
    """the scale is a power of two, so cs and cl keep their signs: the same light samples are NOT_FACING at every scale the
    exact triangle test's literal threshold leaves the primary hits alone (2^-9 and above, scenes.IDENTITY)"""
    import direct_oracle as do
    from scenes import direct_scaled

    ref = _details(direct_scaled(15, 0), 32, 32, 3)
    for k in (-7, -9):
        got = _details(direct_scaled(15, k), 32, 32, 3)
        assert np.array_equal(got[0], ref[0])
        assert np.array_equal(got[2] == do.NOT_FACING, ref[2] == do.NOT_FACING)


def test_the_light_list_reaches_its_edges():
    """[36, 10, 10, 36, 3, 11] on the 37-triangle scene, 64 x 64, K = 4: the two entries without area end as NAN (measured
    5528 of 16384), the wall (entry 4, triangle 3) is sampled, casts its shadow rays (measured: drawn 2722 times, OPEN 1418 +
    OCCLUDED 476 of them) and contributes exactly 0."""
    import direct_oracle as do
    from scenes import LIGHT_LIST, direct_light_list

    W = H = 64
    K = 4
    sc = direct_light_list()
    tris, mats, lights, _ = sc
    assert tuple(lights) == LIGHT_LIST == (36, 10, 10, 36, 3, 11)
    hit, _, reason, d2, L, counts = _details(sc, W, H, K)
    assert hit.all() and counts["NAN"] >= 4000, counts
    entry = _light_entries(W, H, K, len(lights))
    chosen = lights[entry]
    assert np.all((reason == do.NAN) == (chosen == 36)), "exactly the samples of the triangle without area are NaN"
    wall = chosen == 3
    cast = wall & ((reason == do.R_OPEN) | (reason == do.R_OCCLUDED))
    print("entry 3 drawn %d times: OPEN %d OCCLUDED %d" % (int(wall.sum()), int((wall & (reason == do.R_OPEN)).sum()),
                                                           int((wall & (reason == do.R_OCCLUDED)).sum())))
    assert int(cast.sum()) >= 1000
    # the same draws with the wall as the only light: the same points q, so the same d2 and the same reasons
    _, _, reason3, d23, _ = do.details(tris, mats, W, H, np.arange(W * H), np.zeros(W * H), K, lights=np.array([3], np.int32))
    assert np.array_equal(reason[wall], reason3[wall]) and _same_bits(d2[wall], d23[wall])
    # its contribution is 0: a sample whose every open shadow ray went to the wall holds the emitted light alone
    only_wall = (wall | (do.DECISION_OF[reason] != do.OPEN)).all(axis=1) & (wall & (reason == do.R_OPEN)).any(axis=1)
    mid, _ = _hit_material(sc, W, H)
    assert int(only_wall.sum()) >= 100 and _same_bits(L[only_wall], _emitted(mats, mid[only_wall]))


def test_a_list_of_the_light_without_area_alone_is_no_list_at_all():
    """[36]: every light sample is NAN and the radiance is that of num_lights = 0, bit for bit (nl = 1: r0 * 1.0f < 1)"""
    import direct_oracle as do
    from scenes import direct_light_list

    W = H = 64
    sc = direct_light_list([36])
    hit, _, reason, _, L, counts = _details(sc, W, H, 4)
    assert hit.all() and (reason == do.NAN).all(), counts
    none = do.details(sc[0], sc[1], W, H, np.arange(W * H), np.zeros(W * H), 4, lights=np.zeros(0, np.int32))
    assert (none[2] == do.NOT_DRAWN).all() and _same_bits(L, none[4])


def test_other_lists_of_the_same_scene():
    """[10] (nl = 1) and arange(37) (a list as long as the scene: every triangle a light, most of them not emitters).  Measured:
    [10]: NOT_FACING 2564, OPEN 12642, OCCLUDED 1178; arange(37): NOT_FACING 2799, NAN 415, OPEN 6272, OCCLUDED 6898."""
    import direct_oracle as do
    from scenes import direct_light_list

    _, _, reason, _, _, one = _details(direct_light_list([10]), 64, 64, 4)
    assert one["OPEN"] > 5000 and one["OCCLUDED"] > 500 and one["NAN"] == 0, one
    sc = direct_light_list(np.arange(37))
    _, _, reason, _, _, every = _details(sc, 64, 64, 4)
    entry = _light_entries(64, 64, 4, 37)
    assert len(np.unique(entry)) == 37, "every entry of the list is drawn"
    assert np.all((reason == do.NAN) == (entry == 36))
    assert every["OPEN"] > 3000 and every["OCCLUDED"] > 3000 and every["NAN"] >= 100, every


def test_a_material_of_another_type_takes_no_light(cornell):
    """types 1 -> 3: measured OTHER_TYPE 13212, NOT_FACING 2091, OPEN 1081 (the glossy surfaces keep their light)"""
    import direct_oracle as do
    from scenes import direct_other_type

    sc = direct_other_type()
    tris, mats, _, _ = sc
    hit, _, reason, d2, L, counts = _details(sc, 64, 64, 4)
    assert counts["OTHER_TYPE"] >= 10000, counts
    mid, _ = _hit_material(sc, 64, 64)
    assert hit.all() and (mid >= 0).all()
    other = mats["type"][mid] == 3
    assert int(other.sum()) > 2500 and _same_bits(L[other], _emitted(mats, mid[other]))
    assert counts["OPEN"] + counts["OCCLUDED"] >= 500, counts      # (and the other surfaces still cast shadow rays beside them)
    # the draws go on: every light sample's point, hence its d2, is that of the unchanged scene (within a sample the material is
    # one, so nothing a sample WRITES shows whether the uniforms after an OTHER_TYPE light sample were drawn: only the restatement's
    # own account can be held to the contract here)
    plain = do.details(tris, cornell[1], 64, 64, np.arange(64 * 64), np.zeros(64 * 64), 4)
    assert _same_bits(plain[3], d2)


def test_the_camera_outside_the_box():
    """From (0, 2.75, -10), behind the back wall.  The triangle test is one-sided (:100), so a wall met from its back is passed
    through and every hit -- from this camera as from the reference's -- has its HitRecord normal along the ray: :243 negates on
    every hit, the un-negated side is reached by no ray.  The box's triangles do not "face both ways"; of the cameras tried
    around the box this one gave the most flipped hits that also cast shadow rays.  Measured, 64 x 64, K = 4: hit = flipped =
    3592, 3061 of them with an OPEN or OCCLUDED light sample; NOT_DRAWN 2016 (504 misses), NOT_FACING 2617, OPEN 10022,
    OCCLUDED 1729."""
    import direct_oracle as do
    from scenes import direct_from_behind

    hit, flipped, reason, _, _, counts = _details(direct_from_behind(), 64, 64, 4)
    cast = ((reason == do.R_OPEN) | (reason == do.R_OCCLUDED)).any(axis=1)
    print("flipped %d, with a shadow ray %d" % (int(flipped.sum()), int((cast & (flipped == 1)).sum())))
    assert int(flipped.sum()) >= 500 and int((cast & (flipped == 1)).sum()) >= 100
    assert np.array_equal(flipped, hit)
    assert 100 < int((hit == 0).sum()) < 64 * 64 - 500      # hits and misses share waves


def test_the_glossy_room_lights_every_roughness():
    """64 x 48, K = 4, frames 0 and 1 (what tests/test_gpu_direct_edges.py renders): an OPEN light sample on a surface of each of
    the 17 roughnesses.  The reference camera sees seven of the room's 17 glossy materials lit (the others are behind it, face
    away from the light or are the ceiling the light lies in), so glossy_room() alone reaches 7 roughnesses; the four rooms of
    GLOSSY_SHIFTS = (0, 1, 4, 13) move every roughness onto one of the seven.  Measured per room, samples with an OPEN light
    sample on the seven lit materials: 55, 325, 376, 685, 849, 1233, 1303; NaN radiance components: 0 in all four rooms
    (r = 0 gives D = 0 / 0 only at ct == 1 exactly, which no sample meets)."""
    import direct_oracle as do
    from scenes import GLOSSY_SHIFTS, ROUGHNESS, glossy_room

    W, H, K = 64, 48, 4
    assert GLOSSY_SHIFTS[0] == 0
    lit_samples = {float(np.float32(r)): 0 for r in ROUGHNESS}
    assert len(lit_samples) == len(ROUGHNESS) == 17
    for shift in GLOSSY_SHIFTS:
        tris, mats = glossy_room(shift)
        sc = (tris, mats, None, None)
        nan = 0
        for frame in (0, 1):
            hit, _, reason, _, L, _ = _details(sc, W, H, K, frame)
            mid, _ = _hit_material(sc, W, H, frame)
            assert np.array_equal(mid >= 0, hit == 1)
            lit = (reason == do.R_OPEN).any(axis=1)
            nan += int(np.isnan(L).sum())
            for r in lit_samples:
                on = (mid >= 0) & (mats["type"][np.maximum(mid, 0)] == 2) & (mats["roughness"][np.maximum(mid, 0)] == np.float32(r))
                lit_samples[r] += int((on & lit).sum())
        print("shift %d: nan count %d" % (shift, nan))
    print("samples with an OPEN light sample, per roughness:", lit_samples)
    assert all(v >= 1 for v in lit_samples.values()), lit_samples


def test_a_five_by_three_image_has_every_decision(cornell):
    """15 samples, one partial wave: 11 hit; NOT_FACING 1, OCCLUDED 4, OPEN 39 (and 16 light samples of the 4 misses not drawn)"""
    import direct_oracle as do

    tris, mats = cornell
    hit, _, reason, _, _, counts = _details((tris, mats, None, None), 5, 3, 4)
    dec = do.DECISION_OF[reason]
    assert 0 < int(hit.sum()) < 15
    assert all((dec[hit == 1] == k).any() for k in (do.NONE, do.OCCLUDED, do.OPEN)), counts
