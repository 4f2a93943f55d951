"""The oracle against the reference kernel's own program text, bit for bit.

oracle/_ref/libgencolors_ref.so is the reference's kernel file itself, compiled for the host (oracle/Makefile, target `ref`) over
PTSPEC stand-ins for the thirteen OpenCL built-ins it calls (oracle/ref_builtins.cpp; sin, cos and pow are the oracle library's
own).  So whatever differs here is a line of oracle/pt_oracle.c that misreads the reference: an operand order, a conversion, a draw
consumed or not, the strictness of a comparison.  A difference that only a built-in's rounding could make cannot show: the stand-ins
are the contract.

Where the reference checkout exists a missing library is a FAILURE (``__graft_entry__.build()`` makes it); elsewhere the tests that
need it skip, and the fixtures' own test (the last one) still compares them with the oracle.  "Bit for bit" is assert_fb_equal's:
NaN masks equal, every other bit equal.  The reference is fixed at 36 triangles and 16 bounces; smaller scenes run through it padded
with zero-area triangles and through the oracle as they are."""
import json
import os

import numpy as np
import pytest

import reference_cases as rc
import scenes
from conftest import GOLDEN, assert_fb_equal
from oracle import ptoracle, refprog

needs_reference = pytest.mark.skipif(not refprog.reference_present(), reason="no reference checkout on this machine")
REF_GOLDEN = os.path.join(GOLDEN, "reference_program")


@pytest.fixture(scope="module")
def sides():
    """(the compiled reference, the oracle)"""
    assert refprog.available(""), "oracle/_ref/libgencolors_ref.so is missing although the reference checkout exists: run build()"
    return refprog.Side("ref"), refprog.Side("oracle")


@pytest.fixture(scope="module")
def edge():
    """the edge rays with both sides' closest hits, computed once"""
    o, d, cls = rc.edge_rays()
    out = {}
    for which in ("ref", "oracle"):
        S = refprog.Side(which)
        res = [np.zeros(len(o), bool), np.zeros(len(o), np.float32), np.zeros((len(o), 3), np.float32),
               np.zeros((len(o), 3), np.float32), np.zeros(len(o), np.int32)]
        for name in ("cornell", "coincident"):
            k = np.flatnonzero(rc.edge_scene_of(cls) == name)
            part = S.intersect_world(refprog.pad36(rc.scene(name)[0]), o[k], d[k])
            for a, b in zip(res, part):
                a[k] = b
        out[which] = res
    return o, d, cls, out


def _same_hits(got, want, what):
    """hit flags and triangles equal; t, p, n bit for bit where hit"""
    assert np.array_equal(got[0], want[0]), "%s: hit flags differ at %s" % (what, np.flatnonzero(got[0] != want[0])[:8])
    assert np.array_equal(got[4], want[4]), "%s: triangles differ at %s" % (what, np.flatnonzero(got[4] != want[4])[:8])
    h = want[0]
    for a, b, name in zip(got[1:4], want[1:4], ("t", "p", "n")):
        assert_fb_equal(a[h], b[h], "%s: %s" % (what, name))


# ---- whole renders ---------------------------------------------------------------------------------------------------------------
@needs_reference
@pytest.mark.parametrize("variant", ["", "nofma"])
@pytest.mark.parametrize("case", rc.RENDERS, ids=[c[0] for c in rc.RENDERS])
def test_whole_render(case, variant):
    """both conventions' libraries: libgencolors_ref against libptoracle, libgencolors_ref_nofma against libptoracle_nofma"""
    assert refprog.available(variant), "oracle/_ref has no %r library although the reference checkout exists" % variant
    name, scene_name, W, H, frames, nans = case
    tris, mats = rc.scene(scene_name)
    got = refprog.Side("ref", variant).render(refprog.pad36(tris), mats, W, H, frames)
    want = ptoracle.render(tris, mats, W, H, frames, variant=variant)
    assert_fb_equal(got, want, name)
    nan = int(np.isnan(got[:, :3]).sum())
    print("%s%s: %d of %d values NaN" % (name, " (no fma)" if variant else "", nan, got[:, :3].size))
    if nans == "none":
        assert nan == 0
    assert nan <= 0.7 * got[:, :3].size, "more than 70 % NaN: a bit-exact comparison sees too little"
    assert np.all(got[:, 3] == 1.0)


@needs_reference
def test_the_two_conventions_differ():
    """libgencolors_ref_nofma is another program, not a copy: its image differs from the fused one's"""
    tris, mats = rc.scene("cornell")
    a = refprog.Side("ref").render(tris, mats, 40, 24, 3)
    b = refprog.Side("ref", "nofma").render(tris, mats, 40, 24, 3)
    assert not np.array_equal(a, b)


# ---- the fold alone --------------------------------------------------------------------------------------------------------------
@needs_reference
@pytest.mark.parametrize("z", rc.FOLD_FRAMES)
def test_fold(sides, z):
    """one kernel invocation per pixel at frame z, on a prior framebuffer of 0, -0, subnormals, 1, values above 1, negatives, +inf
    and NaN: (readFromGamma(prior) * (z - 1) + sample) / z with int * float4 and float4 / int as the reference's text has them"""
    W, H = rc.FOLD_SIZE
    tris, mats = rc.scene("cornell")
    prior = rc.fold_prior(W, H)
    for v in (0.0, 1e-40, 1.0, 1.5, -0.25, np.inf):
        assert np.any(prior[:, :3] == np.float32(v)), v
    assert np.any(np.isnan(prior)) and np.any(np.signbit(prior) & (prior == 0))
    got = prior.copy()
    for gid in range(W * H):
        refprog.kernel(tris, mats, got, W, H, z, gid)
    want = ptoracle.render(tris, mats, W, H, 1, frame_begin=z, fb=prior.copy())
    assert_fb_equal(got, want, "fold at z = %d" % z)
    assert not np.array_equal(got, prior)


@needs_reference
def test_gamma_functions(sides):
    x = np.concatenate([rc.fold_prior(16, 16), np.random.default_rng(3).uniform(0, 40, (4096, 4)).astype(np.float32)])
    for which, y in (("correct", np.float32(1.0) / np.float32(2.2)), ("read", np.float32(2.2))):
        got = refprog.gamma(which, x)
        assert_fb_equal(got[:, :3], ptoracle.pow_array(x[:, :3], float(y)), which)
        assert np.all(got[:, 3] == 1.0)


# ---- function by function --------------------------------------------------------------------------------------------------------
def _seeds():
    """2^20 seeds: 0, 61, 2^31, 2^32 - 1 and their neighbours, the low 2^16, then random ones"""
    rng = np.random.default_rng(11)
    special = np.array([0, 1, 60, 61, 62, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 2, (1 << 32) - 1, 1 << 16, 0xffff], np.uint32)
    rest = rng.integers(0, 1 << 32, (1 << 20) - len(special) - (1 << 16), dtype=np.uint64).astype(np.uint32)
    s = np.concatenate([special, np.arange(1 << 16, dtype=np.uint32), rest])
    assert s.size == 1 << 20
    return s


@needs_reference
def test_rng(sides):
    R, O = sides
    s = _seeds()
    assert np.array_equal(R.hash(s), O.hash(s))
    for k in (0, 61, 1 << 31, (1 << 32) - 1):                       # the array entry points against the scalar exports
        assert int(O.hash([k])[0]) == ptoracle.hash_u32(k)
        states, vals = ptoracle.random_floats(k, 1)
        a, v = O.random([k])
        assert int(a[0]) == states[0] and v[0] == vals[0]
    ra, rv = R.random(s)
    oa, ov = O.random(s)
    assert np.array_equal(ra, oa)
    assert_fb_equal(rv, ov, "draws")
    assert rv.min() >= 0.0 and rv.max() <= 1.0


@needs_reference
@pytest.mark.parametrize("W,H", [(1, 1), (15, 1), (13, 5), (40, 24), (1240, 1)])
def test_generate_ray(sides, W, H):
    """every pixel, at the seeds of frames 0 and 7"""
    R, O = sides
    gid = np.arange(W * H)
    for frame in (0, 7):
        seed = (gid + ptoracle.hash_u32(frame)).astype(np.uint64).astype(np.uint32)
        ro, rd, rs = R.generate_ray(gid % W, gid // W, W, H, seed)
        oo, od, os_ = O.generate_ray(gid % W, gid // W, W, H, seed)
        assert_fb_equal(ro, oo, "origins")
        assert_fb_equal(rd, od, "directions")
        assert np.array_equal(rs, os_)
        assert not np.isnan(rd).any()


@needs_reference
def test_get_ray(sides, edge):
    R, O = sides
    o, d, _, _ = edge
    ro, rd, rinv, rsign = R.get_ray(o, d)
    oo, od = O.get_ray(o, d)
    assert_fb_equal(ro, oo, "origin")
    assert_fb_equal(rd, od, "dir")
    with np.errstate(all="ignore"):
        assert_fb_equal(rinv, np.float32(1.0) / rd, "invDir")        # (the oracle drops invDir and sign: nothing reads them)
        assert np.array_equal(rsign, (rinv < 0).astype(np.float32))


@needs_reference
def test_intersection_edges(sides, edge):
    """closest hits of the edge rays, and the counts that show the rays still reach their edges"""
    o, d, cls, res = edge
    _same_hits(res["ref"], res["oracle"], "edge rays")
    hit, t, p, n, tri = res["ref"]
    print("edge rays: %d, accepted by the reference: %d" % (len(o), int(hit.sum())))
    assert hit.mean() >= 0.2
    for c, name in enumerate(rc.EDGE_CLASSES):
        k = cls == c
        print("  %-10s %5d rays, %5d accepted" % (name, int(k.sum()), int(hit[k].sum())))
        assert hit[k].sum() >= 1, name
    nf = cls == rc.EDGE_CLASSES.index("non_finite")
    assert (~hit[nf]).sum() >= 50                                    # NaN, infinite and zero rays: no hit, on both sides alike
    # two coincident triangles: the first wins
    co = cls == rc.EDGE_CLASSES.index("coincident")
    on_pair = co & hit & np.isin(tri, (0, 35))
    assert on_pair.sum() >= 40 and np.all(tri[on_pair] == 0)


@needs_reference
def test_intersect_triangle_alone(sides, edge):
    """every edge ray against the triangle it was made for and against that triangle's quad partner, the direction as given; the
    strict t < tmax at tmax == t; det on either side of +-1e-8; u = 0, v = 0 and u + v = 1 on either side of the edge"""
    R, O = sides
    o, d, cls, _ = edge
    tris = refprog.pad36(rc.scene("coincident")[0])
    rng = np.random.default_rng(5)
    tri = rng.integers(0, 36, len(o)).astype(np.int32)
    geo = cls < rc.EDGE_CLASSES.index("coincident")
    tri[geo] = np.arange(int(geo.sum())) % 36                        # the generators run over the 36 triangles in order
    tri[cls == rc.EDGE_CLASSES.index("coincident")] = 0
    dn = R.get_ray(o, d)[1]
    big = np.full(len(o), 1e20, np.float32)
    for t_ in (tri, tri ^ 1):
        got, want = R.intersect_triangle(tris, t_, o, dn, big), O.intersect_triangle(tris, t_, o, dn, big)
        assert np.array_equal(got[0], want[0])
        for a, b in zip(got[1:], want[1:]):
            assert_fb_equal(a, b, "intersectTriangle")
    acc, t, _, _ = R.intersect_triangle(tris, tri, o, dn, big)
    print("intersectTriangle alone: %d of %d accepted" % (int(acc.sum()), len(o)))
    # one triangle alone takes far fewer than the box does: the rays come from both sides and one is culled, and a ray aimed at an
    # edge falls outside it by a rounding about as often as inside.  What the checks below need is every geometric class present
    for c in range(rc.EDGE_CLASSES.index("coincident") + 1):
        assert acc[cls == c].sum() >= 10, rc.EDGE_CLASSES[c]
    # the accepted ones again with tmax == t (rejected: the comparison is strict) and the next float up (accepted)
    k = np.flatnonzero(acc)
    for tmax, expect in ((t[k], False), (np.nextafter(t[k], np.float32(np.inf)), True)):
        for S in (R, O):
            a = S.intersect_triangle(tris, tri[k], o[k], dn[k], tmax)[0]
            assert np.all(a == expect), "t < tmax at tmax = t%s" % (" + 1 ulp" if expect else "")
    # so the second of two coincident triangles loses: same t from both, tmax == t rejects
    c = np.flatnonzero(acc & (cls == rc.EDGE_CLASSES.index("coincident")))
    assert len(c) >= 40
    t35 = R.intersect_triangle(tris, np.full(len(c), 35, np.int32), o[c], dn[c], big[c])[1]
    assert np.array_equal(t35, t[c])


def _normals(rng, n):
    """unit normals: random ones, and ones whose |n.x| lies on either side of 0.001 (the tangent frame's axis switches there)"""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    edge_x = np.array([0.001, 0.0010000001, 0.00099999, 0.0009, 0.0011, 0.0, -0.0, 1.0], np.float32)
    k = n // 2
    x = edge_x[rng.integers(0, len(edge_x), k)] * rng.choice([-1.0, 1.0], k)
    yz = rng.normal(size=(k, 2))
    yz *= (np.sqrt(np.maximum(1.0 - x.astype(np.float64) ** 2, 0.0)) / np.maximum(np.linalg.norm(yz, axis=1), 1e-30))[:, None]
    v[:k, 0], v[:k, 1:] = x, yz
    v = v.astype(np.float32)
    v[:k, 0] = x                                                      # exactly the edge values
    return v


@needs_reference
def test_samplers(sides):
    R, O = sides
    rng = np.random.default_rng(8)
    n = 17 * 600
    nrm = _normals(rng, n)
    assert (np.abs(nrm[:, 0]) > np.float32(0.001)).sum() > 1000 and (np.abs(nrm[:, 0]) <= np.float32(0.001)).sum() > 1000
    seed = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    rough = np.tile(np.array(scenes.ROUGHNESS, np.float32), n // 17)
    a, b = R.sample_hemisphere_cosine(nrm, seed), O.sample_hemisphere_cosine(nrm, seed)
    assert_fb_equal(a[0], b[0], "cosine wi")
    assert np.array_equal(a[1], b[1])
    assert not np.isnan(a[0][np.abs(nrm[:, 0]) < 0.9]).any()
    a, b = R.sample_ggx(nrm, rough, seed), O.sample_ggx(nrm, rough, seed)
    assert_fb_equal(a[0], b[0], "GGX wh")
    assert_fb_equal(a[1], b[1], "GGX cosTheta")
    assert np.array_equal(a[2], b[2])
    ct = np.concatenate([a[1], np.array([0.0, 1.0, -0.0, np.nan, np.inf, 0.5], np.float32).repeat(17)])
    rr = np.concatenate([rough, np.tile(np.array(scenes.ROUGHNESS, np.float32), 6)])
    assert_fb_equal(R.distribution_ggx(ct, rr), O.distribution_ggx(ct, rr), "D")
    v = rng.normal(size=(n, 3)).astype(np.float32)
    assert_fb_equal(R.reflect(v, nrm), O.reflect(v, nrm), "reflect")


@needs_reference
def test_brdf(sides):
    """every material kind at all 17 roughnesses, wo from along the normal to grazing and below the surface: colour, wi, pdf and the
    seed afterwards.  wi and pdf go in as sentinels, so a branch that leaves one untouched must leave it on both sides"""
    R, O = sides
    rng = np.random.default_rng(9)
    _, base = rc.scene("odd_materials")
    mats = np.zeros(17 + len(base), base.dtype)
    mats[:17] = base[8]
    mats["roughness"][:17] = np.array(scenes.ROUGHNESS, np.float32)
    mats[17:] = base                                                  # diffuse, NaN / negative / zero albedo, types 0 and 3
    n = len(mats) * 400
    mi = np.arange(n) % len(mats)
    nrm = _normals(rng, n)
    # wo: the normal tilted by angles from 0 through grazing (cos about +-1e-4) to below the surface
    tang = np.cross(nrm, rng.normal(size=(n, 3)))
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    cos = np.concatenate([rng.uniform(-0.3, 1.0, n - 6 * (n // 10)), rng.uniform(-1e-3, 1e-3, 3 * (n // 10)),
                          rng.uniform(-1e-6, 1e-6, 2 * (n // 10)), np.zeros(n // 10)])
    rng.shuffle(cos)
    wo = (nrm * cos[:, None] + tang * np.sqrt(1 - cos[:, None] ** 2)).astype(np.float32)
    seed = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    wi0, pdf0 = np.full((n, 3), -7.25, np.float32), np.full(n, -3.5, np.float32)
    rcol, rw, rwi, rpdf, rseed = R.brdf(wo, nrm, mats, mi, seed, wi0, pdf0)
    ocol, _, owi, opdf, oseed = O.brdf(wo, nrm, mats, mi, seed, wi0, pdf0)
    assert_fb_equal(rcol, ocol, "colour")
    assert_fb_equal(rwi, owi, "wi")
    assert_fb_equal(rpdf, opdf, "pdf")
    assert np.array_equal(rseed, oseed)
    typ = mats["type"][mi]
    early = (typ == 2) & (rpdf == np.float32(-3.5))                  # return 0.0f: wi written, pdf not, two draws consumed
    other = (typ != 1) & (typ != 2)
    print("Brdf: %d calls, %d diffuse, %d specular of which %d returned early, %d of another type" % (
        n, int((typ == 1).sum()), int((typ == 2).sum()), int(early.sum()), int(other.sum())))
    assert early.sum() >= 100 and np.all(rcol[early] == 0) and not np.any(rwi[early] == np.float32(-7.25))
    assert other.sum() >= 100 and np.all(rwi[other] == np.float32(-7.25)) and np.array_equal(rseed[other], seed[other])
    assert np.all(rcol[other] == 0) and np.all(rw[other] == 1.0)
    assert np.all(rseed[~other] != seed[~other])


@needs_reference
def test_trace_rays(sides, oracle):
    """traceRays from the primary ray and seed of every sample of a 16 x 16 image, frames 0 to 7: the radiance before the fold"""
    R, O = sides
    W = H = 16
    for name in ("cornell", "odd_materials"):
        tris, mats = rc.scene(name)
        for frame in range(8):
            gid = np.arange(W * H)
            seed = (gid + ptoracle.hash_u32(frame)).astype(np.uint64).astype(np.uint32)
            o, d, s = R.generate_ray(gid % W, gid // W, W, H, seed)
            rad, after = R.trace_rays(tris, mats, o, d, s)
            want = np.stack([oracle.radiance(tris, mats, int(g), W, H, frame) for g in gid])
            assert_fb_equal(rad, want, "%s frame %d" % (name, frame))
            orad, oafter = O.trace_rays(tris, mats, o, d, s)
            assert_fb_equal(orad, want, "the oracle's two entry points")
            assert np.array_equal(after, oafter), "seeds after the path differ"


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------
def _fixture(name):
    return np.load(os.path.join(REF_GOLDEN, name + ".npy"))


def _fixture_inputs():
    with open(os.path.join(REF_GOLDEN, "manifest.json")) as f:
        return json.load(f)


def test_fixtures_are_small():
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if os.path.isfile(os.path.join(GOLDEN, f)))
    sizes = [os.path.getsize(os.path.join(REF_GOLDEN, f)) for f in os.listdir(REF_GOLDEN)]
    assert max(sizes) <= largest and sum(sizes) < 256 * 1024, (max(sizes), sum(sizes))


@pytest.mark.parametrize("side", ["oracle", pytest.param("ref", marks=needs_reference)])
def test_fixtures(side):
    """tests/golden/reference_program/ holds what the reference's program wrote (tests/golden/make_reference_golden.py): every
    fixture equals the oracle everywhere, and a fresh run of the compiled reference where that exists"""
    if side == "ref":
        assert refprog.available(""), "oracle/_ref/libgencolors_ref.so is missing although the reference checkout exists"
    S = refprog.Side(side)
    man = _fixture_inputs()
    assert [m["name"] for m in man["renders"]] == [g[0] for g in rc.GOLDEN_RENDERS]
    for name, scene_name, W, H, frames in rc.GOLDEN_RENDERS:
        tris, mats = rc.scene(scene_name)
        if side == "ref":
            tris = refprog.pad36(tris)
        assert_fb_equal(S.render(tris, mats, W, H, frames)[:, :3], _fixture(name), name)
    W, H, frames = rc.GOLDEN_RAYS
    gid = np.arange(W * H)
    for frame in frames:
        seed = (gid + ptoracle.hash_u32(frame)).astype(np.uint64).astype(np.uint32)
        o, d, _ = S.generate_ray(gid % W, gid // W, W, H, seed)
        assert_fb_equal(np.concatenate([o, d], axis=1), _fixture("rays_%dx%d_f%d" % (W, H, frame)), "rays of frame %d" % frame)
    o, d, cls = rc.edge_rays()
    keep = rc.golden_hit_selection(cls)
    rays, hits = _fixture("edge_rays"), _fixture("edge_hits")
    assert_fb_equal(rays[:, :6], np.concatenate([o[keep], d[keep]], axis=1), "the edge rays themselves")
    assert np.array_equal(rays[:, 6].astype(np.int32), cls[keep])
    for name in ("cornell", "coincident"):
        k = np.flatnonzero(rc.edge_scene_of(cls[keep]) == name)
        hit, t, p, n, tri = S.intersect_world(refprog.pad36(rc.scene(name)[0]), o[keep][k], d[keep][k])
        assert np.array_equal(tri, hits[k, 0].astype(np.int32)), name
        assert_fb_equal(np.concatenate([t[:, None], p, n], axis=1)[hit], hits[k, 1:][hit], "edge hits on %s" % name)
