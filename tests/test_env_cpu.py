"""Environment lighting on the CPU: the restatement (tests/env_oracle.c) against the contract's geometry and identities, the proofs that
the cases of tests/env_cases.py reach the edges they are there for, the estimator's unbiasedness and what sampling the sky buys, and
the Python surface without a device."""
import numpy as np
import pytest

import env_cases as ec
import env_oracle as eo
import power_oracle as po
import roulette_oracle as ro
from conftest import assert_fb_equal
from env_scenes import FLOOR_ALBEDO, SKY, SUN_TEXELS, env_map, env_scene

F32 = np.float32


# ---- the mappings ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 16, 64, 2048])
def test_mappings_round_trip(N):
    """the direction of a point of texel (row, col) maps back to that texel: the centres, and random points kept 1e-4 of a texel off
    the texel's edges and the fold lines' rounding"""
    rng = np.random.default_rng(N)
    n = min(N * N, 4096)
    idx = rng.choice(N * N, n, replace=False)
    row, col = idx // N, idx % N
    for off in (np.full((n, 2), 0.5), rng.uniform(1e-4, 1 - 1e-4, (n, 2))):
        ab = np.stack([(col + off[:, 0]) * (2.0 / N) - 1.0, (row + off[:, 1]) * (2.0 / N) - 1.0], 1).astype(F32)
        d, r = eo.direction_of(ab)
        assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=3e-7)
        assert np.all((r > 0.577) & (r <= 1.0 + 1e-6)), "the octahedron lies between its inscribed and circumscribed spheres"
        got = eo.texel_of(d, N)
        bad = np.flatnonzero(got != idx)
        # a point within rounding of a fold line or an edge may land next door; none of these is
        assert bad.size == 0, "N %d: %d points came back in another texel, first %s -> %s" % (N, bad.size, idx[bad[:3]], got[bad[:3]])
        assert np.array_equal(eo.texel_of(d * F32(1e-3), N), got) and np.array_equal(eo.texel_of(d * F32(1e6), N), got), "any length"


def test_stated_indices():
    """all eight octants, the fold lines, the poles, d.y = +-0, +-0 components, NaN and infinite directions give the stated texel"""
    N = 4   # texel = row * 4 + col; a, b in [-1, 1] -> index floor((c + 1) * 2), clamped
    nan, inf = np.nan, np.inf
    cases = [
        ((0, 1, 0), 2 * 4 + 2),            # the zenith: a = b = 0
        ((0, -1, 0), 3 * 4 + 3),           # the nadir: a = b = (1 - 0) * sgn(+0) = 1, clamped
        ((-0.0, -1, -0.0), 3 * 4 + 3),     # sgn(-0) = +1: the same corner
        ((1, 0.0, 0), 2 * 4 + 3),          # the horizon at +x from above: a = 1 (clamped to 3), b = 0
        ((1, -0.0, 0), 2 * 4 + 3),         # d.y = -0 counts as above
        ((1, 1, 1), 2 * 4 + 2), ((-1, 1, 1), 2 * 4 + 1), ((1, 1, -1), 1 * 4 + 2), ((-1, 1, -1), 1 * 4 + 1),          # a, b = +-1/3
        ((1, -1, 1), 3 * 4 + 3), ((-1, -1, 1), 3 * 4 + 0), ((1, -1, -1), 0 * 4 + 3), ((-1, -1, -1), 0 * 4 + 0),      # a, b = +-2/3
        ((1, 0, 1), 3 * 4 + 3),            # the fold line a + b = 1 from above: a = b = 1/2 -> index 3
        ((1, -1e-30, 1), 3 * 4 + 3),       # and from below: a = b = (1 - 1/2) = 1/2
        ((3, -1, 0), 2 * 4 + 3),           # below, b = (1 - 3/4) * sgn(+0) = 1/4 -> 2; a = 1 -> 3
        ((nan, 1, 0), 0), ((0, nan, 0), 0), ((nan, nan, nan), 0),   # s is NaN: both coordinates NaN: index 0
        ((inf, 1, 0), 2 * 4 + 0),          # x = inf / inf = NaN -> column 0; z = 0 / inf = 0 -> row 2
        ((0, 0, 0), 0),                    # 0 / 0 = NaN
        ((0, 1e-40, 0), 2 * 4 + 2),        # a subnormal zenith
    ]
    d = np.array([c[0] for c in cases], F32)
    got = eo.texel_of(d, N)
    for (v, want), g in zip(cases, got):
        assert g == want, "%s: texel %d, stated %d" % (v, g, want)
    assert np.all(eo.texel_of(d, 1) == 0) and np.all(eo.texel_of(d, 2048) < 2048 * 2048)


def test_solid_angle_sums_to_4_pi():
    """the Riemann sum of r^-3 da db over the texel centres is 4 pi: the measure the density and the table's weight rest on"""
    N = 512
    c = ((np.arange(N) + 0.5) * (2.0 / N) - 1.0).astype(F32)
    ab = np.stack(np.meshgrid(c, c, indexing="xy"), -1).reshape(-1, 2)
    _, r = eo.direction_of(ab)
    total = float(np.sum((2.0 / N) ** 2 / r.astype(np.float64) ** 3))
    assert abs(total - 4 * np.pi) < 2e-4, total


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _q(cdf):
    return np.diff(cdf.astype(np.int64))


def test_table_edges():
    """the light table's edges: the largest weight gets 65536, a weight far below it the floor of 1, a subnormal one too; zero, negative
    sums, NaN and overflowing weights get 0; an all-zero map has total 0; N = 1 is one entry"""
    N = 4
    t = np.zeros((N, N, 4), F32)
    t[..., :3] = 1.0
    flat = t.reshape(-1, 4)
    flat[0, :3] = 3e38                 # the sum overflows: infinite, counted as 0
    flat[1, :3] = (1.0, -3.0, 1.0)     # a negative sum
    flat[2, :3] = (np.nan, 1.0, 1.0)
    flat[3, :3] = 0.0
    flat[4, :3] = 1e-44                # subnormal
    flat[5, :3] = 1e-6                 # (1e-6 / 1e4) * 65536 < 1: the floor
    flat[6, :3] = 1e4                  # the largest
    q = _q(eo.table(t))
    assert list(q[:4]) == [0, 0, 0, 0] and q[4] == 1 and q[5] == 1 and q.max() == 65536
    assert np.all(q[7:] >= 1) and np.all(q[7:] < 65536)
    z = eo.table(env_map("zero:4"))
    assert np.all(z == 0) and len(z) == 17
    assert list(eo.table(env_map("grey:1"))) == [0, 65536]
    assert list(eo.table(np.full((1, 1, 3), -1.0, F32))) == [0, 0]


def test_table_follows_the_solid_angle():
    """a constant map's weights are the texels' solid angles: the centre texels (r = 1 at the zenith ... 1 / sqrt 3 on the faces' middles)
    weigh less than the face centres, and q / total times N^2 / 4 times r^3 is the constant 1 / (4 pi) to the quantum"""
    N = 64
    q = _q(eo.table(env_map("grey:64"))).astype(np.float64)
    c = ((np.arange(N) + 0.5) * (2.0 / N) - 1.0).astype(F32)
    _, r = eo.direction_of(np.stack(np.meshgrid(c, c, indexing="xy"), -1).reshape(-1, 2))
    pdf = q / q.sum() * (N * N / 4.0) * r.astype(np.float64) ** 3
    assert np.allclose(pdf, 1 / (4 * np.pi), rtol=2e-3), (pdf.min(), pdf.max())


# ---- the identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["open_panel", "many_open", "open", "floor", "glossy"])
@pytest.mark.parametrize("N", [1, 64])
def test_grey_map_without_samples_is_the_parent(scene, N):
    tris, mats, lights, cam = env_scene(scene)
    g, W, H = env_map("grey:%d" % N), 16, 12
    assert_fb_equal(eo.render(tris, mats, g, W, H, 0, 2, 2, 0, lights=lights, cam=cam),
                    po.render(po.DIRECT, tris, mats, W, H, 0, 2, 2, lights=lights, cam=cam), "direct")
    for B, R, cap in ((4, ec.NEVER, 1.0), (8, 1, 0.95)):
        assert_fb_equal(eo.render(tris, mats, g, W, H, 0, 2, 2, 0, B=B, R=R, cap=cap, lights=lights, cam=cam),
                        ro.render(tris, mats, W, H, 0, 2, 2, B, R, cap, mis=True, power=True, lights=lights, cam=cam), "indirect B %d R %d" % (B, R))


@pytest.mark.parametrize("scene,map", [("open_panel", "sun"), ("many_open", "gradient:16"), ("floor", "gradient:2")])
def test_one_bounce_is_direct(scene, map):
    tris, mats, lights, cam = env_scene(scene)
    a = eo.render(tris, mats, env_map(map), 16, 12, 0, 2, 2, 3, lights=lights, cam=cam)
    b = eo.render(tris, mats, env_map(map), 16, 12, 0, 2, 2, 3, B=1, lights=lights, cam=cam)
    assert_fb_equal(b, a, "B = 1")


def test_no_triangles_show_the_map():
    tris, mats, lights, cam = env_scene("empty")
    t = env_map("gradient:16")
    gid = np.arange(16 * 16, dtype=np.int32)
    for B in (None, 4):
        rad, d = eo.samples(tris, mats, t, 16, 16, gid, np.zeros_like(gid), 1, 1, B=B, lights=lights, cam=cam, details=True)
        assert np.all(d["miss_texel"][:, 0] >= 0)
        assert np.array_equal(rad, t.reshape(-1, 4)[d["miss_texel"][:, 0], :3]), "every sample is the texel of its primary ray"
        assert len(np.unique(d["miss_texel"][:, 0])) > 8


# ---- unbiasedness and what sampling buys ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ke,B", [(0, 2), (0, 4), (1, None), (1, 2), (1, 4)])
def test_floor_under_a_constant_sky_has_the_radiance_albedo_times_sky(Ke, B):
    """the centre pixel of the floor quad over 8 192 frames: within 4 standard errors of albedo * Le (the binary32 product: with Ke = 0
    every sample IS that product and the standard error is 0)"""
    tris, mats, lights, cam = env_scene("floor")
    W = H = 9
    centre = (H // 2) * W + W // 2
    r = eo.sample_frames(tris, mats, env_map("grey:4"), W, H, 8192, 1, Ke, B=B, lights=lights, cam=cam, pixels=[centre])[:, 0, :]
    want = float(F32(FLOOR_ALBEDO) * F32(SKY))
    mean, se = r.mean(0), r.std(0, ddof=1) / np.sqrt(len(r))
    print("Ke %d B %s: mean %s se %s" % (Ke, B, mean, se))
    assert np.all(np.abs(mean - want) <= 4 * se), (mean, se, want)
    if Ke:
        assert np.all(se > 0)


@pytest.fixture(scope="module")
def sun_room():
    """the open room under the sun map, 16 x 16, B = 4, 512 frames, with and without one environment sample per vertex"""
    tris, mats, lights, cam = env_scene("open")
    return tuple(eo.sample_frames(tris, mats, env_map("sun"), 16, 16, 512, 1, Ke, B=4, lights=lights, cam=cam) for Ke in (0, 1))


def test_sampling_the_sun_does_not_change_the_mean(sun_room):
    r0, r1 = sun_room
    d = r1.sum((1, 2)) - r0.sum((1, 2))   # per frame: the image sums' difference
    se = d.std(ddof=1) / np.sqrt(len(d))
    print("difference of the image sums: mean %.3f se %.3f (sums %.1f, %.1f)" % (d.mean(), se, r0.sum((1, 2)).mean(), r1.sum((1, 2)).mean()))
    assert abs(d.mean()) <= 4 * se


def test_sampling_the_sun_lowers_the_variance(sun_room):
    r0, r1 = sun_room
    v0, v1 = r0.var(0, ddof=1).mean(), r1.var(0, ddof=1).mean()
    print("variance per sample: Ke = 0 %.1f, Ke = 1 %.1f, ratio %.3f" % (v0, v1, v1 / v0))
    assert v1 < v0


# ---- the cases reach their edges ------------------------------------------------------------------------------------------------
def _details(cid, frames=None):
    c = ec.BY_ID[cid]
    tris, mats, lights, cam = env_scene(c.scene)
    if c.nl0:
        lights = np.zeros(0, np.int32)
    n = c.W * c.H
    f = c.frames if frames is None else frames
    gid = np.tile(np.arange(n, dtype=np.int32), f)
    frame = np.repeat(np.arange(c.frame_begin, c.frame_begin + f, dtype=np.int32), n)
    return eo.samples(tris, mats, env_map(c.map), c.W, c.H, gid, frame, c.K, c.Ke, B=c.B, R=c.R, cap=c.cap, lights=lights, cam=cam, details=True)


def _counts(reason):
    return {name: int((reason == k).sum()) for k, name in enumerate(eo.REASONS)}


def test_reasons_are_reached_by_their_cases():
    """per environment sample why it ended: each reason is reached by the case that is there for it, and the counts are the restatement's
    (the inputs are fixed)"""
    got = {cid: _counts(_details(cid)[1]["reason"]) for cid in ("panel-K3-Ke3-indirect", "zero-map-indirect", "other-type-direct",
                                                                 "glossy-nan-indirect", "many-sun-lbvh-indirect")}
    print(got)
    mixed = got["panel-K3-Ke3-indirect"]
    assert mixed["OPEN"] > 0 and mixed["OCCLUDED"] > 0 and mixed["BELOW_HORIZON"] > 0 and mixed["NOT_DRAWN"] > 0
    assert mixed["EMPTY_TABLE"] == mixed["OTHER_TYPE"] == mixed["NAN"] == 0
    zero = got["zero-map-indirect"]
    assert zero["EMPTY_TABLE"] > 0 and zero["OPEN"] == zero["OCCLUDED"] == zero["BELOW_HORIZON"] == 0
    assert got["other-type-direct"]["OTHER_TYPE"] > 0
    lb = got["many-sun-lbvh-indirect"]
    assert lb["OPEN"] > 0 and lb["OCCLUDED"] > 0
    assert got == REASON_COUNTS


def test_nan_reason_needs_a_nan_normal():
    """no ray reaches NAN -- the direction of an environment sample is finite and a ray that hits has a finite normal; a NaN ray hits
    nothing --, so the restatement is asked at a vertex of the test's own.  Beside it the other reasons at one vertex"""
    t, up = env_map("gradient:16"), (0.0, 1.0, 0.0)
    nan = (np.nan, 1.0, 0.0)
    assert eo.sample_at(t, 1, (0, 0, 0), nan, up, 7)[0] == eo.R_NAN
    assert eo.sample_at(t, 1, (0, 0, 0), up, up, 7, type=0)[0] in (eo.R_OTHER_TYPE, eo.R_BELOW_HORIZON)
    assert eo.sample_at(env_map("zero:4"), 1, (0, 0, 0), up, up, 7) == (eo.R_EMPTY_TABLE, pytest.approx([0, 0, 0]), -1)
    why = [eo.sample_at(t, 1, (0, 0, 0), up, up, seed)[0] for seed in range(64)]
    assert set(why) == {eo.R_OPEN, eo.R_BELOW_HORIZON}, "in an empty scene a sample is open or below the horizon"
    # the contribution of an open sample under a constant sky, by hand in binary64: f Le cs / pdf with pdf = 1 / (4 pi) to the quantum
    for seed in range(64):
        r, c, texel = eo.sample_at(env_map("grey:64"), 1, (0, 0, 0), up, up, seed, albedo=(0.5, 0.5, 0.5))
        if r == eo.R_OPEN:
            d = np.asarray(Environment_directions(64).reshape(-1, 3)[texel])
            assert abs(c[0] / (0.5 / np.pi * 0.45 * 4 * np.pi) - d[1]) < 0.1, "c = f Le cs / pdf within the texel's extent"


def Environment_directions(N):
    from oclpathtracer_amd.environment import Environment

    return Environment.directions(N)


# per case: why its environment samples ended, as the restatement counts them (fixed inputs, fixed counts)
REASON_COUNTS = {
    "panel-K3-Ke3-indirect": {"NOT_DRAWN": 1245, "BELOW_HORIZON": 117, "OTHER_TYPE": 0, "EMPTY_TABLE": 0, "OPEN": 156, "OCCLUDED": 42, "NAN": 0},
    "zero-map-indirect": {"NOT_DRAWN": 15411, "BELOW_HORIZON": 0, "OTHER_TYPE": 0, "EMPTY_TABLE": 7629, "OPEN": 0, "OCCLUDED": 0, "NAN": 0},
    "other-type-direct": {"NOT_DRAWN": 798, "BELOW_HORIZON": 833, "OTHER_TYPE": 939, "EMPTY_TABLE": 0, "OPEN": 60, "OCCLUDED": 250, "NAN": 0},
    "glossy-nan-indirect": {"NOT_DRAWN": 12037, "BELOW_HORIZON": 1390, "OTHER_TYPE": 0, "EMPTY_TABLE": 0, "OPEN": 179, "OCCLUDED": 1754, "NAN": 0},
    "many-sun-lbvh-indirect": {"NOT_DRAWN": 2488, "BELOW_HORIZON": 461, "OTHER_TYPE": 0, "EMPTY_TABLE": 0, "OPEN": 686, "OCCLUDED": 205, "NAN": 0},
}


def test_weighted_misses():
    """a miss at a later vertex is weighted (wb < 1) when Ke > 0, and left alone at the first vertex, with Ke = 0, where the texel's q is
    0 and where the table is empty"""
    rad, d = _details("panel-B16")
    later = d["miss_texel"][:, 1:] >= 0
    assert later.sum() > 100 and np.all(d["miss_wb"][:, 1:][later] < 1.0) and np.all(d["miss_wb"][:, 1:][later] > 0.0)
    first = d["miss_texel"][:, 0] >= 0
    assert first.sum() > 0 and np.all(d["miss_wb"][:, 0][first] == 1.0)
    _, d0 = _details("open-B4-rr-Ke0")
    assert (d0["miss_texel"][:, 1:] >= 0).sum() > 100 and np.all(d0["miss_wb"] == 1.0), "Ke = 0: unweighted"
    _, dz = _details("zero-map-indirect")
    assert (dz["miss_texel"][:, 1:] >= 0).sum() > 100 and np.all(dz["miss_wb"] == 1.0), "total == 0: wb = 1"
    _, db = _details("bad-map-indirect")
    q = _q(eo.table(env_map("bad:16")))
    hit = db["miss_texel"][:, 1:]
    zero_q = (hit >= 0) & (q[np.maximum(hit, 0)] == 0)
    assert zero_q.sum() > 0 and np.all(db["miss_wb"][:, 1:][zero_q] == 1.0), "q == 0: wb = 1"
    rb = _details("bad-map-indirect")[0]
    assert np.isnan(rad).sum() == 0 and np.isnan(rb).sum() > 0 and np.isinf(rb).sum() > 0, "the NaN and the infinite texel reach the image"
    assert (_details("bad-map-direct")[1]["miss_texel"][:, 0] == 52).sum() > 0, "a primary ray sees the negative texel"


def test_sun_texels_take_most_samples():
    """on the sun map nine tenths of the table's weight lie on the four texels: that is where the environment samples go"""
    q = _q(eo.table(env_map("sun")))
    sun = [r * 64 + c for r, c in SUN_TEXELS]
    share = q[sun].sum() / q.sum()
    assert 0.85 < share < 0.95, share
    _, d = _details("open-sun-40x24-indirect")
    chosen = d["texel"][d["texel"] >= 0]
    assert abs(np.isin(chosen, sun).mean() - share) < 0.03


def test_glossy_paths_go_nan():
    """the glossy room's NaNs are throughputs and densities, not directions: a path whose mask or pb has gone NaN still walks, looks the
    sky up where it leaves, and its miss is weighted by a NaN wb -- defined behaviour, a NaN sample (the index rule's answer for a NaN
    DIRECTION, texel 0, is test_stated_indices')"""
    rad, d = _details("glossy-nan-indirect")
    bad = np.isnan(rad).any(1)
    nan_wb = np.isnan(d["miss_wb"]).any(1)
    print("NaN samples %d, of them with a NaN miss weight %d" % (bad.sum(), (bad & nan_wb).sum()))
    assert bad.sum() > 100 and nan_wb.sum() > 10 and np.all(bad[nan_wb])


# ---- the Python surface, without a device ---------------------------------------------------------------------------------------
def test_environment_construction():
    from oclpathtracer_amd.environment import Environment

    e = Environment(np.ones((4, 4, 3)))
    assert e.size == 4 and e.texels.shape == (4, 4, 4) and e.texels.dtype == F32 and not e.texels.flags.writeable
    assert Environment(np.ones((2, 2, 4))).size == 2
    c = Environment.constant((1, 2, 3), size=8)
    assert c.size == 8 and np.all(c.texels[..., :3] == (1, 2, 3))
    assert Environment.constant(0.45).size == 1
    d = Environment.directions(16)
    assert d.shape == (16, 16, 3) and np.allclose(np.linalg.norm(d, axis=-1), 1.0)
    want, _ = eo.direction_of(np.stack(np.meshgrid(*(((np.arange(16) + 0.5) / 8 - 1,) * 2), indexing="xy"), -1).reshape(-1, 2))
    assert np.allclose(d.reshape(-1, 3), want, atol=1e-6), "directions() are the texel centres' of the contract"
    assert np.array_equal(eo.texel_of(d.reshape(-1, 3), 16), np.arange(256)), "and lie in their own texels"
    f = Environment.from_directions(lambda v: np.maximum(v, 0.0), 16)
    assert np.allclose(f.texels[..., :3], np.maximum(d, 0.0), atol=1e-6)
    s = Environment.sun((0.2, 0.7, 0.1), 2.0, 5000.0, sky=0.45, size=64)
    bright = np.argwhere(s.texels[..., 0] == 5000.0)
    assert 1 <= len(bright) <= 8 and np.all(s.texels[..., :3][s.texels[..., 0] != 5000.0] == F32(0.45))
    sd = d_sun = Environment.directions(64)[tuple(bright[0])]
    assert sd @ (np.array((0.2, 0.7, 0.1)) / np.linalg.norm((0.2, 0.7, 0.1))) > np.cos(np.radians(2.5)), d_sun
    assert len(np.argwhere(Environment.sun((0, 1, 0), 1e-3, 1.0, size=4).texels[..., 0] == 1.0)) == 1, "the nearest texel, always"
    blk = e.block(3)
    assert (blk.size, blk.env_samples, tuple(blk.reserved)) == (4, 3, (0, 0))


@pytest.mark.parametrize("bad", [np.ones((3, 3, 3)), np.ones((4, 2, 3)), np.ones((4, 4)), np.ones((4, 4, 2)), np.ones((4096, 4096, 1)), np.ones((0, 0, 3))])
def test_environment_rejects_a_bad_array(bad):
    from oclpathtracer_amd.environment import Environment

    with pytest.raises(ValueError):
        Environment(bad)


def test_environment_value_errors():
    from oclpathtracer_amd.environment import Environment, check_env_samples

    for size in (0, 3, 4096, -4, 2.5, True):
        with pytest.raises(ValueError):
            Environment.constant(1.0, size=size)
    with pytest.raises(ValueError):
        Environment.from_directions(lambda v: v[..., :2], 4)
    for direction in ((0, 0, 0), (np.nan, 1, 0), (1, 2)):
        with pytest.raises(ValueError):
            Environment.sun(direction, 1.0, 1.0)
    for radius in (0.0, -1.0, 181.0, np.nan):
        with pytest.raises(ValueError):
            Environment.sun((0, 1, 0), radius, 1.0)
    for ke in (-1, 257, 1.5, True):
        with pytest.raises(ValueError):
            check_env_samples(ke)
    assert check_env_samples(0) == 0 and check_env_samples(256) == 256


class _NoDevice:
    """stands where a device stands: a combination that must be refused is refused before the device is touched"""
    def __getattr__(self, name):
        raise AssertionError("the device was touched (%s)" % name)


def test_renderers_refuse_combinations_outside_the_two_kinds(cornell):
    from oclpathtracer_amd.direct import DirectRenderer
    from oclpathtracer_amd.environment import Environment
    from oclpathtracer_amd.indirect import IndirectRenderer

    tris, mats = cornell
    env = Environment.constant(0.45)
    dev = _NoDevice()
    refused = [
        (DirectRenderer, dict(environment=env)),                                                  # the uniform choice
        (DirectRenderer, dict(environment=env, light_choice="power", candidates=4)),              # resampling
        (DirectRenderer, dict(light_choice="power", env_samples=1)),                              # samples of no environment
        (DirectRenderer, dict(environment=env, light_choice="power", env_samples=257)),
        (DirectRenderer, dict(environment=env, light_choice="power", env_samples=-1)),
        (IndirectRenderer, dict(environment=env, light_choice="power", mis=False)),               # non-MIS indirect
        (IndirectRenderer, dict(environment=env, mis=True)),                                      # the uniform choice
        (IndirectRenderer, dict(environment=env, mis=True, light_choice="power", candidates=2)),
    ]
    for cls, kw in refused:
        with pytest.raises(ValueError):
            cls(dev, tris, mats, 8, 8, **kw)
    with pytest.raises(TypeError):
        DirectRenderer(dev, tris, mats, 8, 8, light_choice="power", environment=np.ones((4, 4, 3)))
