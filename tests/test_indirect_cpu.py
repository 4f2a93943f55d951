"""The CPU restatement of pt_render_indirect (tests/indirect_oracle.c) against the statements it repeats, without a GPU.

Two identities pin it bit for bit: with no lights it is the oracle's renderer at the same depth (ptor_render), at one bounce it is
direct illumination's restatement (odi_render).  One statistical check covers what neither identity reaches -- light samples at
later vertices, weighted by the path's mask, in place of the emission found by BRDF rays: the light-sampled estimator and the plain
one must have the same mean."""
import numpy as np
import pytest

import direct_oracle as do
import indirect_oracle as io
from conftest import assert_fb_equal
from indirect_scenes import diffuse_cornell
from scenes import direct_light_list, glossy_room

W, H, FRAMES = 40, 24, 3
NONE = np.zeros(0, np.int32)


@pytest.mark.parametrize("B", [1, 2, 16])
@pytest.mark.parametrize("name", ["cornell", "glossy_room"])
def test_no_lights_is_the_renderer(oracle, cornell, name, B):
    tris, mats = cornell if name == "cornell" else glossy_room(0)
    want = oracle.render(tris, mats, W, H, FRAMES, max_bounces=B)
    for K in (1, 4):   # (K is not looked at without lights)
        assert_fb_equal(io.render(tris, mats, W, H, 0, FRAMES, K, B, lights=NONE), want, "%s B%d K%d" % (name, B, K))


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("name", ["cornell", "light_list"])
def test_one_bounce_is_direct_illumination(cornell, name, K):
    if name == "cornell":
        tris, mats = cornell
        lights = None
    else:
        tris, mats, lights, _ = direct_light_list()
    want = do.render(tris, mats, W, H, 0, FRAMES, K, lights=lights)
    assert_fb_equal(io.render(tris, mats, W, H, 0, FRAMES, K, 1, lights=lights), want, "%s K%d" % (name, K))


def test_the_comparison_is_not_vacuous(oracle, cornell):
    """On the Cornell box at B = 16, K = 1 -- the GPU test's input -- the image is neither the renderer's nor direct illumination's,
    every reason for a path's end occurs, some path reaches vertex B, and light samples at later vertices are occluded and open."""
    tris, mats = cornell
    B, frames = 16, 5
    got = io.render(tris, mats, W, H, 0, frames, 1, B)
    assert not np.array_equal(got, oracle.render(tris, mats, W, H, frames, max_bounces=B))
    assert not np.array_equal(got, do.render(tris, mats, W, H, 0, frames, 1))
    gid, frame = io.all_samples(W, H, frames)
    rad, vertices, end, later = io.samples(tris, mats, W, H, gid, frame, 1, B)
    counts = {"miss": int((end == io.END_MISS).sum()), "pdf": int((end == io.END_PDF).sum()), "depth": int((end == io.END_DEPTH).sum()),
              "reached B": int((vertices == B).sum()), "later open": int(later[:, 0].sum()), "later occluded": int(later[:, 1].sum())}
    print(counts)
    assert all(v > 0 for v in counts.values()), counts
    assert vertices.max() == B and np.isfinite(rad).all()


# ---- unbiasedness ---------------------------------------------------------------------------------------------------------------
# The per-sample radiance before the fold of the all-diffuse Cornell box at B = 4, averaged over a 16 x 16 image and N frames.
# How N and the scale were obtained, with the oracle's PLAIN estimator (lights = []) alone: scale = |mean over frames [0, N) - mean
# over frames [N, 2N)| per channel; N = 200, 400, 800, ... doubled until every channel's scale is below 2 % of its mean.  200 .. 1600
# leave a channel at 2.2 %, 3.8 %, 2.3 %, 2.1 %; N = 3200 is the first to pass, with the figures below (1.4 %, 0.9 %, 1.2 % of the
# mean 1.296, 1.238, 1.016).  The test computes the scale again and checks the constants, so they cannot go stale.
# The light-sampled estimator is NOT the quieter of the two here: the box's light hangs 0.008 below the ceiling, and a light
# sample from a ceiling vertex above it has 1 / d^2 up to 1 / 6.4e-5.  Its value is bounded (about 4.7e5) and its mean right, but one
# such sample (3.76e5, pixel 23 of frame 6065) moves a mean over 256 x 6400 samples by 0.23: at N = 6400 the difference of the two
# estimators is 0.25 against a scale of 0.003.  Up to frame 3200 no such sample occurs.
UNBIASED_N = 3200
UNBIASED_SCALE = (0.01835795, 0.01169497, 0.01260588)


def _mean_radiance(tris, mats, lights, frame_begin, frames):
    gid, frame = io.all_samples(16, 16, frames, frame_begin)
    return io.samples(tris, mats, 16, 16, gid, frame, 1, 4, lights=lights)[0].astype(np.float64).mean(0)


def test_light_sampling_is_unbiased():
    tris, mats = diffuse_cornell()
    N = UNBIASED_N
    plain = _mean_radiance(tris, mats, NONE, 0, N)
    scale = np.abs(plain - _mean_radiance(tris, mats, NONE, N, N))
    nee = _mean_radiance(tris, mats, None, 0, N)
    print("N", N, "plain", plain, "scale", scale, "light-sampled", nee, "difference", np.abs(nee - plain))
    assert np.allclose(scale, UNBIASED_SCALE, rtol=1e-4, atol=0), "the recorded scale is stale: %s" % scale
    assert (scale < 0.02 * plain).all(), scale / plain
    assert (np.abs(nee - plain) <= 3.0 * scale).all(), (np.abs(nee - plain), 3.0 * scale)
