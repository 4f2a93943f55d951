"""Environment lighting on the device (pt_env_table, pt_render_direct_env, pt_render_indirect_env) against the restatement
(tests/env_oracle.c): the table, every case of tests/env_cases.py -- workspace before the fold and framebuffer, bit for bit, NaN
positions equal --, the three identities against the parents' own entry points in the same process, the Python renderers, and every
argument error through the raw C ABI with the framebuffer untouched."""
import ctypes

import numpy as np
import pytest

import env_cases as ec
import env_oracle as eo
from conftest import assert_fb_equal
from env_scenes import env_map, env_scene
from env_support import EnvBuffers, device_env_table, expect
from gpu_support import options
from oclpathtracer_amd import adl, shim

pytestmark = pytest.mark.gpu


def _random_map(N, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros((N, N, 4), np.float32)
    t[..., :3] = rng.uniform(0.0, 4.0, (N, N, 3)) ** 4
    flat = t.reshape(-1, 4)
    if N > 1:
        flat[rng.integers(1, N * N, max(1, N * N // 64)), :3] = 0.0   # texels that emit nothing (never the first: the total stays positive)
    return t


@pytest.mark.parametrize("N", [1, 2, 16, 64, 512, 2048])
def test_table_is_the_restatements(device, N):
    t = _random_map(N, N)
    rc, cdf = device_env_table(device, t)
    assert rc == shim.PT_OK
    want = eo.table(t)
    assert np.array_equal(cdf, want), "N = %d: cdf differs first at %s" % (N, np.flatnonzero(cdf != want)[:4])
    assert int(cdf[-1]) > 0


@pytest.mark.parametrize("name", ["sun", "zero:4", "bad:16", "gradient:1"])
def test_table_of_the_named_maps(device, name):
    rc, cdf = device_env_table(device, env_map(name))
    assert rc == shim.PT_OK
    assert np.array_equal(cdf, eo.table(env_map(name))), name


def _compare(b, c, what, **stripes):
    want_ws, want_fb, start = expect(c, **stripes)
    fb0 = None
    if len(start):
        fb0 = b.sentinel.copy()
        fb0[:len(start)] = start
    rc, fb, ws = b.render(c, fb_init=fb0, **stripes)
    assert rc == shim.PT_OK, "%s: %s" % (what, b.lib.pt_last_error())
    n = len(want_fb)
    held = min(c.frames, c.chunk or c.frames)   # the workspace holds the frames of the last chunk
    last = want_ws[c.frames - (c.frames - 1) % held - 1:] if held < c.frames else want_ws
    assert_fb_equal(ws[:last.size], last, what + ": radiance before the fold")
    assert np.array_equal(ws[held * n * 3:], b.ws_sentinel[held * n * 3:]), what + ": the workspace behind the launch's records was written"
    assert_fb_equal(fb[:n], want_fb, what + ": framebuffer")
    assert np.array_equal(fb[n:], b.sentinel[n:]), what + ": the framebuffer behind the image was written"


@pytest.mark.parametrize("c", ec.CASES, ids=[c.id for c in ec.CASES])
def test_case_is_the_restatements(device, c):
    b = EnvBuffers(device, c.scene, c.map, c.W, c.H, frames=c.chunk or c.frames)
    try:
        if c.stripes is None:
            _compare(b, c, c.id)
        else:
            rows, ranks = c.stripes
            for rank in range(ranks):
                _compare(b, c, "%s rank %d" % (c.id, rank), stripe_rows=rows, n_ranks=ranks, rank=rank)
    finally:
        b.release()


IDENTITY_SCENES = [("open_panel", (1, 0)), ("open_panel", (0, 1)), ("many_tiled_open", (1, 0)), ("many_open", (1, 0)), ("many_open", (0, 0)), ("open", (1, 2))]


@pytest.mark.parametrize("scene,search", IDENTITY_SCENES)
@pytest.mark.parametrize("N", [1, 64])
def test_grey_map_without_samples_is_the_parent(device, scene, search, N):
    """every texel (0.45, 0.45, 0.45) and Ke = 0: pt_render_direct_power's and pt_render_indirect_rr's workspace and framebuffer, with and
    without roulette, from the parents' own entry points in the same process"""
    W, H = 24, 10
    b = EnvBuffers(device, scene, "grey:%d" % N, W, H, frames=2)
    try:
        for B, R, cap in ((None, ec.NEVER, 1.0), (5, ec.NEVER, 1.0), (8, 1, 0.95)):
            c = ec.case("identity", scene, "grey:%d" % N, W, H, 2, K=2, Ke=0, B=B, R=R, cap=cap, search=search)
            rc, fb, ws = b.render(c)
            prc, pfb, pws = b.render(c, parent=True)
            assert rc == shim.PT_OK and prc == shim.PT_OK, b.lib.pt_last_error()
            what = "%s N %d B %s R %d" % (scene, N, B, R)
            assert_fb_equal(ws, pws, what + ": workspace")
            assert_fb_equal(fb, pfb, what + ": framebuffer")
            assert not np.array_equal(fb, b.sentinel), what + ": nothing was rendered"
    finally:
        b.release()


@pytest.mark.parametrize("scene,map,search", [("open_panel", "sun", (1, 0)), ("many_open", "gradient:16", (1, 0)), ("many_tiled_open", "sun", (0, 0))])
def test_one_bounce_is_direct(device, scene, map, search):
    W, H = 24, 10
    b = EnvBuffers(device, scene, map, W, H, frames=2)
    try:
        d = ec.case("direct", scene, map, W, H, 2, K=2, Ke=3, search=search)
        rc, fb, ws = b.render(d)
        irc, ifb, iws = b.render(d._replace(B=1))
        assert rc == shim.PT_OK and irc == shim.PT_OK, b.lib.pt_last_error()
        assert_fb_equal(iws, ws, "workspace")
        assert_fb_equal(ifb, fb, "framebuffer")
    finally:
        b.release()


def test_no_triangles_show_the_map(device):
    """num_triangles == 0: every sample is the texel of its primary ray"""
    W, H = 16, 16
    t = env_map("gradient:16")
    b = EnvBuffers(device, "empty", "gradient:16", W, H, frames=1)
    try:
        for B in (None, 4):
            c = ec.case("empty", "empty", "gradient:16", W, H, 1, Ke=1, B=B)
            rc, fb, ws = b.render(c)
            assert rc == shim.PT_OK, b.lib.pt_last_error()
            got = ws.reshape(W * H, 3)
            flat = t.reshape(-1, 4)[:, :3]
            rows = (got[:, None, :] == flat[None, :, :]).all(-1)
            assert rows.any(1).all(), "a sample is no texel of the map"
            assert len(np.unique(rows.argmax(1))) > 8, "the camera sees more than a few texels"
    finally:
        b.release()


def _renderer_case(device, cls_kw, scene, map, W, H, frames, K, Ke, B, R, cap):
    from oclpathtracer_amd.direct import DirectRenderer
    from oclpathtracer_amd.environment import Environment
    from oclpathtracer_amd.indirect import IndirectRenderer, Roulette

    tris, mats, lights, cam = env_scene(scene)
    env = Environment(env_map(map))
    kw = dict(light_samples=K, lights=lights, camera=cam, chunk_frames=frames, stripe_rows=1, light_choice="power", environment=env,
              env_samples=Ke, **cls_kw)
    r = DirectRenderer(device, tris, mats, W, H, **kw) if B is None else \
        IndirectRenderer(device, tris, mats, W, H, max_bounces=B, mis=True, roulette=None if R == ec.NEVER else Roulette(R, cap), **kw)
    return r, env


def test_python_renderers(device):
    """DirectRenderer / IndirectRenderer with environment= and env_samples= make the restatement's image; moments work as they do
    without; set_environment starts again at frame 0"""
    W, H, frames = 24, 10, 3
    for B, R, cap in ((None, ec.NEVER, 1.0), (4, ec.NEVER, 1.0), (6, 2, 0.95)):
        c = ec.case("py", "open_panel", "sun", W, H, frames, K=1, Ke=2, B=B, R=R, cap=cap)
        want_ws, want_fb, _ = expect(c)
        r, env = _renderer_case(device, dict(moments=True), c.scene, c.map, W, H, frames, c.K, c.Ke, B, R, cap)
        try:
            r.render(frames)
            assert_fb_equal(r.read(), want_fb, "framebuffer B %s" % B)
            var, n = r.variance()
            fin = np.isfinite(want_ws).all(-1)
            assert np.array_equal(n, fin.sum(0).astype(np.uint32)), "the moments count the finite samples"
            w64 = np.where(fin[..., None], want_ws.astype(np.float64), 0.0)
            nn = np.maximum(fin.sum(0), 2)[:, None]
            v = (np.square(w64).sum(0) - w64.sum(0) ** 2 / nn) / (nn - 1)
            assert np.allclose(var[n >= 2], v[n >= 2], rtol=1e-5, atol=1e-9), "variance()"
            assert r.noise().samples == int(fin.sum())
            grey = type(env).constant(0.45, size=4)
            r.set_environment(grey, 0)
            assert r.frames_done == 0
            r.render(1)
            c0 = c._replace(map="grey:4", Ke=0, frames=1)
            assert_fb_equal(r.read(), expect(c0)[1], "after set_environment B %s" % B)
            grey.release()
        finally:
            r.release()
            env.release()


def test_renderer_pass_through(device):
    from oclpathtracer_amd.environment import Environment
    from oclpathtracer_amd.render import Renderer

    tris, mats, lights, cam = env_scene("open_panel")
    env = Environment(env_map("sun"))
    base = Renderer(device, np.array(tris), np.array(mats), 24, 10, stripe_rows=1)
    try:
        for make, B in ((base.direct_renderer, None), (base.indirect_renderer, 4)):
            kw = dict(light_choice="power", environment=env, env_samples=1, chunk_frames=2)
            r = make(**kw) if B is None else make(max_bounces=B, mis=True, **kw)
            try:
                r.render(2)
                c = ec.case("pass", "open_panel", "sun", 24, 10, 2, K=1, Ke=1, B=B)
                assert_fb_equal(r.read(), expect(c)[1], "pass-through B %s" % B)
            finally:
                r.release()
    finally:
        base.release()
        env.release()


def test_renderer_refuses_adaptive_passes_under_an_environment(device):
    r, env = _renderer_case(device, dict(moments=True), "open_panel", "sun", 8, 8, 1, 1, 1, 4, ec.NEVER, 1.0)
    try:
        with pytest.raises(ValueError):
            r.render_adaptive(0.1, max_samples=8)
        with pytest.raises(ValueError):
            r.set_candidates(4)
    finally:
        r.release()
        env.release()


@pytest.mark.parametrize("only,flags,tail,K,B", [("DirectIllumination", (), "_power_envsun.ppm", 4, None),
                                                 ("IndirectIllumination", ("--mis",), "_mis_power_envsun.ppm", 1, 16)])
def test_cpp_harness_env(tmp_path, only, flags, tail, K, B):
    """raytrace_test --lights power --env sun,2 on the Cornell box: the restatement's image under the sun map"""
    from gpu_support import harness_ppm
    from oclpathtracer_amd import scene

    tris, mats = scene.load_model()
    dim, frames = 24, 3
    out, name, pixels = harness_ppm(tmp_path, dim, frames, only, *flags, "--lights", "power", "--env", "sun,2")
    assert name.endswith(tail), name
    assert "(sun sky, 2 environment samples)" in out
    want = eo.render(tris, mats, env_map("sun"), dim, dim, 0, frames, K, 2, B=B)
    assert np.array_equal(pixels, scene.f2c(want[:, :3]))


def test_argument_errors_leave_the_framebuffer_untouched(device):
    """every argument error the two entry points add, through the raw C ABI, each with its code"""
    E_INV, E_RANGE = shim.PT_ERR_INVALID, shim.PT_ERR_RANGE
    W, H = 32, 8   # (the framebuffer and the workspace are large enough to stand in for the map and the table)
    b = EnvBuffers(device, "open_panel", "gradient:16", W, H)
    other = adl.DeviceUtils.allocate(adl.TYPE_HIP, adl.Config(0))
    oe = adl.Buffer(other, b.N * b.N, adl.float4)
    small_e = adl.Buffer(device, b.N * b.N - 1, adl.float4)
    small_c = adl.Buffer(device, b.N * b.N, np.uint64)
    big = adl.Buffer(device, 1 << 16, np.uint8)

    wraps = []

    def wrap(off, nbytes, base=big):
        w = adl.Buffer()
        w.setRawPtr(device, base.m_ptr + off, nbytes)
        wraps.append(w)
        return w
    mis_e, mis_c = wrap(8, b.N * b.N * 16), wrap(4, (b.N * b.N + 1) * 8)
    on_fb = wrap(0, 16 * W * H, base=b.fb)          # the map lying where the framebuffer lies
    on_ws = wrap(0, (b.N * b.N + 1) * 8, base=b.sb)   # the table lying where the workspace lies
    try:
        for form in ("direct", "indirect"):
            def call(env="default", **over):
                if form == "direct":
                    return b.direct(b.direct_params(b.nl), env=env, cam=b.cam, **over)
                return b.indirect(b.params(b.nl), env=env, cam=b.cam, **over)
            assert call(env=None) == E_INV, form
            for size in (0, -1, 3, 24, 4096, 1 << 30):
                assert call(env=b.environment(size=size)) == E_INV, (form, size)
            for ke in (-1, 257):
                assert call(env=b.environment(Ke=ke)) == E_INV, (form, ke)
            for k in (0, 1):
                assert call(env=b.environment(reserved=k)) == E_INV, (form, k)
            assert call(eb=None) == E_INV, form
            assert call(ec=None) == E_INV, form                          # Ke > 0 needs the table
            assert call(eb=mis_e) == E_INV and call(ec=mis_c) == E_INV, form   # misaligned
            assert call(eb=on_fb) == E_INV and call(ec=on_ws) == E_INV, form   # overlapping what the call writes
            assert call(eb=oe) == E_INV, form                            # a buffer of another device
            assert call(eb=small_e) == E_RANGE and call(ec=small_c) == E_RANGE, form
            assert call(env=b.environment(size=32)) == E_RANGE, form      # a larger map than the buffers hold
            b.assert_untouched()
            assert call(env=b.environment(Ke=0), ec=None) == shim.PT_OK, form   # the table is not read when Ke = 0
            b.reset()
        if True:   # the parents' own checks are made as the parents make them
            assert b.indirect(b.params(b.nl), rr=None, cam=b.cam) == E_INV
            assert b.indirect(b.params(b.nl), rr=b.roulette(0, 0.5), cam=b.cam) == E_INV
            assert b.indirect(b.params(b.nl, max_bounces=0), cam=b.cam) == E_INV
            assert b.direct(b.direct_params(b.nl, reserved=2), cam=b.cam) == E_INV
            assert b.direct(b.direct_params(b.nl), lb=None, cam=b.cam) == E_INV     # num_lights > 0 needs the list
            assert b.direct(b.direct_params(b.nl), qb=None, cam=b.cam) == E_INV     # and the light table
        b.assert_untouched()
        # pt_env_table's own
        lib = b.lib
        assert lib.pt_env_table_bytes(16) == 8 * (16 * 16 + 2 + 1) and lib.pt_env_table_bytes(3) == 0 and lib.pt_env_table_bytes(4096) == 0
        assert lib.pt_env_table(device._h, None, b.N, b.ec._h, None) == E_INV
        assert lib.pt_env_table(device._h, b.eb._h, b.N, None, None) == E_INV
        assert lib.pt_env_table(device._h, b.eb._h, 12, b.ec._h, None) == E_INV
        assert lib.pt_env_table(device._h, b.eb._h, 32, b.ec._h, None) == E_RANGE
        assert lib.pt_env_table(device._h, b.eb._h, b.N, small_c._h, None) == E_RANGE
        assert lib.pt_env_table(device._h, mis_e._h, b.N, b.ec._h, None) == E_INV
        assert lib.pt_env_table(device._h, oe._h, b.N, b.ec._h, None) == E_INV
        whole = wrap(0, 1 << 16)
        assert lib.pt_env_table(device._h, whole._h, b.N, wrap(16, (b.N * b.N + 8) * 8)._h, None) == E_INV   # overlapping
    finally:
        for w in wraps + [oe, small_e, small_c, big]:
            w.release()
        adl.DeviceUtils.deallocate(other)
        b.release()
