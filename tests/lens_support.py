"""What tests/test_lens_cpu.py and tests/test_gpu_lens.py share: the two lens cameras, the scenes of the three searches, one render of
every estimator through the Python renderers with its sample workspace, and what the restatement (tests/lens_oracle.py) says of it.
TEST INFRASTRUCTURE (an ordinary module: every assert carries its message)."""
import collections

import numpy as np

import ao_oracle
import direct_oracle as do
import env_oracle
import indirect_oracle
import lens_oracle as lo
import mis_oracle
import power_oracle
import ris_oracle
import ris_scenes
import roulette_oracle
from env_scenes import env_map
from oclpathtracer_amd import scene
from oclpathtracer_amd.camera import Camera

REF_EYE, REF_CENTER = (0.0, 2.75, 4.0), (0.0, 2.75, 3.0)
OBLIQUE = dict(eye=(1.2, 3.4, 4.5), center=(-0.4, 2.2, -1.0), up=(0.1, 1.0, 0.05), fov_y_deg=50.0)


def reference_lens(R=0.05, F=6.0):
    """the reference's camera with a lens"""
    return Camera(REF_EYE, REF_CENTER, lens_radius=R, focus_distance=F)


def oblique_lens(R=0.1, F=5.0):
    """a camera whose holDir and upDir have three non-zero components each, with a lens"""
    c = Camera(lens_radius=R, focus_distance=F, **OBLIQUE)
    d = c.derive()
    assert np.all(d[6:12] != 0.0), "the oblique camera's basis has a zero component"
    return c


CAMERAS = {"reference": reference_lens, "oblique": oblique_lens}

# the three searches: (scene, PT_OPT_ACCEL) -- the table in LDS, the tiled table (brute force forced), the LBVH
SEARCH_SCENES = {
    "lds": (lambda: scene.load_model(), 1),
    "tiled": (ris_scenes.many_lights_tiled, 1),
    "lbvh": (ris_scenes.many_lights_lbvh, 0),
}

ENV_MAP = "sun"   # (tests/env_scenes.py)

# one estimator: the renderer's arguments and the restatement's call
Estimator = collections.namedtuple("Estimator", "name indirect kw")
K, B, M, KE = 2, 4, 4, 1
RR = (1, 0.95)
ESTIMATORS = [
    Estimator("direct", False, dict()),
    Estimator("direct_power", False, dict(light_choice="power")),
    Estimator("direct_ris", False, dict(light_choice="power", candidates=M)),
    Estimator("direct_env", False, dict(light_choice="power", env=True)),
    Estimator("indirect", True, dict()),
    Estimator("indirect_mis", True, dict(mis=True)),
    Estimator("indirect_power_mis", True, dict(mis=True, light_choice="power")),
    Estimator("indirect_rr", True, dict(roulette=RR)),
    Estimator("indirect_ris", True, dict(light_choice="power", candidates=M)),
    Estimator("indirect_env", True, dict(mis=True, light_choice="power", env=True)),
]
BY_NAME = {e.name: e for e in ESTIMATORS}


def env_texels():
    return env_map(ENV_MAP)


def gpu_render(device, tris, mats, est, cam, W, H, frames, *, frame_begin=0, fb_init=None, chunks=None, **stripes):
    """one renderer of estimator ``est``, one render (or one per entry of ``chunks``, frames each): (framebuffer [local pixels, 4], the
    workspace of the last call [its frames, local pixels, 3])"""
    from oclpathtracer_amd.direct import DirectRenderer
    from oclpathtracer_amd.environment import Environment
    from oclpathtracer_amd.indirect import IndirectRenderer, Roulette

    kw = dict(est.kw)
    kw.update(light_samples=K, camera=cam, chunk_frames=max(frames, 1), stripe_rows=1)
    kw.update(stripes)
    if kw.pop("env", False):
        kw.update(environment=Environment(env_texels()), env_samples=KE)
    if "roulette" in kw:
        kw["roulette"] = Roulette(*kw["roulette"])
    r = IndirectRenderer(device, tris, mats, W, H, max_bounces=B, **kw) if est.indirect else DirectRenderer(device, tris, mats, W, H, **kw)
    try:
        if fb_init is not None:
            r.fb.write(np.ascontiguousarray(fb_init, np.float32), r.local_pixels)
        last = frames
        if chunks is None:
            r.render(frames, frame_begin)
        else:
            at = frame_begin
            for n in chunks:
                r.render(n, at)
                at += n
            last = chunks[-1]
        fb = r.read()
        ws = np.zeros((r.chunk_frames, r.local_pixels, 3), np.float32)
        r.samples.read(ws, ws.size)
        device.waitForCompletion()
        return fb, ws[:last]
    finally:
        r.release()


def _oracle(tris, mats, est, cam, W, H, frame_begin, frames, start, **stripes):
    """the restatement's (framebuffer, samples [frames, local pixels, 3]) -- called inside a lens block"""
    gids = do.local_gids(W, H, **stripes)
    gid = np.tile(gids, frames).astype(np.int32)
    frame = np.repeat(np.arange(frame_begin, frame_begin + frames, dtype=np.int32), len(gids))
    kw = est.kw
    power, mis = kw.get("light_choice") == "power", bool(kw.get("mis"))
    R, cap = kw.get("roulette", (roulette_oracle.NEVER, 1.0))
    fr = dict(cam=cam, start=start, **stripes)
    if kw.get("env"):
        t = env_texels()
        b = B if est.indirect else None
        fb = env_oracle.render(tris, mats, t, W, H, frame_begin, frames, K, KE, B=b, **fr)
        ws = env_oracle.samples(tris, mats, t, W, H, gid, frame, K, KE, B=b, cam=cam)
    elif "candidates" in kw:
        b = B if est.indirect else None
        fb = ris_oracle.render(tris, mats, W, H, frame_begin, frames, K, M, B=b, mis=mis, **fr)
        ws = ris_oracle.samples(tris, mats, W, H, gid, frame, K, M, B=b, mis=mis, cam=cam)
        ws = ws[0] if isinstance(ws, tuple) else ws
    elif not est.indirect:
        if power:
            fb = power_oracle.render(power_oracle.DIRECT, tris, mats, W, H, frame_begin, frames, K, **fr)
            ws = power_oracle.samples(power_oracle.DIRECT, tris, mats, W, H, gid, frame, K, cam=cam)
            ws = ws[0] if isinstance(ws, tuple) else ws
        else:
            fb = do.render(tris, mats, W, H, frame_begin, frames, K, **fr)
            ws = do.decisions(tris, mats, W, H, gid, frame, K, cam=cam)[2]
    elif "roulette" in kw:
        fb = roulette_oracle.render(tris, mats, W, H, frame_begin, frames, K, B, R, cap, mis=mis, power=power, **fr)
        ws = roulette_oracle.samples(tris, mats, W, H, gid, frame, K, B, R, cap, mis=mis, power=power, cam=cam)[0]
    elif power:
        fb = power_oracle.render(power_oracle.MIS, tris, mats, W, H, frame_begin, frames, K, B, **fr)
        ws = power_oracle.samples(power_oracle.MIS, tris, mats, W, H, gid, frame, K, B, cam=cam)
        ws = ws[0] if isinstance(ws, tuple) else ws
    elif mis:
        fb = mis_oracle.render(tris, mats, W, H, frame_begin, frames, K, B, **fr)
        ws = mis_oracle.samples(tris, mats, W, H, gid, frame, K, B, cam=cam)
        ws = ws[0] if isinstance(ws, tuple) else ws
    else:
        fb = indirect_oracle.render(tris, mats, W, H, frame_begin, frames, K, B, **fr)
        ws = indirect_oracle.samples(tris, mats, W, H, gid, frame, K, B, cam=cam)
        ws = ws[0] if isinstance(ws, tuple) else ws
    assert fb is not None, "the restatement rejected the camera"
    return fb, np.asarray(ws, np.float32).reshape(frames, len(gids), 3)


def oracle_render(tris, mats, est, cam, W, H, frames, *, frame_begin=0, **stripes):
    """the restatement's (framebuffer after frames [0, frame_begin + frames), samples of the last ``frames`` frames, the framebuffer
    before them -- None at frame 0) with the camera's lens"""
    with lo.lens(*lo.lens_of(cam)):
        start = None
        if frame_begin > 0:
            start = _oracle(tris, mats, est, cam, W, H, 0, frame_begin, None, **stripes)[0]
        fb, ws = _oracle(tris, mats, est, cam, W, H, frame_begin, frames, start, **stripes)
    return fb, ws, start


def ao_counts(tris, cam, W, H, frame_begin, frames, Kao, radius, **stripes):
    """the restatement's {open, hits} per local pixel with the camera's lens"""
    with lo.lens(*lo.lens_of(cam)):
        return ao_oracle.counts(tris, W, H, frame_begin, frames, Kao, radius, cam=cam, **stripes)
