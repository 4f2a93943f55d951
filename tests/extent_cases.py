"""The inputs of tests/test_gpu_extents.py and tests/test_gpu_extents_lists.py -- images and frame numbers at the ends of what the C ABI
accepts -- and what the CPU oracle says of them: one table, so that tests/test_extents_cpu.py proves on exactly the geometries the
device renders that each reaches the corner it is rendered for.  TEST INFRASTRUCTURE.

  TALL   64 x (2^25 - 1): W * H = 2 147 483 584, the last multiple of 64 the ABI accepts.  A rank of a striped render owns a few rows
         however tall the image is: the layouts below have 448 .. 1 984 local pixels, whose global rows, gids and seeds use all 31 bits.
  WIDE   (2^24 + 256) x 127, one row of it: the columns about the image's centre, where the box is, lie at and above 2^23, where
         binary32 has spacing 1 and a jittered x is a neighbouring column's.
  LATE   the Cornell box at 24 x 16 resumed at frame numbers about 2048 (the fold's reciprocal table ends), 2^24 (the float of a
         frame number and of its predecessor coincide) and 2^31 - 1 (the last frame the ABI accepts).
  EMPTY  a rank that owns no row.

Rendered at them: the fused renderer, the lit estimators of LIT (direct, indirect, MIS / power / roulette, RIS, the environment, the
thin lens), ambient occlusion, the features, pt_camera_rays, and the pixel lists (pt_render_indirect_pixels, its RIS form, their fold
and pt_sample_moments_pixels) -- a list renders listed pixels only, which makes WIDE affordable for a lit kernel."""
from __future__ import annotations

import collections
import contextlib

import numpy as np

import ao_oracle
import direct_oracle as do
import env_oracle
import extent_oracle as eo
import feature_oracle as fo
import indirect_oracle as io
import lens_oracle
import moments_oracle as mom
import power_oracle as po
import ris_oracle
import roulette_oracle as ro
from env_scenes import env_map, env_scene
from oclpathtracer_amd.camera import Camera
from scenes import edge_scene

# ---- TALL -------------------------------------------------------------------------------------------------------------------------
TALL_W, TALL_H = 64, 2 ** 25 - 1
TALL_FRAMES = 3
# name -> the stripe layout.  "last_pixel": rows rank + k 2^22, k = 0 .. 7 -- 8 rows, the last one the image's last;  "ragged": k = 7
# would be row 2^25 - 1 = H, 7 rows;  "stripes_of_3": the image's last row, 2^25 - 2 = 3 * 11 184 810, begins stripe 11 184 810 =
# 10 * 2^20 + 699 050 -- ten whole stripes and a stripe of one row, 31 rows
TALL = {
    "last_pixel": dict(stripe_rows=1, n_ranks=2 ** 22, rank=2 ** 22 - 2),
    "ragged": dict(stripe_rows=1, n_ranks=2 ** 22, rank=2 ** 22 - 1),
    "stripes_of_3": dict(stripe_rows=3, n_ranks=2 ** 20, rank=699050),
}
TALL_ROWS = {"last_pixel": 8, "ragged": 7, "stripes_of_3": 31}

# ---- WIDE -------------------------------------------------------------------------------------------------------------------------
WIDE_W, WIDE_H = 2 ** 24 + 256, 127
WIDE_STRIPES = dict(stripe_rows=1, n_ranks=127, rank=40)   # one local row, global row 40
WIDE_ROW = 40
WIDE_FRAMES = 8
WIDE_MASK_FRAMES = 32                                       # the masks' superset is checked over frames 0 .. 31

# ---- LATE -------------------------------------------------------------------------------------------------------------------------
LATE_W, LATE_H = 24, 16
LATE = {"table_end": (2046, 5), "float_ties": (2 ** 24 - 2, 5), "last_frames": (2 ** 31 - 4, 3)}   # name -> (frame_begin, frames)

# ---- EMPTY ------------------------------------------------------------------------------------------------------------------------
EMPTY_W, EMPTY_H = 7, 5
EMPTY_STRIPES = dict(stripe_rows=4, n_ranks=3, rank=2)

# ---- the lit estimators -----------------------------------------------------------------------------------------------------------
# name -> Est: max_bounces (None: direct), mis, power, roulette (R, cap) or None, M candidates (0: no resampling), Ke environment samples
# (0: no environment) and whether the camera has the lens LENS.  K = 1 and B = 6 throughout; the map is env_scenes' "sun".
# The scene is the Cornell box, the reference's camera inside it.  Its environment samples do contribute and its later BRDF rays do leave
# it (the box has no front wall: test_extents_cpu.py's Env proof), so on LATE the env entries stay on it.  No PRIMARY ray of a TALL layout
# leaves it though (64 columns about the image's centre line see floor, back wall and ceiling only), and a proof asks every new estimator
# and the features for local pixels that hit and local pixels that miss: on TALL the entries added after the first three (the env ones
# too), the features, the lists and the lens AO render are rendered on TALL_SCENE, env_scenes' open_panel -- the same room without its
# ceiling, the panel kept --, whose upper rows look at the sky.  LATE renders them on the Cornell box.
Est = collections.namedtuple("Est", "B mis power rr M Ke lens", defaults=(0, 0, False))
LIT_K, LIT_B, LIT_M, LIT_KE = 1, 6, 8, 3
LIT = {"direct": Est(None, False, False, None), "indirect": Est(LIT_B, False, False, None), "mis_power_rr": Est(LIT_B, True, True, (1, 0.5)),
       "ris_direct": Est(None, False, True, None, M=LIT_M), "ris_indirect": Est(LIT_B, True, True, (1, 0.5), M=LIT_M),
       "env_direct": Est(None, False, True, None, Ke=LIT_KE), "env_indirect": Est(LIT_B, True, True, (1, 0.5), Ke=LIT_KE),
       "lens_direct_power": Est(None, False, True, None, lens=True), "lens_indirect_rr": Est(LIT_B, False, False, (1, 0.5), lens=True)}
LIT_OLD = ("direct", "indirect", "mis_power_rr")   # what existed before: on the Cornell box everywhere
LIT_NEW = tuple(k for k in LIT if k not in LIT_OLD)
LIT_FRAMES = 2     # of a TALL lit render
ENV_MAP = "sun"
LENS = (0.05, 4.0)   # lens_radius, focus_distance: the back wall's distance is about 6.8, so nothing the camera sees is in focus
TALL_SCENE = "open_panel"
LIST_EST = "mis_power_rr"   # the estimator of the pixel lists: pt_render_indirect_pixels with MIS, by power, roulette (1, 0.5)
FEATURE_FRAMES = 2
AO_RADIUS, AO_K = 1.5, 2

# (H, stripe_rows, n_ranks, rank) of the layouts tests elsewhere in the suite render or restate (the closed forms of direct_oracle
# must give what the walk over the rows gave)
EXISTING_LAYOUTS = [(16, 1, 1, 0), (24, 1, 1, 0), (64, 16, 1, 0), (31, 5, 1, 0), (31, 5, 3, 0), (31, 5, 3, 1), (31, 5, 3, 2),
                    (16, 3, 3, 0), (16, 3, 3, 1), (16, 3, 3, 2), (30, 4, 3, 1), (48, 8, 4, 1), (33, 4, 2, 0), (33, 4, 2, 1),
                    (24, 16, 3, 1), (8, 4, 8, 3), (64, 16, 2, 1), (40, 16, 8, 2), (40, 16, 8, 3), (47, 5, 3, 0), (5, 4, 3, 2)]


def cornell():
    """(tris, mats, lights, None): the Cornell box, the reference's camera"""
    return edge_scene("cornell")[1]


def tall_gids(name):
    return do.local_gids(TALL_W, TALL_H, **TALL[name])


def wide_columns():
    """the columns of the WIDE row that are read back and compared, as (name, first column, count) blocks and one array of 4 096
    single columns drawn once with a fixed seed: the window about the image's centre (where the box is), both ends of the row, and
    columns all over it"""
    blocks = [("window", WIDE_W // 2 - 128, 257), ("first", 0, 64), ("last", WIDE_W - 64, 64)]
    scattered = np.sort(np.random.default_rng(20261019).choice(WIDE_W, 4096, replace=False)).astype(np.int64)
    return blocks, scattered


def wide_gids(cols):
    return WIDE_ROW * WIDE_W + np.asarray(cols, np.int64)


def window_columns():
    _, first, n = wide_columns()[0][0]
    return np.arange(first, first + n, dtype=np.int64)


def late_start(channels=4):
    """a framebuffer of arbitrary finite values in [0, 1] to resume from, float32 [pixels, 4]"""
    return np.random.default_rng(2048).uniform(0.0, 1.0, (LATE_W * LATE_H, channels)).astype(np.float32)


# ---- what the oracles say: computed once, shared, read-only ---------------------------------------------------------------------
def _fused_window(W, H, frames, frame_begin, depth, gid_key, start_key):
    tris, mats = cornell()[:2]
    gid = _GIDS[gid_key]()
    start = late_start() if start_key else None
    px, st = eo.render_window(tris, mats, W, H, frames, gid, frame_begin=frame_begin, max_bounces=depth, start=start)
    return px, np.array([st["rays"], st["samples"]], np.uint64)


def _wide_all():
    blocks, scattered = wide_columns()
    return wide_gids(np.concatenate([np.arange(f, f + n) for _, f, n in blocks] + [scattered]))


_GIDS = {("tall", name): (lambda name=name: tall_gids(name)) for name in TALL}
_GIDS["late"] = lambda: np.arange(LATE_W * LATE_H)
_GIDS["wide"] = _wide_all


def fused_tall(name):
    """(pixels [local pixels, 4], [rays, samples]) of TALL_FRAMES frames of a TALL layout"""
    return do.once(_fused_window, TALL_W, TALL_H, TALL_FRAMES, 0, 16, ("tall", name), False)


def fused_late(name):
    fb, n = LATE[name]
    return do.once(_fused_window, LATE_W, LATE_H, n, fb, 16, "late", True)


def fused_wide():
    """the pixels of wide_columns(), blocks first and in their order, then the scattered columns"""
    return do.once(_fused_window, WIDE_W, WIDE_H, WIDE_FRAMES, 0, 16, "wide", False)


# ---- the lit estimators ---------------------------------------------------------------------------------------------------------
def lens_camera():
    """the reference's camera with the lens LENS"""
    return Camera((0.0, 2.75, 4.0), (0.0, 2.75, 3.0), lens_radius=LENS[0], focus_distance=LENS[1])


def scene_of(est, tall):
    """(tris, mats, lights or None, camera or None) an estimator is rendered on (the table's comment)"""
    sc = env_scene(TALL_SCENE) if tall and est in LIT_NEW else cornell()
    return sc[0], sc[1], sc[2], (lens_camera() if LIT[est].lens else sc[3])


def _lens_of(e):
    return lens_oracle.lens(*LENS) if e.lens else contextlib.nullcontext()


def lit_samples(est, scene4, W, H, gid, frame, details=False):
    """the restatement's radiance before the fold float32 [n, 3] of the samples (gid[i], frame[i]); with ``details`` (RIS and env only)
    (radiance, the restatement's account of them)"""
    tris, mats, lights, cam = scene4
    e = LIT[est]
    R, cap = e.rr if e.rr is not None else (ro.NEVER, 1.0)
    gid, frame = np.asarray(gid, np.int64), np.asarray(frame, np.int64)
    assert 0 <= gid.min() and gid.max() < 2 ** 31 and 0 <= frame.min() and frame.max() < 2 ** 31
    with _lens_of(e):
        if e.M:
            return ris_oracle.samples(tris, mats, W, H, gid, frame, LIT_K, e.M, B=e.B, R=R, cap=cap, mis=e.mis, lights=lights, cam=cam,
                                      details=details)
        if e.Ke:
            return env_oracle.samples(tris, mats, env_map(ENV_MAP), W, H, gid, frame, LIT_K, e.Ke, B=e.B, R=R, cap=cap, lights=lights, cam=cam,
                                      details=details)
        assert not details
        if e.B is None and e.power:
            return po.samples(po.DIRECT, tris, mats, W, H, gid, frame, LIT_K, lights=lights, cam=cam)
        if e.B is None:
            return do.decisions(tris, mats, W, H, gid, frame, LIT_K, lights=lights, cam=cam)[2]
        if e.rr is None:
            return io.samples(tris, mats, W, H, gid, frame, LIT_K, e.B, lights=lights, cam=cam)[0]
        return ro.samples(tris, mats, W, H, gid, frame, LIT_K, e.B, R, cap, mis=e.mis, power=e.power, lights=lights, cam=cam)[0]


def lit_render(est, scene4, W, H, frame_begin, frames, start=None, **stripes):
    """the restatement's framebuffer float32 [local pixels, 4] of frames [frame_begin, frame_begin + frames) folded into ``start``"""
    tris, mats, lights, cam = scene4
    e = LIT[est]
    R, cap = e.rr if e.rr is not None else (ro.NEVER, 1.0)
    kw = dict(lights=lights, cam=cam, start=start, **stripes)
    with _lens_of(e):
        if e.M:
            fb = ris_oracle.render(tris, mats, W, H, frame_begin, frames, LIT_K, e.M, B=e.B, R=R, cap=cap, mis=e.mis, **kw)
        elif e.Ke:
            fb = env_oracle.render(tris, mats, env_map(ENV_MAP), W, H, frame_begin, frames, LIT_K, e.Ke, B=e.B, R=R, cap=cap, **kw)
        elif e.B is None and e.power:
            fb = po.render(po.DIRECT, tris, mats, W, H, frame_begin, frames, LIT_K, **kw)
        elif e.B is None:
            fb = do.render(tris, mats, W, H, frame_begin, frames, LIT_K, **kw)
        elif e.rr is None:
            fb = io.render(tris, mats, W, H, frame_begin, frames, LIT_K, e.B, **kw)
        else:
            fb = ro.render(tris, mats, W, H, frame_begin, frames, LIT_K, e.B, R, cap, mis=e.mis, power=e.power, **kw)
    assert fb is not None, "the restatement rejected the camera"
    return fb


def _lit(est, W, H, frames, frame_begin, late, **stripes):
    sc = scene_of(est, tall=not late)
    gid, frame = do.sample_ids(W, H, frames, **stripes)
    fb = lit_render(est, sc, W, H, frame_begin, frames, late_start() if late else None, **stripes)
    return fb, lit_samples(est, sc, W, H, gid, frame + frame_begin).reshape(frames, -1, 3)


def lit_tall(est, name):
    """the restatement's (framebuffer [local pixels, 4], radiance [frames, local pixels, 3]) of a lit estimator on a TALL layout"""
    return do.once(_lit, est, TALL_W, TALL_H, LIT_FRAMES, 0, False, **TALL[name])


def lit_late(est, name):
    fb, n = LATE[name]
    return do.once(_lit, est, LATE_W, LATE_H, n, fb, True)


# ---- the fold, per pixel ------------------------------------------------------------------------------------------------------
GAMMA = np.float32(2.2)


def fold(px, rad, z):
    """the renderer's fold (oracle/pt_oracle.c, ptor_sample_pixel's accumulation) of the radiance ``rad`` float32 [n, 3] into the pixels
    ``px`` float32 [n, 4], pixel i with the frame number z[i] -- any integer, as the float conversions of z - 1 and z see it; 0 overwrites
    the pixel.  numpy rounds each binary32 operation on its own; the power is the oracle's.  test_extents_cpu.py pins it to the uniform
    restatements' own fold."""
    from oracle import ptoracle

    px, rad = np.asarray(px, np.float32), np.asarray(rad, np.float32)
    z = np.broadcast_to(np.asarray(z, np.int64), (len(px),))
    inv_gamma = np.float32(1.0) / GAMMA
    zm1, zf = (z - 1).astype(np.float32)[:, None], z.astype(np.float32)[:, None]
    old = ptoracle.pow_array(px[:, :3], float(GAMMA)).reshape(-1, 3)
    with np.errstate(all="ignore"):
        mean = np.where((z == 0)[:, None], rad, (old * zm1 + rad) / zf).astype(np.float32)
    out = np.ones((len(px), 4), np.float32)
    out[:, :3] = ptoracle.pow_array(mean, float(inv_gamma)).reshape(-1, 3)
    return out


def fold_frames(px, rad, first, wrap=True):
    """``fold`` of rad[f] float32 [F, n, 3], f ascending, pixel i with the frame numbers first[i] + f -- taken & 0x7fffffff as
    pt_render_indirect_pixels takes them (include/pt_shim.h), or with ``wrap`` False as the integers they are"""
    px = np.asarray(px, np.float32)
    for f in range(len(rad)):
        z = np.asarray(first, np.int64) + f
        px = fold(px, rad[f], z & 0x7fffffff if wrap else z)
    return px


# ---- pixel lists ----------------------------------------------------------------------------------------------------------------
# the two list entry points: the estimator whose samples a listed pixel receives
LIST_FORMS = {"pixels": LIST_EST, "pixels_ris": "ris_indirect"}
TALL_LIST_LAYOUTS = ("last_pixel", "stripes_of_3")
TALL_LIST_FRAME, TALL_LIST_FRAMES = 2, 2

# LATE lists, all 384 pixels listed: name -> (the slots' frame numbers, frames per slot).  "wrap": the frame numbers are 2^31 - 2,
# 2^31 - 1, 0, 1, and frame 0 overwrites the pixel (pt_shim.h); "mixed": neighbouring lanes of a wave on either side of the reciprocal
# table's end (2046 .. 2049) and of the wrap
_ALTERNATING = np.where(np.arange(LATE_W * LATE_H) % 2 == 0, 2046, 2 ** 31 - 2).astype(np.int64)
LATE_LISTS = {"float_ties": (np.full(LATE_W * LATE_H, 2 ** 24 - 2, np.int64), 5),
              "wrap": (np.full(LATE_W * LATE_H, 2 ** 31 - 2, np.int64), 4),
              "mixed": (_ALTERNATING, 4)}
LATE_LIST_OFFSETS = {"float_ties": (0,), "wrap": (0, 1), "mixed": (0, 1)}   # params->frame_begin, the slots' frames that much lower


def list_frames(first, frames):
    """int64 [frames, listed]: the frame number of item (f, j) -- (slot.frame + frame_begin + f) & 0x7fffffff"""
    return (np.asarray(first, np.int64)[None, :] + np.arange(frames, dtype=np.int64)[:, None]) & 0x7fffffff


def list_samples(form, scene4, W, H, gids, first, frames):
    """float32 [frames, listed, 3]: the workspace of a list render whose slot j is the pixel of global id gids[j] at frame first[j]"""
    z = list_frames(first, frames)
    return lit_samples(LIST_FORMS[form], scene4, W, H, np.tile(gids, frames), z.reshape(-1)).reshape(frames, len(gids), 3)


def tall_list_pixels(name):
    """every third local pixel and the image's last"""
    n = TALL_ROWS[name] * TALL_W
    return np.unique(np.concatenate([np.arange(0, n, 3), [n - 1]])).astype(np.int64)


def _list_tall(form, **stripes):
    sc = scene_of("ris_indirect", tall=True)   # (TALL_SCENE, the reference's camera)
    gids = do.local_gids(TALL_W, TALL_H, **stripes)
    px = np.unique(np.concatenate([np.arange(0, len(gids), 3), [len(gids) - 1]])).astype(np.int64)
    g, f = do.sample_ids(TALL_W, TALL_H, TALL_LIST_FRAME, **stripes)
    rad0 = lit_samples(LIST_EST, sc, TALL_W, TALL_H, g, f).reshape(TALL_LIST_FRAME, -1, 3)
    fb0 = lit_render(LIST_EST, sc, TALL_W, TALL_H, 0, TALL_LIST_FRAME, **stripes)
    m0 = mom.accumulate(rad0)
    ws = list_samples(form, sc, TALL_W, TALL_H, gids[px], np.full(len(px), TALL_LIST_FRAME), TALL_LIST_FRAMES)
    # THE IDENTITY: the uniform restatement's frames 2, 3 folded into its frames 0, 1 at the listed pixels, frames 0, 1 alone elsewhere
    fb1 = fb0.copy()
    fb1[px] = lit_render(LIST_FORMS[form], sc, TALL_W, TALL_H, TALL_LIST_FRAME, TALL_LIST_FRAMES, start=fb0, **stripes)[px]
    m1 = m0.copy()
    m1[px] = mom.accumulate(ws, m0[px])
    return fb0, rad0, m0.view(np.uint8), ws, fb1, m1.view(np.uint8)


def list_tall(form, name):
    """(framebuffer and radiance of the uniform start, its moments as bytes, the list render's workspace [frames, listed, 3], the
    framebuffer and the moments after it) of the TALL list case of a layout"""
    return do.once(_list_tall, form, **TALL[name])


def _list_late(form, case):
    sc = scene_of(LIST_FORMS[form], tall=False)
    first, frames = LATE_LISTS[case]
    ws = list_samples(form, sc, LATE_W, LATE_H, np.arange(LATE_W * LATE_H), first, frames)
    return ws, fold_frames(late_start(), ws, first), mom.accumulate(ws, late_moments()).view(np.uint8)


def list_late(form, case):
    """(workspace [frames, 384, 3], framebuffer, moments as bytes) of a LATE list case, the framebuffer resumed from late_start() and the
    moments from late_moments()"""
    return do.once(_list_late, form, case)


def late_moments():
    """records of arbitrary sums to go on from"""
    rng = np.random.default_rng(56)
    return mom.accumulate(rng.uniform(0.0, 2.0, (3, LATE_W * LATE_H, 3)).astype(np.float32))


# ---- WIDE, through a list ---------------------------------------------------------------------------------------------------------
WIDE_LIST_FRAMES, WIDE_LIST_SCATTERED = 4, 512


def wide_list_columns():
    """the listed columns of the WIDE row, ascending: the three blocks of wide_columns() and every 8th of its scattered columns that
    lies in none of them nor next to one (the two columns on either side of a block hold sentinels)"""
    blocks, scattered = wide_columns()
    far = np.ones(len(scattered), bool)
    for _, first, n in blocks:
        far &= (scattered < first - 2) | (scattered >= first + n + 2)
    some = scattered[far][::8][:WIDE_LIST_SCATTERED]
    assert len(some) == WIDE_LIST_SCATTERED
    return np.unique(np.concatenate([np.arange(f, f + n) for _, f, n in blocks] + [some])).astype(np.int64)


def wide_sentinel_columns():
    """the two columns on either side of each block that the image has"""
    out = []
    for _, first, n in wide_columns()[0]:
        out += [c for c in (first - 2, first - 1, first + n, first + n + 1) if 0 <= c < WIDE_W]
    return np.array(out, np.int64)


def _wide_list():
    sc = cornell()
    cols = wide_list_columns()
    ws = list_samples("pixels", sc, WIDE_W, WIDE_H, wide_gids(cols), np.zeros(len(cols), np.int64), WIDE_LIST_FRAMES)
    return ws, fold_frames(np.zeros((len(cols), 4), np.float32), ws, np.zeros(len(cols), np.int64))


def wide_list():
    """(workspace [frames, listed, 3], the listed pixels [listed, 4]) of the WIDE list render: roulette_oracle.samples and the fold"""
    return do.once(_wide_list)


# ---- features, the lens AO render, the lens rays -------------------------------------------------------------------------------------
def feature_scene(tall):
    sc = env_scene(TALL_SCENE) if tall else cornell()
    return sc[0], sc[1]


def features_tall(name, lens):
    tris, mats = feature_scene(True)
    return fo.once(("tall", name, lens), lambda: fo.samples(tris, mats, TALL_W, TALL_H, FEATURE_FRAMES, cam=lens_camera() if lens else None,
                                                            **TALL[name]))


def features_late(lens):
    tris, mats = feature_scene(False)
    fb, n = LATE["last_frames"]
    return fo.once(("late", lens), lambda: fo.samples(tris, mats, LATE_W, LATE_H, n, frame_begin=fb, cam=lens_camera() if lens else None))


def _ao_lens_tall(**stripes):
    tris = env_scene(TALL_SCENE)[0]
    with lens_oracle.lens(*LENS):
        return (ao_oracle.counts(tris, TALL_W, TALL_H, 0, 2, AO_K, AO_RADIUS, cam=lens_camera(), **stripes),)


def ao_lens_tall(name):
    """uint32 [local rows, W, 2]: the counts of two frames of pt_render_ao under the lens camera"""
    return do.once(_ao_lens_tall, **TALL[name])[0]


def _ao_lens_late():
    tris = cornell()[0]
    fb, n = LATE["last_frames"]
    with lens_oracle.lens(*LENS):
        return (ao_oracle.counts(tris, LATE_W, LATE_H, fb, n, AO_K, AO_RADIUS, cam=lens_camera()),)


def ao_lens_late():
    return do.once(_ao_lens_late)[0]


LENS_RAYS_FRAME = 2 ** 31 - 2


def _lens_rays_late():
    return (lens_oracle.camera_rays(lens_camera(), LATE_W, LATE_H, LENS_RAYS_FRAME),)


def lens_rays_late():
    """float32 [384, 8]: pt_camera_rays' records of the lens camera at the last frame the ABI accepts"""
    return do.once(_lens_rays_late)[0]


