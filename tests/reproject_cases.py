"""What the reprojection tests share: the camera pairs, Cornell-box records from the CPU oracles, and the quality experiment of
profiles/reproject/quality.txt.  Every set of records is computed once per key and handed out read-only.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import math

import numpy as np

import moments_oracle as mo
import reproject_oracle as ro

F = np.float32
_ONCE = {}


def cameras():
    """the reference camera and the two moves of it the issue names, and two more for the device tests"""
    from oclpathtracer_amd.camera import Camera

    ref = Camera.reference()
    s5, c5 = math.sin(math.radians(5.0)), math.cos(math.radians(5.0))
    return dict(
        ref=ref,
        shifted=Camera((0.3, 2.75, 4.0), (0.3, 2.75, 3.0)),                           # eye and centre moved by (0.3, 0, 0)
        panned=Camera(ref.eye, (s5, 2.75, 4.0 - c5)),                                 # 5 degrees about the up axis
        wide=Camera(ref.eye, ref.center, ref.up, 75.0),                               # another field of view
        away=Camera(ref.eye, (0.0, 2.75, 5.0)),                                       # turned round: the scene lies behind it
    )


def _frozen(key, make):
    if key not in _ONCE:
        v = make()
        for a in (v.values() if isinstance(v, dict) else [v]):
            a.setflags(write=False)
        _ONCE[key] = v
    return _ONCE[key]


def feature_records(tris, mats, w, h, cam_name, frames, frame_begin=0):
    """dict feature -> MOMENTS_DTYPE [w * h] of `frames` feature frames under cameras()[cam_name], and "tri": int32 [frames, w * h]"""
    import feature_oracle as fo

    def make():
        fs = fo.samples(tris, mats, w, h, frames, frame_begin=frame_begin, cam=cameras()[cam_name])
        out = {f: mo.accumulate(getattr(fs, f)) for f in fo.FEATURES}
        out["tri"] = fs.tri.copy()
        return out

    return _frozen(("f", w, h, cam_name, frames, frame_begin), make)


def colour_records(tris, mats, w, h, cam_name, begin, frames, K=1, B=4):
    """MOMENTS_DTYPE [w * h]: the indirect-illumination samples of frames [begin, begin + frames) under the camera"""
    return _frozen(("c", w, h, cam_name, begin, frames, K, B), lambda: colour_onto(tris, mats, w, h, cam_name, begin, frames, None, K, B))


def colour_onto(tris, mats, w, h, cam_name, begin, frames, start, K=1, B=4):
    """the same accumulated on top of the records `start` (None: zeros) -- what pt_sample_moments(reset = 0) does"""
    import indirect_oracle as io

    m = start
    for f in range(begin, begin + frames, 32):   # (chunks: the sample arrays stay small)
        k = min(32, begin + frames - f)
        gid, frame = io.all_samples(w, h, k, f)
        m = mo.accumulate(io.samples(tris, mats, w, h, gid, frame, K, B, cam=cameras()[cam_name])[0].reshape(k, w * h, 3), m)
    return m


def mean_image(rec, w, h):
    return mo.resolve(rec)[0].reshape(h, w, 3)


# ---- the quality experiment ------------------------------------------------------------------------------------------------------
QW = QH = 48
QHIST, QNEW, QREF_BEGIN, QREF_FRAMES = 8, 2, 1000, 256


def quality(tris, mats, move, **params):
    """Cornell box 48 x 48, B = 4, K = 1, uniform light choice.  History: frames 0 .. 7 under the reference camera; reference image:
    the mean of frames 1000 .. 1255 under cameras()[move].  A dict of (mse, mean relative mse, median relative mse) of (i) the mean of frames 8 .. 9 under the
    new camera alone, (ii) the re-projected history plus those two frames, (iii) frames 8 .. 17 under the new camera; the share of
    covered pixels that took history and the mean history length over those."""
    w, h = QW, QH
    hist = colour_records(tris, mats, w, h, "ref", 0, QHIST)
    pf = feature_records(tris, mats, w, h, "ref", QHIST)
    cf = feature_records(tris, mats, w, h, move, 1, QHIST)      # one feature frame under the new camera, numbered on
    ref = mean_image(colour_records(tris, mats, w, h, move, QREF_BEGIN, QREF_FRAMES), w, h)
    cams = cameras()
    out, info = ro.reproject(hist, pf["normal"], pf["depth"], cf["normal"], cf["depth"], w, h, cams["ref"], cams[move], **params)
    alone = colour_records(tris, mats, w, h, move, QHIST, QNEW)
    merged = colour_onto(tris, mats, w, h, move, QHIST, QNEW, out)
    perfect = colour_records(tris, mats, w, h, move, QHIST, QHIST + QNEW)
    lum = ref.sum(axis=2)
    den = lum * lum / 3.0 + 0.01

    def figures(rec):
        e2 = ((mean_image(rec, w, h) - ref) ** 2).sum(axis=2)
        return float(e2.mean()), float((e2 / den).mean()), float(np.median(e2 / den))

    covered = cf["depth"]["sum"][:, 1] > 0
    took = out["n"] > 0
    return dict(alone=figures(alone), merged=figures(merged), perfect=figures(perfect), share=float(took[covered].mean()),
                length=float(out["n"][took].mean()) if took.any() else 0.0)
