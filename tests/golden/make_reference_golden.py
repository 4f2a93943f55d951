"""Writes tests/golden/reference_program/: what the reference kernel's own program wrote, run on the host.

Needs oracle/_ref/libgencolors_ref.so (``__graft_entry__.build()`` on a machine with the reference checkout).  The outputs are data
the reference's program computed -- framebuffers, rays, hit records -- and the inputs that this project's own code generated for
them; nothing of the reference's text:

  <case>.npy                 float32 [W * H, 3]: the framebuffer's RGB after the case's frames (tests/reference_cases.GOLDEN_RENDERS)
  rays_40x24_f<frame>.npy    float32 [W * H, 6]: generateRay's origin and direction of every pixel
  edge_rays.npy              float32 [n, 7]: origin, direction (as given, before getRay), class index of about 1 000 edge rays
  edge_hits.npy              float32 [n, 8]: intersectWorld's triangle index (-1: no hit), t, p, n (zeros without a hit)
  manifest.json              the cases by name

Usage:  python tests/golden/make_reference_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import reference_cases as rc  # noqa: E402
from oracle import ptoracle, refprog  # noqa: E402


def main():
    out = os.path.join(HERE, "reference_program")
    os.makedirs(out, exist_ok=True)
    R = refprog.Side("ref")
    manifest = {"renders": [], "rays": [], "edge_classes": list(rc.EDGE_CLASSES)}
    for name, scene_name, W, H, frames in rc.GOLDEN_RENDERS:
        tris, mats = rc.scene(scene_name)
        fb = R.render(refprog.pad36(tris), mats, W, H, frames)
        np.save(os.path.join(out, name + ".npy"), np.ascontiguousarray(fb[:, :3]))
        manifest["renders"].append({"name": name, "scene": scene_name, "W": W, "H": H, "frames": frames,
                                    "nan_values": int(np.isnan(fb[:, :3]).sum())})
    W, H, frames = rc.GOLDEN_RAYS
    gid = np.arange(W * H)
    for frame in frames:
        seed = (gid + ptoracle.hash_u32(frame)).astype(np.uint64).astype(np.uint32)
        o, d, _ = R.generate_ray(gid % W, gid // W, W, H, seed)
        name = "rays_%dx%d_f%d" % (W, H, frame)
        np.save(os.path.join(out, name + ".npy"), np.concatenate([o, d], axis=1))
        manifest["rays"].append({"name": name, "W": W, "H": H, "frame": frame})
    o, d, cls = rc.edge_rays()
    keep = rc.golden_hit_selection(cls)
    o, d, cls = o[keep], d[keep], cls[keep]
    hits = np.zeros((len(o), 8), np.float32)
    for name in ("cornell", "coincident"):
        k = np.flatnonzero(rc.edge_scene_of(cls) == name)
        hit, t, p, n, tri = R.intersect_world(refprog.pad36(rc.scene(name)[0]), o[k], d[k])
        hits[k] = np.concatenate([tri[:, None].astype(np.float32), t[:, None], p, n], axis=1)
    np.save(os.path.join(out, "edge_rays.npy"), np.concatenate([o, d, cls[:, None].astype(np.float32)], axis=1))
    np.save(os.path.join(out, "edge_hits.npy"), hits)
    manifest["edge_rays"] = {"count": int(len(o)), "hits": int((hits[:, 0] >= 0).sum())}
    with open(os.path.join(out, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    sizes = {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    print("%d files, %d bytes, largest %d" % (len(sizes), sum(sizes.values()), max(sizes.values())))


if __name__ == "__main__":
    main()
