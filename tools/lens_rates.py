#!/usr/bin/env python3
"""Informational: what the thin lens (``Camera(lens_radius=, focus_distance=)``) costs ON THE DEVICE, off and on.

SIZE^2 pixels, FRAMES frames per run, K = 1: pt_render_ao, pt_render_direct_power and pt_render_indirect_rr (MIS, lights by power,
roulette (3, 0.95), B = 16) on the Cornell box (brute force) and on the room of 64 emitters with filler (520 triangles, the LBVH): six rows.

(a) Off: the pinhole rate of this tree against another build of the library -- the parent commit's, made with
    ``SRC_DIR=<parent checkout>/oclpathtracer_amd/csrc tools/build_variant.sh parent`` and named with ``--parent``.  Both are measured in
    the same session, in processes of their own that take turns and swap places every round (a library is chosen when a process loads it:
    PT_SHIM_LIB), ROUNDS times.  Per row: min / median / max of either, and whether this tree's median lies inside the parent's own min .. max.
(b) On: R = 0.05, F = 6 against the pinhole, alternating inside one process of this tree's library: the ratio of the times per sample.
    Brute force pays two uniforms, a square root and a sine / cosine per sample; through the LBVH the primary rays' origins no longer
    coincide, and their ratio is reported by itself.
Every run is timed by the device events around the call (pt_event_elapsed_ns), REPS times per process after one warm-up round.
No figure is gated.  usage: python tools/lens_rates.py [rates.txt] [--parent LIB] [--size 1024] [--frames 16] [--reps 5] [--rounds 4]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

args = sys.argv[1:]


def option(name, default):
    if name in args:
        at = args.index(name)
        value = args[at + 1]
        del args[at: at + 2]
        return value
    return default


SIZE = int(option("--size", 1024))
FRAMES = int(option("--frames", 16))
REPS = int(option("--reps", 5))
ROUNDS = int(option("--rounds", 4))
PARENT = option("--parent", None)
MEASURE = option("--measure", None)   # (a child of this tool: "pinhole" or "both")
LENS = (0.05, 6.0)
ROWS = [(s, e) for s in ("Cornell box, brute force (36 triangles)", "64 emitters with filler, LBVH (520 triangles)")
        for e in ("pt_render_ao", "pt_render_direct_power", "pt_render_indirect_rr")]


def measure(with_lens):
    """one process, one device: {row: {"pinhole": [seconds per run], "lens": [...]}} as one JSON line on stdout"""
    from oclpathtracer_amd import adl, scene
    from oclpathtracer_amd.ao import AORenderer
    from oclpathtracer_amd.camera import Camera
    from oclpathtracer_amd.direct import DirectRenderer
    from oclpathtracer_amd.indirect import IndirectRenderer, Roulette
    from ris_scenes import many_lights_lbvh

    assert adl.init()
    dev = adl.DeviceUtils.allocate()
    out = {}
    try:
        ev = adl.SyncObject(dev)
        pin = Camera.reference()
        cams = [("pinhole", pin)] + ([("lens", pin.with_lens(*LENS))] if with_lens else [])
        for what, (tris, mats) in zip(ROWS[::3], (scene.load_model(), many_lights_lbvh())):
            what = what[0]
            lit = dict(light_samples=1, light_choice="power", stripe_rows=1, chunk_frames=FRAMES)
            renderers = (
                ("pt_render_ao", AORenderer(dev, tris, SIZE, SIZE, rays_per_sample=1, stripe_rows=1)),
                ("pt_render_direct_power", DirectRenderer(dev, tris, mats, SIZE, SIZE, **lit)),
                ("pt_render_indirect_rr", IndirectRenderer(dev, tris, mats, SIZE, SIZE, max_bounces=16, mis=True, roulette=Roulette(3, 0.95), **lit)),
            )
            for entry, r in renderers:
                times = {k: [] for k, _ in cams}
                try:
                    for rep in range(REPS + 1):
                        for key, cam in cams:
                            r.set_camera(cam)
                            r.render(FRAMES, 0, sync=ev)
                            ev.waitForCompletion()
                            if rep:
                                times[key].append(ev.getExecutionTimeNanoseconds() * 1e-9)
                finally:
                    r.release()
                out["%s | %s" % (what, entry)] = times
        print(json.dumps(dict(device=dev.getDeviceName(), rows=out)), flush=True)
    finally:
        adl.DeviceUtils.deallocate(dev)


def child(mode, lib=None):
    env = dict(os.environ)
    env.pop("PT_SHIM_LIB", None)
    if lib:
        env["PT_SHIM_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--measure", mode, "--size", str(SIZE), "--frames", str(FRAMES), "--reps", str(REPS)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("lens_rates: the %s process failed (%d)\n%s%s" % (lib or "tree's", r.returncode, r.stdout, r.stderr))
    return json.loads(r.stdout.strip().split("\n")[-1])


def main():
    out_path = (args + [None])[0]
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    new, old, device = {}, {}, "?"
    # (this process never opens the device: the two libraries take turns in processes of their own, and swap places every round)
    for rnd in range(ROUNDS):
        for which in (("parent", "tree") if rnd % 2 == 0 else ("tree", "parent")):
            if which == "parent":
                if PARENT:
                    for k, v in child("pinhole", PARENT)["rows"].items():
                        old.setdefault(k, []).extend(v["pinhole"])
                continue
            got = child("both")
            device = got["device"]
            for k, v in got["rows"].items():
                d = new.setdefault(k, dict(pinhole=[], lens=[]))
                d["pinhole"].extend(v["pinhole"])
                d["lens"].extend(v["lens"])
    nsamples = SIZE * SIZE * FRAMES
    rate = lambda ts: [nsamples / t * 1e-6 for t in ts]
    fmt = lambda v: "%8.1f / %8.1f / %8.1f" % (min(v), float(np.median(v)), max(v))
    emit("%s; %d^2 pixels, %d frames per run, K = 1; indirect: MIS, lights by power, roulette (3, 0.95), B = 16; device events; %d rounds of "
         "%d runs per process after one warm-up round; Msamples/s as min / median / max" % (device, SIZE, FRAMES, ROUNDS, REPS))
    emit("(a) the lens off: the pinhole rate of this tree%s" % (" against the parent commit's library" if PARENT else ""))
    for k in new:
        emit("  %s" % k)
        n = rate(new[k]["pinhole"])
        emit("    this tree   %s" % fmt(n))
        if PARENT:
            o = rate(old[k])
            inside = min(o) <= float(np.median(n)) <= max(o)
            emit("    parent      %s    this tree's median / the parent's %.4f; %s the parent's min .. max"
                 % (fmt(o), float(np.median(n)) / float(np.median(o)), "inside" if inside else "OUTSIDE"))
    emit("(b) the lens on: R = %g, F = %g against the pinhole, same process, alternating" % LENS)
    for k in new:
        tp, tl = float(np.median(new[k]["pinhole"])), float(np.median(new[k]["lens"]))
        emit("  %-75s lens %s    time per sample %.3f of the pinhole's" % (k, fmt(rate(new[k]["lens"])), tl / tp))
    brute = [float(np.median(new[k]["lens"])) / float(np.median(new[k]["pinhole"])) for k in new if "brute" in k]
    lbvh = [float(np.median(new[k]["lens"])) / float(np.median(new[k]["pinhole"])) for k in new if "LBVH" in k]
    emit("  brute force (two uniforms, a square root, a sine / cosine per sample): %s" % ", ".join("%.3f" % x for x in brute))
    emit("  LBVH (and primary rays whose origins no longer coincide):              %s" % ", ".join("%.3f" % x for x in lbvh))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if MEASURE:
        measure(MEASURE == "both")
    else:
        main()
