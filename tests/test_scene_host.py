"""Host logic that needs no GPU: scene ingestion, soup generator, PPM output, stripe index math."""
import os
import struct
import sys

import numpy as np
import pytest

from oclpathtracer_amd import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_rejects_truncated_and_bad_indices(tmp_path):
    blob = open(scene.DEFAULT_SCENE, "rb").read()
    for cut in (0, 3, 10, 100, len(blob) - 1):
        with pytest.raises(ValueError):
            scene.parse_meshes(blob[:cut])
    bad = bytearray(blob)
    struct.pack_into("<i", bad, 12, 99)  # first face index of mesh 0 out of range
    with pytest.raises(ValueError):
        scene.parse_meshes(bytes(bad))
    assert scene.parse_meshes(struct.pack("<i", 0)) == []
    p = tmp_path / "empty.bin"
    p.write_bytes(struct.pack("<i", 0))
    t, m = scene.load_model(str(p))
    assert len(t) == 0 and len(m) == 0


def test_records_are_64_bytes_and_zero_padded():
    t, m = scene.load_model()
    assert t.dtype.itemsize == 64 and m.dtype.itemsize == 64
    assert not t["pad"].any() and not m["pad"].any()
    assert np.all(m["roughness"][m["type"] == scene.DIFFUSE] == 0)  # reference leaves it uninitialised


def test_soup_is_deterministic_and_well_formed():
    a_t, a_m = scene.make_soup(5000)
    b_t, b_m = scene.make_soup(5000)
    assert a_t.tobytes() == b_t.tobytes() and a_m.tobytes() == b_m.tobytes()
    c_t, _ = scene.make_soup(5000, seed=1)
    assert a_t.tobytes() != c_t.tobytes()
    base_t, base_m = scene.load_model()
    assert a_t[:36].tobytes() == base_t.tobytes() and a_m[:18].tobytes() == base_m.tobytes()
    assert len(a_t) == 5000 and len(a_m) == 18 + (5000 - 36 + 1) // 2
    assert a_t["id"].max() == len(a_m) - 1 and a_t["id"][36] == 18
    ext = a_t[36:]
    assert np.all(np.abs(ext["p2"][:, :3] - ext["p1"][:, :3]) <= 0.02 + 1e-6)
    assert ext["p1"][:, 0].min() >= -2.7 and ext["p1"][:, 1].max() <= 5.4 + 1e-6
    assert np.all(a_m["type"][18:] == scene.DIFFUSE) and np.all(a_m["emissive"][18:, :3] == 0)
    with pytest.raises(ValueError):
        scene.make_soup(10)


def test_f2c_and_ppm(tmp_path):
    v = np.array([0, 0.25, 1, 4, np.nan, np.inf, -1.0, 1e-12], np.float32)
    assert scene.f2c(v).tolist() == [0, 127, 255, 255, -2147483648, -2147483648, -2147483648, 0]
    fb = np.zeros((4, 4), np.float32)
    fb[:, :3] = [[0, 0.25, 1], [1, 1, 1], [0.04, 0.09, 0.16], [4, 0, 0]]
    p = tmp_path / "o.ppm"
    scene.write_ppm(str(p), fb, 2, 2)
    assert p.read_text() == "P3\n2 2\n255\n0 127 255 255 255 255 51 76 102 255 0 0 "


@pytest.mark.parametrize("H,stripe,world", [(64, 16, 1), (64, 16, 2), (64, 4, 8), (47, 5, 3), (40, 16, 8), (1, 1, 4), (1024, 16, 8)])
def test_stripe_plan_partitions_rows(H, stripe, world):
    torch = pytest.importorskip("torch")  # noqa: F841
    from oclpathtracer_amd.distributed import StripePlan

    plan = StripePlan(H, stripe, world)
    seen = np.concatenate([plan.global_rows(r) for r in range(world)])
    assert sorted(seen.tolist()) == list(range(H))
    for r in range(world):
        rows = plan.global_rows(r)
        assert len(rows) == plan.local_rows(r)
        # local row lr -> global row, the mapping pt_trace_kernel uses
        lr = np.arange(len(rows))
        g = ((lr // stripe) * world + r) * stripe + lr % stripe
        assert np.array_equal(g, rows)
    assert plan.slab_rows == max(plan.local_rows(r) for r in range(world))


def test_material_side_file_reproduces_reference_assignment(tmp_path):
    """the per-mesh material ifs of RaytraceTest.cpp:145-176 as a data table."""
    import json

    base_t, base_m = scene.load_model()
    meshes = scene.parse_meshes(open(scene.DEFAULT_SCENE, "rb").read())
    table = scene.reference_material_table(len(meshes), [m[0] for m in meshes])
    assert [e["type"] for e in table] == ["diffuse"] * 5 + ["specular"]
    assert table[2]["emissive"][:3] == [30.0, 30.0, 30.0] and table[2]["albedo"][:3] == [0.7, 0.7, 0.7]  # the light
    p = tmp_path / "materials.json"
    p.write_text(json.dumps(table))
    for src in (table, str(p)):
        t, m = scene.load_model(materials=src)
        assert t.tobytes() == base_t.tobytes() and m.tobytes() == base_m.tobytes()
    # a different table changes the materials only
    table[3]["albedo"] = [0.1, 0.2, 0.9]
    table[4]["type"] = "specular"
    table[4]["roughness"] = 0.25
    t, m = scene.load_model(materials=table)
    assert t.tobytes() == base_t.tobytes()
    changed = [i for i in range(len(m)) if m[i].tobytes() != base_m[i].tobytes()]
    assert changed == sorted(set(int(x) for x in t["id"][np.isin(t["id"], changed)]))
    red_id = int(np.argmax(np.all(base_m["albedo"][:, :3] == np.array([0.6, 0, 0], np.float32), axis=1)))
    assert np.allclose(m[red_id]["albedo"], [0.1, 0.2, 0.9, 1.0])
    green_id = int(np.argmax(np.all(base_m["albedo"][:, :3] == np.array([0, 0.6, 0], np.float32), axis=1)))
    assert m[green_id]["type"] == scene.SPECULAR and m[green_id]["roughness"] == np.float32(0.25)
    with pytest.raises(ValueError):
        scene.load_model(materials=table[:3])
    table[0]["type"] = "glass"
    with pytest.raises(ValueError):
        scene.load_model(materials=table)


def test_binary_ppm(tmp_path):
    rgb = np.array([[0, 127, 255], [255, 255, 255], [51, 76, 102], [-2147483648, 300, 7]], np.int32)
    p = tmp_path / "o6.ppm"
    scene.write_ppm_binary(str(p), rgb, 2, 2)
    assert p.read_bytes() == b"P6\n2 2\n255\n" + bytes([0, 127, 255, 255, 255, 255, 51, 76, 102, 0, 255, 7])


def test_bench_names_the_baseline_workloads():
    """bench.py --config k selects BASELINE.json's configs[k] by name; overriding a single value drops the name."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    want = {1: (512, 512, 64, 2, 0), 2: (1024, 1024, 256, 16, 0), 3: (2048, 2048, 1024, 16, 0), 4: (1024, 1024, 256, 16, 1_000_000)}
    for k, (w, h, spp, depth, soup) in want.items():
        a = bench.parse_args(["--config", str(k)])
        assert (a.width, a.height, a.spp, a.depth, a.soup) == (w, h, spp, depth, soup) and a.named
    a = bench.parse_args([])
    assert a.config == 2 and a.named and a.gpus == 1 and a.steps >= 1
    a = bench.parse_args(["--config", "3", "--spp", "8", "--steps", "2"])
    assert (a.width, a.spp, a.steps) == (2048, 8, 2) and not a.named
    a = bench.parse_args(["--soup", "5000", "--spp", "4"])
    assert a.soup == 5000 and not a.named


def test_bench_plain_run_options_and_output_dump(tmp_path):
    """A plain bench.py run measures the headline only (--full adds the rest); --steps is the number of timed steps; --dump-outputs
    writes the last step's image whole, or a fixed seeded sample of its pixels when it is larger than the limit."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", str(tmp_path)])
    assert a.full and a.dump_outputs == str(tmp_path)
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)

    img = np.random.default_rng(1).random((24, 40, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "whole"), img)
    got = np.load(tmp_path / "whole" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)

    bench.DUMP_LIMIT_BYTES, bench.DUMP_SAMPLE_PIXELS = 1024, 50
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), img)
    s = np.load(tmp_path / "s1" / "image_sample.npy")
    idx = np.load(tmp_path / "s1" / "image_sample_pixels.npy")
    assert s.dtype == np.float32 and s.shape == (50, 4) and idx.dtype == np.float64
    assert np.array_equal(s, img.reshape(-1, 4)[idx.astype(np.int64)]) and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "image_sample_pixels.npy"))   # the same pixels every run
    assert not (tmp_path / "s1" / "image.npy").exists()


def test_bench_stops_all_ranks_when_one_fails():
    """spawn_ranks used to wait for rank 0 alone.  Without a GPU every rank exits at once with an error; the parent
    must come back with a non-zero code in seconds, not sit in a rendezvous."""
    import subprocess
    import time

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("a GPU is present: the ranks would run")
    except ImportError:
        pass
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--width", "32",
                        "--height", "32", "--spp", "1"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=170)
    assert p.returncode != 0
    assert b"rank(s) failed first" in p.stderr, p.stderr[-800:]
    assert time.time() - t0 < 150
