#!/usr/bin/env python3
"""A fixed query workload for profilers (rocprofv3 --kernel-trace / --pmc): `reps` closest and then `reps` occluded queries of the
same 2^24 random rays through the Cornell box (the first case of tools/query_rates.py), device tensors in and out.
usage: python tools/query_workload.py [reps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime in the process)

from oclpathtracer_amd import adl, scene  # noqa: E402
from oclpathtracer_amd.query import RayCaster  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
tris, _ = scene.load_model()
pts = np.concatenate([tris["p1"][:, :3], tris["p2"][:, :3], tris["p3"][:, :3]])
assert adl.init()
dev = adl.DeviceUtils.allocate()
try:
    rc = RayCaster(dev, tris)
    n = 1 << 24
    g = torch.Generator(device="cuda").manual_seed(1)
    lo = torch.tensor(pts.min(0), device="cuda")
    hi = torch.tensor(pts.max(0), device="cuda")
    r = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    r[:, :3] = lo + (hi - lo) * torch.rand((n, 3), generator=g, device="cuda")
    r[:, 3] = 1e20
    r[:, 4:7] = torch.randn((n, 3), generator=g, device="cuda")
    for fn in (rc.closest, rc.occluded):
        for _ in range(reps):
            out = fn(r)
        torch.cuda.synchronize()
        del out
    rc.release()
finally:
    adl.DeviceUtils.deallocate(dev)
