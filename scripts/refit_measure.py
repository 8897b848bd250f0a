#!/usr/bin/env python3
"""What a BVH refit costs against a rebuild, and what it does to the tree.

The C5 model (icosphere(6), 81,920 triangles) as one instance and as two, its
vertices alternating between two displaced shapes.  Median of REPS
repetitions after WARM warm-ups, wall time around the call plus sync():
  (a) set_model + model_info()      the rebuild: host gather, binned SAH, re-allocation, upload
  (b) update_model(numpy)           host copy + refit
  (c) update_model(torch GPU)       device copy + refit, and its HIP-event time on the context's stream
Then C5 itself (4096^2, 4 spp per step, STEPS steps after 2 warm-ups): ms per
step on the tree refitted to the displaced shape against the tree built from
it, the two contexts alternating in one process.

    python scripts/refit_measure.py [--small]     one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "raytracer-0_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rt0  # noqa: E402
from rt0 import meshes as M  # noqa: E402
from rt0 import workloads  # noqa: E402

REPS, WARM, STEPS = 20, 3, 8


def med(xs):
    return round(statistics.median(xs), 4)


def timings(wl, level, instances):
    wl = dict(wl, scene_lines=[l for l in wl["scene_lines"] if "TRIANGLE" not in l] +
              [l for l in wl["scene_lines"] if "TRIANGLE" in l] * instances,
              models=[{"kind": "icosphere", "level": level}] * instances)
    if instances == 2:  # the second instance beside the first
        wl["scene_lines"][-1] = wl["scene_lines"][-1].replace("vec3(0.0,", "vec3(1.5,")
    r = rt0.Renderer(64, 64)
    workloads.configure(r, wl)
    _, tri = M.icosphere(level)
    shapes = [M.wavy_icosphere(level, amp=a, freq=f)[0] for a, f in ((0.08, 6.0), (0.12, 4.0))]
    dev = [torch.from_numpy(s).to("cuda:0") for s in shapes]
    n, depth = r.model_info()
    ext = torch.cuda.ExternalStream(r.device_accum()[1], device=torch.device("cuda:0"))
    out = {"triangles": n, "depth": depth, "height_groups": len(rt0.bvh_height_order(r.read_bvh()[0], n)[1]) - 1}

    def run(fn):
        ts = []
        for i in range(WARM + REPS):
            r.sync()
            t0 = time.perf_counter()
            fn(i)
            r.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return med(ts[WARM:])

    def rebuild(i):
        for k in range(instances):
            r.set_model(k, shapes[i & 1], tri)
        r.model_info()

    out["a_set_model_ms"] = run(rebuild)
    out["b_update_numpy_ms"] = run(lambda i: [r.update_model(k, shapes[i & 1]) for k in range(instances)])
    out["c_update_torch_ms"] = run(lambda i: [r.update_model(k, dev[i & 1]) for k in range(instances)])
    ev = []
    for i in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r.sync()
        e0.record(ext)
        for k in range(instances):
            r.update_model(k, dev[i & 1])
        e1.record(ext)
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    out["c_refit_event_ms"] = med(ev[WARM:])
    out["a_over_c"] = round(out["a_set_model_ms"] / out["c_update_torch_ms"], 1)
    r.close()
    return out


def quality(wl, level, size):
    wl = dict(wl, width=size, height=size, models=[{"kind": "icosphere", "level": level}])
    v, tri = M.wavy_icosphere(level, amp=0.12, freq=4.0)
    ctx = {}
    for name in ("refit", "built"):
        r = rt0.Renderer(size, size)
        workloads.configure(r, wl)
        if name == "refit":
            r.model_info()
            r.update_model(0, v)
        else:
            r.set_model(0, v, tri)
        ctx[name] = r
    ms = {"refit": [], "built": []}
    for step in range(2 + STEPS):
        for name, r in ctx.items():
            r.sync()
            t0 = time.perf_counter()
            r.render(1 + step * wl["spp"], wl["spp"])
            r.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(ctx["refit"].read_accum(), ctx["built"].read_accum()))
    return {"refit_ms_per_step": med(ms["refit"][2:]), "built_ms_per_step": med(ms["built"][2:]),
            "same_image": same, "size": size, "spp": wl["spp"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="icosphere(3) and a 256^2 image: a quick check of the script")
    a = ap.parse_args()
    wl = workloads.get("c5")
    level, size = (3, 256) if a.small else (6, wl["width"])
    res = {"one_instance": timings(wl, level, 1), "two_instances": timings(wl, level, 2),
           "c5_after_smooth_deformation": quality(wl, level, size)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
