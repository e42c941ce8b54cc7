#!/usr/bin/env python3
"""Scene timings on one GPU, one JSON line.  HIP-event medians over --iters calls after --warmup
calls, golden SDF weights, f16x3 by default, K instances from oi_amd.scene.sample_scene at each K of --instances:

  scene_ms / scene_shadows_ms    oi_amd.scene.render_scene without / with shadows: one batched march for all instances, the depth
                                 resolve, the full MLP pass at the visible hits, one shade launch; with shadows one shadow batch of
                                 K occluder elements
  crops_ms / crops_shadows_ms    for comparison, the parent's way of getting the same instances: K calls of
                                 oi_amd.trace.render_surface, each on its own crop of W x W pixels of the same scene image (W: the
                                 scene's window) -- which gives neither occlusion between instances nor mutual shadows
No ratio is promised: the two do different work (the scene tests every shadow ray against all K instances)."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, ROOT + "/object-intrinsics_amd"):
    sys.path.insert(0, p)
import torch  # noqa: E402

from bench import build_models  # noqa: E402
from oi_amd import scene, trace  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=64, help="crop resolution of the generator; the scene image is res * 1588 / 256")
ap.add_argument("--instances", default="1,8,32")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--precision", default="f16x3")
args = ap.parse_args()


def median_ms(fn):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


gen, _ = build_models(args.res, 256, 64, 1, args.precision, "cuda")
gen.eval()
out = {"tool": "bench_scene", "precision": args.precision, "res": args.res, "scene_resolution": gen.scene_resolution,
       "iters": args.iters, "warmup": args.warmup, "instances": {}}
with torch.no_grad():
    for K in (int(k) for k in args.instances.split(",")):
        zs, b2ws = scene.sample_scene(gen, K, args.seed)
        s = scene.trace_scene(gen, zs, b2ws)
        crop = copy.copy(gen)            # the same camera and scene image, a crop of W x W pixels per instance
        crop.resolution = s.W

        def crops(shadows):
            for z, b2w in zip(zs, b2ws):
                trace.render_surface(crop, z, b2w, shadows=shadows)

        row = {"window": s.W, "rays": K * s.N, "entered": sum(s.n_entered), "hits": sum(s.n_hit), "visible": sum(s.n_vis)}
        for name, shadows in (("", False), ("_shadows", True)):
            row["scene" + name + "_ms"] = median_ms(lambda: scene.render_scene(gen, zs, b2ws, shadows=shadows))
            row["crops" + name + "_ms"] = median_ms(lambda: crops(shadows))
        out["instances"][str(K)] = row
print(json.dumps(out))
