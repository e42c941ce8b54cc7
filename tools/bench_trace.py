#!/usr/bin/env python3
"""Sphere-traced surface rendering timings on one GPU, one JSON line.  HIP-event medians over --iters
calls after --warmup calls, golden SDF weights, one latent and pose, for each resolution of --res:

  surface_ms            oi_amd.trace.render_surface under the trained light, no shadows
  surface_shadow_ms     the same with cast shadows (one light)
  volume_ms             one frame of oi_amd.inference.render_frames with the inference sampling of bench.py --full
                        (256 + 64 samples per ray), same latent and pose, same session
  readback              surface_ms with the count of rays in flight read every step / every 4th / every 16th step / 'auto'
  mlp_share             share of surface_ms spent in the sdf-only MLP passes (their launches re-timed alone on the same bounds)
  stats                 rays per status, sdf evaluations, steps
and, at --walk-res, the 128-frame light walk: surface_light_walk with and without shadows against inference.light_walk."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, ROOT + "/object-intrinsics_amd"):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_models  # noqa: E402
from oi_amd import inference, trace  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--res", default="64,128,512")
ap.add_argument("--walk-res", type=int, default=128)
ap.add_argument("--walk-frames", type=int, default=128)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--precision", default="f16x3")
ap.add_argument("--no-volume-above", type=int, default=128, help="skip the volume render above this resolution")
args = ap.parse_args()


def median_ms(fn, iters=None):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(iters or args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def setup(R):
    gen, _ = build_models(R, 256, 64, 1, args.precision, "cuda")
    gen.eval()
    z = torch.randn(64, generator=torch.Generator().manual_seed(0))
    np.random.seed(0)
    b2w = torch.tensor(gen.pose_prior(1), dtype=torch.float32)[0]
    return gen, z, b2w


out = {"tool": "bench_trace", "precision": args.precision, "iters": args.iters, "warmup": args.warmup, "res": {}}
with torch.no_grad():
    for R in (int(r) for r in args.res.split(",")):
        gen, z, b2w = setup(R)
        row = {"rays": R * R}
        row["surface_ms"] = median_ms(lambda: trace.render_surface(gen, z, b2w))
        row["surface_shadow_ms"] = median_ms(lambda: trace.render_surface(gen, z, b2w, shadows=True))
        st = trace.render_surface(gen, z, b2w, shadows=True)["stats"]
        row["stats"] = st
        row["evals_per_ray"] = st["n_evals"] / (R * R)
        row["rays_per_s"] = R * R / (row["surface_ms"] * 1e-3)
        row["readback"] = {str(k): median_ms(lambda: trace.render_surface(gen, z, b2w, readback=k)) for k in (1, 4, 16, "auto")}
        row["readback_evals"] = {str(k): trace.render_surface(gen, z, b2w, readback=k)["stats"]["n_evals"] for k in (1, 4, 16, "auto")}
        # the MLP passes alone, on the bounds a read every step gives (the true counts)
        s = trace._Surface(gen, z.cuda().reshape(1, -1), b2w, trace.DEFAULT_BIAS, {"readback": 1})
        steps = s.res.steps.long()
        counts = [int((steps > k).sum()) for k in range(int(steps.max()))]
        pts = torch.randn(R * R, 3, device="cuda") * 0.3

        def mlp_only():
            for c in counts:
                s.field.sdf(pts[:c])
        row["mlp_passes_ms"] = median_ms(mlp_only)
        row["mlp_share"] = row["mlp_passes_ms"] / row["readback"]["1"]
        row["steps_run"] = len(counts)
        if R <= args.no_volume_above:
            row["volume_ms"] = median_ms(lambda: inference.render_frames(gen, [z], [b2w], keys=("image", "normal_map", "shading_map")),
                                         iters=max(3, args.iters // 2))
            row["surface_vs_volume"] = row["surface_ms"] / row["volume_ms"]
        out["res"][str(R)] = row
        del gen
    gen, z, b2w = setup(args.walk_res)
    n = args.walk_frames
    out["light_walk"] = {
        "res": args.walk_res, "frames": n,
        "surface_shadows_ms": median_ms(lambda: inference.surface_light_walk(gen, z, b2w, n_frames=n, shadows=True), iters=5),
        "surface_no_shadows_ms": median_ms(lambda: inference.surface_light_walk(gen, z, b2w, n_frames=n, shadows=False), iters=5),
        "relight_walk_ms": median_ms(lambda: inference.light_walk(gen, z, b2w, n_frames=n, keys=("image",)), iters=3),
        "stats": inference.surface_light_walk(gen, z, b2w, n_frames=n, shadows=True)["stats"]}
print(json.dumps(out))
