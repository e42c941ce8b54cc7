#!/usr/bin/env python3
"""Relighting timings on one GPU, one JSON line.  HIP-event medians over --iters calls after --warmup
calls, with the golden SDF weights, at C2 (64 x 64 pixels, 64 + 64 samples per ray) and at the inference setting of bench.py
(128 x 128, 256 + 64), for each L of --lights:

  capture_ms          oi_amd.relight.capture: one eval Generator.forward(return_raw=True) (ray chunks as the forward takes them)
  relight_ms          one oi_relight_fwd launch for L lights, image only (ops.relight_fwd); per_light_us = relight_ms / L
  relight_maps_ms     the same launch with all five outputs (image, image_no_bg, shading, diffuse, specular)
  capture_gbps        capture bytes (32 per sample) over relight_ms: the launch's one read of the capture
  composite_ms        the same L lights as L oi_composite_fwd calls on the same capture (the grey light only; image only)
  rerender_ms         L re-renders: L x one eval Generator.forward without return_raw (measured once, scaled by L)
  rerender_vs_relight rerender_ms / relight_ms"""
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
from oi_amd import ops  # noqa: E402
from oi_amd import relight as RL  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lights", default="1,16,128")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--precision", default="f16x3")
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


def lights_for(base, n):
    from oi_amd.inference import light_walk_directions
    dirs = light_walk_directions(base.direction, n)
    return [base] + [base.replace(direction=tuple(d), diffuse=(1.0, 0.8, 0.6)) for d in dirs[1:]]


out = {"tool": "bench_relight", "precision": args.precision, "iters": args.iters, "warmup": args.warmup, "settings": {}}
with torch.no_grad():
    for name, (R, S, I) in (("C2", (64, 64, 64)), ("inference", (128, 256, 64))):
        gen, _ = build_models(R, S, I, 1, args.precision, "cuda")
        gen.eval()
        with torch.no_grad():
            gen.light.param_specular.fill_(0.2)
        z = torch.randn(1, 64, generator=torch.Generator().manual_seed(0)).cuda()
        np.random.seed(0)
        b2w = torch.tensor(gen.pose_prior(1), dtype=torch.float32).cuda()
        bg = torch.zeros(1, 3, device="cuda")
        cap = RL.capture(gen, z=z, b2w=b2w)
        N, T = cap.weights.shape
        row = {"rays": N, "samples_per_ray": T, "capture_bytes": cap.nbytes,
               "capture_ms": median_ms(lambda: RL.capture(gen, z=z, b2w=b2w), iters=5)}
        data = {"z": z, "b2w": b2w, "bg_color": bg}
        render_ms = median_ms(lambda: gen(bs=1, it=None, data=data), iters=5)
        base = RL.Light.from_module(gen.light)
        grey = gen.light.packed().detach().clone()
        ldir = gen.light.batch_direction(cap.w2b).contiguous()
        raw = gen(bs=1, it=None, data=data, return_raw=True)["box"]["raw_render_out"]
        dists = torch.full_like(cap.mid_z, 2.0 / S)   # (section lengths are not kept by the forward; timing only)
        row["L"] = {}
        for nl in (int(x) for x in args.lights.split(",")):
            lt = RL.stack_lights(lights_for(base, nl))

            def one(outputs):
                return lambda: ops.relight_fwd(cap.weights, cap.gradients, cap.albedo, cap.mid_z, cap.rays_o, cap.rays_d,
                                               cap.w2b, lt, bg, 1, outputs=outputs)

            def composite_l():
                for _ in range(nl):
                    ops.composite_fwd(raw["sdf"], raw["gradients"], raw["raw_color"], dists,
                                      raw["mid_z_vals"], cap.rays_o, cap.rays_d, ldir, bg, gen.deviation_network.variance,
                                      grey, 1.0, 1, outputs=("image",))

            r = {"relight_ms": median_ms(one(("image",))), "relight_maps_ms": median_ms(one(ops.RELIGHT_OUT))}
            r["per_light_us"] = 1e3 * r["relight_ms"] / nl
            r["capture_gbps"] = cap.nbytes / (r["relight_ms"] * 1e-3) / 1e9
            r["composite_ms"] = median_ms(composite_l, iters=5)
            r["rerender_ms"] = render_ms * nl
            r["rerender_vs_relight"] = r["rerender_ms"] / r["relight_ms"]
            row["L"][str(nl)] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
        row["render_ms"] = round(render_ms, 4)
        row["capture_ms"] = round(row["capture_ms"], 4)
        l1, l16 = row["L"].get("1"), row["L"].get("16")
        if l1 and l16:
            row["launch_growth_1_to_16"] = round(l16["relight_ms"] / l1["relight_ms"], 3)
        out["settings"][name] = row
        del cap, raw, dists, gen
        torch.cuda.empty_cache()
print(json.dumps(out))
