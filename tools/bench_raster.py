#!/usr/bin/env python3
"""Mesh rasteriser timings on one GPU, one JSON line.  HIP-event medians over --iters calls after --warmup
calls, golden SDF weights (f16x3), one latent, sampled poses, crop --crop (default 128), for each mesh of --meshes
(`64t8`: the 64^3 mesh textured at texel 8; `256v`: the 256^3 mesh with vertex colours):

  surface_ms             oi_amd.trace.render_surface of the same view: the traced frame the mesh replaces
  mesh_ms_b1 / _b16      oi_amd.raster.render_mesh per view, 1 and 16 views per launch (the read-back of the statistics included)
  setup_ms / fill_ms / resolve_ms / shade_ms   the stages of one single-view launch alone, and their share of their sum
  surface_over_mesh      surface_ms / mesh_ms_b16
  stats                  render_mesh's class counts for the view: triangles, dropped, empty, small, large, covered"""
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
from oi_amd import mesh, ops, raster, trace  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--crop", type=int, default=128)
ap.add_argument("--meshes", default="64t8,256v")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
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


gen, _ = build_models(args.crop, 256, 64, 1, args.precision, "cuda")
gen.eval()
z = torch.randn(64, generator=torch.Generator().manual_seed(0))
np.random.seed(0)
poses = torch.tensor(gen.pose_prior(16), dtype=torch.float32)
out = {"tool": "bench_raster", "precision": args.precision, "crop": args.crop, "iters": args.iters, "warmup": args.warmup, "mesh": {}}
with torch.no_grad():
    surface_ms = median_ms(lambda: trace.render_surface(gen, z, poses[0]))
    for name in args.meshes.split(","):
        lattice = int(name.split("t")[0].split("v")[0])
        if "t" in name:
            m = mesh.extract_textured_mesh(gen, z=z.reshape(1, -1).cuda(), resolution=lattice, texel=int(name.split("t")[1]))
            base = m.mesh
        else:
            m = base = mesh.extract_intrinsic_mesh(gen, z=z.reshape(1, -1).cuda(), resolution=lattice)
        row = {"surface_ms": surface_ms, "mesh_ms_b1": median_ms(lambda: raster.render_mesh(gen, m, poses[0])),
               "mesh_ms_b16": median_ms(lambda: raster.render_mesh(gen, m, poses)) / len(poses)}
        # the stages of one view alone, on the arrays render_mesh itself uses
        b2w, R, near = raster._check_views(gen, poses[:1], None, 1e-3, "bench_raster")
        _, _, attr = raster._check_mesh(m, None, "bench_raster")
        c2b, b2c, kinv, K, offs, w2b = raster._cameras(gen, b2w, R)
        pos = base.positions.float().contiguous()
        setup = ops.raster_setup(b2c, K, offs, R, pos, base.triangles, near, raster.SMALL_MAX)
        zbuf = ops.raster_fill(c2b, kinv, offs, R, pos, base.triangles, setup)
        g = ops.raster_resolve(c2b, kinv, offs, R, pos, base.triangles, zbuf, **attr)
        lt = trace._stack_lights(gen, None, "cuda", "bench_raster")
        stage = {"setup_ms": median_ms(lambda: ops.raster_setup(b2c, K, offs, R, pos, base.triangles, near, raster.SMALL_MAX)),
                 "fill_ms": median_ms(lambda: ops.raster_fill(c2b, kinv, offs, R, pos, base.triangles, setup)),
                 "resolve_ms": median_ms(lambda: ops.raster_resolve(c2b, kinv, offs, R, pos, base.triangles, zbuf, **attr)),
                 "shade_ms": median_ms(lambda: ops.surface_shade(g["rays_o"][0], g["rays_d"][0], g["t"][0], g["status"][0],
                                                                 g["hit_slot"][0], g["hit_points"][0], g["grad"][0], g["rgb"][0],
                                                                 R * R, w2b[0], lt, None, None))}
        total = sum(stage.values())
        row.update(stage)
        row["share"] = {k[:-3]: round(v / total, 3) for k, v in stage.items()}
        row["surface_over_mesh"] = surface_ms / row["mesh_ms_b16"]
        row["stats"] = raster.render_mesh(gen, m, poses[0])["stats"]
        out["mesh"][name] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}
        del m, base, setup, zbuf, g
        torch.cuda.empty_cache()
print(json.dumps(out))
