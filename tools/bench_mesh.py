#!/usr/bin/env python3
"""Mesh extraction timings on one GPU, one JSON line.  HIP-event medians over --iters calls after
--warmup calls, at each resolution R, with the golden SDF weights (f16x3, latent seed 0, bounds [-1, 1]^3):

  field_ms       the lattice field (oi_sdf_lattice, one launch)
  points_ms      the same R^3 points through the existing sdf-only path on materialised points (oi_sdf_mlp_fwd)
  mc_ms          marching cubes alone on the field (oi_mc_count + its totals copy + oi_mc_emit)
  extract_ms     NeuSRenderer.extract_geometry as a whole (field, marching cubes, mesh to the host, world scaling)
  attr0_ms / attr2_ms   the vertex pass of the intrinsic mesh (mesh.vertex_attributes) on the device
                 mesh with refine = 0 / 2; attr2_vs_extract = attr2_ms / extract_ms; flagged = flagged vertices at refine = 2;
                 residual_before / residual_after = median |sdf| / |grad| at the marching-cubes vertices / after two steps"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, ROOT + "/object-intrinsics_amd"):
    sys.path.insert(0, p)
import torch  # noqa: E402

from oi_amd import mesh  # noqa: E402
from oi_amd.autograd import sdf_mlp  # noqa: E402
from oi_amd.fields import ShapeNetwork, ColorNetwork, SingleVarianceNetwork  # noqa: E402
from oi_amd.renderer import NeuSRenderer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--res", default="128,256,512")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=10)
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


kw = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)
net = ShapeNetwork(os.path.join(ROOT, "tests", "golden", "weights_sdf.npz"), **kw).cuda()
r = NeuSRenderer(None, net, SingleVarianceNetwork(0.3).cuda(), ColorNetwork(**kw).cuda(), 16, 16, 0, 1, 0)
z = torch.randn(1, 64, generator=torch.Generator().manual_seed(0)).cuda()
bmin, bmax = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
out = {"tool": "bench_mesh", "precision": "f16x3", "iters": args.iters, "warmup": args.warmup, "res": {}}
with torch.no_grad():
    _, gamma, beta = r.pack.film(z=z)
    for R in (int(x) for x in args.res.split(",")):
        u = mesh.sdf_lattice(r.pack, bmin, bmax, R, z=z, scale=-1.0)[0]
        xs = torch.linspace(-1.0, 1.0, R, device="cuda")
        xx, yy, zz = torch.meshgrid(xs, xs, xs, indexing="ij")
        pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1).contiguous()
        del xx, yy, zz
        row = {
            "field_ms": median_ms(lambda: mesh.sdf_lattice(r.pack, bmin, bmax, R, z=z, scale=-1.0)),
            "points_ms": median_ms(lambda: sdf_mlp(r.pack, pts, gamma, beta, 1, False, False, False)),
            "mc_ms": median_ms(lambda: mesh.marching_cubes(u, 0.0)),
            "extract_ms": median_ms(lambda: r.extract_geometry(bmin, bmax, R, 0.0, z=z)),
        }
        v, t = mesh.marching_cubes(u, 0.0)
        row["attr0_ms"] = median_ms(lambda: mesh.vertex_attributes(r.pack, v, bmin, bmax, R, z=z, refine=0))
        row["attr2_ms"] = median_ms(lambda: mesh.vertex_attributes(r.pack, v, bmin, bmax, R, z=z, refine=2))
        m = mesh.vertex_attributes(r.pack, v, bmin, bmax, R, z=z, refine=2)
        row.update(attr2_vs_extract=row["attr2_ms"] / row["extract_ms"], flagged=int((m.flags != 0).sum()),
                   residual_before=float(m.residual[0].median()), residual_after=float(m.residual[-1].median()))
        del m
        row.update(n_vertices=int(v.shape[0]), n_triangles=int(t.shape[0]),
                   field_vs_points=row["field_ms"] / row["points_ms"], mc_vs_field=row["mc_ms"] / row["field_ms"])
        out["res"][str(R)] = {k: ((round(x, 4) if abs(x) >= 0.01 else float(f"{x:.4g}")) if isinstance(x, float) else x) for k, x in row.items()}
        del pts, u, v, t
        torch.cuda.empty_cache()
print(json.dumps(out))
