#!/usr/bin/env python3
"""Mesh extraction timings on one GPU, one JSON line.  HIP-event medians over --iters calls after
--warmup calls, at each resolution R, with the golden SDF weights (f16x3, latent seed 0, bounds [-1, 1]^3):

  field_ms       the lattice field (oi_sdf_lattice, one launch)
  points_ms      the same R^3 points through the existing sdf-only path on materialised points (oi_sdf_mlp_fwd)
  mc_ms          marching cubes alone on the field (oi_mc_count + its totals copy + oi_mc_emit)
  extract_ms     NeuSRenderer.extract_geometry as a whole (field, marching cubes, mesh to the host, world scaling)
  attr0_ms / attr2_ms   the vertex pass of the intrinsic mesh (mesh.vertex_attributes) on the device
                 mesh with refine = 0 / 2; attr2_vs_extract = attr2_ms / extract_ms; flagged = flagged vertices at refine = 2;
                 residual_before / residual_after = median |sdf| / |grad| at the marching-cubes vertices / after two steps

--band: the narrow band instead, per resolution (default 128,256,512,1024) and block size 4 and 8, dense
and band timed in the same session:
  field_dense_ms / field_band_ms       sdf_lattice / sdf_lattice_band (coarse pass + classification + band launch + read-back)
  coarse_ms                            the dense kernel on the coarse lattice alone
  extract_dense_ms / extract_band_ms   NeuSRenderer.extract_geometry(band=False / True)
  intrinsic_dense_ms / intrinsic_band_ms   mesh.extract_intrinsic_mesh(refine=2, band=False / True)
  active_fraction (of the blocks), evaluated_fraction a (active-block points / lattice points), points_evaluated, n_triangles,
  identical (vertices, triangles and records byte-identical), bar_ms = 1.5 (a field_dense_ms + coarse_ms), bar_met

--texture [--texel T]: the textured export instead, per resolution (default 64,128), both timed in the
same session:
  intrinsic_ms / textured_ms   mesh.extract_intrinsic_mesh(refine=2) / mesh.extract_textured_mesh(refine=2, texel=T)
  bake_ms                      mesh.bake_textures alone on the extracted mesh; full_pass_ms: one full MLP pass (sdf, gradient,
                               albedo) over as many points as the atlas has texels; bake_ms_per_mtexel / full_pass_ms_per_mtexel
  n_triangles, n_texels (F n_T), atlas = [W, H], flagged texels"""
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
ap.add_argument("--res", default=None)
ap.add_argument("--band", action="store_true")
ap.add_argument("--texture", action="store_true")
ap.add_argument("--texel", type=int, default=8)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
if args.res is None:
    args.res = "128,256,512,1024" if args.band else "64,128" if args.texture else "128,256,512"


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
if args.band:
    out["band"] = {}
    with torch.no_grad():
        for R in (int(x) for x in args.res.split(",")):
            dense = {"field_dense_ms": median_ms(lambda: mesh.sdf_lattice(r.pack, bmin, bmax, R, z=z, scale=-1.0)),
                     "extract_dense_ms": median_ms(lambda: r.extract_geometry(bmin, bmax, R, 0.0, z=z)),
                     "intrinsic_dense_ms": median_ms(lambda: mesh.extract_intrinsic_mesh(r, z=z, resolution=R, refine=2))}
            v0, t0 = r.extract_geometry(bmin, bmax, R, 0.0, z=z)
            m0 = mesh.extract_intrinsic_mesh(r, z=z, resolution=R, refine=2, want_record=True)
            for block in (4, 8):
                nb = (R + block - 1) // block
                row = dict(dense)
                row["field_band_ms"] = median_ms(lambda: mesh.sdf_lattice_band(r.pack, bmin, bmax, R, 0.0, z=z, scale=-1.0, block=block))
                row["coarse_ms"] = median_ms(lambda: mesh.sdf_lattice(r.pack, bmin, bmax, max(nb, 2), z=z, scale=-1.0))
                row["extract_band_ms"] = median_ms(lambda: r.extract_geometry(bmin, bmax, R, 0.0, z=z, band=True, block=block))
                row["intrinsic_band_ms"] = median_ms(lambda: mesh.extract_intrinsic_mesh(r, z=z, resolution=R, refine=2, band=True, block=block))
                _, info = mesh.sdf_lattice_band(r.pack, bmin, bmax, R, 0.0, z=z, scale=-1.0, block=block)
                v1, t1 = r.extract_geometry(bmin, bmax, R, 0.0, z=z, band=True, block=block)
                m1 = mesh.extract_intrinsic_mesh(r, z=z, resolution=R, refine=2, want_record=True, band=True, block=block)
                a = info.active_blocks * block ** 3 / float(R) ** 3
                row.update(active_fraction=info.active_fraction, evaluated_fraction=a, points_evaluated=info.points_evaluated,
                           max_slope=info.max_slope, n_triangles=int(t0.shape[0]),
                           identical=bool(v0.tobytes() == v1.tobytes() and t0.tobytes() == t1.tobytes() and
                                          torch.equal(m0.record, m1.record) and torch.equal(m0.triangles, m1.triangles)),
                           bar_ms=1.5 * (a * row["field_dense_ms"] + row["coarse_ms"]))
                row["bar_met"] = bool(row["field_band_ms"] <= row["bar_ms"])
                out["band"].setdefault(str(R), {})[str(block)] = {k: (round(x, 4) if isinstance(x, float) else x) for k, x in row.items()}
                del m1, v1, t1
            del m0, v0, t0
            torch.cuda.empty_cache()
    print(json.dumps(out))
    sys.exit(0)

if args.texture:
    from oi_amd.fields import LatentField  # noqa: E402
    out.update(texture={}, texel=args.texel)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    with torch.no_grad():
        for R in (int(x) for x in args.res.split(",")):
            m = mesh.extract_intrinsic_mesh(r, z=z, resolution=R, refine=2)
            tm = mesh.bake_textures(r.pack, m, *box, R, z=z, texel=args.texel)
            n = tm.texel_flags.numel()
            fld = LatentField(r.pack, z, None, "bench_mesh").prepare(z, None)
            pts = torch.rand(n, 3, device="cuda") * 2 - 1
            row = {"intrinsic_ms": median_ms(lambda: mesh.extract_intrinsic_mesh(r, z=z, resolution=R, refine=2)),
                   "textured_ms": median_ms(lambda: mesh.extract_textured_mesh(r, z=z, resolution=R, refine=2, texel=args.texel)),
                   "bake_ms": median_ms(lambda: mesh.bake_textures(r.pack, m, *box, R, z=z, texel=args.texel)),
                   "full_pass_ms": median_ms(lambda: fld.full(pts))}
            row.update(bake_ms_per_mtexel=row["bake_ms"] / n * 1e6, full_pass_ms_per_mtexel=row["full_pass_ms"] / n * 1e6,
                       n_triangles=int(m.triangles.shape[0]), n_texels=n, atlas=list(tm.size),
                       flagged=int((tm.texel_flags != 0).sum()))
            out["texture"][str(R)] = {k: (round(x, 4) if isinstance(x, float) else x) for k, x in row.items()}
            del m, tm, pts
            torch.cuda.empty_cache()
    print(json.dumps(out))
    sys.exit(0)

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
