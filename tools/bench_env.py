#!/usr/bin/env python3
"""Environment-lighting timings on one GPU, one JSON line.  HIP-event medians over --iters calls after
--warmup calls, golden SDF weights, one latent and pose at --res:

  capture_ms            oi_amd.trace.capture_transfer at each S of --samples: the primary trace, the full MLP pass at its hits,
                        S secondary rays per visible point through the any-hit loop, the resolve and the G-buffer;
                        transfer_evals: the sdf evaluations of the secondary trace
  shade_ms              TransferCapture.shade at each F of --envs (a capture at the last S): per launch and per frame
  project_ms            EnvLight.from_equirect of a --map He x We radiance map (the kernel, the upload and the read-back)
  light_walk_ms         for comparison, the existing inference.surface_light_walk(shadows=False, ao_samples=S) at
                        --walk-frames frames, per frame, same session: a directional light per frame, scalar ambient occlusion
  env_walk_ms           inference.env_walk at the same S and frame count, per frame (the capture included)

With --glossy only the glossy path is timed:

  prefilter_ms          oi_amd.ops.env_prefilter of a --map He x We radiance map to --glossy-size at --shininess (the two
                        kernels, the map already on the device), and EnvMap.from_equirect (projection and upload included)
  capture_ms            capture_transfer(transfer_samples=64, glossy_samples=G) at G of --glossy-samples; glossy_evals: the sdf
                        evaluations of the reflection-lobe trace
  shade_ms              TransferCapture.shade under F rotations of one EnvMap at each F of --envs: per launch and per frame

With --bounce only the interreflection bounce is timed, each figure beside its counterpart without:

  capture_ms            capture_transfer at each S of --samples with bounces=0 and with bounces=1 (the closest-hit march of the
                        transfer rays, the full MLP pass at their hits, oi_bounce_resolve); bounce_points: those hits
  shade_ms              TransferCapture.shade at each F of --envs on a plain capture (oi_env_shade) and on a bounce capture
                        (oi_env_shade_bounce) at the last S: per launch and per frame"""
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
from oi_amd.envlight import EnvLight, EnvMap  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=128)
ap.add_argument("--samples", default="16,64,256")
ap.add_argument("--envs", default="1,64,256")
ap.add_argument("--walk-frames", type=int, default=128)
ap.add_argument("--map", default="256x512")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--precision", default="f16x3")
ap.add_argument("--glossy", action="store_true")
ap.add_argument("--glossy-size", default="64x128")
ap.add_argument("--glossy-samples", default="16,64")
ap.add_argument("--shininess", type=float, default=10.0)
ap.add_argument("--bounce", action="store_true")
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


gen, _ = build_models(args.res, 256, 64, 1, args.precision, "cuda")
gen.eval()
z = torch.randn(64, generator=torch.Generator().manual_seed(0))
np.random.seed(0)
b2w = torch.tensor(gen.pose_prior(1), dtype=torch.float32)[0]
rs = np.random.RandomState(0)
env = EnvLight(rs.randn(9, 3) * 0.3 + np.eye(9)[0][:, None] * 3.0)
samples, n_envs, n = [int(s) for s in args.samples.split(",")], [int(f) for f in args.envs.split(",")], args.walk_frames
He, We = (int(v) for v in args.map.split("x"))

out = {"tool": "bench_env", "precision": args.precision, "res": args.res, "iters": args.iters, "warmup": args.warmup,
       "capture": {}, "shade": {}, "walk": {}}
if args.glossy:
    from oi_amd import ops
    size = tuple(int(v) for v in args.glossy_size.split("x"))
    out.update(glossy=True, shininess=args.shininess)
    del out["walk"]
    with torch.no_grad():
        img = torch.rand(3, He, We, generator=torch.Generator().manual_seed(1))
        dev_img = img.cuda()[None].contiguous()
        out["prefilter"] = {"map": args.map, "size": args.glossy_size,
                            "prefilter_ms": median_ms(lambda: ops.env_prefilter(dev_img, args.shininess, size)),
                            "from_equirect_ms": median_ms(lambda: EnvMap.from_equirect(img, args.shininess, size))}
        emap = EnvMap.from_equirect(img, args.shininess, size)
        cap = None
        for G in (int(g) for g in args.glossy_samples.split(",")):
            kw = dict(transfer_samples=64, glossy_samples=G, shininess=args.shininess)
            cap = trace.capture_transfer(gen, z, b2w, **kw)
            st = cap.stats()
            out["capture"][str(G)] = {"capture_ms": median_ms(lambda: trace.capture_transfer(gen, z, b2w, **kw)), "hits": st["hit"],
                                      "rays": G * st["hit"], "glossy_evals": st["glossy_evals"], "transfer_evals": st["transfer_evals"]}
        for F in n_envs:
            envs = [emap.rotated(R) for R in inference.env_walk_rotations(F)]
            ms = median_ms(lambda: cap.shade(envs, specular=0.3))
            out["shade"][str(F)] = {"shade_ms": ms, "per_frame_ms": ms / F}
    print(json.dumps(out))
    sys.exit(0)
if args.bounce:
    out.update(bounce=True)
    del out["walk"]
    with torch.no_grad():
        caps = {}
        for S in samples:
            row = {}
            for nb in (0, 1):
                caps[nb] = trace.capture_transfer(gen, z, b2w, transfer_samples=S, bounces=nb)
                st = caps[nb].stats()
                row["bounces=%d" % nb] = {
                    "capture_ms": median_ms(lambda: trace.capture_transfer(gen, z, b2w, transfer_samples=S, bounces=nb)),
                    "hits": st["hit"], "rays": S * st["hit"], "transfer_evals": st["transfer_evals"],
                    "bounce_points": st["bounce_points"]}
            out["capture"][str(S)] = row
        for F in n_envs:
            envs = [env.rotated(R) for R in inference.env_walk_rotations(F)]
            row = {}
            for nb in (0, 1):
                ms = median_ms(lambda: caps[nb].shade(envs))
                row["bounces=%d" % nb] = {"shade_ms": ms, "per_frame_ms": ms / F}
            out["shade"][str(F)] = row
    print(json.dumps(out))
    sys.exit(0)
with torch.no_grad():
    cap = None
    for S in samples:
        cap = trace.capture_transfer(gen, z, b2w, transfer_samples=S)
        st = cap.stats()
        out["capture"][str(S)] = {"capture_ms": median_ms(lambda: trace.capture_transfer(gen, z, b2w, transfer_samples=S)),
                                  "hits": st["hit"], "rays": S * st["hit"], "transfer_evals": st["transfer_evals"],
                                  "primary_evals": st["n_evals"]}
    out["capture"]["0"] = {"capture_ms": median_ms(lambda: trace.capture_transfer(gen, z, b2w, transfer_samples=0))}
    for F in n_envs:
        envs = [env.rotated(R) for R in inference.env_walk_rotations(F)]
        ms = median_ms(lambda: cap.shade(envs))
        out["shade"][str(F)] = {"shade_ms": ms, "per_frame_ms": ms / F}
    img = torch.rand(3, He, We, generator=torch.Generator().manual_seed(1))
    out["project"] = {"map": args.map, "project_ms": median_ms(lambda: EnvLight.from_equirect(img))}
    for S in samples:
        walk = median_ms(lambda: inference.surface_light_walk(gen, z, b2w, n_frames=n, shadows=False, ao_samples=S), iters=5)
        soft = median_ms(lambda: inference.surface_light_walk(gen, z, b2w, n_frames=n, shadows=True, shadow_samples=S,
                                                              light_radius=0.1), iters=3) if S <= 16 else None
        ew = median_ms(lambda: inference.env_walk(gen, z, b2w, env, n_frames=n, transfer_samples=S), iters=5)
        out["walk"][str(S)] = {"frames": n, "light_walk_ao_ms_per_frame": walk / n, "env_walk_ms_per_frame": ew / n,
                               "light_walk_soft_shadow_ms_per_frame": None if soft is None else soft / n}
print(json.dumps(out))
