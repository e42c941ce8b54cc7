#!/usr/bin/env python3
"""Scene timings on one GPU, one JSON line.  HIP-event medians over --iters calls after --warmup
calls, golden SDF weights, f16x3 by default, K instances from oi_amd.scene.sample_scene at each K of --instances:

  scene_ms / scene_shadows_ms    oi_amd.scene.render_scene without / with shadows: one batched march for all instances, the depth
                                 resolve, the full MLP pass at the visible hits, one shade launch; with shadows one shadow batch of
                                 K occluder elements
  crops_ms / crops_shadows_ms    for comparison, the parent's way of getting the same instances: K calls of
                                 oi_amd.trace.render_surface, each on its own crop of W x W pixels of the same scene image (W: the
                                 scene's window) -- which gives neither occlusion between instances nor mutual shadows
With --shadow-samples / --light-radius / --ao-samples the shadowed rows are the sampled ones of DESIGN section 4.21 (soft shadows
and ambient occlusion between the instances; the crops trace theirs against their own instance alone), and --env adds

  scene_env_ms                   oi_amd.scene.render_scene_env with --transfer-samples rays per visible point, every ray tested
                                 against all K instances, under one constant environment
  crops_env_ms                   K calls of oi_amd.trace.render_surface_env on the crops
No ratio is promised: the two do different work (the scene tests every secondary ray against all K instances).
With --env --glossy the glossy lobe of DESIGN section 4.25 is timed per K beside the diffuse rows of the same run:

  scene_gloss_capture_ms         trace_scene + SceneSurface.capture_transfer with --glossy-samples reflection-lobe rays per
                                 visible point on top of the transfer rays, every ray tested against all K instances
  scene_gloss_shade_ms           SceneTransfer.shade of that capture under one prefiltered 64 x 128 map (one launch)
  scene_gloss_ms                 oi_amd.scene.render_scene_env on the glossy path: the two together
With --env --bounce the interreflection bounce between the instances of DESIGN section 4.26 is timed per K beside the plain capture
of the same run:

  scene_env_capture_ms / scene_env_shade_ms        trace_scene + SceneSurface.capture_transfer, and SceneTransfer.shade of it under one
                                                   environment, without the bounce (what scene_env_ms is made of)
  scene_bounce_capture_ms / scene_bounce_shade_ms  the same with bounces=1: the transfer rays marched to their closest hit, the winner
                                                   of every ray, one padded full MLP pass per chunk, the bounce resolve; the shade with
                                                   the bounce transfer
  scene_bounce_ms                oi_amd.scene.render_scene_env(bounces=1): the two together
  bounce_points / n_pad2         the secondary hits evaluated (over all chunks and instances) and the last chunk's padded row length
--skip-crops leaves out the crops_* rows (K single-view renders each).

With --local [--light-size R] each row also gets scene_local_ms / scene_local_hard_ms /
scene_local_sphere16_ms: render_scene under a local light 3 units from the instances' centroid along the trained light's
direction (no shadows, one hard ray, 16 samples of a sphere of radius R), scene_directional_soft16_ms beside them, and the
sdf evaluations of each shadow trace.

With --aa S [--aa-full] the tool measures ONLY, per K and in one session, the frame of render_scene under
the trained light with one sample per pixel (aa_samples=1: the path without the stage), with S samples in the flagged scene
pixels (adaptive), and -- with --aa-full -- with S samples in every scene pixel (aa_adaptive=False); with each the flagged
pixels, the sub-sample rays per instance, the side Q of their virtual image, their sdf evaluations and the steps of the
second chain.

With --ground each row also gets scene_ground_ms: the shadowed frame (scene_shadows_ms's keywords) with
a ground plane oi_amd.scene.Ground.below the instances' visible points (gap 0.02, a disc of radius --ground-extent about their
centroid), and with it ground_pixels, the ground's secondary rays per frame (ground_rays = K * ground_pixels * (shadow samples +
ambient samples)), ground_evals and ground_share, its share of the frame's sdf evaluations."""
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
from oi_amd.envlight import EnvLight, EnvMap  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=64, help="crop resolution of the generator; the scene image is res * 1588 / 256")
ap.add_argument("--instances", default="1,8,32")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--precision", default="f16x3")
ap.add_argument("--shadow-samples", type=int, default=1, help="rays per light and visible point of the shadowed rows")
ap.add_argument("--light-radius", type=float, default=0.0, help="angular radius of the light in radians")
ap.add_argument("--ao-samples", type=int, default=0, help="ambient-occlusion rays per visible point of the shadowed rows")
ap.add_argument("--env", action="store_true", help="also time environment lighting (scene_env_ms / crops_env_ms)")
ap.add_argument("--transfer-samples", type=int, default=64)
ap.add_argument("--glossy", action="store_true", help="with --env: also time the glossy capture and shade (scene_gloss_*_ms)")
ap.add_argument("--glossy-samples", type=int, default=64, help="reflection-lobe rays per visible point")
ap.add_argument("--shininess", type=float, default=10.0)
ap.add_argument("--bounce", action="store_true", help="with --env: also time the capture and shade with bounces=1 (scene_bounce_*_ms)")
ap.add_argument("--skip-crops", action="store_true", help="leave out the crops_* comparison rows")
ap.add_argument("--local", action="store_true", help="also time a local light (oi_amd.relight.LocalLight) above the scene: scene_local_*_ms")
ap.add_argument("--light-size", type=float, default=0.15, help="with --local: radius of the sphere light of the sampled row")
ap.add_argument("--aa", type=int, default=0, help="samples per flagged scene pixel: time anti-aliased frames beside the one-sample frame, only")
ap.add_argument("--aa-full", action="store_true", help="with --aa: also time aa_adaptive=False (every scene pixel flagged)")
ap.add_argument("--ground", action="store_true", help="also time the shadowed frame with a ground plane below the instances: scene_ground_ms")
ap.add_argument("--ground-extent", type=float, default=8.0, help="with --ground: radius of the plane about the instances' centroid")
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


def aa_rows():
    """Per K: the one-sample frame, the adaptive frame and (--aa-full) the fully supersampled frame."""
    rows = {}
    for K in (int(k) for k in args.instances.split(",")):
        zs, b2ws = scene.sample_scene(gen, K, args.seed)
        cases = {"one_sample": dict(aa_samples=1), "adaptive": dict(aa_samples=args.aa)}
        if args.aa_full:
            cases["full"] = dict(aa_samples=args.aa, aa_adaptive=False)
        row = {}
        for name, kw in cases.items():
            frame = lambda: scene.render_scene(gen, zs, b2ws, **kw)
            row[name + "_ms"] = median_ms(frame)
            res = frame()
            s, st = res["scene"], res["stats"][0]
            if name == "one_sample":
                row.update(window=s.W, rays=K * s.N, visible=sum(s.n_vis), n_evals=st["n_evals"], n_steps=st["n_steps"])
            else:
                sub = s.sub
                row[name] = {"aa_pixels": st["aa_pixels"], "aa_share": st["aa_pixels"] / (s.S * s.S), "aa_rays": st["aa_rays"],
                             "Q": 0 if sub is None else sub.S, "aa_visible": 0 if sub is None else sum(sub.n_vis),
                             "aa_evals": st["aa_evals"], "aa_steps": 0 if sub is None else sub.n_steps,
                             "ms_over_one_sample": row[name + "_ms"] / row["one_sample_ms"]}
        rows[str(K)] = row
    return rows


if args.aa:
    with torch.no_grad():
        print(json.dumps({"tool": "bench_scene", "precision": args.precision, "res": args.res, "scene_resolution": gen.scene_resolution,
                          "iters": args.iters, "warmup": args.warmup, "aa_samples": args.aa, "aa": aa_rows()}))
    sys.exit(0)

out = {"tool": "bench_scene", "precision": args.precision, "res": args.res, "scene_resolution": gen.scene_resolution,
       "iters": args.iters, "warmup": args.warmup, "shadow_samples": args.shadow_samples, "light_radius": args.light_radius,
       "ao_samples": args.ao_samples, "transfer_samples": args.transfer_samples if args.env else None,
       "glossy_samples": args.glossy_samples if args.env and args.glossy else None, "bounce": bool(args.env and args.bounce),
       "instances": {}}
soft = dict(shadow_samples=args.shadow_samples, light_radius=args.light_radius, ao_samples=args.ao_samples)
envs = [EnvLight.constant(1.0)]
if (args.glossy or args.bounce) and not args.env:
    ap.error("--glossy and --bounce need --env")
if args.env and args.glossy:   # a sky brighter towards +z, prefiltered once
    rows = torch.linspace(2.0, 0.2, 64)[None, :, None].expand(3, 64, 128)
    maps = [EnvMap.from_equirect(rows.contiguous(), args.shininess, size=(64, 128))]
    gloss = dict(transfer_samples=args.transfer_samples, glossy_samples=args.glossy_samples, shininess=args.shininess)
with torch.no_grad():
    for K in (int(k) for k in args.instances.split(",")):
        zs, b2ws = scene.sample_scene(gen, K, args.seed)
        s = scene.trace_scene(gen, zs, b2ws)
        crop = copy.copy(gen)            # the same camera and scene image, a crop of W x W pixels per instance
        crop.resolution = s.W

        def crops(shadows):
            for z, b2w in zip(zs, b2ws):
                trace.render_surface(crop, z, b2w, shadows=shadows, **(soft if shadows else {}))

        def crops_env():
            for z, b2w in zip(zs, b2ws):
                trace.render_surface_env(crop, z, b2w, envs, transfer_samples=args.transfer_samples)

        row = {"window": s.W, "rays": K * s.N, "entered": sum(s.n_entered), "hits": sum(s.n_hit), "visible": sum(s.n_vis)}
        for name, shadows in (("", False), ("_shadows", True)):
            kw = soft if shadows else {}
            row["scene" + name + "_ms"] = median_ms(lambda: scene.render_scene(gen, zs, b2ws, shadows=shadows, **kw))
            if not args.skip_crops:
                row["crops" + name + "_ms"] = median_ms(lambda: crops(shadows))
        if args.ground:
            pts = s.world_points()[0]
            ground = scene.Ground.below(pts, (0.0, -1.0, 0.0), gap=0.02, extent=args.ground_extent,
                                        centre=tuple(float(x) for x in pts.mean(0)))
            frame = lambda: scene.render_scene(gen, zs, b2ws, shadows=True, ground=ground, **soft)
            row["scene_ground_ms"] = median_ms(frame)
            st = frame()["stats"][0]
            evals = st["n_evals"] + st["shadow_evals"] + st["occlusion_evals"] + st["ground_evals"]
            row.update(ground_pixels=st["ground_pixels"], ground_rays=K * st["ground_pixels"] * (args.shadow_samples + args.ao_samples),
                       ground_evals=st["ground_evals"], ground_share=st["ground_evals"] / max(1, evals))
        if args.env:
            row["scene_env_ms"] = median_ms(lambda: scene.render_scene_env(gen, zs, b2ws, envs, transfer_samples=args.transfer_samples))
            if not args.skip_crops:
                row["crops_env_ms"] = median_ms(crops_env)
        if args.env and args.glossy:
            capture = lambda: scene.trace_scene(gen, zs, b2ws).capture_transfer(args.transfer_samples, 0, scene.MAX_SHADOW_RAYS,
                                                                                 args.glossy_samples, args.shininess)
            cap = capture()
            row["scene_gloss_capture_ms"] = median_ms(capture)
            row["scene_gloss_shade_ms"] = median_ms(lambda: cap.shade(maps))
            row["scene_gloss_ms"] = median_ms(lambda: scene.render_scene_env(gen, zs, b2ws, maps, **gloss))
        if args.env and args.bounce:
            for name, b in (("env", 0), ("bounce", 1)):
                capture = lambda: scene.trace_scene(gen, zs, b2ws).capture_transfer(args.transfer_samples, 0, scene.MAX_SHADOW_RAYS, bounces=b)
                cap = capture()
                row[f"scene_{name}_capture_ms"] = median_ms(capture)
                row[f"scene_{name}_shade_ms"] = median_ms(lambda: cap.shade(envs))
            row["scene_bounce_ms"] = median_ms(lambda: scene.render_scene_env(gen, zs, b2ws, envs, transfer_samples=args.transfer_samples,
                                                                             bounces=1))
            row["bounce_points"] = cap.scene.bounce_points
            row["n_pad2"] = cap.scene.bounce_hits["n_pad2"] if cap.scene.bounce_hits else 0
        if args.local:   # beside the directional rows: no shadows, one hard ray, 16 samples of a light with a size
            from oi_amd.relight import Light, LocalLight
            base = Light.from_module(gen.light)
            centre = tuple(float(x) for x in b2ws[:, :3, 3].mean(0))
            point = LocalLight.from_light(base, 3.0, centre)
            cases = {"directional_soft16": dict(lights=[base], shadows=True, shadow_samples=16, light_radius=0.1),
                     "local": dict(lights=[point]), "local_hard": dict(lights=[point], shadows=True),
                     "local_sphere16": dict(lights=[point.replace(radius=args.light_size)], shadows=True, shadow_samples=16)}
            for name, kw in cases.items():
                row[f"scene_{name}_ms"] = median_ms(lambda: scene.render_scene(gen, zs, b2ws, **kw))
                row[f"scene_{name}_shadow_evals"] = scene.render_scene(gen, zs, b2ws, **kw)["stats"][0]["shadow_evals"]
            row["scene_directional_hard_shadow_evals"] = scene.render_scene(gen, zs, b2ws, shadows=True)["stats"][0]["shadow_evals"]
        out["instances"][str(K)] = row
print(json.dumps(out))
