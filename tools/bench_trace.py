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
and, at --walk-res, the 128-frame light walk: surface_light_walk with and without shadows against inference.light_walk.

With --shadow-samples S > 1 / --light-radius r > 0 / --ao-samples A > 0 each resolution also gets

  soft                  ms per frame of soft shadows alone, ambient occlusion alone and both together, the secondary rays
                        and their LIMIT share, and the sdf evaluations per traced secondary ray through the any-hit step
                        against the full step on the same rays (count read every step)
and the light walk a row with the soft settings.

With --batch E[,E...] the tool measures ONLY the batched walk: --walk-frames frames at --walk-res, a
latent walk between two seeded latents under as many sampled poses, through inference.surface_frames(batch=E) against the
same call's unchanged per-frame loop (batch=1) in the same session, without and with cast shadows:

  loop_ms / batch_ms    ms per frame;   speedup  their ratio
  evals_per_ray         sdf evaluations per primary ray (the stale and the shared bounds included)
  n_pad_over_mean_hit   points per element of the padded full pass over the mean hit count;  padding_waste  its unread share

With --batch E[,E...] --batch-secondary the tool measures ONLY, per E and in one session, the walk through
inference.surface_frames(batch=E) WITH secondary rays -- the --shadow-samples / --light-radius / --ao-samples given, one hard
shadow ray without them -- once with the per-view chains (batch_secondary=False) and once with one chain per stage
(batch_secondary=True), --iters walks after --warmup each:

  loop_ms / batched_ms  ms per frame;   speedup  their ratio;   frames_equal  the two walks' frames, bit for bit
  calls_per_frame       calls into the library per frame, both ways (a begin entry is two launches, every other entry one)
  padding               E * n_pad / sum_e n_hit_e over the walk's groups: the hit slots the shared chains carry per real hit
  shadow_evals, ao_evals  sdf evaluations of the secondary chains per frame, both ways

With --local [--light-size R] [--light-distance D] the tool measures ONLY, per resolution, the frame under
the trained directional light and under a local light (oi_amd.relight.LocalLight) D along the same direction from the object's
centre: no shadows, one hard shadow ray, and 16 samples of a light with a size (angular radius 0.1 / a sphere of radius R),
each with the sdf evaluations of its shadow trace.

With --aa S [--aa-full] the tool measures ONLY, per resolution and in one session, the frame of
render_surface under the trained light with one sample per pixel (aa_samples=1: the path without the stage), with S samples in
the flagged pixels (adaptive), and -- with --aa-full -- with S samples in every pixel (aa_adaptive=False); with each the flagged
pixels, the sub-sample rays, their sdf evaluations and the steps of the second chain."""
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
ap.add_argument("--shadow-samples", type=int, default=1, help="shadow rays per light and visible point")
ap.add_argument("--light-radius", type=float, default=0.0, help="angular radius of the light, radians")
ap.add_argument("--ao-samples", type=int, default=0, help="ambient-occlusion rays per visible point (0: none)")
ap.add_argument("--batch", default="", help="frames per batched primary trace, e.g. 16,128: measure only the batched walk")
ap.add_argument("--batch-secondary", action="store_true", help="with --batch: time the walk with secondary rays, per-view chains against one chain per stage, only")
ap.add_argument("--local", action="store_true", help="time local lights (oi_amd.relight.LocalLight) beside the directional path, only")
ap.add_argument("--light-size", type=float, default=0.15, help="with --local: radius of the sphere light of the sampled row")
ap.add_argument("--light-distance", type=float, default=2.0, help="with --local: distance of the local light from the object's centre")
ap.add_argument("--aa", type=int, default=0, help="samples per flagged pixel: time anti-aliased frames beside the one-sample frame, only")
ap.add_argument("--aa-full", action="store_true", help="with --aa: also time aa_adaptive=False (every pixel flagged)")
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


SOFT = args.shadow_samples > 1 or args.light_radius > 0
SOFT_KW = dict(shadows=True, shadow_samples=args.shadow_samples, light_radius=args.light_radius) if SOFT else {}
AO_KW = dict(ao_samples=args.ao_samples) if args.ao_samples else {}


def secondary(gen, z, b2w):
    """Per secondary trace of one frame: rays, traced rays, LIMIT share, evaluations per traced ray any-hit / full."""
    from oi_amd import lib, ops
    from oi_amd.relight import Light, stack_lights
    s = trace._Surface(gen, z.cuda().reshape(1, -1), b2w, trace.DEFAULT_BIAS, {})
    tol, omega, max_steps, _ = s.kw
    lt = stack_lights(Light.from_module(gen.light), "cuda")
    begins = {}
    if SOFT:
        radius = torch.full((1,), args.light_radius, device="cuda")
        begins["shadow"] = (args.shadow_samples, lambda st: ops.occlusion_light_begin(
            st, s.res.hit_points, s.grad, s.res.hit_index, s.n_hit, lt, radius, args.shadow_samples, s.w2b, s.bias, 0))
    if args.ao_samples:
        begins["ao"] = (args.ao_samples, lambda st: ops.occlusion_ambient_begin(
            st, s.res.hit_points, s.grad, s.res.hit_index, s.n_hit, args.ao_samples, s.bias, 0.5, 0))
    rows = {}
    for name, (S, begin) in begins.items():
        row = {"rays": S * s.n_hit}
        for anyhit in (True, False):
            st = ops.TraceState(S * s.n_hit, ref=s.ro)
            begin(st)
            traced = int(st.counts[0].item())
            n_evals, _ = trace._march(s.field, st, traced, tol, omega, max_steps, 1, anyhit=anyhit)
            ops.trace_finish(st)
            row["traced"] = traced
            row["evals_per_ray_anyhit" if anyhit else "evals_per_ray_full"] = n_evals / max(1, traced)
            if anyhit:
                row["limit_share"] = int((st.status == lib.TRACE_LIMIT).sum()) / max(1, traced)
        rows[name] = row
    return rows


def batched_walk():
    gen, _, _ = setup(args.walk_res)
    n, N = args.walk_frames, args.walk_res ** 2
    g = torch.Generator().manual_seed(0)
    z0, z1 = torch.randn(64, generator=g), torch.randn(64, generator=g)
    zs = [torch.lerp(z0, z1, i / max(1, n - 1)) for i in range(n)]
    np.random.seed(0)
    b2ws = list(torch.tensor(gen.pose_prior(n), dtype=torch.float32))
    keys = ("image", "mask", "normal_map", "depth")
    frames = lambda E, sh: inference.surface_frames(gen, zs, b2ws, keys=keys, shadows=sh, batch=E)
    row = {"res": args.walk_res, "frames": n, "batch": {}}
    loop = {sh: median_ms(lambda: frames(1, sh), iters=5) / n for sh in (False, True)}
    row["loop_ms"], row["loop_shadow_ms"] = loop[False], loop[True]
    row["loop_evals_per_ray"] = float(np.mean([trace.render_surface(gen, z, b)["stats"]["n_evals"] for z, b in zip(zs, b2ws)])) / N
    ref = frames(1, False)
    for E in (int(e) for e in args.batch.split(",")):
        r = {sh: median_ms(lambda: frames(E, sh), iters=5) / n for sh in (False, True)}
        got = frames(E, False)
        same = all(bool(((got[k] == ref[k]) | (got[k].isnan() & ref[k].isnan())).all()) for k in keys)
        evals, pad, hits = 0, 0, 0
        for a in range(0, n, E):
            res = trace.render_surfaces(gen, zs[a:a + E], b2ws[a:a + E])
            t0 = res[0]["trace"]
            evals += t0.n_evals * len(res)                       # every element of a group carries the group's bounds
            pad += len(res) * max(len(o["trace"].hit_index) for o in res)
            hits += sum(len(o["trace"].hit_index) for o in res)
        row["batch"][str(E)] = {"batch_ms": r[False], "batch_shadow_ms": r[True], "speedup": loop[False] / r[False],
                                "speedup_shadow": loop[True] / r[True], "evals_per_ray": evals / (n * N),
                                "n_pad_over_mean_hit": pad / max(1, hits), "padding_waste": 1.0 - hits / max(1, pad),
                                "frames_equal_loop": same}
    return row


def batched_secondary_walk():
    """Per E of --batch: the walk with secondary rays through surface_frames(batch=E), per-view chains against one chain per
    stage, in one session."""
    from oi_amd import lib
    gen, _, _ = setup(args.walk_res)
    n = args.walk_frames
    g = torch.Generator().manual_seed(0)
    z0, z1 = torch.randn(64, generator=g), torch.randn(64, generator=g)
    zs = [torch.lerp(z0, z1, i / max(1, n - 1)) for i in range(n)]
    np.random.seed(0)
    b2ws = list(torch.tensor(gen.pose_prior(n), dtype=torch.float32))
    sec = dict(SOFT_KW or {"shadows": True}, **AO_KW)
    keys = ("image", "mask", "normal_map", "depth", "visibility") + (("ambient_occlusion",) if AO_KW else ())
    frames = lambda E, flag: inference.surface_frames(gen, zs, b2ws, keys=keys, batch=E, batch_secondary=flag, **sec)
    L = lib.load()
    entries = [name for table in lib.SIGS.values() for name in table]

    def calls(fn):
        """Calls into the library during fn(): every entry of the binding table counted on the handle, then put back."""
        count, real = [0], {name: getattr(L, name) for name in entries}

        def counted(f):
            def call(*a):
                count[0] += 1
                return f(*a)
            return call
        for name, f in real.items():
            setattr(L, name, counted(f))
        try:
            fn()
        finally:
            for name, f in real.items():
                setattr(L, name, f)
        return count[0]

    row = {"res": args.walk_res, "frames": n, "secondary": {k: v for k, v in sec.items()}, "batch": {}}
    for E in (int(e) for e in args.batch.split(",")):
        ms = {flag: median_ms(lambda: frames(E, flag)) / n for flag in (False, True)}
        a, b = frames(E, False), frames(E, True)
        same = all(bool(((a[k] == b[k]) | (a[k].isnan() & b[k].isnan())).all()) for k in keys)
        pad = hits = 0
        evals = {False: [0, 0], True: [0, 0]}
        for i in range(0, n, E):
            for flag in (False, True):
                res = trace.render_surfaces(gen, zs[i:i + E], b2ws[i:i + E], batch_secondary=flag, **sec)
                evals[flag][0] += sum(o["stats"]["shadow_evals"] for o in res)
                evals[flag][1] += sum(o["stats"]["ao_evals"] for o in res)
            pad += len(res) * max(len(o["trace"].hit_index) for o in res)
            hits += sum(len(o["trace"].hit_index) for o in res)
        row["batch"][str(E)] = {"loop_ms": ms[False], "batched_ms": ms[True], "speedup": ms[False] / ms[True], "frames_equal": same,
                                "calls_per_frame": {"loop": calls(lambda: frames(E, False)) / n, "batched": calls(lambda: frames(E, True)) / n},
                                "padding": pad / max(1, hits),
                                "shadow_evals": {"loop": evals[False][0] / n, "batched": evals[True][0] / n},
                                "ao_evals": {"loop": evals[False][1] / n, "batched": evals[True][1] / n}}
    return row


def local_rows():
    """Per resolution: the frame under the trained directional light and under a local light at --light-distance along the same
    direction -- no shadows, one hard shadow ray, 16 samples of a light with a size (angular radius 0.1 / sphere radius
    --light-size) -- and the sdf evaluations of each shadow trace."""
    from oi_amd.relight import Light, LocalLight
    rows = {}
    for R in (int(r) for r in args.res.split(",")):
        gen, z, b2w = setup(R)
        base = Light.from_module(gen.light)
        point = LocalLight.from_light(base, args.light_distance, tuple(float(x) for x in b2w[:3, 3]))
        cases = {"directional": dict(lights=[base]), "directional_hard": dict(lights=[base], shadows=True),
                 "directional_soft16": dict(lights=[base], shadows=True, shadow_samples=16, light_radius=0.1),
                 "local": dict(lights=[point]), "local_hard": dict(lights=[point], shadows=True),
                 "local_sphere16": dict(lights=[point.replace(radius=args.light_size)], shadows=True, shadow_samples=16)}
        row = {"rays": R * R}
        for name, kw in cases.items():
            row[name + "_ms"] = median_ms(lambda: trace.render_surface(gen, z, b2w, **kw))
            st = trace.render_surface(gen, z, b2w, **kw)["stats"]
            row[name + "_shadow_evals"] = st["shadow_evals"]
        row["hits"] = st["hit"]
        rows[str(R)] = row
        del gen
    return rows


def aa_rows():
    """Per resolution: the one-sample frame, the adaptive frame and (--aa-full) the fully supersampled frame."""
    rows = {}
    for R in (int(r) for r in args.res.split(",")):
        gen, z, b2w = setup(R)
        cases = {"one_sample": dict(aa_samples=1), "adaptive": dict(aa_samples=args.aa)}
        if args.aa_full:
            cases["full"] = dict(aa_samples=args.aa, aa_adaptive=False)
        row = {"rays": R * R}
        for name, kw in cases.items():
            row[name + "_ms"] = median_ms(lambda: trace.render_surface(gen, z, b2w, **kw))
            out = trace.render_surface(gen, z, b2w, **kw)
            st = out["stats"]
            row["n_evals"], row["n_steps"] = st["n_evals"], st["n_steps"]
            if name != "one_sample":
                sub = out["aa_trace"]
                row[name] = {"aa_pixels": st["aa_pixels"], "aa_share": st["aa_pixels"] / (R * R), "aa_rays": st["aa_rays"],
                             "aa_evals": st["aa_evals"], "aa_steps": 0 if sub is None else sub.n_steps,
                             "ms_over_one_sample": row[name + "_ms"] / row["one_sample_ms"]}
        rows[str(R)] = row
        del gen
    return rows


if args.aa:
    with torch.no_grad():
        print(json.dumps({"tool": "bench_trace", "precision": args.precision, "iters": args.iters, "warmup": args.warmup,
                          "aa_samples": args.aa, "aa": aa_rows()}))
    sys.exit(0)

if args.local:
    with torch.no_grad():
        print(json.dumps({"tool": "bench_trace", "precision": args.precision, "iters": args.iters, "warmup": args.warmup,
                          "light_size": args.light_size, "light_distance": args.light_distance, "local": local_rows()}))
    sys.exit(0)

if args.batch and args.batch_secondary:
    with torch.no_grad():
        print(json.dumps({"tool": "bench_trace", "precision": args.precision, "iters": args.iters, "warmup": args.warmup,
                          "batched_secondary_walk": batched_secondary_walk()}))
    sys.exit(0)

if args.batch:
    with torch.no_grad():
        print(json.dumps({"tool": "bench_trace", "precision": args.precision, "warmup": args.warmup, "batched_walk": batched_walk()}))
    sys.exit(0)

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
        if SOFT or AO_KW:
            soft = {"shadow_samples": args.shadow_samples, "light_radius": args.light_radius, "ao_samples": args.ao_samples}
            if SOFT:
                soft["soft_shadow_ms"] = median_ms(lambda: trace.render_surface(gen, z, b2w, **SOFT_KW))
            if AO_KW:
                soft["ao_ms"] = median_ms(lambda: trace.render_surface(gen, z, b2w, **AO_KW))
            if SOFT and AO_KW:
                soft["soft_shadow_ao_ms"] = median_ms(lambda: trace.render_surface(gen, z, b2w, **SOFT_KW, **AO_KW))
            soft["stats"] = trace.render_surface(gen, z, b2w, **SOFT_KW, **AO_KW)["stats"]
            soft["secondary"] = secondary(gen, z, b2w)
            row["soft"] = soft
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
    if SOFT or AO_KW:
        out["light_walk"]["soft_ms"] = median_ms(lambda: inference.surface_light_walk(gen, z, b2w, n_frames=n, **SOFT_KW, **AO_KW), iters=5)
        out["light_walk"]["soft_stats"] = inference.surface_light_walk(gen, z, b2w, n_frames=n, **SOFT_KW, **AO_KW)["stats"]
print(json.dumps(out))
