"""Inference driver of the path: camera walks, latent walks and light walks at a resolution / depth multiple of the
training configuration, rendered in ray chunks (the second caller of Generator.forward in the reference:
scripts/test.py:231-244, 274-281; src/utils/test.py:55-66, 131-155).  Returns frame tensors; writing
mp4/html is the reference's visualisation stack and out of scope."""
import math

import numpy as np
import torch

from . import generator as G


def scale_config(gen_kwargs, cfg_resolution, test_resolution=None, depth_multiplier=None):
    """update_config of the reference (src/utils/test.py:55-66): multiply n_samples / n_importance, set resolution.
    `gen_kwargs` is the generator's kwargs dict (mutated copy returned)."""
    import copy
    kw = copy.deepcopy(gen_kwargs)
    if depth_multiplier is not None:
        r = kw["renderer"]["kwargs"]
        r["n_importance"] = r["n_importance"] * depth_multiplier
        r["n_samples"] = r["n_samples"] * depth_multiplier
    if test_resolution is not None:
        ratio = test_resolution / cfg_resolution
        kw["resolution"] = int(cfg_resolution * ratio)
        kw["scene_resolution"] = int(kw["scene_resolution"] * ratio)
        kw["camera"]["kwargs"]["resolution"] = kw["scene_resolution"]
    return kw


def slerp(a, b, t):
    """Spherical interpolation of latent codes (src/utils/slerp.py)."""
    an, bn = a / a.norm(dim=-1, keepdim=True), b / b.norm(dim=-1, keepdim=True)
    omega = torch.acos((an * bn).sum(-1, keepdim=True).clamp(-1, 1))
    so = torch.sin(omega)
    return torch.where(so.abs() < 1e-6, (1 - t) * a + t * b, torch.sin((1 - t) * omega) / so * a + torch.sin(t * omega) / so * b)


def rotation_walk(b2w0, n_frames, axis=(0.0, -1.0, 0.0)):
    """b2w poses rotating the object about `axis` through 360 degrees (camera walk of scripts/test.py:231-244)."""
    from scipy.spatial.transform import Rotation as R
    out = []
    ax = np.asarray(axis, dtype=np.float64)
    for i in range(n_frames):
        rot = R.from_rotvec(ax * (2 * math.pi * i / n_frames)).as_matrix()
        m = b2w0.clone()
        m[:3, :3] = b2w0[:3, :3] @ torch.tensor(rot, dtype=torch.float32)
        out.append(m)
    return torch.stack(out)


@torch.no_grad()
def render_frames(gen, zs, b2ws, keys=("image", "mask", "normal_map", "shading_map"), max_ray_batch=None, graphed=False):
    """One frame per (z, b2w) pair, eval mode (perturb off, multi-chunk allowed: generator.py:286-305).
    graphed=True replays one captured hipGraph per frame (oi_amd.graphed.GraphedForward; background fixed to black)."""
    gen.eval()
    gen.renderer.pack.check()  # inf / NaN weights (a broken checkpoint) are reported here, once, not as NaN frames
    if graphed:
        from .graphed import GraphedForward
        old = G.MAX_RAY_BATCH_SIZE
        if max_ray_batch is not None:
            G.MAX_RAY_BATCH_SIZE = max_ray_batch
        try:
            gf = GraphedForward(gen, bs=1, it=gen.iteration(), return_raw=True, keys=keys).recapture()
            dev = gen.it.device
            frames = {k: [] for k in keys}
            for z, b2w in zip(zs, b2ws):
                out = gf(b2w[None].to(dev), z[None].to(dev))
                for k in keys:
                    frames[k].append(out[k][0].clone())
            return {k: torch.stack(v) for k, v in frames.items()}
        finally:
            G.MAX_RAY_BATCH_SIZE = old
    old = G.MAX_RAY_BATCH_SIZE
    if max_ray_batch is not None:
        G.MAX_RAY_BATCH_SIZE = max_ray_batch
    try:
        frames = {k: [] for k in keys}
        dev = gen.it.device
        for z, b2w in zip(zs, b2ws):
            blob = gen(bs=1, it=None, data={"z": z[None].to(dev), "b2w": b2w[None].to(dev)}, return_raw=True)["box"]
            for k in keys:
                frames[k].append(blob["render_out"][k][0])
        return {k: torch.stack(v) for k, v in frames.items()}
    finally:
        G.MAX_RAY_BATCH_SIZE = old


def camera_walk(gen, z, b2w0, n_frames=128, **kw):
    return render_frames(gen, [z] * n_frames, rotation_walk(b2w0, n_frames), **kw)


def latent_walk(gen, z0, z1, b2w, n_frames=128, **kw):
    ts = torch.linspace(0, 1, n_frames)
    return render_frames(gen, [slerp(z0, z1, t) for t in ts], [b2w] * n_frames, **kw)


def light_walk_directions(direction, n_frames, axis=(0.0, -1.0, 0.0)):
    """Unit world-frame light directions turning through 360 degrees about `axis` (rotation_walk's axis convention), frame 0
    = direction / |direction|.  -> (n_frames, 3) float64 numpy."""
    from scipy.spatial.transform import Rotation as R
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    d = d / np.linalg.norm(d)
    ax = np.asarray(axis, dtype=np.float64)
    return np.stack([R.from_rotvec(ax * (2 * math.pi * i / n_frames)).as_matrix() @ d for i in range(n_frames)])


def _frames(cap, out, keys, n):
    """relight's (L, 1, C, H, W) maps and the capture's light-independent maps -> render_frames' {key: (n, C, H, W)}."""
    frames = {}
    for k in keys:
        frames[k] = out[k][:, 0] if k in out else cap.maps[k][0].expand(n, *cap.maps[k].shape[1:])
    return frames


def relight_frames(gen, z, b2w, lights, keys=("image", "mask", "normal_map", "shading_map"), bg=None, max_ray_batch=None):
    """One view (z (z_dim,), b2w (4, 4)) under each of `lights` (oi_amd.relight.Light): one capture, then relight launches
    instead of a render per light.  -> {key: (len(lights), C, H, W)}, as render_frames; the light-independent keys
    (oi_amd.relight.CAPTURE_MAP_KEYS) are the capture's maps, the same for every frame."""
    from . import relight as RL
    cap = RL.capture(gen, z=z[None], b2w=b2w[None], bg=bg, max_ray_batch=max_ray_batch)
    lights = list(lights)
    unknown = [k for k in keys if k not in RL.MAP_KEYS and k not in RL.CAPTURE_MAP_KEYS]
    if unknown:
        raise ValueError(f"relight_frames: keys {unknown} are neither relit maps {RL.MAP_KEYS} nor capture maps "
                         f"{RL.CAPTURE_MAP_KEYS}")
    out = RL.relight(cap, lights, outputs=tuple(k for k in keys if k in RL.MAP_KEYS))
    return _frames(cap, out, keys, len(lights))


def light_walk(gen, z, b2w, n_frames=128, axis=(0, -1, 0), **kw):
    """The light walk of scripts/test.py:256-258, whose function the reference never shipped: the trained light's direction
    turns through 360 degrees about `axis` (rotation_walk's convention) while the view stays; colours and shininess stay
    the trained ones.  Frame 0 is the trained light itself.  One capture, then one relight launch per 256 frames.
    -> {key: (n_frames, C, H, W)} as render_frames (keyword arguments: relight_frames')."""
    from .relight import Light
    base = Light.from_module(gen.light)
    dirs = light_walk_directions(base.direction, n_frames, axis)
    lights = [base] + [base.replace(direction=tuple(d)) for d in dirs[1:]]
    return relight_frames(gen, z, b2w, lights, **kw)


SURFACE_KEYS = ("image", "depth", "position", "normal_map", "normal_object", "albedo", "mask", "visibility", "ambient_occlusion")
AA_KEYS = ("coverage", "aa_mask")   # with aa_samples > 1

# Bytes of device memory per ray of one secondary (shadow / ambient-occlusion) trace: the arrays of an ops.TraceState (rays_o
# 12, rays_d 12, near 4, far 4, t 4, status 1, steps 2, bracket 16, side 1, active 2 x 4, points 12 = 76), the sdf buffer of
# the loop (4) and oi_trace_finish's outputs (hit_index 4, hit_points 12, hit_slot 4).
TRACE_BYTES_PER_RAY = 76 + 4 + 20
# Rays one secondary trace of a light walk may hold: a budget of 2 GiB of device memory for its working set -- small beside
# the card's HBM, and large enough that a 128-frame walk at 128^2 with 16 samples per light (7 M rays) is one trace -- and
# below oi_trace_state's 2^31 rays.
OCCLUSION_MAX_RAYS = min((2 << 30) // TRACE_BYTES_PER_RAY, (1 << 31) - 1)


@torch.no_grad()
def surface_frames(gen, zs, b2ws, keys=("image", "mask", "normal_map", "depth"), lights=None, shadows=False, bg=None, batch=1,
                   aa_samples=1, aa_adaptive=True, aa_plane=0.5, aa_cos=0.5, aa_pattern=None, batch_secondary=False,
                   max_secondary_rays=None, **kw):
    """render_frames by ray / surface intersection (oi_amd.trace.render_surface) instead of the volume render: one frame per
    (z, b2w) pair under ONE light (`lights`: a Light, default the trained one).  -> {key: (n, C, H, W)} for keys of
    SURFACE_KEYS ("visibility" needs shadows=True, "ambient_occlusion" ao_samples > 0).  Keyword arguments: render_surface's
    (bias, tol, omega, max_steps; shadow_samples, light_radius, ao_samples, ao_distance, seed).
    batch: frames per primary trace, 1 .. 1024.  1: one render_surface per frame.  E > 1: the frames go through
    oi_amd.trace.render_surfaces in groups of E (the last group may be smaller) -- one chain of trace steps and one full MLP
    pass per group instead of per frame; shadow and occlusion rays are still traced per frame.  The
    frames are those of batch=1.
    batch_secondary=True (with batch > 1): each group's shadow rays, occlusion rays and shade go through ONE
    chain each as well (render_surfaces' keyword, as max_secondary_rays, the cap on the rays of one such chain); the frames are
    the same, bit for bit.
    aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern: render_surface's anti-aliasing, with the keys
    "coverage" and "aa_mask"; it is per view, so aa_samples > 1 needs batch=1."""
    from . import lib, trace
    from .relight import Light
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or not 1 <= int(batch) <= lib.TRACE_BATCH_MAX_ELEMS:
        raise ValueError(f"surface_frames: batch={batch!r} (an integer, 1 <= batch <= {lib.TRACE_BATCH_MAX_ELEMS})")
    trace._check_batch_secondary(batch_secondary, max_secondary_rays, "surface_frames")
    if batch_secondary and batch == 1:
        raise ValueError("surface_frames: batch_secondary=True with batch=1 (the secondary rays are batched over the views of one "
                         "primary trace: batch > 1)")
    aa = trace._check_aa(aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern, "surface_frames")
    if aa is not None and batch > 1:
        raise ValueError(f"surface_frames: aa_samples={aa_samples!r} with batch={batch!r} (the batched trace has no anti-aliasing "
                         "stage: batch=1)")
    if aa is not None:
        kw.update(aa_samples=aa_samples, aa_adaptive=aa_adaptive, aa_plane=aa_plane, aa_cos=aa_cos, aa_pattern=aa_pattern)
    unknown = [k for k in keys if k not in SURFACE_KEYS + (AA_KEYS if aa is not None else ())]
    if unknown or ("visibility" in keys and not shadows):
        raise ValueError(f"surface_frames: keys {unknown or ['visibility']} (one of {SURFACE_KEYS}; visibility with shadows=True)")
    if "ambient_occlusion" in keys and not kw.get("ao_samples", 0):
        raise ValueError("surface_frames: keys ['ambient_occlusion'] need ao_samples > 0")
    if lights is not None and not isinstance(lights, Light):
        raise TypeError("surface_frames: one Light per walk (surface_light_walk varies the light)")
    gen.eval()
    gen.renderer.pack.check()
    frames = {k: [] for k in keys}
    if batch > 1:
        pairs = list(zip(zs, b2ws))
        for a in range(0, len(pairs), int(batch)):
            group = pairs[a:a + int(batch)]
            for out in trace.render_surfaces(gen, [z for z, _ in group], [b for _, b in group], lights=lights, shadows=shadows,
                                             bg=bg, batch_secondary=bool(batch_secondary),
                                             max_secondary_rays=max_secondary_rays, **kw):
                for k in keys:
                    frames[k].append(out[k][0])
        return {k: torch.stack(v) for k, v in frames.items()}
    for z, b2w in zip(zs, b2ws):
        out = trace.render_surface(gen, z, b2w, lights=lights, shadows=shadows, bg=bg, **kw)
        for k in keys:
            frames[k].append(out[k][0])
    return {k: torch.stack(v) for k, v in frames.items()}


def _walk_surface(gen, lt, what, traced, shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed):
    """The prologue of the four light walks, after their lights are stacked (lt): eval mode, the weights checked, the
    occlusion keywords checked for lt, then ONE trace, traced() -> the surface (a trace._Surface or a scene.SceneSurface).
    -> (the surface, trace._checked_occlusion's tuple)."""
    from . import trace
    gen.eval()
    gen.renderer.pack.check()
    occlusion = trace._checked_occlusion(shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed, lt, what)
    return traced(), occlusion


def _walk_lights(gen, n_frames, axis):
    """The trained light turning through 360 degrees about `axis`, frame 0 the light itself: -> (n_frames, 16) on the
    generator's device."""
    from .relight import Light, stack_lights
    base = Light.from_module(gen.light)
    dirs = light_walk_directions(base.direction, n_frames, axis)
    return stack_lights([base] + [base.replace(direction=tuple(d)) for d in dirs[1:]], gen.it.device)


def _scene_walk(gen, zs, b2ws, what, lights, shadows, bg, bias, window, max_shadow_rays, shadow_samples, light_radius, ao_samples,
                ao_distance, seed, aa, ground, kw):
    """scene_light_walk and scene_light_orbit but for their lights: lights() -> (the stacked lights, the result's own keys).
    The lights are split so that one shadow batch holds at most max_shadow_rays rays, counted per light as instances x the
    largest count of points among the scene, its sub-samples and its ground x the rays per light and point."""
    from . import lib, scene, trace
    scene.check_ground_keyword(ground, trace._check_aa(*aa, what), what)
    lt, extra = lights()
    limit = scene.MAX_SHADOW_RAYS if max_shadow_rays is None else int(max_shadow_rays)
    s, occlusion = _walk_surface(gen, lt, what,
                                 lambda: scene.trace_scene(gen, zs, b2ws, window, trace.DEFAULT_BIAS if bias is None else bias, *aa, **kw),
                                 shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed)
    gs = None if ground is None else s.ground(ground)
    radii, _, samples = occlusion[:3]
    per_light = samples if radii is not None or trace._is_local(lt) else 1
    # (one light above the limit is traced in chunks of samples; one sample above it is refused, naming the count)
    step = limit // max(1, s.E * _most_points(s, gs) * per_light) if shadows else lib.RELIGHT_MAX_LIGHTS
    return _light_walk(s, lt, occlusion, step, bg, limit, gs, **extra)


def _most_points(s, gs=None):
    """The largest count of visible points among the surface, its sub-sample surface and its ground: what bounds a shadow
    trace's rays per light."""
    return max(s.n_points, s.sub.n_points if s.sub is not None else 0, gs.n_g if gs is not None else 0)


def _light_walk(s, lt, occlusion, step, bg, limit=None, ground=None, **extra):
    """The frames of a light walk or orbit over the traced surface s (a trace._Surface or a scene.SceneSurface; trace._Stages)
    under the stacked lights lt, and the dict the four walks return.  The ambient occlusion is traced once; per `step` lights
    (at most 256) one shadow trace and one shade launch, which writes its frames in place.  With an anti-aliasing stage the
    sub-sample surface s.sub, traced once with s, passes the same stages per chunk and s.resolve writes the frames.
    limit: the cap on the rays of one shadow batch of a scene.  ground (a scene.GroundSurface): the plane
    blocks the scene's ambient and directional rays, its own ambient occlusion is traced once, its shadows per chunk of
    lights, and oi_ground_shade writes it into each chunk's frames (no anti-aliasing stage with a ground: the shaded planes
    are views of the walk's frames)."""
    from . import lib, trace
    radii, shadows, samples, ao_samples, ao_distance, seed = occlusion
    n, dev, M, H = lt.shape[0], lt.device, s.n_pixels, s.side
    bgv, gkw = trace._bg(bg, dev), {} if ground is None else {"ground": ground}
    keep = tuple(k for k in ("depth", "mask", "instance") if k in s.OUTPUTS)
    image = torch.empty(n, 3, M, device=dev)
    vis_all = torch.empty(n, M, device=dev) if shadows else None
    matte = torch.empty(n, 3, M, device=dev) if ground is not None else None
    ambient = lambda surface, **kw: surface.ambient(ao_samples, ao_distance, seed, limit, **kw) if ao_samples and surface is not None else None
    ao, g_ao, ao_sub = ambient(s, **gkw), ambient(ground), ambient(s.sub)
    maps = coverage = None
    step = max(1, min(lib.RELIGHT_MAX_LIGHTS, step))
    for a in range(0, n, step):
        b = min(n, a + step)
        visible = lambda surface, **kw: surface.light_visibility(lt[a:b], None if radii is None else radii[a:b], samples, seed, limit,
                                                                 **kw) if shadows and surface is not None else None
        vis = visible(s, **gkw)
        if shadows:
            vis_all[a:b] = vis
        first = maps is None
        out = s._shade(lt[a:b], bgv, vis, keep + ("image",) if first else ("image",), image[a:b] if s.aa is None else None, ao)
        maps = maps or out
        if ground is not None:
            ground_mask, matte[a:b] = ground.shade(out, lt[a:b], visible(ground), g_ao)
        if s.aa is not None:
            _, cov = s.resolve(lt[a:b], bgv, {"image": out["image"], "mask": maps["mask"]}, visible(s.sub), ao_sub, image_out=image[a:b],
                               want_mask=first)
            coverage = cov if first else coverage
    res = {"image": image.view(n, 3, H, H), **{k: maps[k].view(1, 1, H, H) for k in keep}, **extra, "stats": s.stats()}
    if shadows:
        res["visibility"] = vis_all.view(n, 1, H, H)
    if ao_samples:
        res["ambient_occlusion"] = ao.view(1, 1, H, H)
    if s.aa is not None:
        res["coverage"], res["aa_mask"] = coverage.view(1, 1, H, H), (s.edge_slot >= 0).float().view(1, 1, H, H)
    if ground is not None:
        res["ground_mask"], res["shadow_matte"] = ground_mask.view(1, 1, H, H), matte.view(n, 3, H, H)
        for st in res["stats"]:
            st.update(ground_pixels=ground.n_g, ground_evals=ground.evals)
    return res


@torch.no_grad()
def surface_light_walk(gen, z, b2w, n_frames=128, axis=(0, -1, 0), shadows=True, bg=None, bias=None, shadow_samples=1,
                       light_radius=0.0, ao_samples=0, ao_distance=0.5, seed=0, aa_samples=1, aa_adaptive=True, aa_plane=0.5,
                       aa_cos=0.5, aa_pattern=None, **kw):
    """light_walk on the traced surface, with cast shadows: ONE primary trace and ONE full MLP pass at its hits for the whole
    walk, one shadow trace and one shade launch per 256 lights.  Frame 0 is the trained light.  -> {"image": (n_frames, 3,
    H, W), "visibility": (n_frames, 1, H, W) when shadows, "mask" / "depth" (1, 1, H, W), "stats"}.
    shadow_samples, light_radius (a scalar or one value per frame), ao_samples, ao_distance, seed: render_surface's.  Soft shadows trace
    shadow_samples rays per light and visible point, so the lights are split further until one trace holds at most
    OCCLUSION_MAX_RAYS rays; the frames do not depend on the split (rays are independent, the samples keyed on pixel and seed).
    Ambient occlusion does not depend on the light: ONE trace for the walk, returned as "ambient_occlusion" (1, 1, H, W).
    aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern: render_surface's anti-aliasing.  The sub-samples
    are traced ONCE for the walk, then shaded and resolved per chunk of lights; "coverage" and "aa_mask" (1, 1, H, W) are returned
    too, and stats gains aa_pixels, aa_rays, aa_evals."""
    from . import lib, trace
    aa = trace._check_aa(aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern, "surface_light_walk")
    dev, lt = gen.it.device, _walk_lights(gen, n_frames, axis)
    s, occlusion = _walk_surface(gen, lt, "surface_light_walk",
                                 lambda: trace._Surface(gen, z.to(dev).reshape(1, -1), b2w, trace.DEFAULT_BIAS if bias is None else bias, kw, aa=aa),
                                 shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed)
    radii, _, samples = occlusion[:3]   # (radii None, hard shadows: one ray per light and hit, 256 lights per trace)
    step = OCCLUSION_MAX_RAYS // (samples * max(1, _most_points(s))) if radii is not None else lib.RELIGHT_MAX_LIGHTS
    return _light_walk(s, lt, occlusion, step, bg)


@torch.no_grad()
def scene_light_walk(gen, zs, b2ws, n_frames=128, axis=(0, -1, 0), shadows=True, bg=None, bias=None, window=None,
                     max_shadow_rays=None, shadow_samples=1, light_radius=0.0, ao_samples=0, ao_distance=0.5, seed=0, aa_samples=1,
                     aa_adaptive=True, aa_plane=0.5, aa_cos=0.5, aa_pattern=None, ground=None, **kw):
    """surface_light_walk on a scene of K instances (oi_amd.scene): the scene is traced ONCE -- one batched
    march, one depth resolve, one full MLP pass at the visible hits -- and shaded under the walk of lights, each instance
    shadowing itself and the others.  Frame 0 is the trained light.  The lights are split so that one shadow batch holds at
    most max_shadow_rays rays (default oi_amd.scene.MAX_SHADOW_RAYS), counted as K * lights * visible points, and at most 256
    lights; the frames do not depend on the split (rays are independent).  -> {"image": (n_frames, 3, S, S), "visibility":
    (n_frames, 1, S, S) when shadows, "mask" / "depth" / "instance" (1, 1, S, S), "stats"}.
    shadow_samples, light_radius (a scalar or one value per frame), ao_samples, ao_distance, seed: SceneSurface.shade's soft
    shadows and ambient occlusion between the instances; a light whose samples do not fit one batch is
    traced in chunks of samples.  Ambient occlusion does not depend on the light: ONE trace for the walk, returned as
    "ambient_occlusion" (1, 1, S, S).  kw: tol, omega, max_steps, readback of sphere_trace.
    aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern: trace_scene's anti-aliasing.  The sub-samples
    are traced ONCE for the walk, then shaded and resolved per chunk of lights; "coverage" and "aa_mask" (1, 1, S, S) are
    returned too, and stats gains aa_pixels, aa_rays, aa_evals.
    ground (a scene.Ground; not with aa_samples > 1): SceneSurface.shade's ground plane in every frame.  Its
    ambient occlusion is traced ONCE, its shadows per chunk of lights; "ground_mask" (1, 1, S, S) and "shadow_matte" (n_frames,
    3, S, S) are returned too, and stats gains ground_pixels and ground_evals."""
    return _scene_walk(gen, zs, b2ws, "scene_light_walk", lambda: (_walk_lights(gen, n_frames, axis), {}), shadows, bg, bias, window,
                       max_shadow_rays, shadow_samples, light_radius, ao_samples, ao_distance, seed,
                       (aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern), ground, kw)


def light_orbit_positions(centre, radius, n_frames, axis=(0.0, -1.0, 0.0), height=0.0):
    """World-frame positions of a local light on one closed circle of `radius` about the line through `centre` along `axis`
    (rotation_walk's axis convention), in the plane `height` along the unit axis from `centre`.  Frame 0 stands towards the
    world axis that is least aligned with `axis`, made perpendicular to it.  -> (n_frames, 3) float64 numpy."""
    from scipy.spatial.transform import Rotation as R
    c, ax = np.asarray(centre, dtype=np.float64).reshape(3), np.asarray(axis, dtype=np.float64).reshape(3)
    if not (np.isfinite(c).all() and np.isfinite(ax).all() and np.linalg.norm(ax) > 0 and math.isfinite(float(radius))
            and float(radius) > 0 and math.isfinite(float(height))):
        raise ValueError(f"light_orbit_positions: centre={centre!r}, radius={radius!r}, axis={axis!r}, height={height!r} (finite, a "
                         "non-zero axis, radius > 0)")
    if isinstance(n_frames, bool) or not isinstance(n_frames, (int, np.integer)) or int(n_frames) < 1:
        raise ValueError(f"light_orbit_positions: n_frames={n_frames!r} (a positive integer)")
    ax = ax / np.linalg.norm(ax)
    start = np.eye(3)[int(np.argmin(np.abs(ax)))]
    start = start - (start @ ax) * ax
    start = start / np.linalg.norm(start)
    return np.stack([c + float(height) * ax + float(radius) * (R.from_rotvec(ax * (2 * math.pi * i / int(n_frames))).as_matrix() @ start)
                     for i in range(int(n_frames))])


def _orbit_lights(gen, light, n_frames, centre, radius, axis, height, what):
    """The LocalLight `light` at each of light_orbit_positions' positions.  -> (the lights, stacked (n_frames, 20) on the
    generator's device; the orbits' own result key: positions)."""
    from .relight import LocalLight, stack_local_lights
    if not isinstance(light, LocalLight):
        raise TypeError(f"{what}: light must be a LocalLight (surface_light_walk turns a directional light)")
    pos = light_orbit_positions(centre, radius, n_frames, axis, height)
    return stack_local_lights([light.replace(position=tuple(p)) for p in pos], gen.it.device), {"positions": pos}


@torch.no_grad()
def surface_light_orbit(gen, z, b2w, light, n_frames=128, centre=(0.0, 0.0, 0.0), radius=1.5, axis=(0, -1, 0), height=0.0,
                        shadows=True, bg=None, bias=None, shadow_samples=1, ao_samples=0, ao_distance=0.5, seed=0, aa_samples=1,
                        aa_adaptive=True, aa_plane=0.5, aa_cos=0.5, aa_pattern=None, **kw):
    """A local light (oi_amd.relight.LocalLight) carried once round the object while the view stays: ONE
    primary trace and ONE full MLP pass at its hits for the whole orbit, then per 256 positions one trace of shadow rays that
    end at the light and one shade launch.  The positions are light_orbit_positions(centre, radius, n_frames, axis, height) in
    the world frame; everything else about the light stays (a cone keeps its world-frame axis).  The lights are split further
    until one shadow trace holds at most OCCLUSION_MAX_RAYS rays; the frames do not depend on the split.  -> {"image":
    (n_frames, 3, H, W), "visibility": (n_frames, 1, H, W) when shadows, "mask" / "depth" (1, 1, H, W), "positions" (n_frames, 3)
    float64 numpy, "stats"}; with ao_samples also "ambient_occlusion" (1, 1, H, W), ONE trace for the orbit.
    aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern: as surface_light_walk's."""
    from . import lib, trace
    aa = trace._check_aa(aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern, "surface_light_orbit")
    dev = gen.it.device
    lt, extra = _orbit_lights(gen, light, n_frames, centre, radius, axis, height, "surface_light_orbit")
    s, occlusion = _walk_surface(gen, lt, "surface_light_orbit",
                                 lambda: trace._Surface(gen, z.to(dev).reshape(1, -1), b2w, trace.DEFAULT_BIAS if bias is None else bias, kw, aa=aa),
                                 shadows, shadow_samples, 0.0, ao_samples, ao_distance, seed)
    step = OCCLUSION_MAX_RAYS // (occlusion[2] * max(1, _most_points(s))) if shadows else lib.RELIGHT_MAX_LIGHTS   # [2]: shadow_samples
    return _light_walk(s, lt, occlusion, step, bg, **extra)


@torch.no_grad()
def scene_light_orbit(gen, zs, b2ws, light, n_frames=128, centre=(0.0, 0.0, 0.0), radius=1.5, axis=(0, -1, 0), height=0.0,
                      shadows=True, bg=None, bias=None, window=None, max_shadow_rays=None, shadow_samples=1, ao_samples=0,
                      ao_distance=0.5, seed=0, aa_samples=1, aa_adaptive=True, aa_plane=0.5, aa_cos=0.5, aa_pattern=None, ground=None,
                      **kw):
    """surface_light_orbit on a scene of K instances (oi_amd.scene): the scene is traced ONCE and the local light is carried
    round `centre` -- between the instances, if the circle passes there -- each instance shadowing itself and the others as
    far as the light.  The lights are split so that one shadow batch holds at most max_shadow_rays rays (default
    oi_amd.scene.MAX_SHADOW_RAYS), counted as K * lights * shadow_samples * visible points, and at most 256 lights; a light
    whose samples do not fit one batch is traced in chunks of samples.  The frames do not depend on the split.  -> {"image":
    (n_frames, 3, S, S), "visibility": (n_frames, 1, S, S) when shadows, "mask" / "depth" / "instance" (1, 1, S, S),
    "positions", "stats"}; with ao_samples also "ambient_occlusion" (1, 1, S, S).
    aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern, ground: as scene_light_walk's (the ground catches the local light's
    shadows and blocks the instances' ambient rays; it does not block their local-light rays)."""
    lights = lambda: _orbit_lights(gen, light, n_frames, centre, radius, axis, height, "scene_light_orbit")
    return _scene_walk(gen, zs, b2ws, "scene_light_orbit", lights, shadows, bg, bias, window, max_shadow_rays, shadow_samples, 0.0,
                       ao_samples, ao_distance, seed, (aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern), ground, kw)


def env_walk_rotations(n_frames, axis=(0.0, 0.0, 1.0)):
    """World rotations through 360 degrees about `axis` (any non-zero length), frame 0 the identity.  -> n_frames (3, 3)
    float64 arrays."""
    from .envlight import axis_rotation
    if isinstance(n_frames, bool) or not isinstance(n_frames, (int, np.integer)) or n_frames < 1:
        raise ValueError(f"env_walk: n_frames={n_frames!r} (a positive integer)")
    return [axis_rotation(axis, 2 * math.pi * i / n_frames) for i in range(int(n_frames))]


@torch.no_grad()
def env_walk(gen, z, b2w, env, n_frames=128, axis=(0, 0, 1), transfer_samples=64, seed=0, bg=None, bias=None,
             glossy_samples=None, shininess=None, specular=None, bounces=0, **kw):
    """The environment `env` (oi_amd.envlight.EnvLight or EnvMap) turning through 360 degrees about the world `axis` while the
    view stays: ONE capture (oi_amd.trace.capture_transfer: the primary trace, the full MLP pass at its hits and transfer_samples
    secondary rays per visible point), then n_frames rotations of the 9 x 3 coefficients on the host and one shade launch per
    256 frames.  Frame 0 is `env` itself.  -> {"image", "shading": (n_frames, 3, H, W), "transfer": (1, 9, H, W), "mask" /
    "depth" (1, 1, H, W), "stats"}.  An EnvMap takes the glossy path (glossy_samples, shininess: capture_transfer's; specular:
    shade's): the map is prefiltered once, when it is made, and every frame only rotates the lookup; the result also holds
    "specular" (n_frames, 3, H, W) and "spec_visibility".  bounces=1 (an EnvLight only): capture_transfer's one diffuse
    interreflection bounce; the result also holds "indirect" (n_frames, 3, H, W) and "bounce" (1, 3, 9, H, W), and a frame
    costs one dot product more per channel.  Keyword arguments: capture_transfer's (tol, omega, max_steps,
    readback)."""
    from . import trace
    from .envlight import EnvLight, EnvMap
    if not isinstance(env, (EnvLight, EnvMap)):
        raise TypeError(f"env_walk: expected an EnvLight or an EnvMap, got {type(env).__name__}")
    rots = env_walk_rotations(n_frames, axis)
    gen.eval()
    gen.renderer.pack.check()
    cap = trace.capture_transfer(gen, z, b2w, transfer_samples, seed, trace.DEFAULT_BIAS if bias is None else bias, glossy_samples,
                                 shininess, bounces, **kw)
    res = cap.shade([env.rotated(R) for R in rots], bg, specular)
    res.update(transfer=cap.transfer, mask=cap.maps["mask"], depth=cap.maps["depth"], stats=cap.stats())
    if cap.bounce is not None:
        res["bounce"] = cap.bounce
    if cap.glossy_samples is not None:
        res["spec_visibility"] = cap.spec_visibility
    return res


@torch.no_grad()
def scene_env_walk(gen, zs, b2ws, env, n_frames=128, axis=(0, 0, 1), transfer_samples=64, seed=0, bg=None, bias=None, window=None,
                   max_shadow_rays=None, glossy_samples=None, shininess=None, specular=None, bounces=0, ground=None, **kw):
    """env_walk on a scene of K instances (oi_amd.scene): ONE scene trace and ONE capture
    (SceneSurface.capture_transfer: transfer_samples secondary rays per visible point, each tested against every instance),
    then n_frames rotations of the 9 x 3 coefficients on the host and one shade launch per 256 frames.  Frame 0 is `env`
    itself.  -> {"image", "shading": (n_frames, 3, S, S), "transfer": (1, 9, S, S), "mask" / "depth" / "instance" (1, 1, S, S),
    "stats"}.  An EnvMap takes the glossy path (glossy_samples, shininess: capture_transfer's; specular:
    shade's): the map is prefiltered once, when it is made, and every frame only rotates the lookup; the result also holds
    "specular" (n_frames, 3, S, S), "spec_visibility" and "reflection".  bounces=1 (an EnvLight; capture_transfer's rules): one
    diffuse interreflection bounce between the instances, traced once with the capture; the result also
    holds "indirect" (n_frames, 3, S, S) and "bounce" (1, 3, 9, S, S).  kw: tol, omega, max_steps, readback of sphere_trace.
    ground: refused unless None (the environment paths have no ground plane yet)."""
    from .scene import refuse_env_ground
    refuse_env_ground(ground, "scene_env_walk")
    from . import scene, trace
    from .envlight import EnvLight, EnvMap
    if not isinstance(env, (EnvLight, EnvMap)):
        raise TypeError(f"scene_env_walk: expected an EnvLight or an EnvMap, got {type(env).__name__}")
    rots = env_walk_rotations(n_frames, axis)
    samples, _ = trace._check_transfer(transfer_samples, seed, "scene_env_walk")
    trace._check_bounces(bounces, samples, glossy_samples, shininess, "scene_env_walk")
    trace._check_glossy(gen, glossy_samples, shininess, "scene_env_walk")
    gen.eval()
    gen.renderer.pack.check()
    limit = scene.MAX_SHADOW_RAYS if max_shadow_rays is None else int(max_shadow_rays)
    # (the constructor, not trace_scene: the environment paths take no aa_* keyword)
    s = scene.SceneSurface(gen, zs, b2ws, window, trace.DEFAULT_BIAS if bias is None else bias, kw)
    cap = s.capture_transfer(transfer_samples, seed, limit, glossy_samples, shininess, bounces)
    out = cap.shade([env.rotated(R) for R in rots], bg, specular)
    res = {k: out[k] for k in ("image", "shading", "mask", "depth", "instance")}
    res.update(transfer=cap.transfer, stats=cap.scene.stats())
    if cap.bounce is not None:
        res.update(indirect=out["indirect"], bounce=cap.bounce)
    if isinstance(env, EnvMap):
        res.update(specular=out["specular"], spec_visibility=cap.spec_visibility, reflection=cap.reflection)
    return res


@torch.no_grad()
def shade_vertices(positions, normals, albedo, light, eye=None):
    """Phong colour (V, 3) of mesh vertices under `light` (oi_amd.relight.Light; its direction in the mesh's own frame): each
    vertex is a one-sample ray of weight 1 through the relighting launch (oi_relight_fwd with T = 1, one element, identity
    frame, no background).  View direction: towards `eye` (3 floats, the mesh's frame) when given, else along the normal."""
    from . import ops
    from .relight import stack_lights
    V = positions.shape[0]
    dev = positions.device
    if V == 0:
        return torch.empty(0, 3, device=dev)
    if eye is None:
        rays_d, mid_z = -normals, torch.ones(V, 1, device=dev)
        rays_o = positions + normals
    else:
        rays_o = torch.as_tensor(eye, dtype=torch.float32).to(dev).reshape(1, 3).expand(V, 3).contiguous()
        d = positions - rays_o
        mid_z = d.norm(dim=-1, keepdim=True)
        rays_d = d / mid_z.clamp(min=1e-12)
    out = ops.relight_fwd(torch.ones(V, 1, device=dev), normals.view(V, 1, 3), albedo.view(V, 1, 3), mid_z, rays_o, rays_d,
                          torch.eye(4, device=dev)[None], stack_lights(light, dev), None, 1, outputs=("image_no_bg",))
    return out["image_no_bg"][0, 0].t().contiguous()


@torch.no_grad()
def export_mesh(gen, z, path, resolution=256, refine=2, light=None, threshold=0.0, bound_min=(-1.0, -1.0, -1.0),
                bound_max=(1.0, 1.0, 1.0), eye=None, band=False, lipschitz=None, block=None, texture=False, texel=8,
                max_texels=1 << 20):
    """The instance of latent z (z_dim,) or (1, z_dim) as a PLY asset at `path`: triangles, vertices on the surface, analytic
    normals and per-vertex colours (oi_amd.mesh.extract_intrinsic_mesh; save_ply's attribute layout).  Colours are the
    albedo, or with `light` (oi_amd.relight.Light, e.g. Light.from_module(gen.light)) the shaded colour of shade_vertices.
    band=True (lipschitz, block): the field comes from mesh.sdf_lattice_band; the file is the same, the BandInfo is in m.band.
    Checks the weights first (FieldPack.check: an inf / NaN weight is refused before anything is launched).
    -> the IntrinsicMesh that was written (with `shaded` (V, 3) set when a light was given).
    texture=True (texel, max_texels: oi_amd.mesh.extract_textured_mesh's arguments): `path` must end in .obj; the asset is a
    Wavefront OBJ with its .mtl and the baked <stem>_albedo.png and <stem>_normal.png (oi_amd.mesh.save_obj) -- a coarse
    mesh whose texture carries the detail; with `light` the albedo map holds the shaded colour of every texel instead.
    -> the TexturedMesh that was written."""
    from . import mesh, ops
    if texture:
        mesh.obj_file_names(path)                 # ValueError unless it ends in .obj, before anything is launched
        ops.tex_layout(0, texel)                  # and the texel size (host only)
    gen.eval()
    pack = mesh._field_pack(gen, "export_mesh")
    pack.check()
    dev = gen.it.device
    z = z.to(dev).reshape(1, -1)
    if texture:
        shade = None if light is None else (lambda p, n, a: shade_vertices(p, n, a, light, eye))
        tm = mesh.extract_textured_mesh(pack, z=z, resolution=resolution, texel=texel, threshold=threshold,
                                        bound_min=bound_min, bound_max=bound_max, refine=refine, band=band,
                                        lipschitz=lipschitz, block=block, max_texels=max_texels, shade=shade)
        mesh.save_obj(path, tm)
        return tm
    m = mesh.extract_intrinsic_mesh(pack, z=z, resolution=resolution, threshold=threshold, bound_min=bound_min,
                                    bound_max=bound_max, refine=refine, want_record=light is None, band=band,
                                    lipschitz=lipschitz, block=block)
    if light is None:
        record = m.record
    else:
        m.shaded = shade_vertices(m.positions, m.normals, m.albedo, light, eye)
        record = m.record = ops.mesh_vertex_record(m.positions, m.normals, m.shaded) if len(m.positions) else \
            torch.empty(0, mesh.RECORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    mesh.save_ply(path, record, m.triangles)
    return m


MESH_KEYS = ("image", "mask", "normal_map", "normal_object", "depth", "position", "albedo", "triangle", "barycentric")


@torch.no_grad()
def mesh_frames(gen, mesh, b2ws, keys=("image", "mask", "normal_map", "depth"), lights=None, bg=None, batch=16):
    """The camera walk of a FIXED mesh (oi_amd.raster.render_mesh): one frame per pose of b2ws under
    ONE light (`lights`: a Light or LocalLight, default the trained one), `batch` views per raster launch (1 .. 1024).  No
    network is evaluated.  -> what surface_frames returns: {key: (n, C, H, W)} for keys of MESH_KEYS."""
    from . import lib, raster
    from .relight import Light, LocalLight
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or not 1 <= int(batch) <= lib.RASTER_MAX_VIEWS:
        raise ValueError(f"mesh_frames: batch={batch!r} (an integer, 1 <= batch <= {lib.RASTER_MAX_VIEWS})")
    unknown = [k for k in keys if k not in MESH_KEYS]
    if unknown:
        raise ValueError(f"mesh_frames: keys {unknown} (one of {MESH_KEYS})")
    if lights is not None and not isinstance(lights, (Light, LocalLight)):
        raise TypeError("mesh_frames: one Light or LocalLight per walk")
    poses = torch.stack([torch.as_tensor(b).reshape(4, 4) for b in b2ws])
    frames = {k: [] for k in keys}
    for a in range(0, len(poses), int(batch)):
        for out in raster.render_mesh(gen, mesh, poses[a:a + int(batch)], lights=None if lights is None else [lights], bg=bg):
            for k in keys:
                frames[k].append(out[k][0])
    return {k: torch.stack(v) for k, v in frames.items()}


def _psnr(a, b):
    """Peak signal-to-noise ratio in dB of two images with values in [0, 1] (inf when they are equal)."""
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


@torch.no_grad()
def mesh_fidelity(gen, z, mesh, b2ws, lights=None, source=None, **trace_kw):
    """How close the rasterised mesh is to the traced surface it was extracted from, ON THE COMMON MASK (the silhouette is
    mask_iou's; the PSNR figures here exclude it and do not compare with whole-image PSNR): oi_amd.raster.render_mesh against
    oi_amd.trace.render_surface at the same latent z, poses b2ws ((4, 4) or (E, 4, 4)) and lights (no shadows; trace_kw:
    render_surface's tol, omega, max_steps).  -> per view a dict: mask_iou; depth_rms, the RMS difference of the ray
    parameter on the common mask; normal_angle, the mean angle in degrees between the object-space normals there;
    albedo_psnr and image_psnr (the first light's image), both over the pixels of the common mask, so that they measure the
    surface's attributes and not the silhouette, which mask_iou has; common, the pixels of the common mask.  A list of E
    dicts for (E, 4, 4)."""
    from . import raster, trace
    poses = torch.as_tensor(b2ws)
    single = poses.dim() == 2
    poses = poses.reshape(-1, 4, 4)
    got = raster.render_mesh(gen, mesh, poses, lights=lights, source=source)
    out = []
    for b2w, m in zip(poses, got):
        s = trace.render_surface(gen, z, b2w, lights=lights, **trace_kw)
        ma, mb = m["mask"][0, 0] > 0, s["mask"][0, 0] > 0
        both = ma & mb
        n = int(both.sum())
        union = int((ma | mb).sum())
        d = (m["depth"][0, 0][both] - s["depth"][0, 0][both]).double()
        cos = (m["normal_object"][0][:, both] * s["normal_object"][0][:, both]).sum(0).clamp(-1, 1).double()
        out.append({"mask_iou": n / union if union else 1.0,
                    "depth_rms": float((d * d).mean().sqrt()) if n else 0.0,
                    "normal_angle": float(torch.rad2deg(torch.acos(cos)).mean()) if n else 0.0,
                    "albedo_psnr": _psnr(m["albedo"][0][:, both], s["albedo"][0][:, both]) if n else float("inf"),
                    "image_psnr": _psnr(m["image"][0][:, both], s["image"][0][:, both]) if n else float("inf"),
                    "common": n})
    return out[0] if single else out
