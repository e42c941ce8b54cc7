"""Sphere-traced surface rendering on the MI355X (include/oi_trace.h; oi_amd.trace.sphere_trace / render_surface;
oi_amd.inference.surface_frames / surface_light_walk).  The reference is always the fp64 CPU oracle (oracle/oi_oracle.py
through tests/helpers/trace_ref.py) on the golden weights and the seeded latents 0, 1, 2, evaluated AT WHAT THE LIBRARY
RETURNS (its hit points, its shadow-ray origins); the caps come from the rehearsal of tests/test_trace_cpu.py on the oracle
alone, for the same views and lights."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_modules as M
from conftest import load_golden, record_margin, sub_sd
from helpers import mesh_attr_ref as A
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

SDF_BAR = 1e-4      # F1: sdf parity
RGB_BAR = 2e-5      # F2: albedo parity
RELIGHT_BAR = 2e-6  # oi_relight_fwd's bar
PRECISIONS = ["f16x3", "f32"]

_GEN, _VIEW = {}, {}


def make_gen(precision, R=T.R_VIEW):
    if (precision, R) not in _GEN:
        g = load_golden("f5_generator")
        gen = M.build_generator(R, 16, 16, 1, precision).eval()
        gen.color_network.load_state_dict(load_golden("weights_color"))   # the oracle's colour head (helpers.mesh_attr_ref)
        gen.light.load_state_dict(sub_sd(g, "light."))
        with torch.no_grad():
            gen.light.param_specular.fill_(0.35)
            gen.light.param_shininess.fill_(6.0)
        _GEN[(precision, R)] = gen
    return _GEN[(precision, R)]


def lights():
    from oi_amd.relight import Light
    return [Light(direction=d, specular=0.35, shininess=6.0) for d in T.LIGHT_DIRS]


def npd(t):
    return t.detach().cpu().double().numpy()


def run_view(precision, seed, pose):
    """One view through render_surface with shadows under the three test lights; cached per (precision, seed, pose)."""
    key = (precision, seed, pose)
    if key not in _VIEW:
        from oi_amd import trace
        gen = make_gen(precision)
        b2w = T.pose(pose)
        out = trace.render_surface(gen, A.latent(seed)[0], b2w, lights=lights(), shadows=True)
        ro, rd, near, far, w2b = trace._view_rays(gen, b2w)
        _VIEW[key] = dict(out=out, ro=npd(ro), rd=npd(rd), near=npd(near), far=npd(far), w2b=npd(w2b), fld=T.Field(seed), gen=gen,
                          b2w=b2w, ro_t=ro, rd_t=rd, w2b_t=w2b)
    return _VIEW[key]


VIEW_PARAMS = [pytest.param(p, s, q, id=f"{p}-seed{s}-{q}") for p in PRECISIONS for s, q in T.VIEWS]


@pytest.mark.parametrize("precision,seed,pose", VIEW_PARAMS)
def test_primary_rays(precision, seed, pose):
    """Hits lie on the oracle's surface and are the first crossing, misses are misses, the caps of the rehearsal hold, and the
    cost in evaluations is within 2x of the oracle tracer's for the same rays."""
    v = run_view(precision, seed, pose)
    res, fld = v["out"]["trace"], v["fld"]
    t, status, N = npd(res.t), res.status.cpu().numpy(), len(v["ro"])
    hit, miss = status == T.HIT, status == T.MISS
    case = f"trace_primary[{precision},seed={seed},{pose}]"
    on = np.abs(fld.sdf(v["ro"][hit] + t[hit, None] * v["rd"][hit]))
    before = T.segment_min(fld.sdf, v["ro"][hit], v["rd"][hit], v["near"][hit], t[hit] - T.SEGMENT_BACKOFF)
    along = T.segment_min(fld.sdf, v["ro"][miss], v["rd"][miss], v["near"][miss], v["far"][miss])
    t_ref, s_ref, _, in_flight = T.trace(fld.sdf, v["ro"], v["rd"], v["near"], v["far"])
    both = hit & (s_ref == T.HIT)
    stats = {"hit_sdf_worst": float(on.max()), "hit_earlier_min": float(before.min()), "miss_min": float(along.min(initial=np.inf)),
             "status_disagreements": int((status != s_ref).sum()), "t_vs_oracle_trace": float(np.abs(t - t_ref)[both].max()),
             "evals_per_ray": res.n_evals / N, "oracle_evals_per_ray": sum(in_flight) / N}
    for k, val in stats.items():
        record_margin(case, k, val if np.isfinite(val) else 0.0)
    cnt = v["out"]["stats"]
    print(case, stats, cnt)
    assert on.max() <= T.TOL + SDF_BAR
    assert before.min() >= -SDF_BAR and along.min(initial=np.inf) >= -SDF_BAR
    assert cnt["limit"] <= T.LIMIT_CAP * N and cnt["start_inside"] == 0 and cnt["nonfinite"] == 0
    assert cnt["hit"] > 0.15 * N
    assert cnt["hit"] + cnt["miss"] + cnt["limit"] == N == cnt["n_rays"]
    assert stats["evals_per_ray"] <= 2 * stats["oracle_evals_per_ray"]
    steps = res.steps.cpu().numpy()
    assert steps.min() >= 1 and steps.max() <= T.MAX_STEPS and int(steps.sum()) <= res.n_evals
    assert sorted(res.hit_index.cpu().tolist()) == np.nonzero(hit)[0].tolist()


@pytest.mark.parametrize("precision,seed,pose", VIEW_PARAMS)
def test_intrinsics_at_the_visible_point(precision, seed, pose):
    v = run_view(precision, seed, pose)
    out, fld = v["out"], v["fld"]
    H = T.R_VIEW
    status = out["trace"].status.cpu().numpy()
    hit = status == T.HIT
    flat = lambda m: npd(m[0]).reshape(m.shape[1], -1).T          # (1, C, H, W) -> (N, C)
    mask, depth, pos = flat(out["mask"])[:, 0], flat(out["depth"])[:, 0], flat(out["position"])
    assert np.array_equal(mask, hit.astype(np.float64)) and out["mask"].shape == (1, 1, H, H)
    assert np.array_equal(np.isnan(depth), ~hit)
    assert np.array_equal(depth[hit], npd(out["trace"].t)[hit])
    span = np.abs(v["ro"]).max() + np.abs(depth[hit]).max()
    perr = np.abs(v["ro"][hit] + depth[hit, None] * v["rd"][hit] - pos[hit]).max()
    print("position error / ulp(span)", perr / (span * 2.0 ** -23))
    assert perr <= 4 * span * 2.0 ** -23
    s, g, c = fld.full(pos[hit])
    gmax, gmin = float(np.abs(g).max()), float(np.linalg.norm(g, axis=-1).min())
    nbar = SDF_BAR * gmax / gmin
    n_obj, n_world, alb = flat(out["normal_object"]), flat(out["normal_map"]), flat(out["albedo"])
    case = f"trace_intrinsics[{precision},seed={seed},{pose}]"
    n_err, a_err = float(np.abs(n_obj[hit] - A.unit(g)).max()), float(np.abs(alb[hit] - c).max())
    w_err = float(np.abs(n_world[hit] - A.unit(g) @ v["w2b"][:3, :3]).max())     # w2b[:3,:3]^T n
    record_margin(case, "normals", n_err)
    record_margin(case, "albedo", a_err)
    print(case, "normals", n_err, "bar", nbar, "world", w_err, "albedo", a_err, "|g| at hits", gmin, np.linalg.norm(g, axis=-1).max())
    assert n_err < nbar and w_err < nbar + 1e-6 and a_err < RGB_BAR
    for m in (pos, n_obj, n_world, alb):
        assert not m[~hit].any()


@pytest.mark.parametrize("precision,seed,pose", VIEW_PARAMS)
def test_shading(precision, seed, pose):
    from oi_amd import ops, trace
    from oi_amd.relight import stack_lights
    v = run_view(precision, seed, pose)
    gen, z, b2w = v["gen"], A.latent(seed)[0], v["b2w"]
    lt = lights()
    res = v["out"]["trace"]
    hit = res.hit_index.long()
    n = len(hit)
    plain = trace.render_surface(gen, z, b2w, lights=lt)
    img = plain["image"].reshape(len(lt), 3, -1)
    # the T = 1 relighting launch (inference.shade_vertices' path) on the library's own hit arrays
    s = trace._Surface(gen, z.cuda().reshape(1, -1), b2w, T.BIAS, {})
    assert torch.equal(s.res.t, res.t) and torch.equal(s.res.status, res.status)           # identical calls
    slot = s.res.hit_slot[hit].long()
    g, c, tt = s.grad[slot], s.rgb[slot], res.t[hit]
    ro, rd = v["ro_t"][hit].contiguous(), v["rd_t"][hit].contiguous()
    lt_t = stack_lights(lt)
    rel = ops.relight_fwd(torch.ones(n, 1).cuda(), g.view(n, 1, 3), c.view(n, 1, 3), tt.view(n, 1), ro, rd, v["w2b_t"][None], lt_t,
                          None, 1, outputs=("image",))["image"][:, 0]
    ref = T.shade(npd(ro), npd(rd), npd(tt), npd(g), npd(c), v["w2b"], npd(lt_t))
    e_rel, e_ref = float((img[:, :, hit] - rel).abs().max()), float(np.abs(npd(img[:, :, hit]) - ref).max())
    case = f"trace_shading[{precision},seed={seed},{pose}]"
    record_margin(case, "vs_relight_fwd", e_rel)
    record_margin(case, "vs_fp64", e_ref)
    print(case, e_rel, e_ref)
    assert e_rel < RELIGHT_BAR and e_ref < RELIGHT_BAR
    off = torch.ones(img.shape[-1], dtype=torch.bool, device=img.device)
    off[hit] = False
    assert not bool(img[:, :, off].any())                                                  # black background
    for i, one in enumerate(lt):                                                            # light l of L == the 1-light call
        assert torch.equal(trace.render_surface(gen, z, b2w, lights=[one])["image"][0], plain["image"][i])
    bg = (0.25, 0.5, 0.75)
    zero = s.shade(lt_t, trace._bg(bg, "cuda"), torch.zeros(len(lt), s.N).cuda(), outputs=("image",))["image"]
    amb = torch.tensor([l.ambient for l in lt]).cuda()[:, :, None] * c.t()[None]
    assert float((zero[:, :, hit] - amb).abs().max()) < 1e-6
    assert torch.equal(zero[:, :, off], torch.tensor(bg).cuda()[None, :, None].expand(len(lt), 3, int(off.sum())))


@pytest.mark.parametrize("precision,seed,pose", VIEW_PARAMS)
def test_shadows(precision, seed, pose):
    v = run_view(precision, seed, pose)
    out, fld, res = v["out"], v["fld"], v["out"]["trace"]
    st, n_hit, L = out["shadow_trace"], len(res.hit_index), len(T.LIGHT_DIRS)
    status = st.status.cpu().numpy().reshape(L, n_hit)
    o, d, t, far = npd(st.rays_o), npd(st.rays_d), npd(st.t), npd(st.far)
    traced = status != T.BACKFACING
    occl = (status == T.HIT).reshape(-1)
    lit = (status == T.MISS).reshape(-1)
    on = np.abs(fld.sdf(o[occl] + t[occl, None] * d[occl]))
    seg = T.segment_min(fld.sdf, o[lit], d[lit], np.zeros(int(lit.sum())), far[lit])
    si, lim = int((status == T.START_INSIDE).sum()), int((status == T.LIMIT).sum())
    case = f"trace_shadows[{precision},seed={seed},{pose}]"
    stats = {"traced": int(traced.sum()), "occluded": int(occl.sum()), "lit": int(lit.sum()), "start_inside": si, "limit": lim,
             "occluder_sdf_worst": float(on.max(initial=0.0)), "lit_segment_min": float(seg.min(initial=np.inf))}
    print(case, stats)
    record_margin(case, "occluder_sdf_worst", stats["occluder_sdf_worst"])
    record_margin(case, "start_inside_share", si / max(1, stats["traced"]))
    assert stats["traced"] > 0.2 * L * n_hit and stats["lit"] > 0
    assert on.max(initial=0.0) <= T.TOL + SDF_BAR
    assert seg.min(initial=np.inf) >= -SDF_BAR
    assert si <= T.SHADOW_START_INSIDE_CAP * stats["traced"]
    assert not (status == T.NONFINITE).any()
    # the visibility map is the rule applied to the states, 1 off the mask
    vis = npd(out["visibility"]).reshape(L, -1)
    slot = res.hit_slot.cpu().numpy()
    expect = np.ones_like(vis)
    expect[:, slot >= 0] = T.visibility_of(status)[:, slot[slot >= 0]]
    assert np.array_equal(vis, expect)
    # the shadowed image against fp64 at the library's own visibility
    hit = res.hit_index.long()
    from oi_amd import trace
    from oi_amd.relight import stack_lights
    s = trace._Surface(v["gen"], A.latent(seed)[0].cuda().reshape(1, -1), v["b2w"], T.BIAS, {})
    sl = s.res.hit_slot[hit].long()
    ref = T.shade(v["ro"][hit.cpu()], v["rd"][hit.cpu()], npd(res.t[hit]), npd(s.grad[sl]), npd(s.rgb[sl]), v["w2b"],
                  npd(stack_lights(lights())), visibility=vis[:, hit.cpu().numpy()])
    assert np.abs(npd(out["image"].reshape(L, 3, -1)[:, :, hit]) - ref).max() < RELIGHT_BAR


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("seed", T.SEEDS)
def test_a_light_at_the_camera_casts_no_visible_shadow(precision, seed):
    """Direction = minus the view axis: every visible point sees the eye, so every traced pixel is lit except those whose
    shadow ray starts inside (the bias) or runs out of steps."""
    from oi_amd import trace
    from oi_amd.relight import Light
    v = run_view(precision, seed, "centre")
    axis_obj = v["rd"].mean(0)
    d_world = -(v["w2b"][:3, :3].T @ axis_obj)            # object frame -> world
    out = trace.render_surface(v["gen"], A.latent(seed)[0], v["b2w"], lights=[Light(direction=tuple(d_world))], shadows=True)
    status = out["shadow_trace"].status.cpu().numpy()
    traced = status != T.BACKFACING
    other = traced & (status != T.MISS) & (status != T.START_INSIDE) & (status != T.LIMIT)
    print("camera light: traced", int(traced.sum()), "of", len(status), "start_inside", int((status == T.START_INSIDE).sum()),
          "limit", int((status == T.LIMIT).sum()), "occluded", int(other.sum()))
    assert traced.sum() > 0.9 * len(status)
    assert int(other.sum()) == 0
    assert int((status == T.START_INSIDE).sum()) <= T.SHADOW_START_INSIDE_CAP * traced.sum()


def test_light_walk_frame_is_render_surface_under_that_light():
    from oi_amd import inference, trace
    from oi_amd.relight import Light
    gen = make_gen("f16x3")
    z, b2w = A.latent(1)[0], T.pose("off")
    walk = inference.surface_light_walk(gen, z, b2w, n_frames=6, shadows=False)
    base = Light.from_module(gen.light)
    dirs = inference.light_walk_directions(base.direction, 6)
    for i in (0, 2, 5):
        lt = base if i == 0 else base.replace(direction=tuple(dirs[i]))
        one = trace.render_surface(gen, z, b2w, lights=[lt])
        assert torch.equal(walk["image"][i], one["image"][0]), i
    assert torch.equal(walk["mask"], one["mask"]) and walk["image"].shape == (6, 3, T.R_VIEW, T.R_VIEW)
    sh = inference.surface_light_walk(gen, z, b2w, n_frames=6, shadows=True)
    assert sh["visibility"].shape == (6, 1, T.R_VIEW, T.R_VIEW) and float(sh["visibility"].min()) == 0.0
    lit = sh["visibility"].expand(6, 3, -1, -1) == 1
    assert torch.equal(sh["image"][lit], walk["image"][lit])          # a lit pixel is the unshadowed one, bit for bit
    assert bool((sh["image"] <= walk["image"]).all())
    fr = inference.surface_frames(gen, [z, z], [b2w, T.pose("centre")], keys=("image", "depth", "visibility"), shadows=True)
    assert fr["image"].shape == (2, 3, T.R_VIEW, T.R_VIEW) and fr["depth"].shape == (2, 1, T.R_VIEW, T.R_VIEW)
    assert torch.equal(fr["image"][0], sh["image"][0])


def _bundle(n, seed, kind="mixed"):
    """n rays at the object from a camera 3 units away: 'mixed' aims at a disc of radius 0.9, 'hit' at the centre region,
    'miss' passes the unit sphere's rim (0.93 .. 0.97 from the centre, where the field is far from the surface)."""
    rs = np.random.RandomState(seed)
    o = np.tile(np.array([[0.0, 0.0, -3.0]]), (n, 1)) + 0.02 * rs.randn(n, 3)
    ang = rs.rand(n) * 2 * np.pi
    rad = {"mixed": 0.9 * np.sqrt(rs.rand(n)), "hit": 0.02 * rs.rand(n), "miss": 0.93 + 0.04 * rs.rand(n)}[kind]
    target = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(n)], -1)
    d = target - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return torch.from_numpy(o).float().cuda(), torch.from_numpy(d).float().cuda()


def _same(a, b):
    return torch.equal(a.t, b.t) and torch.equal(a.status, b.status) and torch.equal(a.steps, b.steps)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
def test_limit_shapes_and_order_independence(N):
    from oi_amd import trace
    gen = make_gen("f16x3")
    z = A.latent(0).cuda()
    ro, rd = _bundle(N, N)
    ro_g, rd_g = guarded_copy(ro, "rays_o"), guarded_copy(rd, "rays_d")
    a = trace.sphere_trace(gen, ro_g, rd_g, z=z)
    b = trace.sphere_trace(gen, ro_g, rd_g, z=z)
    every = trace.sphere_trace(gen, ro_g, rd_g, z=z, readback=1)
    stale = trace.sphere_trace(gen, ro_g, rd_g, z=z, readback=7)
    assert _same(a, b) and _same(a, every) and _same(a, stale)           # a stale bound changes the cost, not the rays
    assert a.t.shape == (N,) and a.status.shape == (N,) and a.steps.shape == (N,) and a.hit_slot.shape == (N,)
    assert every.n_evals == int(every.steps.sum()) <= a.n_evals <= stale.n_evals or N == 1
    assert sorted(a.hit_index.tolist()) == torch.nonzero(a.status == T.HIT).flatten().tolist()
    idx = a.hit_index.long()
    if len(idx):
        assert float((a.hit_points - (ro + a.t[:, None] * rd)[idx]).abs().max()) < 1e-6
    one = trace.sphere_trace(gen, ro_g, rd_g, z=z, max_steps=1)
    st1 = one.status.cpu().numpy()
    assert set(np.unique(st1)) <= {T.LIMIT, T.HIT} and one.n_steps == 1 and int(one.steps.max()) == 1
    fld = T.Field(0)
    o64, d64 = npd(ro), npd(rd)
    hit = a.status.cpu().numpy() == T.HIT
    if hit.any():
        assert np.abs(fld.sdf(o64[hit] + npd(a.t)[hit, None] * d64[hit])).max() <= T.TOL + SDF_BAR


def test_all_miss_and_all_hit_bundles():
    from oi_amd import trace
    gen = make_gen("f16x3")
    z = A.latent(0).cuda()
    fld = T.Field(0)
    ro, rd = _bundle(65, 5, "miss")
    near, far = (npd(x).reshape(-1) for x in T.O.near_far_from_sphere(ro.cpu().double(), rd.cpu().double()))
    t_ref, s_ref, steps_ref, in_flight = T.trace(fld.sdf, npd(ro), npd(rd), near, far)
    assert (s_ref == T.MISS).all()                                       # the oracle's rehearsal of this bundle
    m = trace.sphere_trace(gen, ro, rd, z=z, readback=1)
    print("all-miss bundle: steps", m.n_steps, "evaluations", m.n_evals, "oracle", sum(in_flight), len(in_flight))
    assert bool((m.status == T.MISS).all()) and len(m.hit_index) == 0
    assert m.n_steps == len(in_flight) < T.MAX_STEPS and m.n_evals == sum(in_flight)
    auto = trace.sphere_trace(gen, ro, rd, z=z)
    assert _same(auto, m) and auto.n_steps < T.MAX_STEPS
    empty = trace.sphere_trace(gen, ro[:0], rd[:0], z=z)
    assert empty.t.shape == (0,) and empty.n_evals == 0 and empty.hit_index.shape == (0,)
    ro, rd = _bundle(300, 6, "hit")
    h = trace.sphere_trace(gen, ro, rd, z=z)
    assert bool((h.status == T.HIT).all()) and sorted(h.hit_index.tolist()) == list(range(300)) and h.n_steps < T.MAX_STEPS


@pytest.mark.parametrize("L", [1, 256])
def test_light_counts(L):
    from oi_amd import trace
    from oi_amd.relight import Light
    gen = make_gen("f16x3", 16)
    z, b2w = A.latent(2)[0], T.pose("centre")
    rs = np.random.RandomState(L)
    lt = [Light(direction=tuple(rs.randn(3)), specular=0.2) for _ in range(L)]
    out = trace.render_surface(gen, z, b2w, lights=lt, shadows=True)
    assert out["image"].shape == (L, 3, 16, 16) and out["visibility"].shape == (L, 1, 16, 16)
    assert out["stats"]["hit"] > 0 and bool(torch.isfinite(out["image"]).all())
    k = L - 1
    one = trace.render_surface(gen, z, b2w, lights=[lt[k]], shadows=True)
    assert torch.equal(one["image"][0], out["image"][k]) and torch.equal(one["visibility"][0], out["visibility"][k])
    with pytest.raises(ValueError, match="lights"):
        trace.render_surface(gen, z, b2w, lights=lt + [lt[0]] * (257 - L))


def _guarded_pass(N, seed):
    """Every entry of include/oi_trace.h through the C ABI on guarded buffers: a sphere of radius 0.5 as the field (evaluated
    by torch between the steps), against the float64 restatement."""
    from oi_amd import lib, ops
    L_ = lib.load()
    ro, rd = _bundle(N, seed)
    near, far = T.O.near_far_from_sphere(ro, rd)
    # (must_write is judged per 4-byte element; for the int16 step counts a byte of a legitimate value can equal the poison
    #  byte at its position, so they carry guards only and are compared with the restatement below)
    g = lambda sh, dt=torch.float32, what="?", mw=True: guarded_empty(sh, dt, what=what, must_write=mw)
    p = lambda t_: ctypes.c_void_p(t_.data_ptr())
    arr = dict(rays_o=guarded_copy(ro, "rays_o"), rays_d=guarded_copy(rd, "rays_d"), near_=guarded_copy(near.reshape(-1), "near"),
               far_=guarded_copy(far.reshape(-1), "far"), t=g((N,), what="t"), status=g((N,), torch.uint8, "status"),
               steps=g((N,), torch.int16, "steps", False), bracket=g((N, 4), what="bracket"), side=g((N,), torch.uint8, "side"),
               active=g((2, N), torch.int32, "active", False), points=g((N, 3), what="points"),
               counts=g((lib.TRACE_COUNT_WORDS,), torch.int32, "counts"))
    S = lib.TraceState()
    S.N = N
    for k_, v_ in arr.items():
        setattr(S, k_, p(v_))
    st = ops._stream()
    sphere = lambda pts: pts.norm(dim=-1) - 0.5
    assert L_.oi_trace_begin(ctypes.byref(S), st) == 0
    assert arr["counts"][0].item() == N and not bool(arr["counts"][1:].any())
    bound, k = N, 0
    while bound > 0 and k < T.MAX_STEPS:
        sdf = guarded_copy(sphere(arr["points"][:bound]), "sdf")
        assert L_.oi_trace_step(ctypes.byref(S), p(sdf), bound, k, T.TOL, T.OMEGA, st) == 0
        k += 1
        bound = int(arr["counts"][k].item()) if k % 2 == 0 else bound       # a stale bound every other step
    hit_index, hit_points = g((N,), torch.int32, "hit_index", False), g((N, 3), what="hit_points", mw=False)
    hit_slot = g((N,), torch.int32, "hit_slot")
    assert L_.oi_trace_finish(ctypes.byref(S), p(hit_index), p(hit_points), p(hit_slot), st) == 0
    n_hit = int(arr["counts"][-1].item())
    t_ref, s_ref, steps_ref, _ = T.trace(lambda x: np.linalg.norm(x, axis=-1) - 0.5, npd(ro), npd(rd), npd(near).reshape(-1),
                                         npd(far).reshape(-1))
    status = arr["status"].cpu().numpy()
    assert np.array_equal(status, s_ref) and n_hit == int((s_ref == T.HIT).sum())
    assert np.abs(npd(arr["t"]) - t_ref)[s_ref == T.HIT].max(initial=0.0) < 1e-5
    assert np.abs(arr["steps"].cpu().numpy() - steps_ref).max() <= 1      # fp32 against fp64 at the tolerance
    slot = hit_slot.cpu().numpy()
    assert sorted(hit_index[:n_hit].cpu().tolist()) == np.nonzero(slot >= 0)[0].tolist() == np.nonzero(status == T.HIT)[0].tolist()
    if n_hit == 0:
        return
    # shadow rays of the hits under two lights, their visibility, and the shading
    hp = guarded_copy(hit_points[:n_hit], "hit_points")
    grad = guarded_copy(hp * 2.0, "grad")                                   # the sphere's gradient direction
    rgb = guarded_copy(torch.rand(n_hit, 3).cuda(), "rgb")
    Lt = 2
    lts = guarded_copy(torch.tensor([T.light_block((0.3, -0.8, -0.5)), T.light_block((0.0, 0.0, -1.0))]).cuda(), "lights")
    w2b = guarded_copy(torch.eye(4).cuda(), "w2b")
    Q = Lt * n_hit
    sh = dict(rays_o=g((Q, 3), what="s_rays_o"), rays_d=g((Q, 3), what="s_rays_d"), near_=g((Q,), what="s_near"), far_=g((Q,), what="s_far"),
              t=g((Q,), what="s_t"), status=g((Q,), torch.uint8, "s_status"), steps=g((Q,), torch.int16, "s_steps", False),
              bracket=g((Q, 4), what="s_bracket"), side=g((Q,), torch.uint8, "s_side"), active=g((2, Q), torch.int32, "s_active", False),
              points=g((Q, 3), what="s_points", mw=False), counts=g((lib.TRACE_COUNT_WORDS,), torch.int32, "s_counts"))
    S2 = lib.TraceState()
    S2.N = Q
    for k_, v_ in sh.items():
        setattr(S2, k_, p(v_))
    assert L_.oi_trace_shadow_begin(ctypes.byref(S2), p(hp), p(grad), n_hit, p(lts), Lt, p(w2b), T.BIAS, st) == 0
    T.assert_secondary_begin_state(sh)
    bound, k = int(sh["counts"][0].item()), 0
    s0 = sh["status"].cpu().numpy()
    assert bound == int((s0 == T.MARCH).sum()) and set(np.unique(s0)) <= {T.MARCH, T.BACKFACING}
    while bound > 0 and k < T.MAX_STEPS:
        sdf = guarded_copy(sphere(sh["points"][:bound]), "s_sdf")
        assert L_.oi_trace_step(ctypes.byref(S2), p(sdf), bound, k, T.TOL, T.OMEGA, st) == 0
        k += 1
        bound = int(sh["counts"][k].item())
    s1 = sh["status"].cpu().numpy()
    assert set(np.unique(s1)) <= {T.MISS, T.BACKFACING}                      # a convex body casts no shadow on itself
    for li in range(Lt):
        l = T.light_object_dir(npd(lts[li, :3]), np.eye(4))
        o_ref, far_ref, traced = T.shadow_rays(npd(hp), npd(grad), l)
        sl = slice(li * n_hit, (li + 1) * n_hit)
        assert np.array_equal(s0[sl] == T.MARCH, traced) or np.abs((A.unit(npd(grad)) @ l)[(s0[sl] == T.MARCH) != traced]).max() < 1e-6
        assert np.abs(npd(sh["rays_o"][sl]) - o_ref).max() < 1e-6 and np.abs(npd(sh["far_"][sl]) - far_ref).max() < 1e-5
    vis = g((Lt, N), what="visibility")
    assert L_.oi_trace_visibility(p(sh["status"]), p(hit_slot), N, n_hit, Lt, p(vis), st) == 0
    exp = np.ones((Lt, N))
    exp[:, slot >= 0] = T.visibility_of(s1.reshape(Lt, n_hit))[:, slot[slot >= 0]]
    assert np.array_equal(npd(vis), exp)
    P = lib.SurfaceParams()
    P.N, P.n_hit, P.L = N, n_hit, Lt
    outs = dict(depth=g((N,), what="depth"), position=g((N, 3), what="position"), normal=g((N, 3), what="normal"),
                normal_world=g((N, 3), what="normal_world"), albedo=g((N, 3), what="albedo"), mask=g((N,), what="mask"),
                image=g((Lt, 3, N), what="image"))
    bg = guarded_copy(torch.tensor([0.1, 0.2, 0.3]).cuda(), "bg")
    for k_, v_ in dict(rays_o=arr["rays_o"], rays_d=arr["rays_d"], t=arr["t"], status=arr["status"], hit_slot=hit_slot, hit_points=hp,
                       grad=grad, rgb=rgb, w2b=w2b, lights=lts, bg=bg, visibility=vis, **outs).items():
        setattr(P, k_, p(v_))
    assert L_.oi_surface_shade(ctypes.byref(P), st) == 0
    hit = status == T.HIT
    idx = hit_index[:n_hit].long()
    ref = T.shade(npd(ro[idx]), npd(rd[idx]), npd(arr["t"][idx]), npd(grad), npd(rgb), np.eye(4), npd(lts), visibility=npd(vis[:, idx]))
    assert np.abs(npd(outs["image"][:, :, idx]) - ref).max() < RELIGHT_BAR
    assert np.array_equal(npd(outs["mask"]), hit.astype(np.float64)) and np.array_equal(np.isnan(npd(outs["depth"])), ~hit)
    assert torch.equal(outs["albedo"][idx], rgb) and torch.equal(outs["position"][idx], hp)
    assert torch.equal(outs["image"][:, :, ~torch.from_numpy(hit).cuda()], bg[None, :, None].expand(Lt, 3, int((~hit).sum())))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
def test_guarded_shapes(N):
    _guarded_pass(N, seed=N)


@pytest.mark.parametrize("seed,pose", [(0, "off"), (2, "centre")])
def test_bf16_is_measured(seed, pose):
    """bf16 (one bf16 MFMA per contraction): measured and recorded only -- no bar is set in advance.  The structural caps
    (every ray ends in a terminal state, the counts add up) still hold."""
    v = run_view("bf16", seed, pose)
    res, fld = v["out"]["trace"], v["fld"]
    t, status = npd(res.t), res.status.cpu().numpy()
    hit = status == T.HIT
    on = np.abs(fld.sdf(v["ro"][hit] + t[hit, None] * v["rd"][hit]))
    cnt = v["out"]["stats"]
    case = f"trace_bf16[seed={seed},{pose}]"
    record_margin(case, "hit_sdf_worst", float(on.max()))
    record_margin(case, "limit_share", cnt["limit"] / len(t))
    print(case, "worst |oracle sdf| at hits", float(on.max()), "median", float(np.median(on)), cnt)
    assert cnt["hit"] + cnt["miss"] + cnt["limit"] + cnt["start_inside"] + cnt["nonfinite"] == len(t)
    assert status.max() <= T.NONFINITE
