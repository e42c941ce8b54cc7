"""Local lights on the traced surface on the MI355X (include/oi_local_light.h; oi_amd.trace; oi_amd.inference.surface_light_orbit;
DESIGN section 4.27): point, spot and sphere lights that stand in the world, with shadow rays that end at the light.

The reference is the fp64 restatement of tests/helpers/local_light_ref.py, which touches no code under test; the analytic
cases and the golden lights are the ones tests/test_local_light_cpu.py rehearses on the CPU.

Bars:
  RAY_BAR, FAR_BAR   1e-6 on origins and directions, 1e-5 on far: tests/test_gpu_occlusion.py's bars for the same comparison.
                     The margins measured against the restatement are recorded (record_margin) and stand in DESIGN 4.27.
  RELIGHT_BAR        2e-6, the directional image's bar, for lights whose att is of order 1 at the object.
  STATES             per ray exactly the fp64 any-hit trace of the restatement's rays outside occlusion_ref.TANGENCY_BAND of
                     tangency to either sphere; at most EXCLUDED_CAP of the rays may lie in the band.
  DIRECTIONAL LIMIT  3 / D of the light's largest colour (the direction and att each deviate by at most ~|p| / D <= 1 / D, and
                     the Phong terms are Lipschitz in them with constants below 1 and 2) plus RELIGHT_BAR."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_occlusion as OC
import test_gpu_trace as G
from conftest import record_margin
from helpers import local_light_ref as LL
from helpers import mesh_attr_ref as A
from helpers import occlusion_ref as R
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

SDF_BAR, RELIGHT_BAR, PRECISIONS, npd = G.SDF_BAR, G.RELIGHT_BAR, G.PRECISIONS, G.npd
RAY_BAR, FAR_BAR = OC.RAY_BAR, OC.FAR_BAR
_p, _cuda, _bits = OC._p, OC._cuda, OC._bits
NEW_OPS = ("local_light_begin", "surface_shade_local", "scene_local_light_begin", "scene_shade_local")


def golden_lights(pose):
    from oi_amd.relight import LocalLight
    return [LocalLight(position=tuple(p), radius=g["radius"], reference_distance=g["reference_distance"], **LL.GOLDEN_COLOURS)
            for p, g in zip(LL.golden_positions(pose), LL.GOLDEN_LIGHTS)]


def stacked(lights):
    from oi_amd.relight import stack_local_lights
    return stack_local_lights(lights, "cuda")


def _begin(S, hp, grad, hit_index, n_hit, lts, L, samples, w2b, seed, bias=T.BIAS):
    from oi_amd import lib, ops
    return lib.load().oi_local_light_begin(ctypes.byref(S), _p(hp), _p(grad), _p(hit_index), n_hit, _p(lts), L, samples, _p(w2b), bias,
                                           seed, ops._stream())


def _compare_rays(case, arr_o, arr_d, arr_far, status0, ref, nrm):
    """Begin rays (L, S, n, ...) against the restatement's: the bars, the margins, and the states up to n . d rounding across 0."""
    e_o = float(np.abs(arr_o - ref["o"]).max())
    traced = ref["status"] == LL.MARCH
    known = ref["status"] != LL.MISS                                             # (inside the light: the direction is zeros)
    e_d = float(np.abs(arr_d - ref["d"])[known].max(initial=0.0))
    e_f = float(np.abs(arr_far - ref["far"])[traced & (status0 == T.MARCH)].max(initial=0.0))
    print(case, "origins", e_o, "directions", e_d, "far", e_f)
    record_margin(case, "directions", e_d)
    record_margin(case, "far", e_f)
    assert e_o < RAY_BAR and e_d < RAY_BAR and e_f < FAR_BAR
    differ = status0 != ref["status"]
    ndd = (nrm[None, None] * ref["d"]).sum(-1)
    assert not differ.any() or (np.abs(ndd[differ]).max() < RAY_BAR and not (ref["status"][differ] == LL.MISS).any())


# ---------------------------------------------------------------------------------------------------------------------
# 1. begin rays on a golden view
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_begin_rays_against_the_restatement(precision):
    from oi_amd import ops
    seed, pose = R.SOFT_VIEWS[1]
    gen, s = OC.surface(precision, seed, pose)
    lights = golden_lights(pose)
    lt, L, S, n = stacked(lights), 2, R.SOFT_S, s.n_hit
    st = ops.TraceState(L * S * n, ref=s.ro)
    ops.local_light_begin(st, s.res.hit_points, s.grad, s.res.hit_index, n, lt, S, s.w2b, T.BIAS, R.SEED)
    pix, pts, grad, w2b = s.res.hit_index.cpu().numpy(), npd(s.res.hit_points), npd(s.grad), npd(s.w2b)
    refs = [LL.rays(pts, grad, pix, rec, w2b, S, R.SEED) for rec in npd(lt)]
    ref = {k: np.stack([r[k] for r in refs]) for k in ("o", "d", "far", "status")}
    status0 = st.status.cpu().numpy().reshape(L, S, n)
    _compare_rays(f"local_light_rays[{precision}]", npd(st.rays_o).reshape(L, S, n, 3), npd(st.rays_d).reshape(L, S, n, 3),
                  npd(st.far).reshape(L, S, n), status0, ref, A.unit(grad))
    T.assert_secondary_begin_state({k: getattr(st, a) for k, a in (("counts", "counts"), ("status", "status"), ("active", "active"),
                                    ("points", "points"), ("rays_o", "rays_o"), ("bracket", "bracket"), ("side", "side"), ("t", "t"),
                                    ("near_", "near"))})
    assert int(st.counts[0].item()) == int((status0 == T.MARCH).sum()) > 0
    # the point light: every sample is the axis; far never exceeds the distance to the light
    d0 = npd(st.rays_d).reshape(L, S, n, 3)[0]
    assert np.abs(d0 - d0[:1]).max() == 0
    assert (npd(st.far).reshape(L, S, n)[0] <= refs[0]["dc"][None] + FAR_BAR).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the analytic cases through the C ABI on guarded buffers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["below", "above", "sphere"])
def test_analytic_cases(name):
    c = LL.analytic_case(name)
    S, n_hit, pix = c["S"], len(c["points"]), c["pix"]
    hp, grad = guarded_copy(_cuda(c["points"]), "hit_points"), guarded_copy(_cuda(c["grad"]), "grad")
    hit_index = guarded_copy(_cuda(pix, torch.int32), "hit_index")
    lts, w2b = guarded_copy(_cuda([c["light"]]), "lights"), guarded_copy(torch.eye(4).cuda(), "w2b")
    arr, St = OC._guarded_state(S * n_hit, "ll")
    assert _begin(St, hp, grad, hit_index, n_hit, lts, 1, S, w2b, R.SEED, LL.ANALYTIC_BIAS) == 0
    assert int(arr["counts"][0].item()) == S * n_hit                              # every sample faces the light
    T.assert_secondary_begin_state(arr)
    ref = LL.rays(npd(hp), npd(grad), pix, npd(lts)[0], np.eye(4), S, R.SEED, bias=LL.ANALYTIC_BIAS)
    assert ref["traced"].all()
    e_d = float(np.abs(npd(arr["rays_d"]).reshape(S, n_hit, 3) - ref["d"]).max())
    e_f = float(np.abs(npd(arr["far_"]).reshape(S, n_hit) - ref["far"]).max())
    record_margin(f"local_light_analytic[{name}]", "directions", e_d)
    record_margin(f"local_light_analytic[{name}]", "far", e_f)
    assert np.abs(npd(arr["rays_o"]).reshape(S, n_hit, 3) - ref["o"]).max() < RAY_BAR and e_d < RAY_BAR and e_f < FAR_BAR
    k = OC._anyhit_loop(arr, St, OC._two_spheres, 256)
    _, s_ref, _, _ = R.trace_anyhit(R.two_spheres, ref["o"], ref["d"], np.zeros(S * n_hit), ref["far"], max_steps=256)
    band = c["band"].reshape(-1)
    status = arr["status"].cpu().numpy()
    print(f"local light analytic[{name}]: steps", k, "excluded", int(band.sum()), "of", band.size, "disagreements in the band",
          int((status != s_ref)[band].sum()), "states", np.bincount(status).tolist(), "directions", e_d, "far", e_f)
    assert band.sum() <= R.EXCLUDED_CAP * band.size
    assert np.array_equal(status[~band], s_ref[~band])
    assert np.array_equal(s_ref[~band] == T.MISS, c["lit"].reshape(-1)[~band])    # the machine and the exact intersection agree
    slot = guarded_copy(torch.arange(n_hit, dtype=torch.int32).cuda(), "hit_slot")
    vis = npd(OC._resolve(arr["status"], slot, n_hit, n_hit, 1, S))[0]
    assert np.array_equal(vis, R.resolve(status, np.arange(n_hit), n_hit, 1, S)[0])
    r_xy, clean = c["r_xy"], ~c["band"].any(0)
    if name == "below":                                                           # the ray stops at the light: no shadow
        assert (vis == 1).all()
    elif name == "above":
        assert int((vis == 0).sum()) == 148 and int((vis == 1).sum()) == 108
        assert r_xy[vis == 0].max() <= 0.178 and round(float(r_xy[vis == 1].min()), 3) >= 0.186
    else:
        assert np.array_equal(vis[clean], c["vis"][clean])
        assert r_xy[vis == 0].max() <= 0.121 and (vis[r_xy < 0.11] == 0).all()
        assert ((vis > 0) & (vis < 1)).mean() >= 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 3. guarded shapes
# ---------------------------------------------------------------------------------------------------------------------
SHAPE_LIGHTS = [LL.record((0.3, 0.2, 1.4)), LL.record((0.9, 0.1, 0.7), 0.2)]      # a point light and a sphere light


def _shape_case(n_hit, S, L, seed, lights=None, backfacing=False):
    """oi_local_light_begin, the any-hit march and the resolve through the C ABI on guarded buffers, twice (the second time with
    stale bounds).  -> the first run's arrays, the slots."""
    rs = np.random.RandomState(seed)
    nrm = rs.randn(n_hit, 3)
    nrm[:, 2] = np.abs(nrm[:, 2]) + (1.0 if backfacing else 0.0)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    recs = (SHAPE_LIGHTS if lights is None else lights)[:L]
    N = n_hit + 3                                                                # three pixels off the mask
    slot_np = np.full(N, -1)
    slot_np[rs.permutation(N)[:n_hit]] = np.arange(n_hit)
    pix = np.zeros(n_hit, dtype=np.int64)
    pix[slot_np[slot_np >= 0]] = np.nonzero(slot_np >= 0)[0]
    hp, grad = guarded_copy(_cuda(nrm * R.R0), "hit_points"), guarded_copy(_cuda(nrm * 1.7), "grad")
    hit_index, slot = guarded_copy(_cuda(pix, torch.int32), "hit_index"), guarded_copy(_cuda(slot_np, torch.int32), "hit_slot")
    lts, w2b = guarded_copy(_cuda(recs), "lights"), guarded_copy(torch.eye(4).cuda(), "w2b")
    runs = []
    for rep in range(2):
        arr, St = OC._guarded_state(L * S * n_hit, f"ll{rep}")
        assert _begin(St, hp, grad, hit_index, n_hit, lts, L, S, w2b, seed) == 0
        T.assert_secondary_begin_state(arr)
        s0 = arr["status"].cpu().numpy()
        assert set(np.unique(s0)) <= {T.MARCH, T.MISS, T.BACKFACING} and int(arr["counts"][0].item()) == int((s0 == T.MARCH).sum())
        assert not bool(arr["counts"][1:].any())
        far0 = npd(arr["far_"])
        k = OC._anyhit_loop(arr, St, OC._two_spheres, T.MAX_STEPS, stale=rep == 1)
        vis = OC._resolve(arr["status"], slot, N, n_hit, L, S)
        runs.append(dict(arr=arr, vis=vis, k=k, s0=s0, far0=far0))
    a, b = runs
    for name in ("rays_o", "rays_d", "near_", "far_", "t", "status", "steps"):
        assert torch.equal(_bits(a["arr"][name]), _bits(b["arr"][name])), name         # per ray, whatever the slots and bounds
    assert torch.equal(a["vis"], b["vis"])
    status = a["arr"]["status"].cpu().numpy()
    assert status.max() <= T.BACKFACING
    assert np.array_equal(npd(a["vis"]), R.resolve(status, slot_np, n_hit, L, S))
    assert (npd(a["vis"])[:, slot_np < 0] == 1).all()
    refs = [LL.rays(npd(hp), npd(grad), pix, rec, np.eye(4), S, seed) for rec in npd(lts)]
    ref = {k_: np.stack([r[k_] for r in refs]) for k_ in ("o", "d", "far", "status")}
    sh = (L, S, n_hit)
    _compare_rays(f"local_light_shapes[{n_hit},{S},{L}]", npd(a["arr"]["rays_o"]).reshape(*sh, 3), npd(a["arr"]["rays_d"]).reshape(*sh, 3),
                  a["far0"].reshape(sh), a["s0"].reshape(sh), ref, A.unit(npd(grad)))
    return a, slot_np


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("n_hit", [1, 63, 64, 65])
def test_guarded_shapes(n_hit, S, L):
    _shape_case(n_hit, S, L, seed=n_hit * 100 + S * 3 + L)


def test_guarded_every_ray_backfacing():
    a, slot = _shape_case(65, 3, 2, seed=9, lights=[LL.record((0.0, 0.0, -3.0)), LL.record((0.1, 0.0, -2.5), 0.3)], backfacing=True)
    assert (a["s0"] == T.BACKFACING).all() and int(a["arr"]["counts"][0].item()) == 0 and a["k"] == 0
    assert not bool(a["arr"]["steps"].any())
    assert (npd(a["vis"])[:, slot >= 0] == 0).all()


def test_guarded_every_origin_inside_the_light():
    a, slot = _shape_case(65, 3, 1, seed=5, lights=[LL.record((0.0, 0.0, 0.0), 0.6)])
    assert (a["s0"] == T.MISS).all() and int(a["arr"]["counts"][0].item()) == 0 and a["k"] == 0
    assert not bool(a["arr"]["steps"].any()) and not bool(a["arr"]["far_"].any())
    assert (npd(a["vis"]) == 1).all()


def test_guarded_256_samples():
    a, _ = _shape_case(5, 256, 1, seed=4, lights=SHAPE_LIGHTS[1:])
    assert a["arr"]["status"].shape == (1280,)
    vis = npd(a["vis"])
    assert np.array_equal(vis * 256, np.round(vis * 256))


def test_guarded_shade_with_256_lights():
    """oi_surface_shade_local on guarded buffers: N = 65 pixels, three of them off the mask, L = 256 lights (points, spheres and
    cones), random visibility and occlusion, against the fp64 restatement; the G-buffer against oi_surface_shade's bytes."""
    from oi_amd import lib, ops
    L_, st = lib.load(), ops._stream()
    N, Lt, n_hit = 65, 256, 62
    rs = np.random.RandomState(11)
    nrm = rs.randn(n_hit, 3)
    nrm[:, 2] = -np.abs(nrm[:, 2]) - 0.3                                          # the side that faces the eye
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    pts = nrm * R.R0
    eye = np.array([0.0, 0.0, -3.0]) + 0.02 * rs.randn(N, 3)
    slot_np = np.full(N, -1)
    slot_np[rs.permutation(N)[:n_hit]] = np.arange(n_hit)
    on = np.nonzero(slot_np >= 0)[0]
    rd = np.tile([[0.0, 0.0, 1.0]], (N, 1))
    rd[on] = pts[slot_np[on]] - eye[on]
    tt = np.linalg.norm(rd, axis=-1)
    rd /= tt[:, None]
    status = np.where(slot_np >= 0, T.HIT, T.MISS)
    recs = []
    for i in range(Lt):
        pos = rs.randn(3)
        pos = pos / np.linalg.norm(pos) * (0.9 + 1.5 * rs.rand()) * np.array([1, 1, -1 if pos[2] > 0 else 1])
        cone = dict(cone_axis=tuple(-pos + 0.2 * rs.randn(3)), cone_inner=0.2 + 0.1 * rs.rand(), cone_outer=0.5 + 0.3 * rs.rand()) if i % 3 == 2 else {}
        recs.append(LL.record(tuple(pos), 0.1 * (i % 2), tuple(rs.rand(3) * 0.4), tuple(rs.rand(3)), tuple(rs.rand(3) * 0.5), 2.0 + 10 * rs.rand(),
                              0.8 + rs.rand(), **cone))
    g = lambda sh, what: guarded_empty(sh, what=what)
    inp = dict(rays_o=guarded_copy(_cuda(eye), "rays_o"), rays_d=guarded_copy(_cuda(rd), "rays_d"), t=guarded_copy(_cuda(tt), "t"),
               status=guarded_copy(_cuda(status, torch.uint8), "status"), hit_slot=guarded_copy(_cuda(slot_np, torch.int32), "hit_slot"),
               hit_points=guarded_copy(_cuda(pts), "hp"), grad=guarded_copy(_cuda(nrm * 2.0), "grad"),
               rgb=guarded_copy(torch.rand(n_hit, 3).cuda(), "rgb"), w2b=guarded_copy(torch.eye(4).cuda(), "w2b"),
               lights=guarded_copy(_cuda(recs), "lights"), bg=guarded_copy(torch.tensor([0.1, 0.2, 0.3]).cuda(), "bg"),
               visibility=guarded_copy(torch.rand(Lt, N).cuda(), "vis"), ambient_occlusion=guarded_copy(torch.rand(N).cuda(), "ao"))
    names = ("depth", "position", "normal", "normal_world", "albedo", "mask")
    shapes = dict(depth=(N,), position=(N, 3), normal=(N, 3), normal_world=(N, 3), albedo=(N, 3), mask=(N,))
    outs = {k: g(shapes[k], k) for k in names}
    outs["image"] = g((Lt, 3, N), "image")
    P = lib.SurfaceAoParams()
    P.N, P.n_hit, P.L = N, n_hit, Lt
    for k_, v_ in {**inp, **outs}.items():
        setattr(P, k_, _p(v_))
    assert L_.oi_surface_shade_local(ctypes.byref(P), st) == 0
    ref = LL.shade(npd(inp["rays_o"])[on], npd(inp["hit_points"])[slot_np[on]], npd(inp["grad"])[slot_np[on]], npd(inp["rgb"])[slot_np[on]],
                   np.eye(4), npd(inp["lights"]), npd(inp["visibility"])[:, on], npd(inp["ambient_occlusion"])[on])
    err = np.abs(npd(outs["image"])[:, :, on] - ref).max((1, 2))
    # These lights are not the golden ones: att reaches ~5, the exponents 12, the cones are narrow.  Per light, from the number
    # formats (eps = 2^-24): the unit direction l, the unit axis and a dot product carry about 3 roundings each; att 4; the
    # specular base al = v . r about 6, raised to the shininess; the cone's smoothstep has slope <= 1.5 / (cos_inner - cos_outer)
    # in the cosine (10 eps).  All of it scales with att (diffuse + specular).
    lt64, eps = npd(inp["lights"]), 2.0 ** -24
    att = np.stack([LL.factors(pts[slot_np[on]], rec, np.eye(4))[1].max() for rec in lt64])
    peak = att * (lt64[:, 8:11].max(1) + lt64[:, 12:15].max(1))
    cone = np.where(lt64[:, 11] > -1, 1.5 * 10 / np.maximum(lt64[:, 19] - lt64[:, 11], 1e-3), 0.0)
    bar = RELIGHT_BAR + eps * (16 + 6 * lt64[:, 15] + cone) * peak
    print("local_light_shade_256: worst error over bar", float((err / bar).max()), "worst error", float(err.max()), "bars", float(bar.min()),
          float(bar.max()))
    record_margin("local_light_shade_256", "error_over_bar", float((err / bar).max()))
    assert (err < bar).all()
    off = slot_np < 0
    assert off.sum() == 3 and torch.equal(outs["image"][:, :, torch.from_numpy(off).cuda()], inp["bg"][None, :, None].expand(Lt, 3, 3))
    # the G-buffer: oi_surface_shade's bytes
    Q = lib.SurfaceParams()
    Q.N, Q.n_hit, Q.L = N, n_hit, 0
    base = {k: g(shapes[k], "b_" + k) for k in names}
    for k_, v_ in {**{k: v for k, v in inp.items() if k not in ("lights", "visibility", "ambient_occlusion")}, **base}.items():
        setattr(Q, k_, _p(v_))
    assert L_.oi_surface_shade(ctypes.byref(Q), st) == 0
    for k in names:
        assert torch.equal(_bits(outs[k]), _bits(base[k])), k


# ---------------------------------------------------------------------------------------------------------------------
# 4 - 6. the shade on a golden view
# ---------------------------------------------------------------------------------------------------------------------
def _shade_args(s, lt, bg=(0.1, 0.2, 0.3)):
    from oi_amd import trace
    r = s.res
    return (s.ro, s.rd, r.t, r.status, r.hit_slot, r.hit_points, s.grad, s.rgb, s.n_hit, s.w2b, lt, trace._bg(bg, "cuda"))


def _fp64_image(s, recs, vis=None, ao=None):
    hit = s.res.hit_index.long()
    v = None if vis is None else npd(vis)[:, hit.cpu().numpy()]
    a = None if ao is None else npd(ao)[hit.cpu().numpy()]
    return LL.shade(npd(s.ro[hit]), npd(s.res.hit_points), npd(s.grad), npd(s.rgb), npd(s.w2b), recs, v, a), hit


@pytest.mark.parametrize("precision", PRECISIONS)
def test_shade_against_the_restatement(precision):
    from oi_amd import ops
    seed, pose = R.SOFT_VIEWS[0]
    gen, s = OC.surface(precision, seed, pose)
    lights = golden_lights(pose)
    lights.append(lights[0].replace(cone_axis=tuple(-np.asarray(LL.golden_positions(pose)[0]) + np.asarray(T.pose(pose)[:3, 3])),
                                    cone_inner=0.3, cone_outer=0.9))
    lt = stacked(lights)
    L, N = lt.shape[0], s.N
    vis, ao = torch.rand(L, N).cuda(), torch.rand(N).cuda()
    for v, a in ((None, None), (vis, None), (vis, ao)):
        out = ops.surface_shade_local(*_shade_args(s, lt), v, a)
        ref, hit = _fp64_image(s, npd(lt), v, a)
        err = float(np.abs(npd(out["image"])[:, :, hit.cpu().numpy()] - ref).max())
        record_margin(f"local_light_shade[{precision}]", "image_vs_fp64", err)
        print(f"local_light_shade[{precision}] image against fp64", err, "largest value", float(np.abs(ref).max()))
        assert err < RELIGHT_BAR
        base = ops.surface_shade(*_shade_args(s, None), None, tuple(ops.SURFACE_OUT))
        for k in ops.SURFACE_OUT:                                                 # the G-buffer: oi_surface_shade's bytes
            assert torch.equal(_bits(out[k]), _bits(base[k])), k
        off = s.res.status != T.HIT
        assert torch.equal(out["image"][:, :, off], torch.tensor([0.1, 0.2, 0.3]).cuda()[None, :, None].expand(L, 3, int(off.sum())))
        for l in range(L):                                                        # result l of an L-light launch: the 1-light launch
            one = ops.surface_shade_local(*_shade_args(s, lt[l:l + 1]), None if v is None else v[l:l + 1], a, ("image",))
            assert torch.equal(_bits(one["image"][0]), _bits(out["image"][l])), l


@pytest.mark.parametrize("precision", PRECISIONS)
def test_directional_limit(precision):
    from oi_amd import ops
    from oi_amd.relight import Light, LocalLight, stack_lights
    seed, pose = R.SOFT_VIEWS[0]
    gen, s = OC.surface(precision, seed, pose)
    D = 1e3
    centre = tuple(float(x) for x in T.pose(pose)[:3, 3])                          # the object's centre in the world
    for d in T.LIGHT_DIRS[:2]:
        light = Light(direction=d, ambient=(0.2, 0.3, 0.25), diffuse=(0.7, 0.5, 0.6), specular=(0.35, 0.3, 0.2), shininess=6.0)
        a = ops.surface_shade(*_shade_args(s, stack_lights([light], "cuda")), None, ("image",))["image"]
        b = ops.surface_shade_local(*_shade_args(s, stacked([LocalLight.from_light(light, D, centre)])), None, None, ("image",))["image"]
        dev = float((a - b).abs().max())
        record_margin(f"local_light_limit[{precision}]", "deviation_times_D", dev * D)
        print(f"local_light_limit[{precision}] deviation", dev, "bound", 3.0 / D * 0.7 + RELIGHT_BAR)
        assert dev <= 3.0 / D * max(light.diffuse + light.specular) + RELIGHT_BAR


@pytest.mark.parametrize("precision", PRECISIONS)
def test_cone(precision):
    from oi_amd import ops
    seed, pose = R.SOFT_VIEWS[0]
    gen, s = OC.surface(precision, seed, pose)
    plain = golden_lights(pose)[0]
    hit = s.res.hit_index.long()
    pts, w2b = npd(s.res.hit_points), npd(s.w2b)
    # the cone: from the restatement, aimed at the visible points' centroid with half-angles at the 30th and 70th percentile
    rec = npd(stacked([plain]))[0]
    l, _, _ = LL.factors(pts, rec, w2b)
    q, _ = LL.in_frame(rec, w2b)
    axis_box = pts.mean(0) - q
    axis_box /= np.linalg.norm(axis_box)
    ang = np.arccos(np.clip(-(l @ axis_box), -1, 1))
    inner, outer = float(np.percentile(ang, 30)), float(np.percentile(ang, 70))
    axis_world = tuple(w2b[:3, :3].T @ axis_box)
    spot = plain.replace(cone_axis=axis_world, cone_inner=inner, cone_outer=outer)
    img = {}
    for name, lt in (("plain", plain), ("spot", spot)):
        img[name] = ops.surface_shade_local(*_shade_args(s, stacked([lt])), None, None, ("image", "albedo"))
    c = -(l @ (w2b[:3, :3] @ (np.asarray(axis_world) / np.linalg.norm(axis_world))))
    margin = 1e-5                                                                 # a pixel is classified only clear of the cone's edges
    outside, inside = c < np.cos(outer) - margin, c > np.cos(inner) + margin
    between = (c > np.cos(outer) + margin) & (c < np.cos(inner) - margin)
    assert outside.sum() > 5 and inside.sum() > 5 and between.sum() > 5
    sp, pl = img["spot"]["image"][0][:, hit], img["plain"]["image"][0][:, hit]
    amb = torch.tensor(plain.ambient).cuda()[:, None] * img["spot"]["albedo"][hit].T
    o_, i_, b_ = (torch.from_numpy(m).cuda() for m in (outside, inside, between))
    assert torch.equal(sp[:, o_], amb[:, o_])                                      # outside: ambient x albedo, bit for bit
    assert torch.equal(_bits(sp[:, i_].contiguous()), _bits(pl[:, i_].contiguous()))   # inside: the light without a cone
    ref, _ = _fp64_image(s, npd(stacked([spot])))
    assert float(np.abs(npd(sp) - ref[0]).max()) < RELIGHT_BAR
    assert (npd(sp[:, b_]) <= npd(pl[:, b_]) + 1e-7).all() and (npd(sp[:, b_]).sum(0) < npd(pl[:, b_]).sum(0)).any()


# ---------------------------------------------------------------------------------------------------------------------
# 7. render_surface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("seed,pose", R.SOFT_VIEWS)
def test_render_surface_with_local_lights(precision, S, seed, pose):
    from oi_amd import trace
    gen = G.make_gen(precision, R.R_SOFT)
    z, b2w = A.latent(seed)[0], T.pose(pose)
    lights = golden_lights(pose)
    out = trace.render_surface(gen, z, b2w, lights=lights, shadows=True, shadow_samples=S, seed=R.SEED, bg=(0.1, 0.2, 0.3))
    H, L = R.R_SOFT, 2
    assert set(out) == {"depth", "position", "normal_map", "normal_object", "albedo", "mask", "image", "visibility", "shadow_trace",
                        "stats", "trace"}
    assert out["image"].shape == (L, 3, H, H) and out["visibility"].shape == (L, 1, H, H)
    res, st, fld = out["trace"], out["shadow_trace"], T.Field(seed)
    n_hit = len(res.hit_index)
    assert st.N == L * S * n_hit
    status = st.status.cpu().numpy()
    o, d, t, far = npd(st.rays_o), npd(st.rays_d), npd(st.t), npd(st.far)
    lit, occl = (status == T.MISS) & (far > 0), status == T.HIT
    seg = T.segment_min(fld.sdf, o[lit], d[lit], np.zeros(int(lit.sum())), far[lit])
    at = fld.sdf(o[occl] + t[occl, None] * d[occl])
    lim, si, nf = (int((status == c).sum()) for c in (T.LIMIT, T.START_INSIDE, T.NONFINITE))
    traced = int((status != T.BACKFACING).sum())
    case = f"local_light_golden[{precision},seed={seed},{pose},S={S}]"
    print(case, dict(rays=st.N, traced=traced, lit=int(lit.sum()), occluded=int(occl.sum()), limit=lim))
    record_margin(case, "limit_share", lim / max(1, traced))
    assert lit.sum() > 0 and seg.min(initial=np.inf) >= -SDF_BAR and at.max(initial=-np.inf) <= T.TOL + SDF_BAR
    assert lim <= R.LIMIT_CAP * traced and si == 0 and nf == 0 and status.max() <= T.BACKFACING
    # the rays: the restatement's, and they end at the light
    _, s = OC.surface(precision, seed, pose)
    assert torch.equal(s.res.t, res.t) and torch.equal(s.res.status, res.status)
    sl = s.res.hit_slot[res.hit_index.long()].long()
    grad, rgb = npd(s.grad[sl]), npd(s.rgb[sl])
    w2b = npd(s.w2b)
    refs = [LL.rays(npd(res.hit_points), grad, res.hit_index.cpu().numpy(), rec, w2b, S, R.SEED) for rec in npd(stacked(lights))]
    ref = {k: np.stack([r[k] for r in refs]) for k in ("o", "d", "far", "status")}
    sh = (L, S, n_hit)
    begin = np.where(status.reshape(sh) == T.BACKFACING, T.BACKFACING, np.where(far.reshape(sh) > 0, T.MARCH, T.MISS))
    _compare_rays(case, o.reshape(*sh, 3), d.reshape(*sh, 3), far.reshape(sh), begin, ref, A.unit(grad))
    vis = npd(out["visibility"]).reshape(L, -1)
    assert np.array_equal(vis, R.resolve(status, res.hit_slot.cpu().numpy(), n_hit, L, S))
    assert set(np.unique(vis * S)) <= set(range(S + 1))
    hit = res.hit_index.long().cpu().numpy()
    image = LL.shade(npd(s.ro)[hit], npd(res.hit_points), grad, rgb, w2b, npd(stacked(lights)), vis[:, hit])
    err = float(np.abs(npd(out["image"]).reshape(L, 3, -1)[:, :, hit] - image).max())
    record_margin(case, "image_vs_fp64", err)
    assert err < RELIGHT_BAR
    if S == 4 and seed == R.SOFT_VIEWS[0][0]:
        # one element of render_surfaces is render_surface
        both = trace.render_surfaces(gen, [z, A.latent(1)[0]], [b2w, b2w], lights=lights, shadows=True, shadow_samples=S, seed=R.SEED,
                                     bg=(0.1, 0.2, 0.3))
        for k in ("image", "visibility", "depth", "mask"):
            assert torch.equal(_bits(both[0][k]), _bits(out[k])), k
        for bad in (dict(light_radius=0.1), dict(lights=lights + G.lights()[:1])):
            with pytest.raises(ValueError):
                trace.render_surface(gen, z, b2w, **{**dict(lights=lights, shadows=True), **bad})


@pytest.mark.parametrize("precision", PRECISIONS)
def test_directional_lights_launch_no_new_entry(precision, monkeypatch):
    from oi_amd import ops, trace
    gen = G.make_gen(precision, R.R_SOFT)
    z, b2w = A.latent(0)[0], T.pose("centre")
    kw = dict(lights=G.lights(), shadows=True, shadow_samples=R.SOFT_S, light_radius=R.SOFT_RADIUS, ao_samples=R.AO_S, seed=R.SEED)
    plain = trace.render_surface(gen, z, b2w, **kw)

    def refuse(*a, **k):
        raise AssertionError("an entry of include/oi_local_light.h ran under directional lights")
    for name in NEW_OPS:
        monkeypatch.setattr(ops, name, refuse)
    same = trace.render_surface(gen, z, b2w, **kw)
    default = trace.render_surface(gen, z, b2w)
    monkeypatch.undo()
    assert set(plain) == set(same) and default["image"].shape[0] == 1
    for k, v in plain.items():
        if torch.is_tensor(v):
            assert torch.equal(_bits(v), _bits(same[k])), k


# ---------------------------------------------------------------------------------------------------------------------
# 9. the orbit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_surface_light_orbit(precision, monkeypatch):
    from oi_amd import inference, ops, trace
    gen = G.make_gen(precision, R.R_SOFT)
    seed, pose = R.SOFT_VIEWS[1]
    z, b2w = A.latent(seed)[0], T.pose(pose)
    light = golden_lights(pose)[1]
    centre = tuple(float(x) for x in b2w[:3, 3])
    kw = dict(n_frames=5, centre=centre, radius=1.6, height=0.4, shadows=True, shadow_samples=R.SOFT_S, seed=R.SEED)
    whole = inference.surface_light_orbit(gen, z, b2w, light, **kw)
    H = R.R_SOFT
    assert whole["image"].shape == (5, 3, H, H) and whole["visibility"].shape == (5, 1, H, H) and whole["positions"].shape == (5, 3)
    assert np.allclose(whole["positions"], inference.light_orbit_positions(centre, 1.6, 5, height=0.4))
    n_hit = whole["stats"]["hit"]
    sizes, begin = [], ops.local_light_begin

    def counting(st, *a, **k):
        sizes.append(st.N)
        return begin(st, *a, **k)
    monkeypatch.setattr(ops, "local_light_begin", counting)
    monkeypatch.setattr(inference, "OCCLUSION_MAX_RAYS", 2 * R.SOFT_S * n_hit)      # two lights per trace: 2 + 2 + 1
    split = inference.surface_light_orbit(gen, z, b2w, light, **kw)
    monkeypatch.undo()
    assert sizes == [2 * R.SOFT_S * n_hit] * 2 + [R.SOFT_S * n_hit]
    for k in ("image", "visibility", "mask", "depth"):
        assert torch.equal(_bits(whole[k]), _bits(split[k])), k
    for f in (0, 3):                                                              # frame f: render_surface under the light at position f
        one = trace.render_surface(gen, z, b2w, lights=[light.replace(position=tuple(whole["positions"][f]))], shadows=True,
                                   shadow_samples=R.SOFT_S, seed=R.SEED)
        assert torch.equal(_bits(one["image"][0]), _bits(whole["image"][f])) and torch.equal(one["visibility"][0], whole["visibility"][f])
    with pytest.raises(TypeError):
        inference.surface_light_orbit(gen, z, b2w, G.lights()[0], n_frames=2)
