"""Soft shadows and ambient occlusion on the MI355X (include/oi_occlusion.h; oi_amd.trace.render_surface's shadow_samples /
light_radius / ao_samples; oi_amd.inference.surface_light_walk).  The references: the hard-shadow entries of include/oi_trace.h
where the new ones must reproduce them bit for bit, the fp64 restatement tests/helpers/occlusion_ref.py, the fp64 oracle's
field on the golden weights (the caps are those rehearsed on the oracle alone by tests/test_occlusion_cpu.py, for the same
views, lights, radius and sample counts), and an analytic two-sphere scene whose occlusion is known."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_trace as G
from conftest import record_margin
from helpers import mesh_attr_ref as A
from helpers import occlusion_ref as R
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

SDF_BAR, RELIGHT_BAR, PRECISIONS, npd = G.SDF_BAR, G.RELIGHT_BAR, G.PRECISIONS, G.npd
# shadow-ray origins and directions / far against the restatement: the bars of test_gpu_trace's shadow rays
RAY_BAR, FAR_BAR = 1e-6, 1e-5

_SOFT = {}


def soft_lights():
    from oi_amd.relight import Light
    return [Light(direction=d, specular=0.35, shininess=6.0) for d in R.SOFT_LIGHTS]


def surface(precision, seed, pose):
    """A traced 24 x 24 golden view and what the light-dependent stages reuse (oi_amd.trace._Surface)."""
    from oi_amd import trace
    gen = G.make_gen(precision, R.R_SOFT)
    return gen, trace._Surface(gen, A.latent(seed)[0].cuda().reshape(1, -1), T.pose(pose), T.BIAS, {})


def run_soft(precision, seed, pose):
    """render_surface with soft shadows and ambient occlusion at the rehearsed settings; cached."""
    key = (precision, seed, pose)
    if key not in _SOFT:
        from oi_amd import trace
        gen = G.make_gen(precision, R.R_SOFT)
        b2w = T.pose(pose)
        out = trace.render_surface(gen, A.latent(seed)[0], b2w, lights=soft_lights(), shadows=True, shadow_samples=R.SOFT_S,
                                   light_radius=R.SOFT_RADIUS, ao_samples=R.AO_S, ao_distance=R.AO_DISTANCE, seed=R.SEED)
        ro, rd, _, _, w2b = trace._view_rays(gen, b2w)
        # the gradient and albedo at the hits, in the order of out's hit list (a second, identical trace; slots may differ)
        _, s = surface(precision, seed, pose)
        hit = out["trace"].hit_index.long()
        assert torch.equal(s.res.t, out["trace"].t) and torch.equal(s.res.status, out["trace"].status)
        sl = s.res.hit_slot[hit].long()
        _SOFT[key] = dict(out=out, ro=npd(ro), rd=npd(rd), w2b=npd(w2b), grad=npd(s.grad[sl]), rgb=npd(s.rgb[sl]), hit=hit,
                          fld=T.Field(seed), gen=gen, b2w=b2w)
    return _SOFT[key]


def _state_arrays(st):
    return dict(rays_o=st.rays_o, rays_d=st.rays_d, near=st.near, far=st.far, t=st.t, status=st.status, steps=st.steps,
                bracket=st.bracket, side=st.side)


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


@pytest.mark.parametrize("precision", PRECISIONS)
def test_identity_with_the_hard_path(precision, monkeypatch):
    from oi_amd import ops, trace
    from oi_amd.relight import stack_lights
    gen, s = surface(precision, 0, "centre")
    lt = stack_lights(G.lights(), "cuda")
    L, n_hit, N = lt.shape[0], s.n_hit, s.N
    assert L == 3 and n_hit > 50
    hard, soft = ops.TraceState(L * n_hit, ref=s.ro), ops.TraceState(L * n_hit, ref=s.ro)
    ops.trace_shadow_begin(hard, s.res.hit_points, s.grad, n_hit, lt, s.w2b, T.BIAS)
    ops.occlusion_light_begin(soft, s.res.hit_points, s.grad, s.res.hit_index, n_hit, lt, torch.zeros(L).cuda(), 1, s.w2b, T.BIAS,
                              seed=12345)
    for name, a in _state_arrays(hard).items():
        assert torch.equal(_bits(a), _bits(_state_arrays(soft)[name])), name
    assert torch.equal(hard.counts, soft.counts)
    n0 = int(hard.counts[0].item())
    assert 0 < n0 < L * n_hit and sorted(hard.active[0, :n0].tolist()) == sorted(soft.active[0, :n0].tolist())
    # the resolve at S = 1 is the visibility map
    trace._march(s.field, hard, n0, *s.kw)
    ops.trace_finish(hard)
    vis = ops.trace_visibility(hard.status, s.res.hit_slot, N, n_hit, L)
    assert torch.equal(vis, ops.occlusion_resolve(hard.status, s.res.hit_slot, N, n_hit, L, 1))
    assert float(vis.min()) == 0.0 and float(vis.max()) == 1.0
    # the shade entry without an occlusion factor is oi_surface_shade, every output
    r = s.res
    args = (s.ro, s.rd, r.t, r.status, r.hit_slot, r.hit_points, s.grad, s.rgb, n_hit, s.w2b, lt, trace._bg((0.1, 0.2, 0.3), "cuda"))
    for v in (None, vis):
        a, b = ops.surface_shade(*args, v), ops.surface_shade_ao(*args, v, None)
        assert set(a) == set(b) == set(ops.SURFACE_OUT) | {"image"}
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
    # render_surface at the default new arguments: the call without them, and none of the new entries runs
    z, b2w = A.latent(0)[0], T.pose("centre")
    plain = trace.render_surface(gen, z, b2w, lights=G.lights(), shadows=True)

    def refuse(*a, **k):
        raise AssertionError("an entry of include/oi_occlusion.h ran on the default path")
    for name in ("occlusion_light_begin", "occlusion_ambient_begin", "occlusion_step", "occlusion_resolve", "surface_shade_ao"):
        monkeypatch.setattr(ops, name, refuse)
    same = trace.render_surface(gen, z, b2w, lights=G.lights(), shadows=True, shadow_samples=1, light_radius=0.0, ao_samples=0,
                                ao_distance=0.5, seed=0)
    monkeypatch.undo()
    assert set(plain) == set(same) and "ambient_occlusion" not in same
    for k, v in plain.items():
        if torch.is_tensor(v):
            assert torch.equal(_bits(v), _bits(same[k])), k
    assert plain["stats"] == same["stats"] and same["stats"]["ao_evals"] == 0

    def shadow_states(o):   # per light and pixel on the mask: the slots of two primary traces need not be the same
        sl = o["trace"].hit_slot
        return o["shadow_trace"].status.view(L, n_hit)[:, sl[sl >= 0].long()]
    assert torch.equal(shadow_states(plain), shadow_states(same)) and same["shadow_trace"].N == L * n_hit


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rays_against_the_restatement(precision):
    v = run_soft(precision, *R.SOFT_VIEWS[0])
    out = v["out"]
    res = out["trace"]
    n_hit, L, S = len(res.hit_index), len(R.SOFT_LIGHTS), R.SOFT_S
    pix, pts = res.hit_index.cpu().numpy(), npd(res.hit_points)
    nrm = A.unit(v["grad"])
    case = f"occlusion_rays[{precision}]"

    def compare(st, ref, shape, what):
        o, d, far, traced = ref
        ko, kd, kfar = npd(st.rays_o).reshape(*shape, 3), npd(st.rays_d).reshape(*shape, 3), npd(st.far).reshape(shape)
        e_o, e_d, e_f = float(np.abs(ko - o).max()), float(np.abs(kd - d).max()), float(np.abs(kfar - far).max())
        print(case, what, "origins", e_o, "directions", e_d, "far", e_f)
        record_margin(case, what + "_directions", e_d)
        assert e_o < RAY_BAR and e_d < RAY_BAR and e_f < FAR_BAR
        assert np.abs(np.linalg.norm(kd, axis=-1) - 1).max() < RAY_BAR
        k_traced = st.status.cpu().numpy().reshape(shape) != T.BACKFACING
        differ = k_traced != traced                                            # only where n . d rounds across zero
        assert not differ.any() or np.abs((nrm * d).sum(-1)[differ]).max() < RAY_BAR
        assert not npd(st.near).any()

    lo, ld, lfar, ltr = (np.stack(x) for x in zip(*[R.light_rays(pts, v["grad"], pix, T.light_object_dir(dd, v["w2b"]), R.SOFT_RADIUS, S,
                                                              R.SEED) for dd in R.SOFT_LIGHTS]))
    compare(out["shadow_trace"], (lo, ld, lfar, ltr), (L, S, n_hit), "light")
    # every sample lies in its light's cap
    kd = npd(out["shadow_trace"].rays_d).reshape(L, S, n_hit, 3)
    for i, dd in enumerate(R.SOFT_LIGHTS):
        assert ((kd[i] * T.light_object_dir(dd, v["w2b"])).sum(-1) >= np.cos(R.SOFT_RADIUS) - RAY_BAR).all()
    compare(out["ao_trace"], R.ambient_rays(pts, v["grad"], pix, R.AO_S, R.SEED), (R.AO_S, n_hit), "ambient")
    assert float(out["ao_trace"].far.max()) <= R.AO_DISTANCE


@pytest.mark.parametrize("precision", PRECISIONS)
def test_anyhit_against_full_on_the_gpu(precision):
    from oi_amd import ops, trace
    from oi_amd.relight import stack_lights
    gen, s = surface(precision, *R.SOFT_VIEWS[0])
    lt = stack_lights(soft_lights(), "cuda")
    L, n_hit, N = lt.shape[0], s.n_hit, s.N
    radius = torch.full((L,), R.SOFT_RADIUS).cuda()
    tol, omega, max_steps, _ = s.kw

    def light(st):
        ops.occlusion_light_begin(st, s.res.hit_points, s.grad, s.res.hit_index, n_hit, lt, radius, R.SOFT_S, s.w2b, T.BIAS, R.SEED)

    def ambient(st):
        ops.occlusion_ambient_begin(st, s.res.hit_points, s.grad, s.res.hit_index, n_hit, R.AO_S, T.BIAS, R.AO_DISTANCE, R.SEED)

    for what, begin, Lq, S in (("light", light, L, R.SOFT_S), ("ambient", ambient, 1, R.AO_S)):
        vis, evals = {}, {}
        for anyhit in (False, True):
            st = ops.TraceState(Lq * S * n_hit, ref=s.ro)
            begin(st)
            evals[anyhit], _ = trace._march(s.field, st, int(st.counts[0].item()), tol, omega, max_steps, 1, anyhit=anyhit)
            if anyhit:
                assert not bool((st.status == T.REFINE).any())
                assert evals[True] == int(st.steps.sum())                      # a count read every step: no stale slot
            ops.trace_finish(st)
            vis[anyhit] = ops.occlusion_resolve(st.status, s.res.hit_slot, N, n_hit, Lq, S)
        print(f"occlusion_anyhit[{precision},{what}] evaluations any-hit", evals[True], "full", evals[False])
        record_margin(f"occlusion_anyhit[{precision},{what}]", "evals_anyhit_over_full", evals[True] / max(1, evals[False]))
        assert torch.equal(vis[True], vis[False])
        assert evals[True] <= evals[False]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("seed,pose", R.SOFT_VIEWS)
def test_soft_shadows_and_ambient_occlusion_against_the_oracle(precision, seed, pose):
    v = run_soft(precision, seed, pose)
    out, fld, res = v["out"], v["fld"], v["out"]["trace"]
    n_hit, L = len(res.hit_index), len(R.SOFT_LIGHTS)
    slot = res.hit_slot.cpu().numpy()
    case = f"occlusion_golden[{precision},seed={seed},{pose}]"
    maps = {}
    for what, st, Lq, S in (("light", out["shadow_trace"], L, R.SOFT_S), ("ambient", out["ao_trace"], 1, R.AO_S)):
        assert st.N == Lq * S * n_hit
        status = st.status.cpu().numpy()
        o, d, t, far = npd(st.rays_o), npd(st.rays_d), npd(st.t), npd(st.far)
        lit, occl = status == T.MISS, status == T.HIT
        traced = int((status != T.BACKFACING).sum())
        seg = T.segment_min(fld.sdf, o[lit], d[lit], np.zeros(int(lit.sum())), far[lit])
        at = fld.sdf(o[occl] + t[occl, None] * d[occl])
        lim, si, nf = (int((status == c).sum()) for c in (T.LIMIT, T.START_INSIDE, T.NONFINITE))
        stats = {"rays": st.N, "traced": traced, "lit": int(lit.sum()), "occluded": int(occl.sum()), "limit": lim,
                 "lit_segment_min": float(seg.min(initial=np.inf)), "occluder_sdf_max": float(at.max(initial=-np.inf))}
        print(case, what, stats)
        record_margin(case, what + "_limit_share", lim / max(1, traced))
        assert traced > 0.5 * st.N and lit.sum() > 0
        assert seg.min(initial=np.inf) >= -SDF_BAR
        assert at.max(initial=-np.inf) <= T.TOL + SDF_BAR
        assert lim <= R.LIMIT_CAP * traced
        assert si == 0 and nf == 0 and status.max() <= T.BACKFACING
        maps[what] = R.resolve(status, slot, n_hit, Lq, S)
    H = R.R_SOFT
    vis, ao = npd(out["visibility"]).reshape(L, -1), npd(out["ambient_occlusion"]).reshape(-1)
    assert out["visibility"].shape == (L, 1, H, H) and out["ambient_occlusion"].shape == (1, 1, H, H)
    assert np.array_equal(vis, maps["light"]) and np.array_equal(ao, maps["ambient"][0])
    assert set(np.unique(vis * R.SOFT_S)) <= set(range(R.SOFT_S + 1))
    assert out["stats"]["ao_evals"] > 0 and out["stats"]["shadow_evals"] > 0
    from oi_amd.relight import stack_lights
    hit = v["hit"].cpu().numpy()
    ref = R.shade(v["ro"][hit], v["rd"][hit], npd(res.t)[hit], v["grad"], v["rgb"], v["w2b"], npd(stack_lights(soft_lights())),
                  vis[:, hit], ao[hit])
    err = float(np.abs(npd(out["image"]).reshape(L, 3, -1)[:, :, hit] - ref).max())
    record_margin(case, "image_vs_fp64", err)
    print(case, "image against fp64", err)
    assert err < RELIGHT_BAR


# ---------------------------------------------------------------------------------------------------------------------
# through the C ABI on guarded buffers, the field evaluated by torch between the steps
# ---------------------------------------------------------------------------------------------------------------------
_p = lambda t_: ctypes.c_void_p(t_.data_ptr())


def _two_spheres(pts):
    c0, c1 = (torch.tensor(c, dtype=torch.float32, device=pts.device) for c in (R.C0, R.C1))
    return torch.minimum((pts - c0).norm(dim=-1) - R.R0, (pts - c1).norm(dim=-1) - R.R1)


def _guarded_state(Q, tag, rays=None):
    """An oi_trace_state of Q rays on guarded, poisoned buffers; rays: (rays_o, rays_d, near, far) of a primary trace, held as
    guarded inputs.  (The int16 step counts and the partly written lists carry guards only, as in
    test_gpu_trace._guarded_pass.)"""
    from oi_amd import lib
    g = lambda sh, dt=torch.float32, what="?", mw=True: guarded_empty(sh, dt, what=f"{tag}_{what}", must_write=mw)
    if rays is None:
        arr = dict(rays_o=g((Q, 3), what="rays_o"), rays_d=g((Q, 3), what="rays_d"), near_=g((Q,), what="near"), far_=g((Q,), what="far"))
    else:
        arr = {k_: guarded_copy(v_, f"{tag}_{k_}") for k_, v_ in zip(("rays_o", "rays_d", "near_", "far_"), rays)}
    arr.update(t=g((Q,), what="t"), status=g((Q,), torch.uint8, "status"), steps=g((Q,), torch.int16, "steps", False),
               bracket=g((Q, 4), what="bracket"), side=g((Q,), torch.uint8, "side"), active=g((2, Q), torch.int32, "active", False),
               points=g((Q, 3), what="points", mw=False), counts=g((lib.TRACE_COUNT_WORDS,), torch.int32, "counts"))
    S = lib.TraceState()
    S.N = Q
    for k_, v_ in arr.items():
        setattr(S, k_, _p(v_))
    return arr, S


def _anyhit_loop(arr, S, field, max_steps, stale=False):
    """oi_occlusion_step until no ray is in flight, then oi_trace_finish.  -> steps run."""
    from oi_amd import lib, ops
    L_, st = lib.load(), ops._stream()
    Q = S.N
    bound, k = int(arr["counts"][0].item()), 0
    assert bound == int((arr["status"] == T.MARCH).sum())
    while bound > 0 and k < max_steps:
        sdf = guarded_copy(field(arr["points"][:bound]), "sdf")
        assert L_.oi_occlusion_step(ctypes.byref(S), _p(sdf), bound, k, T.TOL, T.OMEGA, st) == 0
        k += 1
        bound = int(arr["counts"][k].item()) if not stale or k % 2 == 0 else bound       # a stale bound every other step
    assert not bool((arr["status"] == T.REFINE).any())
    hit_index = guarded_empty((Q,), torch.int32, what="f_hit_index", must_write=False)
    hit_points = guarded_empty((Q, 3), what="f_hit_points", must_write=False)
    hit_slot = guarded_empty((Q,), torch.int32, what="f_hit_slot")
    assert L_.oi_trace_finish(ctypes.byref(S), _p(hit_index), _p(hit_points), _p(hit_slot), st) == 0
    return k


def _light_begin(S, hp, grad, hit_index, n_hit, lts, radius, L, samples, w2b, seed, bias=T.BIAS):
    from oi_amd import lib, ops
    return lib.load().oi_occlusion_light_begin(ctypes.byref(S), _p(hp), _p(grad), _p(hit_index), n_hit, _p(lts), _p(radius), L, samples,
                                               _p(w2b), bias, seed, ops._stream())


def _resolve(status, hit_slot, N, n_hit, L, samples):
    from oi_amd import lib, ops
    out = guarded_empty((L, N), what="resolved")
    assert lib.load().oi_occlusion_resolve(_p(status), _p(hit_slot), N, n_hit, L, samples, _p(out), ops._stream()) == 0
    return out


def _cuda(x, dt=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dt).cuda()


def test_analytic_occluder_penumbra():
    """A sphere of radius 0.1 at height 0.8 above a sphere of radius 0.5, a light of angular radius 0.15 along the axis, 64
    samples at each of 16 x 16 points on top of the large sphere: per ray the state of the fp64 any-hit trace of the
    restatement's own rays (rays within 1e-4 of tangency to the occluder aside), an umbra, a lit rim and a penumbra between."""
    p64, n64 = R.analytic_patch()
    n_hit, S = len(p64), R.ANALYTIC_S
    pix = np.arange(n_hit) * 3 + 5
    hp, grad = guarded_copy(_cuda(p64), "hit_points"), guarded_copy(_cuda(n64 * 2.5), "grad")      # any positive multiple of n
    hit_index = guarded_copy(_cuda(pix, torch.int32), "hit_index")
    lts = guarded_copy(_cuda([T.light_block(R.ANALYTIC_AXIS)]), "lights")
    radius, w2b = guarded_copy(_cuda([R.ANALYTIC_RADIUS]), "radius"), guarded_copy(torch.eye(4).cuda(), "w2b")
    arr, St = _guarded_state(S * n_hit, "an")
    assert _light_begin(St, hp, grad, hit_index, n_hit, lts, radius, 1, S, w2b, R.SEED) == 0
    assert int(arr["counts"][0].item()) == S * n_hit                               # every sample faces the light
    T.assert_secondary_begin_state(arr)
    k = _anyhit_loop(arr, St, _two_spheres, 256)
    # the oracle: the restatement's rays through the fp64 machine
    o, d, far, traced = R.light_rays(npd(hp), npd(grad), pix, np.array(R.ANALYTIC_AXIS), R.ANALYTIC_RADIUS, S, R.SEED)
    assert traced.all()
    assert np.abs(npd(arr["rays_o"]).reshape(S, n_hit, 3) - o).max() < RAY_BAR
    assert np.abs(npd(arr["rays_d"]).reshape(S, n_hit, 3) - d).max() < RAY_BAR
    _, s_ref, _, _ = R.trace_anyhit(R.two_spheres, o, d, np.zeros(S * n_hit), far, max_steps=256)
    band = np.abs(R.closest_approach(o, d, far).reshape(-1) - R.R1) < R.TANGENCY_BAND
    status = arr["status"].cpu().numpy()
    print("analytic occluder: steps", k, "excluded", int(band.sum()), "of", band.size, "disagreements in the band",
          int((status != s_ref)[band].sum()), "states", np.bincount(status).tolist())
    assert band.sum() <= R.EXCLUDED_CAP * band.size
    assert np.array_equal(status[~band], s_ref[~band])
    slot = guarded_copy(torch.arange(n_hit, dtype=torch.int32).cuda(), "hit_slot")
    vis = npd(_resolve(arr["status"], slot, n_hit, n_hit, 1, S))[0]
    assert np.array_equal(vis, R.resolve(status, np.arange(n_hit), n_hit, 1, S)[0])
    r_xy = np.linalg.norm(p64[:, :2], axis=-1)
    # under the occluder's centre its disc (angular radius asin(0.1 / 0.29) = 0.35) covers the cap (0.15); at 0.2 from the
    # axis the disc (0.26 about a direction 0.53 off the axis) and the cap are 0.12 apart
    assert (r_xy < 0.03).sum() >= 4 and (vis[r_xy < 0.03] == 0).all()
    assert (r_xy > 0.2).sum() >= 50 and (vis[r_xy > 0.2] == 1).all()
    assert ((vis > 0) & (vis < 1)).mean() >= 0.10


def test_analytic_ambient_occlusion():
    """The point under the small sphere sees it in its hemisphere; a point on the large sphere's equator sees nothing."""
    from oi_amd import lib, ops
    pts = np.array([[0.0, 0.0, R.R0], [R.R0, 0.0, 0.0]])
    n_hit, S = 2, 64
    hp, grad = guarded_copy(_cuda(pts), "hit_points"), guarded_copy(_cuda(pts / R.R0), "grad")
    pix = np.array([11, 4])
    hit_index = guarded_copy(_cuda(pix, torch.int32), "hit_index")
    arr, St = _guarded_state(S * n_hit, "ao")
    assert lib.load().oi_occlusion_ambient_begin(ctypes.byref(St), _p(hp), _p(grad), _p(hit_index), n_hit, S, T.BIAS, 0.5, R.SEED,
                                                 ops._stream()) == 0
    assert int(arr["counts"][0].item()) == S * n_hit
    T.assert_secondary_begin_state(arr)
    o, d, far, _ = R.ambient_rays(pts, pts / R.R0, pix, S, R.SEED, distance=0.5)
    assert np.abs(npd(arr["rays_d"]).reshape(S, n_hit, 3) - d).max() < RAY_BAR and np.abs(npd(arr["far_"]).reshape(S, n_hit) - far).max() < FAR_BAR
    _anyhit_loop(arr, St, _two_spheres, 256)
    slot = guarded_copy(torch.tensor([1, -1, 0], dtype=torch.int32).cuda(), "hit_slot")   # three pixels, the middle one off the mask
    ao = npd(_resolve(arr["status"], slot, 3, n_hit, 1, S))[0]
    print("analytic ambient occlusion: equator", ao[0], "off the mask", ao[1], "under the occluder", ao[2])
    assert ao[0] == 1.0 and ao[1] == 1.0 and 0.5 < ao[2] < 1.0
    # cosine-weighted share of a disc of angular radius asin(0.1 / 0.29) about the normal: sin^2 = 0.119; S = 64 samples
    assert abs((1.0 - ao[2]) - (R.R1 / (R.C1[2] - R.R0 - T.BIAS)) ** 2) < 4.0 / S


def _shape_case(n_hit, S, L, seed, backfacing=False):
    """Every new entry through the C ABI on guarded buffers, twice.  -> the states of one run."""
    from oi_amd import lib, ops
    rs = np.random.RandomState(seed)
    nrm = rs.randn(n_hit, 3)
    # the upper half of the large sphere; within 55 degrees of its top where every sample of a cap about -z must face away
    nrm[:, 2] = np.abs(nrm[:, 2]) + (1.0 if backfacing else 0.0)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    dirs = [(0.0, 0.0, -1.0)] * L if backfacing else [(0.0, 0.0, 1.0), (0.9, 0.1, 0.3)][:L]
    N = n_hit + 3                                                              # three pixels off the mask
    slot_np = np.full(N, -1)
    slot_np[rs.permutation(N)[:n_hit]] = np.arange(n_hit)
    pix = np.zeros(n_hit, dtype=np.int64)
    pix[slot_np[slot_np >= 0]] = np.nonzero(slot_np >= 0)[0]
    hp, grad = guarded_copy(_cuda(nrm * R.R0), "hit_points"), guarded_copy(_cuda(nrm * 1.7), "grad")
    hit_index, slot = guarded_copy(_cuda(pix, torch.int32), "hit_index"), guarded_copy(_cuda(slot_np, torch.int32), "hit_slot")
    lts = guarded_copy(_cuda([T.light_block(dd) for dd in dirs]), "lights")
    radius, w2b = guarded_copy(_cuda([0.3, 0.0][:L]), "radius"), guarded_copy(torch.eye(4).cuda(), "w2b")
    runs = []
    for rep in range(2):
        arr, St = _guarded_state(L * S * n_hit, f"sh{rep}")
        assert _light_begin(St, hp, grad, hit_index, n_hit, lts, radius, L, S, w2b, seed) == 0
        T.assert_secondary_begin_state(arr)
        s0 = arr["status"].cpu().numpy()
        assert set(np.unique(s0)) <= {T.MARCH, T.BACKFACING} and int(arr["counts"][0].item()) == int((s0 == T.MARCH).sum())
        assert not bool(arr["counts"][1:].any())
        k = _anyhit_loop(arr, St, _two_spheres, T.MAX_STEPS, stale=rep == 1)
        vis = _resolve(arr["status"], slot, N, n_hit, L, S)
        # the ambient rays of the same points, as far as 0.3
        amb, Sa = _guarded_state(S * n_hit, f"am{rep}")
        assert lib.load().oi_occlusion_ambient_begin(ctypes.byref(Sa), _p(hp), _p(grad), _p(hit_index), n_hit, S, T.BIAS, 0.3, seed,
                                                     ops._stream()) == 0
        assert int(amb["counts"][0].item()) == S * n_hit and bool((amb["status"] == T.MARCH).all())
        T.assert_secondary_begin_state(amb)
        _anyhit_loop(amb, Sa, _two_spheres, T.MAX_STEPS, stale=rep == 1)
        ao = _resolve(amb["status"], slot, N, n_hit, 1, S)
        runs.append(dict(arr=arr, vis=vis, k=k, s0=s0, amb=amb, ao=ao))
    a, b = runs
    for name in ("rays_o", "rays_d", "near_", "far_", "t", "status", "steps"):
        assert torch.equal(_bits(a["amb"][name]), _bits(b["amb"][name])), "ambient " + name
    assert torch.equal(a["ao"], b["ao"])
    ao_o, ao_d, ao_far, _ = R.ambient_rays(npd(hp), npd(grad), pix, S, seed, distance=0.3)
    assert np.abs(npd(a["amb"]["rays_o"]).reshape(S, n_hit, 3) - ao_o).max() < RAY_BAR
    assert np.abs(npd(a["amb"]["rays_d"]).reshape(S, n_hit, 3) - ao_d).max() < RAY_BAR
    assert np.abs(npd(a["amb"]["far_"]).reshape(S, n_hit) - ao_far).max() < FAR_BAR and float(a["amb"]["far_"].max()) <= float(np.float32(0.3))
    ao_status = a["amb"]["status"].cpu().numpy()
    assert ao_status.max() <= T.NONFINITE                                        # terminal, and no ambient ray faces away
    assert np.array_equal(npd(a["ao"]), R.resolve(ao_status, slot_np, n_hit, 1, S))
    for name in ("rays_o", "rays_d", "near_", "far_", "t", "status", "steps"):
        assert torch.equal(_bits(a["arr"][name]), _bits(b["arr"][name])), name         # per ray, whatever the slots and bounds
    assert torch.equal(a["vis"], b["vis"])
    status = a["arr"]["status"].cpu().numpy()
    assert status.max() <= T.BACKFACING
    assert np.array_equal(npd(a["vis"]), R.resolve(status, slot_np, n_hit, L, S))
    assert (npd(a["vis"])[:, slot_np < 0] == 1).all()
    o, d, far, traced = (np.stack(x) for x in zip(*[R.light_rays(npd(hp), npd(grad), pix, T.light_object_dir(dd, np.eye(4)), r, S, seed)
                                                    for dd, r in zip(dirs, [0.3, 0.0])]))
    assert np.abs(npd(a["arr"]["rays_d"]).reshape(L, S, n_hit, 3) - d).max() < RAY_BAR
    assert np.abs(npd(a["arr"]["rays_o"]).reshape(L, S, n_hit, 3) - o).max() < RAY_BAR
    differ = (a["s0"].reshape(L, S, n_hit) == T.MARCH) != traced
    assert not differ.any() or np.abs((A.unit(npd(grad))[None, None] * d).sum(-1)[differ]).max() < RAY_BAR
    return a, slot_np


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("n_hit", [1, 63, 64, 65])
def test_guarded_shapes(n_hit, S, L):
    _shape_case(n_hit, S, L, seed=n_hit * 100 + S * 3 + L)


def test_guarded_every_ray_backfacing():
    a, slot = _shape_case(65, 3, 2, seed=9, backfacing=True)
    assert (a["s0"] == T.BACKFACING).all() and int(a["arr"]["counts"][0].item()) == 0 and a["k"] == 0
    assert not bool(a["arr"]["steps"].any())                                     # nothing marched
    assert (npd(a["vis"])[:, slot >= 0] == 0).all()


def test_guarded_256_samples():
    a, _ = _shape_case(5, 256, 1, seed=4)
    assert a["arr"]["status"].shape == (1280,)
    vis = npd(a["vis"])
    assert np.array_equal(vis * 256, np.round(vis * 256))


def test_guarded_shade_with_an_occlusion_factor():
    """oi_surface_shade_ao on guarded buffers: a primary trace of the large sphere, random visibility and occlusion."""
    from oi_amd import lib, ops
    L_, st = lib.load(), ops._stream()
    N, Lt = 65, 2
    ro, rd = G._bundle(N, 3)
    near, far = T.O.near_far_from_sphere(ro, rd)
    arr, S = _guarded_state(N, "pr", (ro, rd, near.reshape(-1), far.reshape(-1)))
    assert L_.oi_trace_begin(ctypes.byref(S), st) == 0
    sphere = lambda pts: pts.norm(dim=-1) - R.R0
    bound, k = N, 0
    while bound > 0 and k < T.MAX_STEPS:
        sdf = guarded_copy(sphere(arr["points"][:bound]), "sdf")
        assert L_.oi_trace_step(ctypes.byref(S), _p(sdf), bound, k, T.TOL, T.OMEGA, st) == 0
        k += 1
        bound = int(arr["counts"][k].item())
    hit_index = guarded_empty((N,), torch.int32, what="hit_index", must_write=False)
    hit_points = guarded_empty((N, 3), what="hit_points", must_write=False)
    hit_slot = guarded_empty((N,), torch.int32, what="hit_slot")
    assert L_.oi_trace_finish(ctypes.byref(S), _p(hit_index), _p(hit_points), _p(hit_slot), st) == 0
    n_hit = int(arr["counts"][-1].item())
    assert 0 < n_hit < N
    hp = guarded_copy(hit_points[:n_hit], "hp")
    grad, rgb = guarded_copy(hp * 2.0, "grad"), guarded_copy(torch.rand(n_hit, 3).cuda(), "rgb")
    lts = guarded_copy(_cuda([T.light_block((0.3, -0.8, -0.5)), T.light_block((0.0, 0.0, -1.0))]), "lights")
    w2b, bg = guarded_copy(torch.eye(4).cuda(), "w2b"), guarded_copy(torch.tensor([0.1, 0.2, 0.3]).cuda(), "bg")
    vis, ao = guarded_copy(torch.rand(Lt, N).cuda(), "vis"), guarded_copy(torch.rand(N).cuda(), "ao")
    g = lambda sh, what: guarded_empty(sh, what=what)
    outs = dict(depth=g((N,), "depth"), position=g((N, 3), "position"), normal=g((N, 3), "normal"), normal_world=g((N, 3), "normal_world"),
                albedo=g((N, 3), "albedo"), mask=g((N,), "mask"), image=g((Lt, 3, N), "image"))
    P = lib.SurfaceAoParams()
    P.N, P.n_hit, P.L = N, n_hit, Lt
    for k_, v_ in dict(rays_o=arr["rays_o"], rays_d=arr["rays_d"], t=arr["t"], status=arr["status"], hit_slot=hit_slot, hit_points=hp,
                       grad=grad, rgb=rgb, w2b=w2b, lights=lts, bg=bg, visibility=vis, ambient_occlusion=ao, **outs).items():
        setattr(P, k_, _p(v_))
    assert L_.oi_surface_shade_ao(ctypes.byref(P), st) == 0
    idx = hit_index[:n_hit].long()
    ref = R.shade(npd(ro[idx]), npd(rd[idx]), npd(arr["t"][idx]), npd(grad), npd(rgb), np.eye(4), npd(lts), npd(vis[:, idx]), npd(ao[idx]))
    assert np.abs(npd(outs["image"][:, :, idx]) - ref).max() < RELIGHT_BAR
    off = arr["status"] != T.HIT
    assert torch.equal(outs["image"][:, :, off], bg[None, :, None].expand(Lt, 3, int(off.sum())))
    # an occlusion factor of 1 everywhere changes nothing but the rounding of one product
    one = guarded_copy(torch.ones(N).cuda(), "ao1")
    P.ambient_occlusion = _p(one)
    img1 = g((Lt, 3, N), "image1")
    P.image = _p(img1)
    for k_ in ("depth", "position", "normal", "normal_world", "albedo", "mask"):
        setattr(P, k_, None)
    assert L_.oi_surface_shade_ao(ctypes.byref(P), st) == 0
    P.ambient_occlusion = None
    img0 = g((Lt, 3, N), "image0")
    P.image = _p(img0)
    assert L_.oi_surface_shade_ao(ctypes.byref(P), st) == 0
    assert torch.equal(img0, img1)                                               # 1 * c_a is c_a


@pytest.mark.parametrize("precision", PRECISIONS)
def test_surface_frames_pass_the_new_arguments_through(precision):
    from oi_amd import inference, trace
    gen = G.make_gen(precision, R.R_SOFT)
    zs, b2ws = [A.latent(0)[0], A.latent(1)[0]], [T.pose("centre"), T.pose("off")]
    kw = dict(shadows=True, shadow_samples=R.SOFT_S, light_radius=R.SOFT_RADIUS, ao_samples=R.AO_S, ao_distance=R.AO_DISTANCE, seed=R.SEED)
    keys = ("image", "visibility", "ambient_occlusion", "mask")
    fr = inference.surface_frames(gen, zs, b2ws, keys=keys, **kw)
    H = R.R_SOFT
    assert fr["image"].shape == (2, 3, H, H) and fr["visibility"].shape == fr["ambient_occlusion"].shape == (2, 1, H, H)
    for i, (z, b2w) in enumerate(zip(zs, b2ws)):
        one = trace.render_surface(gen, z, b2w, **kw)
        for k in keys:
            assert torch.equal(fr[k][i], one[k][0]), (k, i)
    hard = inference.surface_frames(gen, zs, b2ws, keys=("image", "visibility"), shadows=True)
    assert set(np.unique(npd(hard["visibility"]))) <= {0.0, 1.0}
    assert set(np.unique(npd(fr["visibility"]) * R.SOFT_S)) <= set(range(R.SOFT_S + 1))
    # ambient occlusion alone, without shadows
    other = inference.surface_frames(gen, zs[:1], b2ws[:1], keys=("ambient_occlusion",), ao_samples=R.AO_S, seed=R.SEED + 1)
    assert other["ambient_occlusion"].shape == (1, 1, H, H)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_split_light_walk_is_the_unsplit_one(precision, monkeypatch):
    from oi_amd import inference
    gen = G.make_gen(precision, R.R_SOFT)
    z, b2w = A.latent(1)[0], T.pose("off")
    radii = [R.SOFT_RADIUS, 0.05, R.SOFT_RADIUS, 0.02, 0.15]                      # one value per frame
    kw = dict(n_frames=5, shadows=True, shadow_samples=R.SOFT_S, light_radius=radii, ao_samples=R.AO_S, seed=R.SEED)
    whole = inference.surface_light_walk(gen, z, b2w, **kw)
    scalar = inference.surface_light_walk(gen, z, b2w, **{**kw, "light_radius": R.SOFT_RADIUS})
    for i in (0, 2):                                                              # the frames whose radius is the scalar's
        assert torch.equal(whole["image"][i], scalar["image"][i]) and torch.equal(whole["visibility"][i], scalar["visibility"][i])
    assert torch.equal(whole["ambient_occlusion"], scalar["ambient_occlusion"])
    with pytest.raises(ValueError, match="light_radius"):
        inference.surface_light_walk(gen, z, b2w, **{**kw, "light_radius": radii[:4]})
    n_hit = whole["stats"]["hit"]
    assert n_hit > 50 and 5 * R.SOFT_S * n_hit <= inference.OCCLUSION_MAX_RAYS
    from oi_amd import ops
    sizes = []
    begin = ops.occlusion_light_begin

    def counting(st, *a, **k):
        sizes.append(st.N)
        return begin(st, *a, **k)
    monkeypatch.setattr(ops, "occlusion_light_begin", counting)
    monkeypatch.setattr(inference, "OCCLUSION_MAX_RAYS", 2 * R.SOFT_S * n_hit + 1)
    split = inference.surface_light_walk(gen, z, b2w, **kw)
    assert sizes == [2 * R.SOFT_S * n_hit, 2 * R.SOFT_S * n_hit, R.SOFT_S * n_hit]   # three chunks: 2 + 2 + 1 lights
    for k in ("image", "visibility", "ambient_occlusion", "mask"):
        assert torch.equal(whole[k], split[k]), k
    assert torch.equal(_bits(whole["depth"]), _bits(split["depth"]))
    assert whole["image"].shape == (5, 3, R.R_SOFT, R.R_SOFT) and whole["visibility"].shape == (5, 1, R.R_SOFT, R.R_SOFT)
    vis = whole["visibility"]
    assert 0.0 <= float(vis.min()) and float(vis.max()) == 1.0
    # the hard walk is untouched by the cap
    hard = inference.surface_light_walk(gen, z, b2w, n_frames=5, shadows=True)
    assert sizes[3:] == [] and set(np.unique(npd(hard["visibility"]))) <= {0.0, 1.0}
