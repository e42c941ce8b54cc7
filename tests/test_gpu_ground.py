"""The ground plane of a scene on the MI355X (include/oi_ground.h; oi_amd.scene.Ground / GroundSurface).

The layer's own decisions -- which scene pixels are ground, the construction of the ground points' secondary rays in every
element, the combination across elements and chunks, the shade with its matte, the plane as occluder of the instances' rays
-- are checked against the float64 restatement of tests/helpers/ground_ref.py, which touches no code under test, and on the
analytic two-sphere scene against closed forms (tests/test_ground_cpu.py rehearses its conditions on float64 alone).  Exact
properties are checked bit for bit: a split trace against the unsplit one, an L-light launch against the 1-light launches, two
runs, ground=None against a call without the keyword.

Bars (eps = 2^-24):
  CLASSIFY      the ground pixels are the restatement's on the kernel's own owner map and float32 ray parameters, except where
                float32 may decide either way: |n . d + 1e-6| < 1e-5 (ground_ref.ND_BAND), ||p - c| - R_g| < 1e-4 (RIM_BAND), or
                |t_g - t_owner| within ground_ref.t_bar.  On the analytic scene the owner and its depth are the closed form's, with
                scene_ref's exclusions (silhouettes, depth ties below AN_DEPTH_GAP).
  GROUND_T      ground_ref.t_bar: the roundings of (h - n . o) / (n . d) on the float32 ray of make_ray; it scales with 1 / |n . d|.
  DIRECTIONS    caps and hemisphere: 1e-6 against the restatement, the bar tests/test_gpu_scene_light.py holds the shared
                __device__ function to, for the same reason (the compiler contracts its sums of products differently per
                kernel).  Local lights (the aimed sample, another function): 1e-6 + eps / sin_max + 2 eps |o| / dc, the least
                sin_max = R / dc and dc over the case: m = u1 (1 - cos_max) cancels for a light that subtends a small angle -- an
                absolute error eps in 1 - cos_max ~ sin_max^2 / 2 passes into sin(alpha) = sqrt(m (2 - m)) as at most eps /
                sin_max (tests/test_gpu_scene_local_light.py's reasoning) -- and the axis (q - o) / dc carries the rounding of
                o = p + bias n.  The restatement is fed the kernel's own float32 ground points; the kernel's world direction is
                read back from element 0's ray with the float64 transpose of its rotation.
  CULL          the entered set of every element is the restatement's cull of the KERNEL'S OWN float32 ray, except where |c2 - 1|
                <= 4 eps (|o|^2 + 1) or |near - limit| <= 1e-5 (limit: `distance`, or t_light): test_gpu_scene_light.py's edges.
  COUNTS        exact: integers.
  SHADE         ground_ref.shade_bar, written out there: the roundings of (ambient ao + diffuse max(n . l, 0) k) albedo fed the
                kernel's own float32 points; the matte's bar is that of the quotient of two such values.
  OCCLUDE       statuses exact against the restatement on the kernel's own rays, outside |t - limit| <= 1e-5 and ||p - c| - R_g|
                <= 1e-5.
  ANALYTIC      hard-shadow visibility and, per ambient ray, "escaped every sphere" exact against ray-versus-sphere in float64
                outside |closest approach - 0.5| < 1e-3 (scene_ref.AN_SHADOW_EDGE); at most 1 % of the rays in the band
                (occlusion_ref.EXCLUDED_CAP)."""
import types

import numpy as np
import pytest
import torch

import test_gpu_scene as GS
import test_gpu_scene_light as GL
import test_gpu_trace as G
from conftest import record_margin
from helpers import ground_ref as GR
from helpers import local_light_ref as LL
from helpers import occlusion_ref as R
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T
from helpers.guarded import guarded_empty, guarded_ops  # noqa: F401  (fixture)
from test_gpu_trace_batch import biteq

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

npd = G.npd
EPS = 2.0 ** -24
SEED = GR.SEED
UP = (0.0, -1.0, 0.0)                             # the world's up in the example camera's frame
RADII = GL.RADII                                  # one radius 0 among non-zero ones
INF = float("inf")
# kind, W, samples, L
CASES = [("pair", 9, 4, 2), ("single", 12, 1, 1), ("pair", 12, 1, 2), ("single", 9, 4, 1)]
_AN = {}


def f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32).cuda().contiguous()


def cuts_of(S):
    return {1: [[1]], 4: [[4], [1, 1, 1, 1], [1, 3]]}[S]


# ---------------------------------------------------------------------------------------------------------------------
# the analytic two-sphere scene through the ops wrappers (test_gpu_scene._analytic's sequence), the field |x| - 0.5 by torch
# ---------------------------------------------------------------------------------------------------------------------
def sphere_march(st, anyhit=False):
    from oi_amd import ops
    step = ops.trace_batch_step_anyhit if anyhit else ops.trace_batch_step
    sdf = torch.zeros(st.E, st.N).cuda()
    bound, k = int(st.live[0].item()), 0
    while bound > 0 and k < T.MAX_MAX_STEPS:
        sdf[:, :bound] = st.points[:, :bound].norm(dim=-1) - SR.RADIUS
        step(st, sdf, bound, k, T.TOL, T.OMEGA)
        k += 1
        bound = int(st.live[k].item())


def analytic():
    """The traced analytic scene; computed once and never modified."""
    if "a" not in _AN:
        from oi_amd import ops
        sc = SR.analytic_scene()
        E, W, S = 2, sc["W"], sc["S"]
        a = types.SimpleNamespace(sc=sc, E=E, W=W, S=S, N=W * W, bias=T.BIAS)
        a.c2b, a.b2w, a.kinv, a.c2w = f32(sc["c2b"]), f32(sc["b2w"]), f32(sc["K_inv"]), f32(sc["c2w"])
        a.w2b = f32(np.stack([SR.rigid_inverse(m) for m in sc["b2w"]]))
        a.window = torch.tensor(sc["origins"], dtype=torch.int32).cuda()
        st = ops.trace_batch_state_empty(E, W * W, a.c2b)
        ops.scene_begin(st, a.c2b, a.kinv, a.window, W, S)
        sphere_march(st)
        ops.trace_batch_finish(st)
        a.state = st
        a.owner, a.owner_ray = ops.scene_resolve(st, a.window, W, S)
        a.vis_index, a.vis_slot = ops.scene_visible(st, a.owner, a.window, W, S)
        a.n_pad, a.n_vis = int(st.live[-1].item()), st.counts[:, -1].tolist()
        a.points = ops.trace_batch_gather(st, a.vis_index, a.n_pad)
        a.grad, a.rgb = (2.0 * a.points).contiguous(), torch.full_like(a.points, 0.5)
        a.offset = torch.tensor(SR.offsets(a.n_vis), dtype=torch.int32).cuda()
        _AN["a"] = a
    return _AN["a"]


def ground_on(s, rec64):
    """oi_ground_begin on the scene s (the analytic namespace or a SceneSurface) and the host's sort.  -> namespace: record, t,
    index (ascending), n_g, args (what ground_rays_begin and ground_shade take first)."""
    from oi_amd import ops
    rec = f32(rec64)
    t, index, count = ops.ground_begin(s.c2w, s.kinv, s.S, rec, s.owner, s.owner_ray, s.state.t, s.window, s.W, s.E)
    n_g = int(count.item())
    index = torch.sort(index[:n_g]).values.contiguous()
    return types.SimpleNamespace(record=rec, t=t, index=index, n_g=n_g, args=(s.c2w, s.kinv, s.S, rec, t, index, n_g))


def ground_sampled(s, g, S, cuts, march, lt=None, radius=None, distance=None, seed=SEED):
    """The sequence of include/oi_ground.h through the ops wrappers, chunk by chunk.  -> chunks (the finished states), count,
    out (L, n_g)."""
    from oi_amd import ops
    L = 1 if lt is None else lt.shape[0]
    count, out = ops._new(g.record, L, g.n_g).view(torch.int32), ops._new(g.record, L, g.n_g)
    chunks, j0 = [], 0
    for c in cuts:
        sb = ops.trace_batch_state_empty(s.E, L * c * g.n_g, g.record)
        ops.ground_rays_begin(sb, *g.args, s.w2b, s.bias, S, j0, c, seed, lt, radius, distance)
        if int(sb.live[0].item()):
            march(sb)
            ops.trace_batch_finish(sb)
        ops.ground_resolve(sb.status, s.E, g.n_g, L, S, j0, c, count, out, j0 + c == S)
        chunks.append(sb)
        j0 += c
    return chunks, count, out


def field_march(s):
    from oi_amd import trace
    return lambda sb: trace._march_batch(s.field, sb, *s.kw, bound=int(sb.live[0].item()), anyhit=True)


def world_rays(sb, b2w64, E, shape):
    """Element 0's rays of the chunk sb taken to the world in float64: o, d of shape `shape` + (3,)."""
    o, d = npd(sb.rays_o[0]), npd(sb.rays_d[0])
    return (SR.transform(b2w64[0], o)).reshape(shape + (3,)), (d @ b2w64[0][:3, :3].T).reshape(shape + (3,))


def owner_depth(s):
    """(S * S,) float64: the owner's float32 ray parameter per scene pixel (inf where nothing owns it), and the owner map."""
    owner, ray = s.owner.cpu().numpy().astype(np.int64), s.owner_ray.cpu().numpy().astype(np.int64)
    t = npd(s.state.t)
    return owner, np.where(owner >= 0, t[np.maximum(owner, 0), np.maximum(ray, 0)], np.inf)


def golden_ground(s, gap=0.02, disc=None, **kw):
    """The plane the instances of the golden scene s stand on.  disc: a radius about the instances' centre, which keeps the
    ground points within reach of float32 comparisons (an unbounded plane runs to the horizon, t_g in the thousands)."""
    from oi_amd import scene
    if disc is not None:
        kw.update(extent=disc, centre=tuple(npd(s.world_points()[0]).mean(0)))
    return scene.Ground.below(s.world_points()[0], UP, gap=gap, **kw)


def kernel_points(gs):
    """(n_g, 3) float64: the kernel's own float32 ground points (oi_ground_shade's position map: the same device function)."""
    from oi_amd import ops
    M = gs.scene.S ** 2
    maps = {"position": torch.zeros(M, 3, device="cuda")}
    ops.ground_shade(*gs._args(), GL.lights_t(1), maps)
    return npd(maps["position"][gs.index.long()])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the analytic scene on a plane
# ---------------------------------------------------------------------------------------------------------------------
def test_analytic_two_spheres_on_a_plane():
    a = analytic()
    sc = a.sc
    cf = SR.analytic_closed_form(sc)
    rec = GR.analytic_record()
    g64 = GR.analytic_ground(sc, cf, rec)
    g = ground_on(a, rec)
    M = a.S * a.S
    mask = np.zeros(M, dtype=bool)
    mask[g.index.cpu().numpy()] = True
    t = npd(g.t)
    assert np.array_equal(np.isnan(t), ~mask) and g.index.dtype == torch.int32
    owned = cf["owner"] >= 0
    tie = owned & g64["front"] & (np.abs(g64["t_all"] - np.where(owned, cf["depth"], 0.0)) < SR.AN_DEPTH_GAP)
    band = (np.abs(g64["nd"] + GR.FRONT) < GR.ND_BAND) | (np.abs(g64["rim"]) < GR.RIM_BAND)
    keep = ~(band | tie | cf["excluded"])
    assert band.sum() + tie.sum() <= R.EXCLUDED_CAP * M
    assert np.array_equal(mask[keep], g64["ground"][keep]) and g.n_g >= 300
    both = mask & g64["ground"]
    ratio = float((np.abs(t[both] - g64["t"][both]) / GR.t_bar(g64["o"], g64["d"][both], rec)).max())
    record_margin("ground_analytic", "t_error_over_bar", ratio)
    assert ratio <= 1.0
    assert not (mask & (a.owner.cpu().numpy() >= 0)).any()                # this plane hides no instance
    # the hard shadows of the two spheres
    lt = f32([T.light_block(GR.AN_GROUND_LIGHT)])
    chunks, count, vis = ground_sampled(a, g, 1, [1], lambda sb: sphere_march(sb, True), lt, f32([0.0]))
    q = g.index.cpu().numpy()
    sh = GR.analytic_shadows(g64)
    col = np.full(M, -1)
    col[sh["q"]] = np.arange(len(sh["q"]))
    common = col[q] >= 0
    k = col[q][common]
    ok = ~sh["band"].any(0)[k]
    n_band = int((~ok).sum())
    assert n_band <= R.EXCLUDED_CAP * len(k) and common.mean() > 0.99
    got = npd(vis)[0][common]
    assert np.array_equal(got[ok], sh["lit"][k][ok].astype(np.float64))
    by = [int(((got == 0) & sh["blocked"][e][k]).sum()) for e in range(2)]
    assert min(by) >= 10, by                                              # otherwise the test shows nothing
    assert set(np.unique(chunks[0].status.cpu().numpy())) <= {T.MISS, T.HIT}
    # the ambient rays: per ray, escaped every sphere
    S, dist = GR.AN_AO_S, GR.AN_AO_DISTANCE
    chunks, count, ao = ground_sampled(a, g, S, [S], lambda sb: sphere_march(sb, True), distance=dist)
    st = chunks[0].status.cpu().numpy().reshape(a.E, S, g.n_g)
    o, d = world_rays(chunks[0], sc["b2w"], a.E, (S, g.n_g))
    assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-6 and (d @ rec[:3] > 0).all() and not (st == T.BACKFACING).any()
    blocked, in_band = SL.sphere_blocks(o, d, dist)
    sure = ~in_band.any(0)
    esc = SL.escaped(st)
    assert (~sure).mean() <= R.EXCLUDED_CAP
    assert np.array_equal(esc[sure], ~blocked.any(0)[sure])
    assert np.array_equal(count.cpu().numpy()[0], esc.sum(0)) and biteq(ao, (count.float() / S))
    share = float(1 - esc.mean())
    print(f"analytic ground: {g.n_g} ground pixels, t error / bar {ratio:.3g}, shadowed by sphere {by}, in the shadow band {n_band}, "
          f"ambient rays blocked {share:.3f}, in the band {float((~sure).mean()):.4f}")
    assert 0.05 <= share <= 0.2


# ---------------------------------------------------------------------------------------------------------------------
# 2. a plane that cuts an instance
# ---------------------------------------------------------------------------------------------------------------------
def test_plane_that_cuts_an_instance():
    from oi_amd import ops
    a = analytic()
    sc = a.sc
    cf = SR.analytic_closed_form(sc)
    rec = GR.analytic_record(GR.AN_CUT_OFFSET)
    g64 = GR.analytic_ground(sc, cf, rec)
    g = ground_on(a, rec)
    M = a.S * a.S
    mask = np.zeros(M, dtype=bool)
    mask[g.index.cpu().numpy()] = True
    owned = cf["owner"] >= 0
    tie = owned & g64["front"] & (np.abs(g64["t_all"] - np.where(owned, cf["depth"], 0.0)) < SR.AN_DEPTH_GAP)
    band = (np.abs(g64["nd"] + GR.FRONT) < GR.ND_BAND) | (np.abs(g64["rim"]) < GR.RIM_BAND)
    assert tie.sum() <= SR.AN_CAP * (owned & g64["front"]).sum()
    keep = ~(band | tie | cf["excluded"])
    assert np.array_equal(mask[keep], g64["ground"][keep])
    owner = a.owner.cpu().numpy()
    hides = mask & (owner >= 0)
    assert int(hides.sum()) >= 10 and int(((owner >= 0) & ~mask & g64["front"]).sum()) >= 10      # both orders of depth occur
    lt = f32([T.light_block(GR.AN_GROUND_LIGHT), T.light_block(T.LIGHT_DIRS[0])])
    out = ops.scene_shade(a.state, a.W, a.S, a.owner, a.owner_ray, a.vis_slot, a.points, a.grad, a.rgb, a.n_pad, a.w2b, a.b2w, lt)
    before = {k: v.clone() for k, v in out.items()}
    maps = {k: v for k, v in out.items() if k in ops.GROUND_OUT}
    gmask, matte = ops.ground_shade(*g.args, lt, maps)
    h = torch.from_numpy(hides).cuda()
    on = torch.from_numpy(mask).cuda()
    assert bool((out["instance"][h] == -1).all()) and bool((before["instance"][h] >= 0).all())
    assert bool((out["mask"][h] == 0).all()) and bool((before["mask"][h] == 1).all())
    assert biteq(out["depth"][on], g.t[on]) and bool((out["depth"][h] < before["depth"][h]).all())
    assert bool((out["instance"][on] == -1).all()) and not bool(out["mask"][on].any())
    assert biteq(gmask, on.float()) and bool((matte[:, :, on] == 1).all()) and bool((matte[:, :, ~on] == 1).all())
    for k, v in out.items():                                              # nothing is written off the ground
        assert biteq(v[..., ~on] if k == "image" else v[~on], before[k][..., ~on] if k == "image" else before[k][~on]), k
    nw, alb = npd(out["normal_world"])[mask], npd(out["albedo"])[mask]
    assert np.array_equal(nw, np.broadcast_to(npd(g.record)[:3], nw.shape)) and np.array_equal(alb, np.broadcast_to(npd(g.record)[4:7], alb.shape))
    pos = npd(out["position"])[mask]
    # on the plane: t_g's error moves the point along the ray, |n . d| of it off the plane; the fma rounds each coordinate once
    lim = np.abs(g64["nd"][mask]) * GR.t_bar(g64["o"], g64["d"][mask], rec) + (GR.RAY_EPS * npd(g.t)[mask] + np.abs(pos).sum(-1) + 1) * EPS
    assert (np.abs(pos @ rec[:3] - rec[3]) <= lim).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. rays in every element
# ---------------------------------------------------------------------------------------------------------------------
def local_records(s, rec64):
    """Two local lights over the scene: a sphere light high above the instances, and a point light inside the unit sphere of
    instance 0, 0.85 above its box origin, so that t_light cuts the chords of the rays aimed at it."""
    c = npd(s.world_points()[0]).mean(0)
    n = np.asarray(rec64[:3])
    return np.array([LL.record(tuple(c + 2.5 * n + (0.4, 0.0, -0.3)), 0.1, reference_distance=2.5),
                     LL.record(tuple(npd(s.b2w)[0][:3, 3] + 0.85 * n), 0.0, reference_distance=1.5)])


@pytest.mark.parametrize("mode", ["caps", "hemisphere", "local"])
@pytest.mark.parametrize("kind,W,S,L", CASES)
def test_rays_in_every_element(kind, W, S, L, mode):
    from oi_amd import lib, ops
    s = GS.traced("f32", kind, W)
    gs = s.ground(golden_ground(s, disc=6.0))
    rec = npd(gs.record)
    n, E = gs.n_g, s.E
    j0, c = (1, 3) if S == 4 else (0, 1)
    distance = 2.0 if kind == "pair" else INF
    Lr = 1 if mode == "hemisphere" else L
    loc = local_records(s, rec)[:L]
    if mode == "caps":
        kw, rkw = dict(lights=GL.lights_t(L), radius=GL.radius_t(L)), dict(light_dirs=[l.direction for l in GS.lights(L)], radius=RADII[L])
    elif mode == "hemisphere":
        kw, rkw = dict(distance=distance), dict(distance=distance)
    else:
        kw, rkw = dict(lights=f32(loc)), dict(local=loc)
    sb = ops.trace_batch_state_empty(E, Lr * c * n, gs.record)
    ops.ground_rays_begin(sb, *gs._args(), s.w2b, s.bias, S, j0, c, SEED, **kw)
    pix = gs.index.cpu().numpy().astype(np.int64)
    w2b = npd(s.w2b)
    b2w = np.stack([SR.rigid_inverse(m) for m in w2b])
    p = kernel_points(gs)
    shape = (E, Lr, c, n)
    o, d = npd(sb.rays_o).reshape(shape + (3,)), npd(sb.rays_d).reshape(shape + (3,))
    near, far = npd(sb.near).reshape(shape), npd(sb.far).reshape(shape)
    status = sb.status.cpu().numpy().reshape(shape)
    d_world = d[0] @ b2w[0][:3, :3].T
    drawn = GR.rays(rec, p, pix, w2b, s.bias, S, j0, c, SEED, **rkw)
    err = float(np.abs(d_world - drawn["d_world"]).max())
    bar = 1e-6
    if mode == "local":
        ow = p + s.bias * rec[:3]
        dc = np.stack([np.linalg.norm(lt[:3] - ow, axis=-1) for lt in loc])
        sin_max = np.where(loc[:, 3:4] > 0, loc[:, 3:4] / dc, np.inf)
        bar += EPS / float(sin_max.min()) + 2 * EPS * float(np.abs(ow).max()) / float(dc.min())
    record_margin(f"ground_directions[{kind},W={W},S={S},L={Lr},{mode}]", "error_over_bar", err / bar)
    assert err <= bar
    inside = np.broadcast_to(~drawn["traced"] & (drawn["d_world"] == 0).all(-1), d_world.shape[:-1])
    assert np.abs(np.linalg.norm(d_world, axis=-1) - 1)[~inside].max() < 1e-6
    if mode == "caps" and L == 2:                                         # radius 0: every sample is the light's direction
        assert np.abs(d_world[1] - d_world[1][:1]).max() == 0
    # every element's ray from the kernel's own directions
    r = GR.rays(rec, p, pix, w2b, s.bias, S, j0, c, SEED, d_world=d_world, **rkw)
    ndd = d_world @ rec[:3]
    sure = (np.abs(ndd) > 1e-6) | inside
    back = status == T.BACKFACING
    assert np.array_equal(back.all(0), back.any(0))                       # facing away: BACKFACING in every element
    assert np.array_equal(back[0][sure], (~r["traced"] & ~inside)[sure])
    assert set(np.unique(status)) <= {T.MARCH, T.MISS, T.BACKFACING} and not sb.steps.any()
    ow = p + s.bias * rec[:3]
    for e in range(E):                                                    # the biased point (one fma) through the rigid transform
        o_bar = SR.transform_bar(w2b[e], ow) + 2 * EPS * np.abs(ow).max()
        assert (np.abs(o[e] - r["o"][e]) <= o_bar[None, None]).all(), e
    assert float(np.abs(d - r["d"]).max()) <= 1e-6
    # the cull of the kernel's own ray
    with np.errstate(divide="ignore", invalid="ignore"):
        ent, ne, fa, c2 = SR.cull(o, d)
    limit = np.broadcast_to(r["limit"], shape)
    expect = ent & (ne < limit) & np.broadcast_to(r["traced"], shape)
    edge = (np.abs(c2 - 1) <= 4 * EPS * ((o ** 2).sum(-1) + 1)) | (np.abs(ne - limit) <= 1e-5)
    cmp_ = np.broadcast_to(sure, shape) & ~edge
    entered = status == T.MARCH
    assert np.array_equal(entered[cmp_], expect[cmp_])
    n_edge = int((edge & ~back).sum())
    assert n_edge <= 0.001 * status.size + 2
    both = cmp_ & entered
    tol = 1e-5 / np.sqrt(np.maximum(1 - c2[both], 1e-4))
    assert (np.abs(near[both] - ne[both]) <= tol).all() and (np.abs(far[both] - np.minimum(fa, limit)[both]) <= tol + 1e-5).all()
    assert not near[~entered].any() and not far[~entered].any()
    if mode != "caps":                                                    # clipped: no ray reaches past its limit
        assert (far[entered] <= limit[entered] + 1e-5).all()
        if np.isfinite(limit).all():
            assert (np.abs(far - limit)[entered & (fa > limit + 1e-4)] <= 1e-5).all()
    if mode == "local":
        assert np.isfinite(limit).all()
        if L == 2:
            assert (entered & (fa > limit + 1e-4)).any()                  # t_light cuts chords: the light inside instance 0's sphere
    assert entered.any() and (status == T.MISS).any()
    # the state: oi_scene_shadow_begin's
    counts, live = sb.counts.cpu().numpy(), sb.live.cpu().numpy()
    flat = entered.reshape(E, -1)
    t, br = npd(sb.t), npd(sb.bracket)
    assert np.array_equal(t, npd(sb.near)) and np.array_equal(br[..., 0], t) and not br[..., 1].any() and not sb.side.any()
    for e in range(E):
        n_ent = int(flat[e].sum())
        assert counts[e, 0] == n_ent and not counts[e, 1:].any()
        act = sb.active[e, 0, :n_ent].cpu().numpy()
        assert sorted(act.tolist()) == np.nonzero(flat[e])[0].tolist()
        pts = npd(sb.points[e])
        want = npd(sb.rays_o[e])[act] + npd(sb.near[e])[act, None] * npd(sb.rays_d[e])[act]
        assert np.abs(pts[:n_ent] - want).max(initial=0.0) <= 2e-6 and not pts[n_ent:].any()
    assert live[0] == counts[:, 0].max() and not live[1:].any() and len(live) == lib.TRACE_COUNT_WORDS
    print(f"ground rays[{kind},W={W},S={S},L={Lr},{mode}] n_g {n} (mod 256: {n % 256}) entered {counts[:, 0].tolist()} of {Lr * c * n} "
          f"worst direction error {err:.3g} rays on an edge {n_edge}")


def test_an_instance_beyond_the_lamp_throws_no_shadow():
    """A lamp between the ground and the instances: every ray ends at the lamp, below them.  The same lamp above them: shadows."""
    s = GS.traced("f32", "pair", 9)
    gs = s.ground(golden_ground(s, gap=0.4, disc=6.0))
    rec = npd(gs.record)
    c = npd(s.world_points()[0]).mean(0)
    foot = c - (c @ rec[:3] - rec[3]) * rec[:3]                           # the centre's foot on the plane
    low = f32([LL.record(tuple(foot + 0.2 * rec[:3]), 0.05)])
    high = f32([LL.record(tuple(foot + 3.0 * rec[:3]), 0.05)])
    v_low, v_high = gs.local_visibility(low, 4, SEED), gs.local_visibility(high, 4, SEED)
    st = gs.last.status.cpu().numpy()
    assert v_low.shape == (1, gs.n_g) and float((v_low < 1).float().mean()) <= R.LIMIT_CAP
    assert int((v_high < 1).sum()) >= 10 and set(np.unique(st)) <= {T.MISS, T.HIT, T.LIMIT, T.BACKFACING}
    print("lamp below the instances: share of ground points not fully lit", float((v_low < 1).float().mean()), "lamp above:",
          int((v_high < 1).sum()), "of", gs.n_g)


# ---------------------------------------------------------------------------------------------------------------------
# 4. bitwise properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", GS.PRECISIONS)
def test_split_equals_unsplit_and_lights_are_independent(precision):
    from oi_amd import ops, scene
    s = GS.traced(precision, "pair", 9)
    g = golden_ground(s, disc=6.0)
    gs = s.ground(g)
    S, L = 4, 2
    lt, rad, loc = GL.lights_t(L), GL.radius_t(L), f32(local_records(s, npd(gs.record)))
    ns = types.SimpleNamespace(E=s.E, w2b=s.w2b, bias=s.bias)
    view = types.SimpleNamespace(record=gs.record, n_g=gs.n_g, args=gs._args())
    for name, kw in (("caps", dict(lt=lt, radius=rad)), ("hemisphere", dict(distance=2.0)), ("local", dict(lt=loc))):
        outs = [ground_sampled(ns, view, S, cuts, field_march(s), **kw) for cuts in cuts_of(S)]
        for chunks, count, out in outs[1:]:
            assert biteq(out, outs[0][2]) and torch.equal(count, outs[0][1]), name
        whole = outs[0][0][0].status.cpu().numpy().reshape(s.E, -1, S, gs.n_g)
        parts = np.concatenate([sb.status.cpu().numpy().reshape(s.E, -1, c, gs.n_g) for sb, c in zip(outs[2][0], [1, 3])], 2)
        assert np.array_equal(whole, parts), name
        count_ref, out_ref = GR.counts([whole], S)
        assert np.array_equal(outs[0][1].cpu().numpy(), count_ref) and np.array_equal(npd(outs[0][2]), out_ref), name
        host = {"caps": lambda m: gs.visibility(lt, rad, S, SEED, m), "hemisphere": lambda m: gs.ambient(S, 2.0, SEED, m)[None],
                "local": lambda m: gs.local_visibility(loc, S, SEED, m)}[name]
        Lr = 1 if name == "hemisphere" else L
        assert biteq(host(scene.MAX_SHADOW_RAYS), outs[0][2]) and biteq(host(s.E * Lr * gs.n_g * 3), outs[0][2]), name
        assert float(outs[0][2].min()) < 1, name                                             # something is shadowed
    # an L-light launch equals the 1-light launches, directional and local
    vis, ao = gs.visibility(lt, rad, S, SEED), gs.ambient(S, 2.0, SEED)
    for lights in (lt, loc):
        maps = lambda Ln: {"image": torch.zeros(Ln, 3, s.S * s.S, device="cuda")}
        m2 = maps(L)
        gm2, mt2 = ops.ground_shade(*gs._args(), lights, m2, vis, ao)
        for l in range(L):
            m1 = maps(1)
            gm1, mt1 = ops.ground_shade(*gs._args(), lights[l:l + 1].contiguous(), m1, vis[l:l + 1].contiguous(), ao)
            assert biteq(m1["image"][0], m2["image"][l]) and biteq(mt1[0], mt2[l]) and biteq(gm1, gm2)
    # two runs give identical bytes, the compaction's order notwithstanding
    again = scene.GroundSurface(s, g)
    assert torch.equal(again.index, gs.index) and biteq(again.t, gs.t) and torch.equal(again.slot, gs.slot)
    kw = dict(shadows=True, bg=(0.25, 0.5, 0.75), shadow_samples=4, light_radius=0.1, ao_samples=4, ao_distance=2.0, seed=SEED, ground=g)
    one, two = s.shade(GS.lights(L), **kw), s.shade(GS.lights(L), **kw)
    assert set(one) == set(two) and {"ground_mask", "shadow_matte"} <= set(one)
    for k in one:
        if k != "stats":
            assert biteq(one[k], two[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 5. ground_t and the shade against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,W", [("pair", 9), ("single", 12)])
def test_ground_t_and_shade_against_the_restatement(kind, W):
    from oi_amd import ops
    s = GS.traced("f32", kind, W)
    M, L = s.S * s.S, 2
    for g in (golden_ground(s), golden_ground(s, gap=0.1, disc=3.0, albedo=(0.9, 0.5, 0.2))):
        gs = s.ground(g)
        rec = npd(gs.record)
        owner, t_owner = owner_depth(s)
        cls = GR.classify(npd(s.c2w), npd(s.kinv), s.S, rec, owner, t_owner)
        bar = GR.t_bar(cls["o"], cls["d"], rec)
        band = (np.abs(cls["nd"] + GR.FRONT) < GR.ND_BAND) | (np.abs(cls["rim"]) < GR.RIM_BAND) | \
            ((owner >= 0) & (np.abs(cls["t_all"] - t_owner) <= bar))
        mask = np.zeros(M, dtype=bool)
        mask[gs.index.cpu().numpy()] = True
        # (the band: at most the horizon's row of pixels, where n . d passes 0, and 1 % on the rim and on depth ties)
        assert np.array_equal(mask[~band], cls["ground"][~band]) and band.sum() <= s.S + 0.01 * M and gs.n_g > 50
        assert torch.equal(gs.slot[gs.index.long()], torch.arange(gs.n_g, dtype=torch.int32, device="cuda")) and int((gs.slot >= 0).sum()) == gs.n_g
        both = mask & cls["ground"]
        t = npd(gs.t)
        ratio = float((np.abs(t[both] - cls["t"][both]) / bar[both]).max())
        record_margin(f"ground_t[{kind},W={W},extent={g.extent}]", "error_over_bar", ratio)
        assert ratio <= 1.0 and np.array_equal(np.isnan(t), ~mask)
        # the shade, fed the kernel's own points
        lt, loc = GL.lights_t(L), local_records(s, rec)
        loc[1] = LL.record(tuple(loc[1][:3]), 0.0, reference_distance=1.5, cone_axis=(0.6, 1.0, -0.2), cone_inner=0.3, cone_outer=1.0)
        rs = np.random.RandomState(3)
        vis, ao = f32(rs.rand(L, gs.n_g)), f32(rs.rand(gs.n_g))
        q = gs.index.long()
        for name, lights, local in (("directional", lt, False), ("local", f32(loc), True)):
            maps = {"image": torch.zeros(L, 3, M, device="cuda"), "position": torch.zeros(M, 3, device="cuda"),
                    "depth": torch.zeros(M, device="cuda")}
            gmask, matte = ops.ground_shade(*gs._args(), lights, maps, vis, ao)
            p = npd(maps["position"][q])
            assert biteq(maps["depth"][q], gs.t[q])
            # the point: the float32 ray's direction error times t, and the fma's rounding of each coordinate
            assert (np.abs(p - (cls["o"] + t[mask, None] * cls["d"][mask])) <= ((GR.RAY_EPS * t[mask])[:, None] + np.abs(p) + 1) * EPS).all()
            img, mat, bar_i, bar_m = GR.shade(rec, p, npd(lights), local, npd(vis), npd(ao))
            e_i = np.abs(npd(maps["image"][:, :, q]) - img)
            e_m = np.abs(npd(matte[:, :, q]) - mat)
            ri, rm = float((e_i / np.maximum(bar_i, 1e-300)).max()), float((e_m / np.maximum(bar_m, 1e-300)).max())
            record_margin(f"ground_shade[{kind},W={W},{name},extent={g.extent}]", "error_over_bar", max(ri, rm))
            print(f"ground shade[{kind},W={W},{name}] n_g {gs.n_g} image error / bar {ri:.3g} matte error / bar {rm:.3g}")
            assert (e_i <= bar_i).all() and (e_m <= bar_m).all()
            off = torch.ones(M, dtype=torch.bool, device="cuda")
            off[q] = False
            assert not bool(maps["image"][:, :, off].any()) and bool((matte[:, :, off] == 1).all()) and biteq(gmask, (~off).float())
            assert float(npd(matte[:, :, q]).min()) < 1 and float(img.max()) > 0.05
            if local:
                assert LL.factors(p, npd(lights)[1], np.eye(4))[2].max() > 0             # the cone reaches the ground


# ---------------------------------------------------------------------------------------------------------------------
# 6. the ground as occluder of the instances' rays
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,W", [("pair", 9), ("single", 12)])
def test_ground_occludes_the_instances_rays(kind, W):
    from oi_amd import ops, trace
    s = GS.traced("f32", kind, W)
    g = golden_ground(s, disc=3.0)
    gs = s.ground(g)
    rec, b2w = npd(gs.record), npd(s.b2w)
    pos, nrm, elem = s.world_points()
    n, E = sum(s.n_vis), s.E
    elem_np = elem.cpu().numpy()

    def check(sb, limit, name):
        before = sb.status.clone()
        o, d = npd(sb.rays_o), npd(sb.rays_d)
        saved = [x.clone() for x in (sb.rays_o, sb.rays_d, sb.t, sb.near, sb.far, sb.steps)]
        ops.ground_occlude(sb, gs.record, elem, s.b2w, n, limit)
        after = sb.status.cpu().numpy()
        want, t, rim = GR.occlude(before.cpu().numpy(), o, d, elem_np, b2w, rec, limit)
        band = (np.abs(t - limit) <= 1e-5) | (np.abs(rim) <= 1e-5)
        assert np.array_equal(after[:, ~band], want[:, ~band]) and band.mean() <= 0.01, name
        b = before.cpu().numpy()
        changed = b != after
        assert changed.any() and (b[changed] == T.MISS).all() and (after[changed] == T.HIT).all(), name
        rows, cols = np.nonzero(changed)
        assert np.array_equal(rows, elem_np[cols % n]), name                 # only the owner's row
        for x, y in zip(saved, (sb.rays_o, sb.rays_d, sb.t, sb.near, sb.far, sb.steps)):
            assert torch.equal(x, y), name                                   # nothing else is touched
        return int(changed.sum())

    # ambient rays, one chunk of three of four samples
    S, j0, c, dist = 4, 1, 3, 2.0
    pixel = s.point_pixels()
    sb = ops.trace_batch_state_empty(E, c * n, pos)
    ops.scene_occlusion_begin(sb, s.points, s.grad, s.n_pad, s.offset, elem, pixel, pos, nrm, n, s.w2b, s.bias, S, j0, c, SEED, None, None, dist)
    trace._march_batch(s.field, sb, *s.kw, bound=int(sb.live[0].item()), anyhit=True)
    ops.trace_batch_finish(sb)
    n_amb = check(sb, dist, "ambient")
    # directional rays of a light below the plane (the hard ray's layout, Sc = 1) and of one above it
    lt = f32([T.light_block(T.LIGHT_DIRS[2]), T.light_block(T.LIGHT_DIRS[0])])
    sb = ops.trace_batch_state_empty(E, 2 * n, pos)
    ops.scene_shadow_begin(sb, s.points, s.grad, s.n_pad, s.offset, elem, pos, nrm, n, lt, s.w2b, s.bias)
    trace._march_batch(s.field, sb, *s.kw, bound=int(sb.live[0].item()))
    ops.trace_batch_finish(sb)
    below = sb.status.clone()
    n_dir = check(sb, INF, "directional")
    assert torch.equal(sb.status[:, n:], below[:, n:])                       # the light above the plane: nothing changes
    print(f"ground occlude[{kind},W={W}]: ambient rays turned {n_amb} of {E * c * n}, directional {n_dir} of {E * 2 * n}")


@pytest.mark.parametrize("precision", GS.PRECISIONS)
def test_ambient_with_a_ground_darkens_the_instances(precision):
    s = GS.traced(precision, "pair", 9)
    g = golden_ground(s, gap=0.02)
    free, grounded = s.ambient(4, 2.0, SEED), s.ambient(4, 2.0, SEED, ground=g)
    assert bool((grounded <= free).all()) and int((grounded < free).sum()) >= 10
    off = s.owner < 0
    assert bool((grounded[off] == 1).all())
    assert biteq(s.ambient(4, 2.0, SEED), free)                              # and without the keyword nothing changed
    lt = GL.lights_t(2)
    assert bool((s.visibility(lt, None, 1, SEED, ground=g) <= s.visibility(lt, None, 1, SEED)).all())
    assert bool((s.visibility(lt, RADII[2], 4, SEED, ground=g) <= s.visibility(lt, RADII[2], 4, SEED)).all())
    print("ambient with the ground: darker pixels", int((grounded < free).sum()), "of", int((~off).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# 7. the public interface: ground=None, the composed maps, composite_over, the walks
# ---------------------------------------------------------------------------------------------------------------------
def count_launches(monkeypatch, fn):
    """fn() and the number of kernel-launching calls it made through oi_amd.ops (every wrapper takes the stream once)."""
    from oi_amd import ops
    calls = [0]
    orig = ops._stream

    def counted():
        calls[0] += 1
        return orig()
    monkeypatch.setattr(ops, "_stream", counted)
    try:
        return fn(), calls[0]
    finally:
        monkeypatch.setattr(ops, "_stream", orig)


@pytest.mark.parametrize("precision", GS.PRECISIONS)
def test_shade_with_and_without_a_ground(precision, monkeypatch):
    from oi_amd import scene
    from oi_amd.relight import LocalLight
    s = GS.traced(precision, "pair", 9)
    S, L = s.S, 2
    kw = dict(shadows=True, bg=(0.25, 0.5, 0.75), shadow_samples=4, light_radius=0.1, ao_samples=16, ao_distance=2.0, seed=SEED)
    s.shade(GS.lights(L), **kw)                                              # (the scene's world points and pixel keys are computed once)
    base, n0 = count_launches(monkeypatch, lambda: s.shade(GS.lights(L), **kw))
    none, n1 = count_launches(monkeypatch, lambda: s.shade(GS.lights(L), ground=None, **kw))
    assert n0 == n1 and set(base) == set(none)
    for k in base:
        if k != "stats":
            assert biteq(base[k], none[k]), k
    assert "ground_pixels" not in base["stats"][0]
    g = golden_ground(s)
    res = s.shade(GS.lights(L), ground=g, **kw)
    gs = s.ground(g)
    assert res["ground_mask"].shape == (1, 1, S, S) and res["shadow_matte"].shape == (L, 3, S, S) and res["image"].shape == (L, 3, S, S)
    on = res["ground_mask"].view(-1) > 0
    assert int(on.sum()) == gs.n_g == res["stats"][0]["ground_pixels"] and res["stats"][0]["ground_evals"] > 0
    assert torch.equal(on, gs.slot >= 0)
    # the maps are composed: the ground's values on its pixels, the scene's elsewhere (the instances now know the ground)
    assert bool((res["mask"].view(-1)[on] == 0).all()) and bool((res["instance"].view(-1)[on] == -1).all())
    assert biteq(res["depth"].view(-1)[on], gs.t[on]) and biteq(res["depth"].view(-1)[~on], base["depth"].view(-1)[~on])
    assert biteq(res["mask"].view(-1)[~on], base["mask"].view(-1)[~on])
    matte, image = res["shadow_matte"].view(L, 3, -1), res["image"].view(L, 3, -1)
    assert bool((matte[:, :, ~on] == 1).all()) and bool((matte <= 1).all()) and bool((matte > 0).all())
    assert int((matte[0, 0] < 1).sum()) >= 10                                # shadows and contact darkening reach the plane
    vis, ao = gs.visibility(GL.lights_t(L), GL.radius_t(L) * 0 + 0.1, 4, SEED), gs.ambient(16, 2.0, SEED)
    # (under either light: the first stands in front of the instances, so most of its shadow falls behind them as the camera
    # sees the plane, at a grazing angle)
    assert int((vis < 1).any(0).sum()) >= 10 and int((ao < 1).sum()) >= 10
    sky = (s.owner < 0) & ~on
    assert biteq(image[:, :, sky], base["image"].view(L, 3, -1)[:, :, sky])  # the background stays
    assert bool((res["ambient_occlusion"] <= base["ambient_occlusion"]).all())
    # composite_over: the image on the instances' mask, photo * matte elsewhere
    photo = torch.rand(3, S, S, device="cuda")
    comp = scene.composite_over(res, photo)
    m = (res["mask"] > 0).expand(L, 3, S, S)
    assert comp.shape == (L, 3, S, S) and biteq(comp[m], res["image"][m]) and biteq(comp[~m], (photo[None] * res["shadow_matte"])[~m])
    # local lights catch shadows on the ground too
    lamp = LocalLight(position=tuple(npd(s.world_points()[0]).mean(0) + 2.5 * np.asarray(UP)), radius=0.1, reference_distance=2.5)
    loc = s.shade([lamp], shadows=True, shadow_samples=4, ao_samples=4, ao_distance=2.0, seed=SEED, ground=g)
    assert int((loc["shadow_matte"][0, 0].view(-1)[on] < 1).sum()) >= 10 and loc["shadow_matte"].shape == (1, 3, S, S)
    # render_scene passes the keyword through
    zs, b2ws = GS.instances("pair")
    full = scene.render_scene(GS.make_gen(precision), zs, b2ws, GS.lights(1), shadows=True, ao_samples=16, window=9, seed=SEED, ground=g)
    assert int((full["shadow_matte"][0, 0] < 1).sum()) >= 10 and int(full["ground_mask"].sum()) == gs.n_g


def test_walks_with_and_without_a_ground(monkeypatch):
    from oi_amd import inference, scene
    from oi_amd.relight import LocalLight
    precision = "f16x3"
    gen = GS.make_gen(precision)
    zs, b2ws = GS.instances("pair")
    s = GS.traced(precision, "pair", 9)
    g = golden_ground(s)
    lamp = LocalLight(position=(0.0, -2.0, 0.0), radius=0.1, reference_distance=2.0)
    kw = dict(n_frames=3, window=9, shadow_samples=4, ao_samples=4, ao_distance=2.0, seed=SEED)
    walks = {"walk": lambda **k: inference.scene_light_walk(gen, zs, b2ws, light_radius=0.1, **kw, **k),
             "orbit": lambda **k: inference.scene_light_orbit(gen, zs, b2ws, lamp, centre=tuple(npd(s.world_points()[0]).mean(0)), radius=2.0,
                                                            height=2.0, **kw, **k)}
    for name, walk in walks.items():
        base, n0 = count_launches(monkeypatch, walk)
        none, n1 = count_launches(monkeypatch, lambda: walk(ground=None))
        assert n0 == n1 and set(base) == set(none), name
        for k in base:
            if torch.is_tensor(base[k]):
                assert biteq(base[k], none[k]), (name, k)
        res = walk(ground=g)
        n_vis = sum(s.n_vis)
        n_g = int(res["ground_mask"].sum())
        split = walk(ground=g, max_shadow_rays=s.E * 4 * max(n_vis, n_g))                  # one light per chunk
        assert res["shadow_matte"].shape == (3, 3, s.S, s.S) and res["stats"][0]["ground_pixels"] == n_g > 100, name
        for k in res:
            if torch.is_tensor(res[k]):
                assert biteq(res[k], split[k]), (name, k)
        on = res["ground_mask"].view(-1) > 0
        assert bool((res["mask"].view(-1)[on] == 0).all()) and bool((res["instance"].view(-1)[on] == -1).all()), name
        assert int((res["shadow_matte"][:, 0].reshape(3, -1)[:, on] < 1).sum()) >= 10, name
        if name == "walk":                                                     # frame 0 is the trained light: shade's own result
            from oi_amd.relight import Light
            one = s.shade([Light.from_module(gen.light)], shadows=True, shadow_samples=4, light_radius=0.1, ao_samples=4, ao_distance=2.0,
                          seed=SEED, ground=g)
            assert biteq(one["image"][0], res["image"][0]) and biteq(one["shadow_matte"][0], res["shadow_matte"][0])
