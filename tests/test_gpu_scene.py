"""Scenes of many instances on the MI355X (include/oi_scene.h; oi_amd.scene; oi_amd.inference.scene_light_walk; DESIGN section
4.19).

Exact properties are checked bit for bit against the library's own single-instance paths, which tests/test_gpu_trace.py and
tests/test_gpu_trace_batch.py hold against the fp64 oracle: the rays against ops.gen_rays, the march against sphere_trace on
each element alone, the shading against ops.surface_shade on the owner's slices, the own-instance shadows against
oi_trace_shadow_begin + the single march.  The scene layer's own decisions -- cull, depth resolve, visible lists, visibility
combination -- are checked against the float64 restatement of tests/helpers/scene_ref.py, which touches no code under test.

Independent answers:
  * WORLD POSITIONS against the restatement fed the kernel's float32 inputs.  The kernel computes each component as three
    products and three sums with contraction off (m_a0 p_0 + m_a1 p_1 + m_a2 p_2 + m_a3): each product is rounded once and
    passes through at most three rounded sums, the translation through at most three, so |error| <= 2^-24 (4 sum_k |m_ak p_k| +
    3 |m_a3|) to first order; the bar is 1.01 x that (scene_ref.transform_bar).  With |p| <= 1, a rotation and |translation|
    <= 12 that is at most 2.5e-6.
  * THE ANALYTIC TWO-SPHERE SCENE (two fields |x| - 0.5, sphere 1 between the light and sphere 0 and partly in front of it)
    against the closed-form nearest ray-sphere intersection and the closed-form shadow.  Depth bar per pixel: the march ends at
    |sdf| <= tol = 1e-5; the float32 rays (direction and c2b rounded: 2 x 6e-8 x 6.5), t (half an ulp of 6: 2.4e-7), the
    origin (2.4e-7) and the evaluation of the norm (1e-7) move the sampled sdf by less than 1.5e-6, taken as 3e-6; a sdf error
    e moves t by e / cos(incidence), so the bar is (1e-5 + 3e-6) / sqrt(1 - (rho / 0.5)^2) with rho the ray's closest approach
    to the centre: at most 2.1e-4 at the 1e-3 silhouette exclusion, 1.3e-5 head on.  Exclusions are the issue's: depths within
    1e-4 of each other, closest approach within 1e-3 of the silhouette, shadow ray's closest approach within 1e-3 of 0.5; at
    most 3 % of the owned pixels / visible points (tests/test_scene_cpu.py checks the closed form alone stays within it).
  * THE GOLDEN FIELD, TWO INSTANCES, against the fp64 oracle tracer (helpers.trace_ref.trace on the oracle's field) fed the
    library's own float32 rays, near and far: owner and depth where the oracle's statuses agree with the library's and its
    two nearest depths differ by more than 1e-4; the depth bar is tests/test_gpu_trace.py::test_primary_rays', unchanged: the
    oracle's |sdf| at the library's hit point o + depth d is at most T.TOL + G.SDF_BAR.  The distance to the oracle
    tracer's own depth is recorded (record_margin) and printed, as test_primary_rays does."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_trace as G
import test_scene_cpu as C
from conftest import record_margin
from helpers import mesh_attr_ref as A
from helpers import scene_ref as SR
from helpers import trace_ref as T
from helpers.guarded import guarded_empty, guarded_ops  # noqa: F401  (fixture)
from test_gpu_trace_batch import biteq

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS = G.PRECISIONS
SHAPES = [("pair", 9), ("triple", 12), ("triple", 16), ("offscreen", 12), ("single", 9), ("twice", 12)]
_SCENES, _ORACLE = {}, {}
npd = G.npd


def make_gen(precision):
    return G.make_gen(precision, C.R_SCENE)


def instances(kind):
    seeds, poses = zip(*SR.scene_poses(kind))
    return torch.cat([A.latent(s) for s in seeds]), torch.stack(poses)


def traced(precision, kind, W):
    """trace_scene of a test scene, computed once and never modified."""
    key = (precision, kind, W)
    if key not in _SCENES:
        from oi_amd import scene
        zs, b2ws = instances(kind)
        _SCENES[key] = scene.trace_scene(make_gen(precision), zs, b2ws, window=W)
    return _SCENES[key]


def lights(L):
    return G.lights()[:L]


def begun(kind, W):
    """oi_scene_begin alone on a test scene.  -> state, c2b, kinv, window (device), origins (numpy), S."""
    from oi_amd import ops, scene
    gen = make_gen("f32")
    _, b2ws = instances(kind)
    E = len(b2ws)
    Wn, origins = scene.scene_windows(gen, b2ws, W)
    prior = gen.sample_prior(E, {"b2w": b2ws.cuda()})
    c2b = prior["c2b"].contiguous()
    kinv = gen._kinv(c2b.device)
    window = torch.from_numpy(origins.astype(np.int32)).to(c2b.device)
    st = ops.trace_batch_state_empty(E, Wn * Wn, c2b)
    ops.scene_begin(st, c2b, kinv, window, Wn, gen.scene_resolution)
    return st, c2b, kinv, window, origins, gen.scene_resolution


def in_image(origins, e, W, S):
    X, Y = SR.window_pixels(origins[e], W)
    return X, Y, (X >= 0) & (X < S) & (Y >= 0) & (Y < S)


@pytest.mark.parametrize("kind,W", SHAPES)
def test_rays_and_cull(kind, W):
    """Every ray the begin kernel writes is ops.gen_rays' ray of its scene pixel, bit for bit; the entered set is the
    restatement's cull of the kernel's own float32 rays; the state is oi_trace_batch_begin's for the entered rays, compacted
    within each element."""
    from oi_amd import lib, ops
    st, c2b, kinv, window, origins, S = begun(kind, W)
    E, N = st.E, st.N
    ro, rd, _, _ = ops.gen_rays(c2b, kinv, torch.zeros(E, 2, device=c2b.device), S)
    counts, live = st.counts.cpu().numpy(), st.live.cpu().numpy()
    edge_total = 0
    for e in range(E):
        X, Y, ok = in_image(origins, e, W, S)
        idx = torch.from_numpy(np.nonzero(ok)[0]).cuda()
        Xt, Yt = torch.from_numpy(X[ok]).cuda(), torch.from_numpy(Y[ok]).cuda()
        assert biteq(st.rays_o[e][idx], ro[e][Yt, Xt]) and biteq(st.rays_d[e][idx], rd[e][Yt, Xt])
        o, d = npd(st.rays_o[e]), npd(st.rays_d[e])
        ent, near, far, c2 = SR.cull(o, d)
        ent &= ok
        status, steps = st.status[e].cpu().numpy(), st.steps[e].cpu().numpy()
        got = status == T.MARCH
        edge = np.abs(c2 - 1) <= 4 * 2.0 ** -24 * ((o * o).sum(-1) + 1)
        edge_total += int((edge & ok).sum())
        assert np.array_equal(got[~edge], ent[~edge]) and set(np.unique(status)) <= {T.MARCH, T.MISS} and not steps.any()
        assert not got[~ok].any()                                   # a pixel outside the image is never traced
        nr, fr, t = npd(st.near[e]), npd(st.far[e]), npd(st.t[e])
        assert np.array_equal(t, nr) and not nr[~got].any() and not fr[~got].any()
        both = got & ent
        # float32 against float64 of mid -+ h at |o| ~ 12: the chord's ends lose sqrt(1 - c2)'s cancellation near the rim
        tol = 1e-5 / np.sqrt(np.maximum(1 - c2[both], 1e-4))
        assert (np.abs(nr[both] - near[both]) <= tol).all() and (np.abs(fr[both] - far[both]) <= tol).all()
        assert (fr[both] > nr[both]).all() and (nr[both] >= 0).all()
        n_ent = int(got.sum())
        assert counts[e, 0] == n_ent and not counts[e, 1:].any()
        act = st.active[e, 0, :n_ent].cpu().numpy()
        assert sorted(act.tolist()) == np.nonzero(got)[0].tolist()   # compacted within the element, in no fixed order
        pts = npd(st.points[e])
        expect = (o[act] + nr[act, None] * d[act])
        assert np.abs(pts[:n_ent] - expect).max(initial=0.0) <= 1e-6 and not pts[n_ent:].any()
        br = npd(st.bracket[e])
        assert np.array_equal(br[:, 0], nr) and np.array_equal(br[:, 2], nr) and not br[:, 1].any() and not br[:, 3].any()
        assert not st.side[e].any()
    print(f"scene_begin[{kind},W={W}] entered", counts[:, 0].tolist(), "rays on the cull's edge", edge_total)
    assert edge_total == 0                                           # (checked for these poses on the CPU, too)
    assert live[0] == counts[:, 0].max() and not live[1:].any() and len(live) == lib.TRACE_COUNT_WORDS
    if kind == "offscreen":
        assert counts[1, 0] == 0 and counts[0, 0] > 0
    if kind == "triple":                                             # the third window lies half outside the image
        X, Y, ok = in_image(origins, 2, W, S)
        assert 0.4 * N <= ok.sum() <= 0.6 * N and counts[2, 0] > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W", SHAPES)
def test_trace_resolve_and_visible_lists(precision, kind, W):
    from oi_amd import lib, trace
    s = traced(precision, kind, W)
    st, E, N, S = s.state, s.E, s.N, s.S
    gen = make_gen(precision)
    zs, _ = instances(kind)
    origins = s.window.cpu().numpy()
    status, t = st.status.cpu().numpy(), st.t.cpu().numpy()
    # per element: t, status and steps of the entered rays are sphere_trace's on that element alone
    for e in range(E):
        ent = torch.nonzero(st.steps[e] > 0).flatten()
        assert len(ent) == s.n_entered[e]
        culled = st.steps[e] == 0
        assert bool((st.status[e][culled] == T.MISS).all())
        if len(ent) == 0:
            continue
        ref = trace.sphere_trace(gen, st.rays_o[e][ent], st.rays_d[e][ent], st.near[e][ent], st.far[e][ent], z=zs[e:e + 1].cuda())
        assert torch.equal(st.t[e][ent], ref.t) and torch.equal(st.status[e][ent], ref.status) and torch.equal(st.steps[e][ent], ref.steps)
        assert s.n_hit[e] == int((ref.status == T.HIT).sum())
    assert status.max() <= T.NONFINITE
    # resolve: the numpy arg-min with the tie rule
    owner_ref, ray_ref = SR.resolve(status, t, origins, W, S)
    if s.owner is None:
        assert not (status == T.HIT).any() and s.n_pad == 0
        return
    owner, owner_ray = s.owner.cpu().numpy(), s.owner_ray.cpu().numpy()
    assert np.array_equal(owner, owner_ref) and np.array_equal(owner_ray, ray_ref)
    if kind == "twice":                                              # one instance entered twice: element 0 owns every pixel
        assert set(np.unique(owner)) == {-1, 0} and (owner == 0).sum() == s.n_hit[0] == s.n_hit[1] and s.n_vis == [s.n_hit[0], 0]
    if kind == "pair":
        assert (owner == 0).sum() > 0 and (owner == 1).sum() > 0 and sum(s.n_vis) <= sum(s.n_hit)
    # visible lists: a permutation of the restatement's sets, vis_slot their inverse, the counts, live[last]
    sets = SR.visible_sets(owner_ref, ray_ref, E)
    counts, live = st.counts.cpu().numpy(), st.live.cpu().numpy()
    assert [len(x) for x in sets] == s.n_vis == counts[:, -1].tolist() and live[-1] == max(s.n_vis) == s.n_pad
    vis_slot = s.vis_slot.cpu().numpy()
    for e in range(E):
        mine = np.nonzero(vis_slot[e] >= 0)[0]
        assert np.array_equal(mine, sets[e]) and sorted(vis_slot[e][mine].tolist()) == list(range(len(mine)))
        # the gathered points: o + t d of the visible rays at their slots, then the coordinate origin
        pts = s.points[e]
        idx = torch.from_numpy(mine).cuda()
        slot = torch.from_numpy(vis_slot[e][mine]).cuda().long()
        want = st.rays_o[e][idx].double() + st.t[e][idx].double()[:, None] * st.rays_d[e][idx].double()
        assert len(mine) == 0 or float((pts[slot].double() - want).abs().max()) <= 1e-6
        assert not bool(pts[len(mine):].any())
    assert s.points.shape == (E, s.n_pad, 3) and s.grad.shape == (E, s.n_pad, 3) and s.offset.tolist() == SR.offsets(s.n_vis).tolist()
    stats = s.stats()
    for e in range(E):
        assert stats[e]["entered"] + stats[e]["culled"] == N and stats[e]["hits"] == s.n_hit[e] == stats[e]["hit"]
        assert stats[e]["visible"] == s.n_vis[e] and sum(stats[e][k] for k in lib.TRACE_STATUS_NAMES.values()) == N


def _owner_status(s, e):
    """Element e's status with the hits that do not own their pixel turned into misses: what oi_surface_shade on the element
    alone must see to read only the visible hits."""
    status = torch.zeros_like(s.state.status[e])
    status[s.vis_slot[e] >= 0] = T.HIT
    return status


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W,L", [("pair", 9, 1), ("triple", 12, 3), ("triple", 16, 1), ("single", 9, 3), ("twice", 12, 1)])
def test_shade_equals_surface_shade_on_the_owner(precision, kind, W, L):
    from oi_amd import ops
    from oi_amd.relight import stack_lights
    s = traced(precision, kind, W)
    st, E, S, M = s.state, s.E, s.S, s.S * s.S
    bg = (0.25, 0.5, 0.75)
    out = s.shade(lights(L), shadows=True, bg=bg)
    assert out["image"].shape == (L, 3, S, S) and out["visibility"].shape == (L, 1, S, S)
    for k in ("depth", "mask", "instance"):
        assert out[k].shape == (1, 1, S, S)
    for k in ("position", "normal_map", "albedo"):
        assert out[k].shape == (1, 3, S, S)
    flat = lambda m: m[0].reshape(m.shape[1], -1).t()
    owner, owner_ray = s.owner.long(), s.owner_ray.long()
    assert torch.equal(out["instance"].view(-1), s.owner) and out["instance"].dtype == torch.int32
    lt, bgt = stack_lights(lights(L), "cuda"), torch.tensor(bg).cuda()
    vis = out["visibility"].view(L, M)
    img = out["image"].view(L, 3, M)
    for e in range(E):
        q = torch.nonzero(owner == e).flatten()
        r = owner_ray[q]
        vis_e = torch.ones(L, s.N).cuda()
        vis_e[:, r] = vis[:, q]
        ref = ops.surface_shade(st.rays_o[e], st.rays_d[e], st.t[e], _owner_status(s, e), s.vis_slot[e], s.points[e], s.grad[e],
                                s.rgb[e], s.n_pad, s.w2b[e], lt, bgt, vis_e)
        assert biteq(img[:, :, q], ref["image"][:, :, r]), e
        assert biteq(flat(out["normal_map"])[q], ref["normal_world"][r]) and biteq(flat(out["albedo"])[q], ref["albedo"][r])
        assert biteq(out["depth"].view(-1)[q], ref["depth"][r]) and biteq(out["mask"].view(-1)[q], ref["mask"][r])
        assert bool((ref["mask"][r] == 1).all()) and torch.equal(out["depth"].view(-1)[q], st.t[e][r])
    off = owner < 0
    n_off = int(off.sum())
    assert n_off > 0 and torch.equal(img[:, :, off], bgt[None, :, None].expand(L, 3, n_off))
    assert bool(torch.isnan(out["depth"].view(-1)[off]).all()) and not bool(out["mask"].view(-1)[off].any())
    for k in ("position", "normal_map", "albedo"):
        assert not bool(flat(out[k])[off].any())
    assert bool((vis[:, off] == 1).all()) and set(np.unique(vis.cpu().numpy())) <= {0.0, 1.0}
    # the visibility is the restatement's combination of the shadow states
    n_vis = sum(s.n_vis)
    sh = s.shadow.status.cpu().numpy().reshape(E, L, n_vis)
    expect = SR.combine_visibility(sh, s.owner.cpu().numpy(), s.owner_ray.cpu().numpy(), s.vis_slot.cpu().numpy(), s.offset.cpu().numpy())
    assert np.array_equal(npd(vis), expect)
    assert set(np.unique(sh)) <= {T.MISS, T.HIT, T.LIMIT, T.START_INSIDE, T.BACKFACING}
    back = sh == T.BACKFACING
    assert np.array_equal(back.all(0), back.any(0))                  # a point facing away is BACKFACING in every element
    # without shadows: the same maps, an image at least as bright
    plain = s.shade(lights(L), bg=bg)
    assert "visibility" not in plain and biteq(plain["depth"], out["depth"]) and biteq(plain["albedo"], out["albedo"])
    assert bool((plain["image"] >= out["image"]).all())
    lit = (vis == 1)[:, None, :].expand(L, 3, M)
    assert torch.equal(plain["image"].view(L, 3, M)[lit], img[lit])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("W,L", [(9, 1), (12, 3)])
def test_own_instance_shadows_equal_the_single_shadow_trace(precision, W, L):
    """E = 1: the shadow statuses (and the evaluations each ray took) are oi_trace_shadow_begin's plus the single march's on
    the same hit points, bit for bit."""
    from oi_amd import ops, trace
    from oi_amd.relight import stack_lights
    s = traced(precision, "single", W)
    lt = stack_lights(lights(L), "cuda")
    s.visibility(lt)
    sb, n = s.shadow, s.n_vis[0]
    assert s.E == 1 and n > 0 and sb.N == L * n
    one = ops.TraceState(L * n, ref=s.points)
    pts, grad = s.points[0, :n].contiguous(), s.grad[0, :n].contiguous()
    ops.trace_shadow_begin(one, pts, grad, n, lt, s.w2b[0], s.bias)
    trace._march(s.field, one, int(one.counts[0].item()), *s.kw)
    ops.trace_finish(one)
    assert torch.equal(sb.status[0], one.status) and torch.equal(sb.steps[0], one.steps)
    # the rays are one __device__ function's in both kernels; the compiler contracts its sums of products differently in the
    # two (packed multiplies, another product fused), so origins, directions and far agree to the last bits, not bit for bit
    traced_ = one.status != T.BACKFACING                             # (a ray facing away is not traced: its far is not compared)
    close = lambda x, y: float((x - y).abs().max()) <= 1e-6
    assert close(sb.rays_o[0], one.rays_o) and close(sb.rays_d[0], one.rays_d) and close(sb.far[0][traced_], one.far[traced_])
    assert int(traced_.sum()) > 0
    assert not bool(sb.near[0].any())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_scenes(precision):
    """A window half outside the image, an instance wholly off screen, a scene without any hit, E = 1: none writes outside
    its buffers (the guarded arenas), and the other elements are what they are without the odd one."""
    from oi_amd import scene
    gen = make_gen(precision)
    bg = (0.25, 0.5, 0.75)
    W = 12
    S = gen.scene_resolution
    # an instance wholly off screen: zero rays entered; element 0 is what it is in the pair (same pose, same window)
    zs, b2ws = instances("offscreen")
    off = scene.render_scene(gen, zs, b2ws, lights=lights(3), shadows=True, bg=bg, window=W)
    so, sp = off["scene"], traced(precision, "pair", W)
    assert so.n_entered[1] == 0 and so.n_hit[1] == 0 and so.n_vis[1] == 0 and so.n_entered[0] == sp.n_entered[0] > 0
    assert torch.equal(so.state.t[0], sp.state.t[0]) and torch.equal(so.state.status[0], sp.state.status[0])
    assert bool((so.state.status[1] == T.MISS).all()) and not bool(so.state.steps[1].any())
    assert set(np.unique(off["instance"].cpu().numpy())) == {-1, 0}
    alone = scene.render_scene(gen, zs[:1], b2ws[:1], lights=lights(3), shadows=True, bg=bg, window=W)      # E = 1
    for k in ("image", "depth", "mask", "position", "normal_map", "albedo", "visibility", "instance"):
        assert biteq(off[k], alone[k]), k
    # a window half outside the image
    tri = traced(precision, "triple", W)
    out = tri.shade(lights(1), shadows=True, bg=bg)
    assert tri.n_entered[2] > 0 and int(tri.window[2, 0]) < 0 and (out["instance"] == 2).sum() == tri.n_vis[2]
    assert bool(torch.isfinite(out["image"]).all())
    # a scene without any hit: nothing after the begin stage, bg everywhere
    zs, b2ws = instances("nothing")
    none = scene.render_scene(gen, zs, b2ws, lights=lights(3), shadows=True, bg=bg, window=W)
    sn = none["scene"]
    assert sn.n_pad == 0 and sn.n_entered == [0, 0] and sn.n_evals == 0 and sn.owner is None and sn.shadow is None
    assert torch.equal(none["image"], torch.tensor(bg).cuda()[None, :, None, None].expand(3, 3, S, S))
    assert bool(torch.isnan(none["depth"]).all()) and not bool(none["mask"].any()) and bool((none["instance"] == -1).all())
    assert bool((none["visibility"] == 1).all()) and not bool(none["position"].any())
    assert all(x["miss"] == W * W and x["culled"] == W * W for x in none["stats"])
    # rays entered and nothing hit: one step, the whole window aimed beside the object (max_steps = 1 leaves LIMIT only)
    zs, b2ws = instances("single")
    lim = scene.render_scene(gen, zs, b2ws, window=W, max_steps=1, bg=bg)
    if lim["scene"].n_pad == 0:
        assert lim["scene"].owner is None and bool((lim["instance"] == -1).all())
    assert lim["stats"][0]["limit"] + lim["stats"][0]["hit"] + lim["stats"][0]["miss"] == W * W


def test_shade_refuses_a_shadow_batch_above_the_limit():
    s = traced("f16x3", "pair", 9)
    n = s.E * 3 * sum(s.n_vis)
    with pytest.raises(ValueError, match=str(n)):
        s.shade(lights(3), shadows=True, max_shadow_rays=n - 1)
    s.shade(lights(3), shadows=True, max_shadow_rays=n)
    with pytest.raises(ValueError, match="lights"):
        s.shade(G.lights() * 86)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_light_walk_split_equals_unsplit(precision):
    from oi_amd import inference, scene
    from oi_amd.relight import Light
    gen = make_gen(precision)
    zs, b2ws = instances("pair")
    s = traced(precision, "pair", 12)
    whole = inference.scene_light_walk(gen, zs, b2ws, n_frames=5, window=12)
    split = inference.scene_light_walk(gen, zs, b2ws, n_frames=5, window=12, max_shadow_rays=2 * s.E * sum(s.n_vis))
    for k in ("image", "visibility", "mask", "depth", "instance"):
        assert biteq(whole[k], split[k]), k
    S = gen.scene_resolution
    assert whole["image"].shape == (5, 3, S, S) and whole["visibility"].shape == (5, 1, S, S)
    assert split["stats"][0]["shadow_evals"] > 0 and float(whole["visibility"].min()) == 0.0
    # frame 0 is render_scene under the trained light
    one = scene.render_scene(gen, zs, b2ws, lights=[Light.from_module(gen.light)], shadows=True, window=12)
    assert biteq(one["image"][0], whole["image"][0]) and biteq(one["depth"], whole["depth"])
    plain = inference.scene_light_walk(gen, zs, b2ws, n_frames=5, window=12, shadows=False)
    assert "visibility" not in plain and bool((plain["image"] >= whole["image"]).all())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W", [("triple", 16), ("pair", 9)])
def test_world_positions(precision, kind, W):
    """The position map and oi_scene_points' list against the float64 restatement fed the kernel's float32 inputs; the bar is
    the one derived in this file's docstring."""
    s = traced(precision, kind, W)
    out = s.shade(lights(1))
    pos = npd(out["position"][0].reshape(3, -1).t())
    owner, owner_ray, vis_slot = s.owner.cpu().numpy(), s.owner_ray.cpu().numpy(), s.vis_slot.cpu().numpy()
    wp, wn, elem = s.world_points()
    assert wp.shape == (sum(s.n_vis), 3) and elem.dtype == torch.int32
    worst = 0.0
    for e in range(s.E):
        q = np.nonzero(owner == e)[0]
        slot = vis_slot[e, owner_ray[q]]
        p = npd(s.points[e])[slot]
        m = npd(s.b2w[e])
        ref, bar = SR.transform(m, p), SR.transform_bar(m, p)
        err = np.abs(pos[q] - ref)
        worst = max(worst, float((err / bar).max(initial=0.0)))
        assert (err <= bar).all()
        g = int(s.offset[e]) + slot
        assert np.array_equal(npd(wp)[g], pos[q]) and (elem.cpu().numpy()[g] == e).all()
        n_map = npd(out["normal_map"][0].reshape(3, -1).t())[q]
        assert np.abs(npd(wn)[g] - n_map).max(initial=0.0) <= 1e-6 and np.abs(np.linalg.norm(npd(wn)[g], axis=-1) - 1).max(initial=0.0) < 1e-5
    record_margin(f"scene_world_positions[{precision},{kind},W={W}]", "error_over_bar", worst)
    print(f"scene_world_positions[{precision},{kind},W={W}] worst error / bar", worst, "largest bar", float(bar.max(initial=0.0)))


def _analytic(E_only=None):
    """The analytic two-sphere scene through the ops wrappers, the field |x| - 0.5 evaluated by torch between the steps.
    E_only = 1: sphere 0 alone."""
    from oi_amd import ops
    sc = SR.analytic_scene()
    E = E_only or 2
    W, S = sc["W"], sc["S"]
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32).cuda().contiguous()
    c2b, b2w, kinv = f32(sc["c2b"][:E]), f32(sc["b2w"][:E]), f32(sc["K_inv"])
    w2b = f32(np.stack([SR.rigid_inverse(m) for m in sc["b2w"][:E]]))
    window = torch.tensor(sc["origins"][:E], dtype=torch.int32).cuda()
    sphere = lambda pts: pts.norm(dim=-1) - SR.RADIUS

    def march(st):
        # up to OI_TRACE_MAX_STEPS steps: on an exact distance field a ray at incidence cos(a) closes in on the surface by the
        # factor 1 - cos(a) per step, 160 steps at the 1e-3 silhouette exclusion
        sdf = torch.zeros(E, st.N).cuda()
        bound, k = int(st.live[0].item()), 0
        while bound > 0 and k < T.MAX_MAX_STEPS:
            sdf[:, :bound] = sphere(st.points[:, :bound])
            ops.trace_batch_step(st, sdf, bound, k, T.TOL, T.OMEGA)
            k += 1
            bound = int(st.live[k].item())

    st = ops.trace_batch_state_empty(E, W * W, c2b)
    ops.scene_begin(st, c2b, kinv, window, W, S)
    march(st)
    ops.trace_batch_finish(st)
    n_hit = st.counts[:, -1].tolist()
    owner, owner_ray = ops.scene_resolve(st, window, W, S)
    vis_index, vis_slot = ops.scene_visible(st, owner, window, W, S)
    n_pad, n_vis = int(st.live[-1].item()), st.counts[:, -1].tolist()
    pts = ops.trace_batch_gather(st, vis_index, n_pad)
    grad, rgb = (2.0 * pts).contiguous(), torch.full_like(pts, 0.5)
    offset = torch.tensor(SR.offsets(n_vis), dtype=torch.int32).cuda()
    pos, nrm, elem = ops.scene_points(st, pts, grad, n_pad, offset, sum(n_vis), b2w, w2b)
    lt = torch.tensor([T.light_block(tuple(float(x) for x in sc["light"]))], dtype=torch.float32).cuda()
    sb = ops.trace_batch_state_empty(E, sum(n_vis), pos)
    ops.scene_shadow_begin(sb, pts, grad, n_pad, offset, elem, pos, nrm, sum(n_vis), lt, w2b, T.BIAS)
    march(sb)
    ops.trace_batch_finish(sb)
    vis = ops.scene_visibility(sb.status, owner, owner_ray, vis_slot, offset, E, W * W, 1, sum(n_vis), S)
    out = ops.scene_shade(st, W, S, owner, owner_ray, vis_slot, pts, grad, rgb, n_pad, w2b, b2w, lt, None, vis)
    return dict(sc=sc, st=st, sb=sb, owner=owner.cpu().numpy(), depth=npd(out["depth"]), vis=npd(vis)[0], out=out, n_hit=n_hit,
                n_vis=n_vis, pos=npd(out["position"]))


def test_analytic_two_sphere_scene():
    a, alone = _analytic(), _analytic(1)
    sc = a["sc"]
    cf = SR.analytic_closed_form(sc)
    owner, depth = a["owner"], a["depth"]
    owned = cf["owner"] >= 0
    keep = ~cf["excluded"]
    n_excl = int((cf["excluded"] & owned).sum())
    assert n_excl <= SR.AN_CAP * owned.sum()                          # a condition on the scene, not a measurement
    assert np.array_equal(owner[keep], cf["owner"][keep])
    cmp_ = keep & owned
    err = np.abs(depth[cmp_] - cf["depth"][cmp_])
    ratio = float((err / cf["bar"][cmp_]).max())
    record_margin("scene_analytic", "depth_error_over_bar", ratio)
    print("analytic scene: owned", int(owned.sum()), "excluded", n_excl, "worst depth error", float(err.max()), "worst error / bar", ratio,
          "hits", a["n_hit"], "visible", a["n_vis"])
    assert (err <= cf["bar"][cmp_]).all()
    assert np.array_equal(np.isnan(depth), owner < 0) and sum(a["n_vis"]) < sum(a["n_hit"])       # sphere 1 hides hits of sphere 0
    # world positions lie on the spheres
    for e in range(2):
        q = owner == e
        assert np.abs(np.linalg.norm(a["pos"][q] - SR.AN_CENTRES[e], axis=-1) - SR.RADIUS).max() < 2e-5
    # the shadow sphere 1 throws on sphere 0
    q0 = np.nonzero(cf["on0"])[0]
    ok = keep[q0] & (owner[q0] == 0) & ~cf["shadow_excluded"]
    n_sh_excl = int(cf["shadow_excluded"].sum())
    assert n_sh_excl <= SR.AN_CAP * len(q0)
    assert np.array_equal(a["vis"][q0][ok], cf["lit"][ok].astype(np.float64))
    same = ok & (alone["owner"][q0] == 0)
    by_other = same & (alone["vis"][q0] == 1) & (a["vis"][q0] == 0)
    print("analytic scene: sphere-0 points compared", int(ok.sum()), "lit", int(a["vis"][q0][ok].sum()), "shadowed by sphere 1 only",
          int(by_other.sum()), "shadow exclusions", n_sh_excl)
    assert by_other.sum() > 5                                         # otherwise the test shows nothing
    assert np.array_equal(alone["vis"][q0][same], cf["lit_alone"][same].astype(np.float64))
    # sphere 1 is convex and nothing stands before it: its points are lit wherever they face the light
    sh = a["sb"].status.cpu().numpy()
    assert set(np.unique(sh)) <= {T.MISS, T.HIT, T.BACKFACING}


def oracle_pair(s):
    """The fp64 oracle tracer on the library's own float32 rays of the golden 'pair' scene, once per window."""
    if s.W not in _ORACLE:
        st = s.state
        _ORACLE[s.W] = C.golden_pair_oracle(npd(st.rays_o), npd(st.rays_d), npd(st.near), npd(st.far), st.steps.cpu().numpy() > 0,
                                            s.window.cpu().numpy(), s.W, s.S)
    return _ORACLE[s.W]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_golden_pair_against_the_oracle_tracer(precision):
    s = traced(precision, "pair", C.GOLDEN_W)
    st, S, W = s.state, s.S, s.W
    o_status, o_t, o_owner, o_ray, gap = oracle_pair(s)
    status = st.status.cpu().numpy()
    origins = s.window.cpu().numpy()
    agree = np.ones(S * S, dtype=bool)                                # every element covering the pixel ended as on the oracle
    for e in range(2):
        X, Y, ok = in_image(origins, e, W, S)
        agree[(Y * S + X)[ok]] &= (status[e] == o_status[e])[ok]
    owner, owner_ray = s.owner.cpu().numpy(), s.owner_ray.cpu().numpy()
    owned = (owner >= 0) | (o_owner >= 0)
    keep = agree & (gap > C.ORACLE_DEPTH_GAP)
    n_excl = int((owned & ~keep).sum())
    assert n_excl <= C.ORACLE_CAP * owned.sum()                       # a condition, checked on the oracle alone on the CPU too
    assert np.array_equal(owner[keep], o_owner[keep]) and np.array_equal(owner_ray[keep], o_ray[keep])
    out = s.shade(lights(1))
    depth = npd(out["depth"].view(-1))
    worst_sdf = worst_t = 0.0
    for e, (seed, _) in enumerate(SR.scene_poses("pair")):
        q = np.nonzero(keep & (owner == e))[0]
        r = owner_ray[q]
        pts = npd(st.rays_o[e])[r] + depth[q, None] * npd(st.rays_d[e])[r]
        on = np.abs(T.Field(seed).sdf(pts))
        worst_sdf = max(worst_sdf, float(on.max(initial=0.0)))
        worst_t = max(worst_t, float(np.abs(depth[q] - o_t[e][r]).max(initial=0.0)))
        assert len(q) > 20
    case = f"scene_golden_pair[{precision}]"
    record_margin(case, "hit_sdf_worst", worst_sdf)
    record_margin(case, "depth_vs_oracle_trace", worst_t)
    print(case, "owned", int(owned.sum()), "excluded", n_excl, "status disagreements", int((status != o_status).sum()),
          "worst oracle |sdf| at the depth", worst_sdf, "bar", T.TOL + G.SDF_BAR, "worst |depth - oracle depth|", worst_t)
    assert worst_sdf <= T.TOL + G.SDF_BAR
    # mutual shadows: with the light behind instance 1 as seen from instance 0, instance 1 darkens points of instance 0 that
    # are lit when it is not there
    from oi_amd import scene
    from oi_amd.relight import Light
    zs, b2ws = instances("pair")
    towards = tuple((b2ws[1][:3, 3] - b2ws[0][:3, 3]).tolist())
    lt = [Light(direction=towards)]
    both = s.shade(lt, shadows=True)
    alone = scene.render_scene(make_gen(precision), zs[:1], b2ws[:1], lights=lt, shadows=True, window=W)
    mine = (both["instance"] == 0) & (alone["instance"] == 0)
    darker = mine & (alone["visibility"] == 1) & (both["visibility"] == 0)
    brighter = mine & (alone["visibility"] == 0) & (both["visibility"] == 1)
    print(case, "points of instance 0 shadowed by instance 1 only:", int(darker.sum()), "of", int(mine.sum()))
    assert int(darker.sum()) > 0 and int(brighter.sum()) == 0


def test_c_abi_rejects_invalid_arguments_and_launches_nothing():
    """The refusals of tests/test_scene_cpu.py on real, poisoned device arrays: each returns a negative status with its text,
    and no array is touched."""
    from oi_amd import lib
    L = lib.load()
    E, N = 3, 16
    g = lambda sh, dt=torch.float32: guarded_empty(sh, dt, what="untouched", must_write=False)
    shapes = dict(rays_o=(E, N, 3), rays_d=(E, N, 3), near_=(E, N), far_=(E, N), t=(E, N), bracket=(E, N, 4), points=(E, N, 3))
    arr = {k: g(sh) for k, sh in shapes.items()}
    arr.update(status=g((E, N), torch.uint8), side=g((E, N), torch.uint8), steps=g((E, N), torch.int16),
               active=g((E, 2, N), torch.int32), counts=g((E, lib.TRACE_COUNT_WORDS), torch.int32))
    other = g((1024 * 8,))                                  # live, windows, owner maps, lists ...: never dereferenced
    p = lambda t_: ctypes.c_void_p(t_.data_ptr())
    cases = C.invalid_argument_cases(lib, L, p(other), {k: p(v) for k, v in arr.items()})
    for call, entry, text in cases:
        rc = call()
        msg = L.oi_last_error().decode()
        assert rc < 0 and msg.startswith(entry) and text in msg, (entry, text, rc, msg)
    torch.cuda.synchronize()
    for k, v in list(arr.items()) + [("other", other)]:
        fresh = guarded_empty(tuple(v.shape), v.dtype, what="pattern", must_write=False)
        assert torch.equal(v.view(torch.uint8), fresh.view(torch.uint8)), k                 # still poison: nothing ran
