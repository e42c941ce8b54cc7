"""Local lights in scenes of many instances on the MI355X (include/oi_local_light.h; oi_amd.scene; oi_amd.inference.scene_light_orbit;
DESIGN section 4.27): a light that stands between the instances, shadow rays that end at it, every ray against every instance.

Exact properties are checked bit for bit against the library's own single-view entries (tests/test_gpu_local_light.py holds
those against the fp64 restatement): the image of an owned pixel against oi_surface_shade_local on the owner's slices, a split
trace against the unsplit one, K = 1 against the single view.  The layer's own decisions -- the ray in an element that does not
own the point, the cull, the clip to the light, the combination across elements and chunks -- are checked against
tests/helpers/local_light_ref.py and scene_light_ref.py, which touch no code under test.

Bars: those tests/test_gpu_scene_light.py uses for the same comparisons -- 1e-6 on the owner's origins, directions and far
against the single-view entry (the drawn direction against the fp64 restatement: DIRECTION_BAR below); for another element the restatement is fed the kernel's own float32 direction: origins 2e-5
(|o| up to ~12), directions 1e-6, near / far 1e-5 / sqrt(1 - c2) (far also where it is t_light: 1e-5), the entered set exact
outside the cull's edge |c2 - 1| <= 4 eps (|o|^2 + 1) and the clip's edge |near - t_light| <= 1e-5; counts exact."""
import numpy as np
import pytest
import torch

import test_gpu_scene as GS
import test_gpu_trace as G
from conftest import record_margin
from helpers import local_light_ref as LL
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T
from helpers.guarded import guarded_ops  # noqa: F401  (fixture)
from test_gpu_scene_light import cuts_of, scene_arrays
from test_gpu_trace_batch import biteq

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS, npd = G.PRECISIONS, G.npd
EPS = 2.0 ** -24
SEED = SL.SEED
NEW_OPS = ("local_light_begin", "surface_shade_local", "scene_local_light_begin", "scene_shade_local")
# The drawn direction against the fp64 restatement.  The header's m = u1 (1 - cos_max) cancels for a light that subtends a small
# angle: the triple's third instance sees the sphere light (radius 0.15) from 6 units, sin_max = 0.025, 1 - cos_max = 3e-4 with
# an absolute fp32 error of ~6e-8 (2e-4 relative), which sin(alpha) = sqrt(m (2 - m)) ~ 0.025 passes on as ~2e-6 in the
# direction.  Measured here: 1.79e-6 (pair: below 1e-6).  The arithmetic is the header's and stays; the bar is 2.8 x the margin
# measured against the restatement (the project's rule: at most 3 x), DESIGN section 4.27.
DIRECTION_BAR = 5e-6
COLOURS = dict(ambient=(0.2, 0.25, 0.3), diffuse=(0.7, 0.6, 0.5), specular=(0.3, 0.2, 0.35), shininess=6.0)


def centres(kind):
    return [np.asarray(p[:3, 3], dtype=np.float64) for _, p in SR.scene_poses(kind)]


def scene_lights(kind):
    """A point light between the first two instances (beside the first one of a single instance) and a sphere light off to
    the side, in the world frame."""
    from oi_amd.relight import LocalLight
    c = centres(kind)
    mid = (c[0] + c[1]) / 2 if len(c) > 1 else c[0] + np.array([0.3, -0.2, -0.9])
    return [LocalLight(position=tuple(mid), reference_distance=0.8, **COLOURS),
            LocalLight(position=tuple(c[0] + np.array([-1.2, -0.9, -0.6])), radius=0.15, reference_distance=1.4, **COLOURS)]


def stacked(lights):
    from oi_amd.relight import stack_local_lights
    return stack_local_lights(lights, "cuda")


def sampled(s, S, cuts, lt, seed=SEED):
    """The sequence of include/oi_local_light.h for a scene through the ops wrappers, chunk by chunk.  -> chunks (the finished
    batch states), their begin states (status, near, far copies), count, out."""
    from oi_amd import ops, trace
    pos, nrm, elem = s.world_points()
    pixel = s.point_pixels()
    n_vis, L, M = sum(s.n_vis), lt.shape[0], s.S * s.S
    count, out = ops._new(pos, L, M).view(torch.int32), ops._new(pos, L, M)
    chunks, begins, j0 = [], [], 0
    for c in cuts:
        sb = ops.trace_batch_state_empty(s.E, L * c * n_vis, pos)
        ops.scene_local_light_begin(sb, s.points, s.grad, s.n_pad, s.offset, elem, pixel, pos, nrm, n_vis, s.w2b, s.bias, S, j0, c, lt, seed)
        begins.append(dict(status=sb.status.clone(), counts=sb.counts.clone(), live=sb.live.clone()))
        bound = int(sb.live[0].item())
        if bound:
            trace._march_batch(s.field, sb, *s.kw, bound=bound, anyhit=True)
            ops.trace_batch_finish(sb)
        ops.scene_occlusion_resolve(sb.status, s.owner, s.owner_ray, s.vis_slot, s.offset, s.E, s.N, L, S, j0, c, n_vis, s.S, count, out,
                                    j0 + c == S)
        chunks.append(sb)
        j0 += c
    return dict(chunks=chunks, begins=begins, count=count, out=out)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W", [("pair", 9), ("triple", 12)])
def test_rays_in_every_element(precision, kind, W):
    """One uneven chunk of oi_scene_local_light_begin: the owner's ray against oi_local_light_begin on the owner's slices, every
    other element's ray, cull and clip against the restatement fed the kernel's own direction."""
    from oi_amd import ops
    s = GS.traced(precision, kind, W)
    lights = scene_lights(kind)
    lt, L, S, j0, c = stacked(lights), 2, 4, 1, 3
    pos, nrm, elem = s.world_points()
    pixel = s.point_pixels()
    n, E = sum(s.n_vis), s.E
    sb = ops.trace_batch_state_empty(E, L * c * n, pos)
    ops.scene_local_light_begin(sb, s.points, s.grad, s.n_pad, s.offset, elem, pixel, pos, nrm, n, s.w2b, s.bias, S, j0, c, lt, SEED)
    a = scene_arrays(s)
    elem_np, off = elem.cpu().numpy(), a["offset"]
    sh = (E, L, c, n)
    o, d = npd(sb.rays_o).reshape(*sh, 3), npd(sb.rays_d).reshape(*sh, 3)
    near, far, status = npd(sb.near).reshape(sh), npd(sb.far).reshape(sh), sb.status.cpu().numpy().reshape(sh)
    assert set(np.unique(status)) <= {T.MARCH, T.MISS, T.BACKFACING} and not sb.steps.any()
    back = status == T.BACKFACING
    assert np.array_equal(back.all(0), back.any(0))                               # facing away: BACKFACING in every element
    mine = np.broadcast_to((elem_np[None] == np.arange(E)[:, None])[:, None, None, :], sh)
    entered = status == T.MARCH
    assert not near[mine].any() and entered[mine & ~back].all() and not near[~entered].any() and not far[~entered].any()
    worst = 0.0
    for e in range(E):
        sel = np.nonzero(elem_np == e)[0]
        ne = len(sel)
        if ne == 0:
            continue
        # the owner's rays: the single-view entry on the owner's slices, samples j0 .. j0 + c - 1 of S
        one = ops.TraceState(L * S * ne, ref=s.points)
        ops.local_light_begin(one, s.points[e, :ne].contiguous(), s.grad[e, :ne].contiguous(), pixel[sel[0]:sel[0] + ne].contiguous(), ne,
                              lt, S, s.w2b[e], s.bias, SEED)
        pick = lambda x, *t: npd(x).reshape(L, S, ne, *t)[:, j0:j0 + c]
        assert sel[0] == off[e] and np.array_equal(sel, off[e] + np.arange(ne))
        st1 = one.status.cpu().numpy().reshape(L, S, ne)[:, j0:j0 + c]
        assert np.array_equal(status[e][:, :, sel], st1)
        close = lambda x, y: float(np.abs(x - y).max()) <= 1e-6
        assert close(o[e][:, :, sel], pick(one.rays_o, 3)) and close(d[e][:, :, sel], pick(one.rays_d, 3)) and close(far[e][:, :, sel], pick(one.far))
        # every other element: the restatement's rule on the kernel's own direction and its fp64 t_light
        pts, grad = npd(s.points[e, :ne]), npd(s.grad[e, :ne])
        for l in range(L):
            r = LL.rays(pts, grad, pixel[sel].cpu().numpy(), npd(lt[l]), a["w2b"][e], S, SEED, bias=s.bias, j0=j0, Sc=c)
            d_own = d[e, l][:, sel]
            worst = max(worst, float(np.abs(d_own - r["d"]).max()))
            o_world = npd(pos)[sel] + s.bias * npd(nrm)[sel]
            for eo in range(E):
                if eo == e:
                    continue
                ro, rd, rnear, rfar, rent, c2 = LL.other_element(o_world, d_own, a["w2b"][e], a["w2b"][eo], r["t_light"])
                traced = r["traced"] & (np.abs((SL.unit(grad)[None] * d_own).sum(-1)) > 1e-6)
                edge = (np.abs(c2 - 1) <= 4 * EPS * ((ro ** 2).sum(-1) + 1)) | (np.abs(SR.cull(ro, rd)[1] - r["t_light"]) <= 1e-5)
                cmp_ = traced & ~edge
                got = status[eo, l][:, sel]
                assert np.array_equal((got == T.MARCH)[cmp_], rent[cmp_]) and (got[cmp_ & ~rent] == T.MISS).all()
                assert float(np.abs(o[eo, l][:, sel] - ro)[cmp_].max(initial=0.0)) <= 2e-5
                assert float(np.abs(d[eo, l][:, sel] - rd)[cmp_].max(initial=0.0)) <= 1e-6
                both = cmp_ & rent
                tol = 1e-5 / np.sqrt(np.maximum(1 - c2[both], 1e-4))
                assert (np.abs(near[eo, l][:, sel][both] - rnear[both]) <= tol).all() and (np.abs(far[eo, l][:, sel][both] - rfar[both]) <= tol).all()
                assert (far[eo, l][:, sel][both] <= r["t_light"][both] + 1e-5).all()       # no ray goes on beyond the light
    record_margin(f"scene_local_light_directions[{precision},{kind}]", "error_over_bar", worst / DIRECTION_BAR)
    print(f"scene_local_light rays[{precision},{kind}] worst direction error against the restatement {worst:.3g}")
    assert worst <= DIRECTION_BAR
    if E > 1:
        assert (entered & ~mine).any() and ((status == T.MISS) & ~mine).any()
    counts, live = sb.counts.cpu().numpy(), sb.live.cpu().numpy()
    flat = entered.reshape(E, -1)
    for e in range(E):
        n_ent = int(flat[e].sum())
        assert counts[e, 0] == n_ent and not counts[e, 1:].any()
        assert sorted(sb.active[e, 0, :n_ent].cpu().numpy().tolist()) == np.nonzero(flat[e])[0].tolist()
    assert live[0] == counts[:, 0].max() and not live[1:].any()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W", [("pair", 9), ("triple", 12)])
def test_visibility_and_chunks(precision, kind, W):
    """Per-pixel visibility against the restatement's combination of the finished states; a split trace (chunks of 1, and 1 + 3)
    equals the unsplit one byte for byte; SceneSurface.local_visibility under a small max_shadow_rays is the same map."""
    s = GS.traced(precision, kind, W)
    lt, S = stacked(scene_lights(kind)), 4
    L, n, E, a = 2, sum(s.n_vis), s.E, scene_arrays(s)
    runs = [sampled(s, S, cuts, lt) for cuts in cuts_of(S)]
    whole = runs[0]
    for r, cuts in zip(runs, cuts_of(S)):
        sts = [sb.status.cpu().numpy().reshape(E, L, c, n) for sb, c in zip(r["chunks"], cuts)]
        count, out = SL.counts(sts, a["owner"], a["owner_ray"], a["vis_slot"], a["offset"], S)
        assert np.array_equal(r["count"].cpu().numpy(), count) and np.array_equal(npd(r["out"]), out)
        assert biteq(r["out"], whole["out"]) and torch.equal(r["count"], whole["count"])
        joined = np.concatenate(sts, axis=2)
        assert np.array_equal(joined, whole["chunks"][0].status.cpu().numpy().reshape(E, L, S, n))     # per ray, whatever the chunk
        assert joined.max() <= T.BACKFACING
    vis = npd(whole["out"])
    assert set(np.unique(vis * S)) <= set(range(S + 1)) and (vis[:, a["owner"] < 0] == 1).all() and 0 < vis[:, a["owner"] >= 0].mean() < 1
    for limit in (E * L * n * S, E * L * n * 3, E * L * n):
        assert biteq(s.local_visibility(lt, S, SEED, max_shadow_rays=limit), whole["out"]), limit
    with pytest.raises(ValueError, match="max_shadow_rays"):
        s.local_visibility(lt, S, SEED, max_shadow_rays=E * L * n - 1)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_point_light_between_two_instances(precision):
    """The pair's objects stay within 0.8 of their centres, which are 1.73 apart: seen from a point of one, the other lies
    wholly beyond the light at the midpoint (0.86 from either centre).  The light's rays end there, so its visibility against
    every instance is its visibility against the owner alone; the directional light along the same axis goes on and is blocked."""
    from oi_amd.relight import Light, stack_lights
    s = GS.traced(precision, "pair", 9)
    c = centres("pair")
    half = np.linalg.norm(c[1] - c[0]) / 2
    extent = float(s.points.norm(dim=-1).max())
    assert s.E == 2 and min(s.n_vis) > 0 and extent < 0.8 < half
    lt = stacked(scene_lights("pair")[:1])
    n, a = sum(s.n_vis), scene_arrays(s)
    vis = s.local_visibility(lt, 1, SEED)
    st = s.shadow.status.cpu().numpy().reshape(2, 1, 1, n)
    elem = s.world_points()[2].cpu().numpy()
    own = st[elem, 0, 0, np.arange(n)]
    other = st[1 - elem, 0, 0, np.arange(n)]
    assert (other[own != T.BACKFACING] == T.MISS).all() and (st[:, 0, 0][:, own == T.BACKFACING] == T.BACKFACING).all()
    marched = s.shadow.steps.cpu().numpy().reshape(2, n)[1 - elem, np.arange(n)] > 0
    assert marched.any()                                                          # some rays did enter the other's unit sphere
    own_only = np.where(own[None] == T.MISS, T.MISS, T.HIT) * np.ones((2, 1), dtype=np.int64)
    _, expect = SL.counts([own_only.reshape(2, 1, 1, n)], a["owner"], a["owner_ray"], a["vis_slot"], a["offset"], 1)
    assert np.array_equal(npd(vis), expect) and 0 < npd(vis)[:, a["owner"] >= 0].mean() < 1
    # the directional lights along the axis, from either side
    axis = (c[1] - c[0]) / (2 * half)
    dl = stack_lights([Light(direction=tuple(axis)), Light(direction=tuple(-axis))], "cuda")
    s.visibility(dl)
    sd = s.shadow.status.cpu().numpy().reshape(2, 2, n)
    own_d, other_d = sd[elem, :, np.arange(n)].T, sd[1 - elem, :, np.arange(n)].T
    blocked = (own_d == T.MISS) & (other_d != T.MISS)
    print(f"point light between[{precision}] extent {extent:.3f} directional rays blocked by the other instance", int(blocked.sum()))
    assert blocked.any()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W", [("pair", 9), ("triple", 12), ("single", 9)])
def test_shade_is_the_single_view_shade_on_the_owner(precision, kind, W, monkeypatch):
    from oi_amd import ops
    s = GS.traced(precision, kind, W)
    lights = scene_lights(kind)
    lt, L, S, M = stacked(lights), 2, s.S, s.S * s.S
    bg = (0.25, 0.5, 0.75)
    out = s.shade(lights, shadows=True, bg=bg, shadow_samples=4, seed=SEED)
    assert set(out) == {"depth", "position", "normal_map", "albedo", "mask", "instance", "image", "visibility", "stats"}
    assert out["image"].shape == (L, 3, S, S) and out["visibility"].shape == (L, 1, S, S)
    plain = s.shade(GS.lights(1), bg=bg)
    for k in ("depth", "position", "normal_map", "albedo", "mask", "instance"):   # the G-buffer: oi_scene_shade's bytes
        assert biteq(out[k], plain[k]), k
    owner, owner_ray = s.owner.long(), s.owner_ray.long()
    vis, img, bgt = out["visibility"].view(L, M), out["image"].view(L, 3, M), torch.tensor(bg).cuda()
    ao = torch.rand(M).cuda()
    with_ao = s._shade(lt, bgt, vis, ("image",), ao=ao)["image"]
    for e in range(s.E):
        q = torch.nonzero(owner == e).flatten()
        r = owner_ray[q]
        vis_e, ao_e = torch.ones(L, s.N).cuda(), torch.ones(s.N).cuda()
        vis_e[:, r], ao_e[r] = vis[:, q], ao[q]
        args = (s.state.rays_o[e], s.state.rays_d[e], s.state.t[e], GS._owner_status(s, e), s.vis_slot[e], s.points[e], s.grad[e], s.rgb[e],
                s.n_pad, s.w2b[e], lt, bgt, vis_e)
        assert biteq(img[:, :, q], ops.surface_shade_local(*args, None, ("image",))["image"][:, :, r]), e
        assert biteq(with_ao[:, :, q], ops.surface_shade_local(*args, ao_e, ("image",))["image"][:, :, r]), e
    off = owner < 0
    assert torch.equal(img[:, :, off], bgt[None, :, None].expand(L, 3, int(off.sum())))
    no_shadow = s.shade(lights, bg=bg)
    assert "visibility" not in no_shadow and bool((no_shadow["image"] >= out["image"]).all())
    for bad in (dict(light_radius=0.1, shadows=True), dict(lights=lights + GS.lights(1))):
        with pytest.raises(ValueError):
            s.shade(**{**dict(lights=lights), **bad})

    # directional lights: none of the new entries runs, and the bytes are a second call's
    def refuse(*a_, **k_):
        raise AssertionError("an entry of include/oi_local_light.h ran under directional lights")
    kw = dict(shadows=True, shadow_samples=4, light_radius=0.1, ao_samples=4, seed=SEED)
    first = s.shade(GS.lights(2), **kw)
    for name in NEW_OPS:
        monkeypatch.setattr(ops, name, refuse)
    again = s.shade(GS.lights(2), **kw)
    monkeypatch.undo()
    for k in ("image", "visibility", "ambient_occlusion"):
        assert biteq(first[k], again[k]), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_instance_equals_the_single_view(precision):
    """K = 1: statuses and steps are oi_local_light_begin's plus the single any-hit march's on the owner's slices; the
    visibility and the image on the window are the single view's (the bars of tests/test_gpu_scene_light.py's same test)."""
    from oi_amd import ops, trace
    s = GS.traced(precision, "single", 9)
    n, S, L = s.n_vis[0], 4, 2
    lt = stacked(scene_lights("single"))
    pixel = s.point_pixels()
    pts, grad = s.points[0, :n].contiguous(), s.grad[0, :n].contiguous()
    hit_slot = torch.full((s.S * s.S,), -1, dtype=torch.int32, device="cuda")
    hit_slot[pixel.long()] = torch.arange(n, dtype=torch.int32, device="cuda")
    run = sampled(s, S, [S], lt)
    one = ops.TraceState(L * S * n, ref=s.points)
    ops.local_light_begin(one, pts, grad, pixel, n, lt, S, s.w2b[0], s.bias, SEED)
    trace._march(s.field, one, int(one.counts[0].item()), *s.kw, anyhit=True)
    ops.trace_finish(one)
    sb = run["chunks"][0]
    assert torch.equal(sb.status[0], one.status) and torch.equal(sb.steps[0], one.steps)
    traced_ = one.far > 0
    close = lambda x, y: float((x - y).abs().max()) <= 1e-6
    assert close(sb.rays_o[0], one.rays_o) and close(sb.rays_d[0], one.rays_d) and close(sb.far[0][traced_], one.far[traced_])
    assert biteq(run["out"], ops.occlusion_resolve(one.status, hit_slot, s.S * s.S, n, L, S))
    assert int((one.status == T.MISS).sum()) > 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_scene_light_orbit(precision, monkeypatch):
    from oi_amd import inference, scene
    gen = GS.make_gen(precision)
    zs, b2ws = GS.instances("pair")
    light = scene_lights("pair")[1]
    c = centres("pair")
    kw = dict(n_frames=5, centre=tuple((c[0] + c[1]) / 2), radius=1.9, height=0.5, shadows=True, shadow_samples=4, seed=SEED, window=9)
    whole = inference.scene_light_orbit(gen, zs, b2ws, light, **kw)
    S = gen.scene_resolution
    assert whole["image"].shape == (5, 3, S, S) and whole["visibility"].shape == (5, 1, S, S) and whole["positions"].shape == (5, 3)
    st = whole["stats"]
    per_sample = len(st) * sum(x["visible"] for x in st)
    # two lights per batch: 2 + 2 + 1; then one light in chunks of three samples
    for limit in (2 * 4 * per_sample, 3 * per_sample):
        split = inference.scene_light_orbit(gen, zs, b2ws, light, max_shadow_rays=limit, **kw)
        for k in ("image", "visibility", "mask", "depth", "instance"):
            assert biteq(whole[k], split[k]), (k, limit)
    for f in (0, 3):
        one = scene.render_scene(gen, zs, b2ws, lights=[light.replace(position=tuple(whole["positions"][f]))], shadows=True,
                                 shadow_samples=4, seed=SEED, window=9)
        assert biteq(one["image"][0], whole["image"][f]) and biteq(one["visibility"][0], whole["visibility"][f])
