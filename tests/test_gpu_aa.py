"""Adaptive anti-aliasing of the traced renderer on the MI355X (include/oi_aa.h; oi_amd.trace.render_surface(aa_samples=...);
oi_amd.inference.surface_light_walk).

The references are tests/helpers/aa_ref.py -- the classification and the resolve restated in numpy fp32 in the header's operation
order (bit for bit), the sub-pixel rays in float64 -- and the library's own entries where the stage claims to add nothing new:
oi_gen_rays for a zero offset, oi_trace_begin for the started state, sphere_trace and oi_surface_shade for the sub-samples.

Bars: the project's ray bars (origins, near and far 1e-5, directions 2e-6); everything else is exact.  The flagged share is held
to the cap the rehearsal on the oracle sets (tests/test_aa_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import test_aa_cpu as AC
import test_gpu_local_light as LLT
import test_gpu_occlusion as OC
import test_gpu_trace as G
from conftest import record_margin
from helpers import aa_ref as AR
from helpers import mesh_attr_ref as A
from helpers import occlusion_ref as R
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS, npd = G.PRECISIONS, G.npd
_p, _cuda, _bits = OC._p, OC._cuda, OC._bits
ORIGIN_BAR, DIRECTION_BAR = 1e-5, 2e-6
R_AA, BG = AC.R_AA, (0.1, 0.2, 0.3)
AA_OPS = ("aa_classify", "aa_begin", "aa_resolve")
UNCHANGED = ("depth", "position", "normal_map", "normal_object", "albedo", "mask", "visibility", "ambient_occlusion")


def view(precision, seed, pose, R_=R_AA):
    return G.make_gen(precision, R_), A.latent(seed)[0], T.pose(pose)


class Spy:
    """Records what the three ops of include/oi_aa.h were given and returned while they run unchanged."""

    def __init__(self, monkeypatch):
        from oi_amd import ops
        self.classify, self.begin, self.resolve = [], [], []
        classify, begin, resolve = ops.aa_classify, ops.aa_begin, ops.aa_resolve

        def aa_classify(*a, **k):
            out = classify(*a, **k)
            self.classify.append(out)
            return out

        def aa_begin(st, c2b, kinv, offs, R_, edge_index, n_edge, offsets):
            begin(st, c2b, kinv, offs, R_, edge_index, n_edge, offsets)
            self.begin.append(dict(st=st, c2b=c2b, kinv=kinv, offs=offs, R=R_, edge_index=edge_index, n_edge=n_edge, offsets=offsets))

        def aa_resolve(centre, sub, edge_slot, n_edge, S, out=None):
            res = resolve(centre, sub, edge_slot, n_edge, S, out=out)
            self.resolve.append(dict(centre=centre, sub=sub, edge_slot=edge_slot, n_edge=n_edge, S=S, out=res))
            return res
        for name, fn in zip(AA_OPS, (aa_classify, aa_begin, aa_resolve)):
            monkeypatch.setattr(ops, name, fn)


def _f32(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the default path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_sample_is_the_call_without_the_keywords(precision, monkeypatch):
    from oi_amd import ops, trace
    gen, z, b2w = view(precision, 0, "centre")
    kw = dict(lights=G.lights(), shadows=True, bg=BG)
    plain = trace.render_surface(gen, z, b2w, **kw)

    def refuse(*a, **k):
        raise AssertionError("an entry of include/oi_aa.h ran with aa_samples=1")
    for name in AA_OPS:
        monkeypatch.setattr(ops, name, refuse)
    same = trace.render_surface(gen, z, b2w, aa_samples=1, aa_adaptive=True, aa_plane=0.5, aa_cos=0.5, aa_pattern=None, **kw)
    full = trace.render_surface(gen, z, b2w, aa_samples=1, aa_adaptive=False, aa_pattern=[[0.0, 0.0]], **kw)
    monkeypatch.undo()
    for other in (same, full):
        assert set(plain) == set(other) and "coverage" not in other and "aa_pixels" not in other["stats"]
        for k, v in plain.items():
            if torch.is_tensor(v):
                assert _same_bits(v, other[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 2. the classification
# ---------------------------------------------------------------------------------------------------------------------
def _check_classify(edge_index, edge_slot, count, ref):
    """The flagged set is the restatement's, the list and the slots are inverse to each other, the count matches."""
    n, slot = int(count.item()), edge_slot.cpu().numpy()
    index = edge_index.cpu().numpy()[:n]
    assert np.array_equal(slot >= 0, ref)
    assert n == int(ref.sum()) and sorted(index.tolist()) == np.nonzero(ref)[0].tolist()
    assert np.array_equal(slot[index], np.arange(n)) and slot.max(initial=-1) == n - 1 and slot.min(initial=-1) >= -1
    return set(index.tolist())


@pytest.mark.parametrize("seed,pose", R.SOFT_VIEWS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_classification_is_the_restatement(precision, seed, pose):
    from oi_amd import ops
    _, s = OC.surface(precision, seed, pose)
    r, H = s.res, R_AA
    args = (r.status, r.hit_slot, r.hit_points, s.grad, s.n_hit, H, H)
    ref = AR.classify(_f32(r.status), _f32(r.hit_slot), _f32(r.hit_points), _f32(s.grad), H, H)
    first = _check_classify(*ops.aa_classify(*args), ref)
    assert first == _check_classify(*ops.aa_classify(*args), ref)                  # two calls: the same set, whatever the slots
    share = ref.mean()
    record_margin(f"aa_classify[{precision},seed={seed},{pose}]", "flagged_share", share)
    print(f"aa_classify[{precision},seed={seed},{pose}]: flagged {int(ref.sum())} of {ref.size} ({share:.3f})")
    assert 0 < share <= AC.FLAGGED_CAP
    for plane, cos in ((0.1, 0.5), (0.5, 0.95), (0.0, 0.0)):                       # other thresholds: the plane and normal criteria fire
        ref2 = AR.classify(_f32(r.status), _f32(r.hit_slot), _f32(r.hit_points), _f32(s.grad), H, H, plane, cos)
        _check_classify(*ops.aa_classify(*args, plane, cos), ref2)


@pytest.mark.parametrize("name", AR.SYNTHETIC)
def test_classification_of_the_synthetic_surfaces(name):
    from oi_amd import ops
    a, expected = AR.synthetic(name)
    H, W = a["H"], a["W"]
    dev = [_cuda(a["status"], torch.uint8), _cuda(a["hit_slot"], torch.int32), _cuda(a["hit_points"]), _cuda(a["grad"])]
    for kw in (dict(), dict(plane=0.99), dict(cos=0.9)):
        ref = AR.classify(**a, **kw)
        _check_classify(*ops.aa_classify(*dev, H * W, H, W, kw.get("plane", 0.5), kw.get("cos", 0.5)), ref)
        if not kw:
            img = ref.reshape(H, W)
            assert tuple(np.nonzero(img.any(0))[0].tolist()) == tuple(expected) and np.array_equal(img.all(0), img.any(0))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the sub-pixel rays
# ---------------------------------------------------------------------------------------------------------------------
def _flagged_view(precision, seed, pose):
    """A traced view, its camera and its flagged pixels."""
    from oi_amd import ops, trace
    gen, z, b2w = view(precision, seed, pose)
    _, s = OC.surface(precision, seed, pose)
    ro, rd, near, far, w2b, c2b, kinv, offs = trace._view_rays_camera(gen, b2w)
    assert _same_bits(ro, s.ro) and _same_bits(rd, s.rd)
    edge_index, edge_slot, count = ops.aa_classify(s.res.status, s.res.hit_slot, s.res.hit_points, s.grad, s.n_hit, R_AA, R_AA)
    return dict(gen=gen, s=s, ro=ro, rd=rd, near=near, far=far, cam=(c2b, kinv, offs), edge_index=edge_index, n_edge=int(count.item()))


@pytest.mark.parametrize("seed,pose", R.SOFT_VIEWS)
def test_rays(seed, pose):
    from oi_amd import ops
    v = _flagged_view("f32", seed, pose)
    n, S = v["n_edge"], 4
    pix = v["edge_index"][:n].long()
    # an all-zero pattern: oi_gen_rays' ray of the pixel, bit for bit, for every sample
    st = ops.TraceState((S - 1) * n, ref=v["ro"])
    ops.aa_begin(st, *v["cam"], R_AA, v["edge_index"], n, torch.zeros(S, 2).cuda())
    for name, got, ref in (("rays_o", st.rays_o, v["ro"]), ("rays_d", st.rays_d, v["rd"]), ("near", st.near, v["near"]), ("far", st.far, v["far"])):
        assert _same_bits(got, ref[pix].repeat(S - 1, *([1] * (ref.dim() - 1)))), name
    # the R2 pattern against the float64 restatement
    pat = AR.r2_pattern(S)
    st = ops.TraceState((S - 1) * n, ref=v["ro"])
    ops.aa_begin(st, *v["cam"], R_AA, v["edge_index"], n, torch.from_numpy(pat).cuda())
    o, d, near, far = AR.sub_rays(*(npd(c) for c in v["cam"]), R_AA, pix.cpu().numpy(), pat)
    errs = dict(origins=np.abs(npd(st.rays_o) - o).max(), directions=np.abs(npd(st.rays_d) - d).max(),
                near=np.abs(npd(st.near) - near).max(), far=np.abs(npd(st.far) - far).max())
    for k, e in errs.items():
        record_margin(f"aa_rays[seed={seed},{pose}]", k, e)
    print(f"aa_rays[seed={seed},{pose}]", errs)
    assert errs["origins"] < ORIGIN_BAR and errs["near"] < ORIGIN_BAR and errs["far"] < ORIGIN_BAR and errs["directions"] < DIRECTION_BAR
    assert not _same_bits(st.rays_d, v["rd"][pix].repeat(S - 1, 1))                # the offsets do move the rays
    # everything else the entry writes: oi_trace_begin's bytes on a copy of those rays
    twin = ops.TraceState(st.N, st.rays_o.clone(), st.rays_d.clone(), st.near.clone(), st.far.clone())
    ops.trace_begin(twin)
    for name in ("t", "status", "steps", "bracket", "side", "points", "counts"):
        assert _same_bits(getattr(st, name), getattr(twin, name)), name
    assert torch.equal(st.active[0], twin.active[0]) and torch.equal(st.active[0], torch.arange(st.N, dtype=torch.int32).cuda())


# ---------------------------------------------------------------------------------------------------------------------
# 4. march and shade add nothing new
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sub_samples_are_sphere_trace_and_surface_shade(precision, monkeypatch):
    from oi_amd import ops, trace
    from oi_amd.fields import LatentField
    from oi_amd.relight import stack_lights
    gen, z, b2w = view(precision, 1, "off")
    spy = Spy(monkeypatch)
    out = trace.render_surface(gen, z, b2w, lights=G.lights(), bg=BG, aa_samples=4)
    monkeypatch.undo()
    (b,), (img, cov) = spy.begin, spy.resolve
    st, sub = b["st"], out["aa_trace"]
    assert st.N == 3 * b["n_edge"] == out["stats"]["aa_rays"] and out["stats"]["aa_pixels"] == b["n_edge"] > 0
    flagged = b["edge_index"][:b["n_edge"]]
    assert bool((flagged[1:] > flagged[:-1]).all())                                # the host lists the flagged pixels in ascending order
    zc = z.cuda().reshape(1, -1)
    res = trace.sphere_trace(gen, st.rays_o, st.rays_d, st.near, st.far, z=zc)
    for name in ("t", "status", "steps"):
        assert _same_bits(getattr(res, name), getattr(sub, name)), name
    assert res.n_evals == sub.n_evals == out["stats"]["aa_evals"] > 0
    fld = LatentField(gen, zc, None, "test").prepare(zc, None)
    _, grad, rgb = fld.full(res.hit_points)
    w2b = trace._view_rays(gen, b2w)[4]
    lt = stack_lights(G.lights(), "cuda")
    shaded = ops.surface_shade(st.rays_o, st.rays_d, res.t, res.status, res.hit_slot, res.hit_points, grad, rgb, len(res.hit_index), w2b,
                               lt, trace._bg(BG, "cuda"), None, ("mask", "image"))
    assert _same_bits(shaded["image"].view(9, -1), img["sub"]) and _same_bits(shaded["mask"].view(1, -1), cov["sub"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the resolve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_resolve_and_the_unchanged_maps(precision, monkeypatch):
    from oi_amd import trace
    gen, z, b2w = view(precision, 0, "centre")
    S = 4
    kw = dict(lights=G.lights(), bg=BG, shadows=True, ao_samples=R.AO_S, seed=R.SEED)
    one = trace.render_surface(gen, z, b2w, **kw)
    spy = Spy(monkeypatch)
    out = trace.render_surface(gen, z, b2w, aa_samples=S, **kw)
    monkeypatch.undo()
    img, cov = spy.resolve
    L, N = 3, R_AA * R_AA
    slot = img["edge_slot"].cpu().numpy()
    flagged = slot >= 0
    assert img["S"] == cov["S"] == S and img["n_edge"] == int(flagged.sum()) == out["stats"]["aa_pixels"]
    assert np.array_equal(_f32(out["aa_mask"]).reshape(-1), flagged.astype(np.float32))
    # the centre planes are the one-sample call's, and the results are the fp32 restatement of (centre, sub-samples)
    assert _same_bits(img["centre"].view(L, 3, R_AA, R_AA), one["image"]) and _same_bits(cov["centre"].view(1, 1, R_AA, R_AA), one["mask"])
    ref_img = AR.resolve(_f32(one["image"]).reshape(3 * L, N), _f32(img["sub"]), slot, S)
    ref_cov = AR.resolve(_f32(one["mask"]).reshape(1, N), _f32(cov["sub"]), slot, S)
    image, coverage = _f32(out["image"]).reshape(3 * L, N), _f32(out["coverage"]).reshape(1, N)
    assert np.array_equal(image.view(np.uint32), ref_img.view(np.uint32))
    assert np.array_equal(coverage.view(np.uint32), ref_cov.view(np.uint32))
    assert np.array_equal(image[:, ~flagged].view(np.uint32), _f32(one["image"]).reshape(3 * L, N)[:, ~flagged].view(np.uint32))
    assert (image[:, flagged] != _f32(one["image"]).reshape(3 * L, N)[:, flagged]).any()
    k = coverage[0] * S
    assert np.array_equal(k, np.round(k)) and k.min() >= 0 and k.max() <= S
    assert np.array_equal(coverage[0][~flagged], _f32(one["mask"]).reshape(N)[~flagged])
    assert ((coverage[0] > 0) & (coverage[0] < 1)).any()                             # the outline blends
    for name in UNCHANGED:                                                           # the centre sample's, byte for byte
        assert _same_bits(out[name], one[name]), name
    assert set(out) - set(one) == {"coverage", "aa_mask", "aa_trace"}


# ---------------------------------------------------------------------------------------------------------------------
# 6. adaptive against full
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_adaptive_is_full_at_the_flagged_pixels(precision, monkeypatch):
    from oi_amd import ops, trace
    gen, z, b2w = view(precision, 1, "off")
    kw = dict(lights=G.lights(), bg=BG, shadows=True, aa_samples=4)
    adaptive = trace.render_surface(gen, z, b2w, **kw)

    def refuse(*a, **k):
        raise AssertionError("oi_aa_classify ran with aa_adaptive=False")
    monkeypatch.setattr(ops, "aa_classify", refuse)
    full = trace.render_surface(gen, z, b2w, aa_adaptive=False, **kw)
    monkeypatch.undo()
    N = R_AA * R_AA
    assert full["stats"]["aa_pixels"] == N and bool((full["aa_mask"] == 1).all()) and full["stats"]["aa_rays"] == 3 * N
    on = adaptive["aa_mask"].view(-1) > 0
    assert 0 < int(on.sum()) == adaptive["stats"]["aa_pixels"] < N
    assert _same_bits(adaptive["image"].view(9, N)[:, on], full["image"].view(9, N)[:, on])
    assert _same_bits(adaptive["coverage"].view(N)[on], full["coverage"].view(N)[on])


# ---------------------------------------------------------------------------------------------------------------------
# 7. it anti-aliases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_adaptive_samples_approach_the_converged_image(precision):
    from oi_amd import trace
    gen, z, b2w = view(precision, 0, "centre", T.R_VIEW)
    kw = dict(lights=G.lights(), bg=BG)
    one = trace.render_surface(gen, z, b2w, **kw)
    eight = trace.render_surface(gen, z, b2w, aa_samples=8, **kw)
    ref = trace.render_surface(gen, z, b2w, aa_samples=64, aa_adaptive=False, **kw)
    on = (eight["aa_mask"].view(-1) > 0).cpu().numpy()
    N = T.R_VIEW ** 2
    err = lambda o: float(np.abs(npd(o["image"]) - npd(ref["image"])).reshape(9, N)[:, on].mean())
    e1, e8 = err(one), err(eight)
    case = f"aa_converges[{precision}]"
    record_margin(case, "one_sample", e1)
    record_margin(case, "adaptive_8", e8)
    record_margin(case, "ratio", e8 / e1)
    print(case, "flagged", int(on.sum()), "of", N, "mean |image - S64|: one sample", e1, "adaptive 8", e8, "ratio", e8 / e1)
    assert on.sum() > 0 and e8 < e1


# ---------------------------------------------------------------------------------------------------------------------
# 8. shadows, ambient occlusion and local lights go through
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("local", [False, True], ids=["directional", "local"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_soft_shadows_occlusion_and_local_lights(precision, local):
    from oi_amd import trace
    seed, pose = R.SOFT_VIEWS[1]
    gen, z, b2w = view(precision, seed, pose)
    kw = dict(shadows=True, shadow_samples=4, ao_samples=4, seed=R.SEED, bg=BG)
    kw.update(dict(lights=LLT.golden_lights(pose)) if local else dict(lights=G.lights(), light_radius=0.05))
    one = trace.render_surface(gen, z, b2w, **kw)
    out = trace.render_surface(gen, z, b2w, aa_samples=4, **kw)
    L, N = out["image"].shape[0], R_AA * R_AA
    assert bool(torch.isfinite(out["image"]).all()) and out["image"].shape == one["image"].shape
    off = out["aa_mask"].view(-1) == 0
    assert 0 < int(off.sum()) < N
    assert _same_bits(out["image"].view(3 * L, N)[:, off], one["image"].view(3 * L, N)[:, off])
    for name in UNCHANGED:
        assert _same_bits(out[name], one[name]), name
    # the sampled sub-sample rays are keyed by the sub-sample ray index, which follows the pixel order: the frame is reproducible
    again = trace.render_surface(gen, z, b2w, aa_samples=4, **kw)
    assert _same_bits(out["image"], again["image"]) and _same_bits(out["aa_trace"].status, again["aa_trace"].status)
    st = out["stats"]
    assert st["aa_evals"] > out["aa_trace"].n_evals > 0 and st["aa_rays"] == 3 * st["aa_pixels"]      # shadow and occlusion rays of the sub-samples


# ---------------------------------------------------------------------------------------------------------------------
# 9. the light walk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_light_walk_traces_the_sub_samples_once(precision, monkeypatch):
    from oi_amd import inference, trace
    from oi_amd.relight import Light
    gen, z, b2w = view(precision, 1, "off")
    spy = Spy(monkeypatch)
    walk = inference.surface_light_walk(gen, z, b2w, n_frames=5, aa_samples=4, bg=BG)
    monkeypatch.undo()
    assert len(spy.begin) == 1 and len(spy.classify) == 1
    assert walk["image"].shape == (5, 3, R_AA, R_AA) and walk["stats"]["aa_pixels"] == spy.begin[0]["n_edge"] > 0
    base = Light.from_module(gen.light)
    dirs = inference.light_walk_directions(base.direction, 5)
    for i in range(5):
        lt = base if i == 0 else base.replace(direction=tuple(dirs[i]))
        one = trace.render_surface(gen, z, b2w, lights=[lt], shadows=True, bg=BG, aa_samples=4)
        assert torch.equal(walk["image"][i], one["image"][0]), i
        assert torch.equal(walk["visibility"][i], one["visibility"][0]), i
    for name in ("mask", "coverage", "aa_mask"):
        assert torch.equal(walk[name], one[name]), name
    plain = inference.surface_light_walk(gen, z, b2w, n_frames=5, bg=BG)
    off = (walk["aa_mask"].view(-1) == 0)
    assert torch.equal(plain["image"].view(15, -1)[:, off], walk["image"].view(15, -1)[:, off]) and "coverage" not in plain
    # frame 0 is the trained light: surface_frames' frame with the same keywords
    fr = inference.surface_frames(gen, [z], [b2w], keys=("image", "coverage", "aa_mask"), shadows=True, bg=BG, aa_samples=4)
    assert torch.equal(fr["image"][0], walk["image"][0]) and torch.equal(fr["coverage"], walk["coverage"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_light_orbit_traces_the_sub_samples_once(precision, monkeypatch):
    from oi_amd import inference, trace
    seed, pose = R.SOFT_VIEWS[1]
    gen, z, b2w = view(precision, seed, pose)
    light = LLT.golden_lights(pose)[1]
    kw = dict(shadows=True, shadow_samples=R.SOFT_S, seed=R.SEED, bg=BG, aa_samples=4)
    spy = Spy(monkeypatch)
    orbit = inference.surface_light_orbit(gen, z, b2w, light, n_frames=3, centre=tuple(float(x) for x in b2w[:3, 3]), radius=1.6, height=0.4, **kw)
    monkeypatch.undo()
    assert len(spy.begin) == 1 and orbit["image"].shape == (3, 3, R_AA, R_AA)
    for f in range(3):
        one = trace.render_surface(gen, z, b2w, lights=[light.replace(position=tuple(orbit["positions"][f]))], **kw)
        assert torch.equal(orbit["image"][f], one["image"][0]) and torch.equal(orbit["visibility"][f], one["visibility"][0]), f
    assert torch.equal(orbit["coverage"], one["coverage"]) and torch.equal(orbit["aa_mask"], one["aa_mask"])


WALK_KW = dict(shadows=True, shadow_samples=4, ao_samples=4, aa_samples=2, bg=BG, seed=R.SEED)
WALK_MAPS = ("mask", "depth", "ambient_occlusion", "coverage", "aa_mask")   # what does not depend on the light


def walk_frames_are_single_renders(walk, single, lights, maps):
    """Every stage at once through the walk loop: frame k is the single render under light k alone, bit for bit (NaN depth
    included), and the light-independent maps are that render's."""
    assert len(lights) == walk["image"].shape[0] == 3
    for k, lt in enumerate(lights):
        one = single(lt)
        for name in maps:
            per_frame = walk[name].shape[0] == 3
            assert _same_bits(walk[name][k] if per_frame else walk[name], one[name][0] if per_frame else one[name]), (k, name)


@pytest.mark.parametrize("entry", ["walk", "orbit"])
def test_walk_frames_are_the_single_renders(entry):
    from oi_amd import inference, trace
    from oi_amd.relight import Light
    seed, pose = R.SOFT_VIEWS[1]
    gen, z, b2w = view("f16x3", seed, pose)
    if entry == "walk":
        base = Light.from_module(gen.light)
        lights = [base] + [base.replace(direction=tuple(d)) for d in inference.light_walk_directions(base.direction, 3)[1:]]
        walk = inference.surface_light_walk(gen, z, b2w, n_frames=3, **WALK_KW)
    else:
        light = LLT.golden_lights(pose)[1]
        walk = inference.surface_light_orbit(gen, z, b2w, light, n_frames=3, centre=tuple(float(x) for x in b2w[:3, 3]), radius=1.6,
                                             height=0.4, **WALK_KW)
        lights = [light.replace(position=tuple(p)) for p in walk["positions"]]
    assert walk["stats"]["aa_pixels"] > 0 and walk["stats"]["shadow_evals"] > 0 and walk["stats"]["ao_evals"] > 0
    walk_frames_are_single_renders(walk, lambda lt: trace.render_surface(gen, z, b2w, lights=[lt], **WALK_KW), lights,
                                   ("image", "visibility") + WALK_MAPS)


# ---------------------------------------------------------------------------------------------------------------------
# 10. guarded shapes through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _classify_case(H, W, share, seed):
    """oi_aa_classify on guarded buffers for a random H x W trace with `share` of the pixels hit."""
    from oi_amd import lib, ops
    rs = np.random.RandomState(seed)
    N = H * W
    hit = rs.rand(N) < share if 0 < share < 1 else np.full(N, share >= 1)
    n_hit = int(hit.sum())
    slot = np.full(N, -1, np.int32)
    slot[np.nonzero(hit)[0]] = rs.permutation(n_hit).astype(np.int32)
    status = np.where(hit, T.HIT, rs.choice([T.MISS, T.LIMIT], N)).astype(np.uint8)
    pts, grad = rs.randn(max(n_hit, 1), 3).astype(np.float32) * 0.3, rs.randn(max(n_hit, 1), 3).astype(np.float32)
    d_status, d_slot = guarded_copy(_cuda(status, torch.uint8), "status"), guarded_copy(_cuda(slot, torch.int32), "hit_slot")
    d_pts, d_grad = guarded_copy(_cuda(pts[:n_hit]), "hit_points"), guarded_copy(_cuda(grad[:n_hit]), "grad")
    edge_index = guarded_empty((N,), torch.int32, what="edge_index", must_write=False)
    edge_slot, count = guarded_empty((N,), torch.int32, what="edge_slot"), guarded_empty((1,), torch.int32, what="count")
    rc = lib.load().oi_aa_classify(_p(d_status), _p(d_slot), _p(d_pts) if n_hit else None, _p(d_grad) if n_hit else None, n_hit, H, W,
                                   0.5, 0.5, _p(edge_index), _p(edge_slot), _p(count), ops._stream())
    assert rc == 0
    ref = AR.classify(status, slot, pts[:n_hit], grad[:n_hit], H, W)
    _check_classify(edge_index, edge_slot, count, ref)
    return ref


@pytest.mark.parametrize("H,W", [(3, 5), (17, 16)])
def test_guarded_classify(H, W):
    mixed = _classify_case(H, W, 0.6, seed=H)
    assert 0 < mixed.sum()
    _classify_case(H, W, 1.0, seed=H + 1)                                            # every pixel hit: random normals flag them
    assert _classify_case(H, W, 0.0, seed=H + 2).sum() == 0                          # no pixel hit: count 0, every slot -1


@pytest.mark.parametrize("n_edge,S", [(1, 2), (257, 64)])
def test_guarded_begin(n_edge, S):
    from oi_amd import lib, ops, trace
    gen, _, b2w = view("f32", 0, "off")
    cam = trace._view_rays_camera(gen, b2w)[5:]
    rs = np.random.RandomState(n_edge)
    pix = rs.permutation(R_AA * R_AA)[:n_edge].astype(np.int32)
    pat = AR.r2_pattern(S)
    c2b, kinv, offs = (guarded_copy(c, n) for c, n in zip(cam, ("c2b", "kinv", "offs")))
    edge_index, offsets = guarded_copy(_cuda(pix, torch.int32), "edge_index"), guarded_copy(_cuda(pat), "offsets")
    Q = (S - 1) * n_edge
    arr, St = OC._guarded_state(Q, "aa")
    assert lib.load().oi_aa_begin(ctypes.byref(St), _p(c2b), _p(kinv), _p(offs), R_AA, _p(edge_index), n_edge, _p(offsets), S,
                                  ops._stream()) == 0
    o, d, near, far = AR.sub_rays(*(npd(c) for c in cam), R_AA, pix, pat)
    assert np.abs(npd(arr["rays_o"]) - o).max() < ORIGIN_BAR and np.abs(npd(arr["rays_d"]) - d).max() < DIRECTION_BAR
    assert np.abs(npd(arr["near_"]) - near).max() < ORIGIN_BAR and np.abs(npd(arr["far_"]) - far).max() < ORIGIN_BAR
    assert torch.equal(arr["t"], arr["near_"]) and bool((arr["status"] == T.MARCH).all()) and not bool(arr["steps"].any())
    assert not bool(_bits(arr["side"]).any()) and torch.equal(arr["active"][0], torch.arange(Q, dtype=torch.int32).cuda())
    assert int(arr["counts"][0].item()) == Q and not bool(arr["counts"][1:].any())
    pts = torch.addcmul(arr["rays_o"].double(), arr["near_"].double()[:, None], arr["rays_d"].double())
    assert float((arr["points"].double() - pts).abs().max()) <= 2.0 ** -23           # every point written: o + near d, one rounding (coordinates below 4)
    assert torch.equal(arr["bracket"], torch.stack([arr["near_"], torch.zeros_like(arr["near_"])] * 2, -1))


@pytest.mark.parametrize("P,n_edge,S", [(1, 40, 2), (9, 100, 64), (1, 0, 4), (9, 0, 2)])
def test_guarded_resolve(P, n_edge, S):
    from oi_amd import lib, ops
    N = 17 * 16
    rs = np.random.RandomState(P * 1000 + n_edge + S)
    slot = np.full(N, -1, np.int32)
    slot[rs.permutation(N)[:n_edge]] = rs.permutation(n_edge).astype(np.int32)
    centre, sub = rs.rand(P, N).astype(np.float32), rs.rand(P, (S - 1) * n_edge).astype(np.float32)
    d_centre, d_slot = guarded_copy(_cuda(centre), "centre"), guarded_copy(_cuda(slot, torch.int32), "edge_slot")
    d_sub = guarded_copy(_cuda(sub), "sub") if n_edge else None
    out = guarded_empty((P, N), what="out")
    assert lib.load().oi_aa_resolve(_p(d_centre), _p(d_sub) if n_edge else None, _p(d_slot), N, n_edge, S, P, _p(out), ops._stream()) == 0
    ref = AR.resolve(centre, sub, slot, S)
    assert np.array_equal(_f32(out).view(np.uint32), ref.view(np.uint32))
    if n_edge == 0:
        assert _same_bits(out, d_centre)


def test_refused_arguments_launch_nothing():
    from oi_amd import lib, ops
    L_, st = lib.load(), ops._stream()
    buf = torch.zeros(64, device="cuda")
    p = _p(buf)
    assert L_.oi_aa_classify(p, p, p, p, 1, 2, 2, 1.0, 0.5, p, p, p, st) != 0        # plane_threshold outside [0, 1)
    assert L_.oi_aa_classify(p, p, p, p, 1, 2, 2, 0.5, float("nan"), p, p, p, st) != 0
    assert L_.oi_aa_classify(p, p, p, p, 5, 2, 2, 0.5, 0.5, p, p, p, st) != 0        # more hits than pixels
    assert L_.oi_aa_classify(p, p, None, p, 1, 2, 2, 0.5, 0.5, p, p, p, st) != 0
    assert L_.oi_aa_resolve(p, p, p, 4, 2, 1, 1, p, st) != 0                          # S = 1
    assert L_.oi_aa_resolve(p, p, p, 4, 2, 65, 1, p, st) != 0
    assert L_.oi_aa_resolve(p, None, p, 4, 2, 2, 1, p, st) != 0                       # sub missing with flagged pixels
    assert L_.oi_aa_resolve(p, p, p, 4, 5, 2, 1, p, st) != 0                          # more flagged pixels than pixels
    arr, St = OC._guarded_state(6, "refused")
    for a in arr.values():                                                            # nothing may be written: fill what the guards expect
        a.view(torch.uint8).zero_()
    assert L_.oi_aa_begin(ctypes.byref(St), p, p, p, 8, p, 3, p, 2, st) != 0          # N = 6 is not (S - 1) * n_edge = 3
    assert L_.oi_aa_begin(ctypes.byref(St), p, p, p, 1, p, 6, p, 2, st) != 0          # R = 1
    assert L_.oi_aa_begin(ctypes.byref(St), p, p, p, 8, p, 6, p, 1, st) != 0          # S = 1
    assert L_.oi_aa_begin(ctypes.byref(St), p, p, None, 8, p, 6, p, 2, st) != 0
    assert not bool(buf.any())
