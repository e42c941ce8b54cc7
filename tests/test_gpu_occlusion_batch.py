"""The secondary rays and the shade of E views in one chain on the MI355X (include/oi_occlusion_batch.h;
oi_amd.trace.render_surfaces(batch_secondary=True); oi_amd.inference.surface_frames).

The reference of everything here is the library's own single-view path, bit for bit: the begin entries of oi_trace.h,
oi_occlusion.h and oi_local_light.h for the rays, render_surface's shadow_trace / ao_trace for the marched states and
render_surface's maps for the maps (each tested against the fp64 restatements by tests/test_gpu_trace.py,
tests/test_gpu_occlusion.py and tests/test_gpu_local_light.py).  Nothing is compared within a tolerance: the batched kernels
call the single-view device functions on an element's slices, per-ray results depend neither on the slot nor on the bound, and
the resolve adds integers and divides once.

Views: the three of helpers/trace_batch_ref.BATCH_VIEWS at 48 x 48 (their hit counts differ, so the padded hit lists have
padding slots) and a fourth whose rays all miss (n_hit_e == 0): trace_batch_ref.away_rays(130), repeated to the view's 2304
rays, put in place of the rays of the pose AWAY (tests/test_occlusion_batch_cpu.py rehearses on the oracle that each
misses on its first sample).  L = 2 lights, S = 3 shadow samples of radius 0.1, A = 5 ambient samples; Sc = 2 makes the
chunks [0, 2) and [2, 3) ragged."""
import copy

import numpy as np
import pytest
import torch

import test_gpu_trace as G
from conftest import record_margin
from helpers import mesh_attr_ref as A
from helpers import trace_batch_ref as B
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS = G.PRECISIONS
NL, S, NA, RADIUS, SEED, AO_DISTANCE = 2, 3, 5, 0.1, 11, 0.5
AWAY = "away"
AWAY_POSE = T.pose("centre").clone()      # recognised by identity: its rays are replaced by the away rays
VIEWS4 = B.BATCH_VIEWS + ((0, AWAY),)
MAPS = ("visibility", "ambient_occlusion", "image", "depth", "mask", "position", "normal_map", "normal_object", "albedo")
SINGLE_OPS = ("trace_shadow_begin", "occlusion_light_begin", "occlusion_ambient_begin", "local_light_begin", "trace_visibility",
              "occlusion_resolve", "surface_shade", "surface_shade_ao", "surface_shade_local")
BATCH_OPS = ("occlusion_batch_begin", "occlusion_batch_resolve", "surface_shade_batch")
OTHER_OPS = ("trace_batch_begin", "trace_batch_finish", "trace_batch_gather", "trace_finish")
MLP_ENTRIES = ("oi_sdf_mlp_fwd_segments", "oi_sdf_mlp_fwd")

_REF, _PRIMARY = {}, {}


def biteq(a, b):
    """Equal bit for bit (NaN included: the depth off the mask)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def pose_of(name):
    return AWAY_POSE if name == AWAY else T.pose(name)


@pytest.fixture(autouse=True)
def away_view(monkeypatch):
    """The view without a hit: the rays of the pose AWAY_POSE are the rehearsed away rays, for render_surface and
    render_surfaces alike (both take their rays from trace._view_rays_camera)."""
    from oi_amd import trace
    real = trace._view_rays_camera

    def rays(gen, b2w):
        out = real(gen, b2w)
        if b2w is not AWAY_POSE:
            return out
        n = out[0].shape[0]
        o, d, near, far = (torch.from_numpy(np.resize(x, (n,) + x.shape[1:])).float().cuda().contiguous() for x in B.away_rays(130))
        return (o, d, near, far) + tuple(out[4:])

    monkeypatch.setattr(trace, "_view_rays_camera", rays)


def local_lights():
    from oi_amd.relight import LocalLight
    return [LocalLight(position=(0.3, -1.2, -1.4), specular=0.35, shininess=6.0),                       # a point light
            LocalLight(position=(-0.9, -0.4, -1.0), radius=0.2, reference_distance=1.5, specular=0.35, shininess=6.0)]


def config(name):
    """render_surface's keywords of the three cases."""
    if name == "hard":
        return dict(lights=G.lights()[:NL], shadows=True)
    if name == "soft":
        return dict(lights=G.lights()[:NL], shadows=True, shadow_samples=S, light_radius=RADIUS, ao_samples=NA, ao_distance=AO_DISTANCE,
                    seed=SEED)
    return dict(lights=local_lights(), shadows=True, shadow_samples=S, seed=SEED)


def latents(views):
    return [A.latent(s)[0] for s, _ in views]


def reference(precision, name, view):
    """render_surface of one view under a configuration; computed once, never modified."""
    key = (precision, name, view)
    if key not in _REF:
        from oi_amd import trace
        seed, pose = view
        _REF[key] = trace.render_surface(G.make_gen(precision), A.latent(seed)[0], pose_of(pose), **config(name))
    return _REF[key]


def batched(precision, name, views, **kw):
    from oi_amd import trace
    return trace.render_surfaces(G.make_gen(precision), latents(views), [pose_of(p) for _, p in views], **config(name), **kw)


def same_maps(out, ref, what):
    for k in MAPS:
        assert (k in out) == (k in ref), (what, k)
        if k in ref:
            assert biteq(out[k], ref[k]), (what, k, float((out[k] - ref[k]).nan_to_num().abs().max()))


def primary(precision, views=VIEWS4):
    """The batched primary trace and the full pass of `views`, as render_surfaces runs them: what the begin entries read.
    Computed once, never modified."""
    key = (precision, views)
    if key not in _PRIMARY:
        from oi_amd import ops, trace
        from oi_amd.fields import LatentField
        gen = G.make_gen(precision)
        zs = trace._latents(latents(views), gen.it.device)
        field = LatentField(gen, zs, None, "test", batch_ok=True)
        gen.eval()
        field.prepare(zs, None)
        rays = [trace._view_rays(gen, pose_of(p)) for _, p in views]
        ro, rd, near, far = (torch.stack([v[i] for v in rays]) for i in range(4))
        st = ops.TraceBatchState(len(views), ro.shape[1], ro, rd, near, far)
        kw, bias = trace._Surface.params(trace.DEFAULT_BIAS, {})
        res = trace._trace_batch(field, st, *kw)
        _, grad, rgb = field.full(res.hit_points_padded.view(-1, 3))
        E, n_pad = len(views), res.n_pad
        _PRIMARY[key] = dict(gen=gen, field=field, st=st, res=res, grad=grad.view(E, n_pad, 3), rgb=rgb.view(E, n_pad, 3), kw=kw,
                             bias=bias, w2b=torch.stack([v[4] for v in rays]).contiguous(), E=E, N=st.N, n_pad=n_pad)
    return _PRIMARY[key]


def test_the_views_are_ragged():
    p = primary("f32")
    n = p["res"].n_hit
    assert len(set(n[:3])) > 1 and n[3] == 0 and min(n[:3]) > 0 and p["n_pad"] == max(n)          # the hit counts differ: padding slots
    assert bool((p["res"][3].status == T.MISS).all())


# ---------------------------------------------------------------------------------------------------------------------
# rays: oi_occlusion_batch_begin against the single-view begin entries
# ---------------------------------------------------------------------------------------------------------------------
def _single_begin(mode, p, e, lt, radius, samples):
    from oi_amd import lib, ops
    n = p["res"].n_hit[e]
    L = 1 if mode == lib.OCCLUSION_BATCH_HEMISPHERE else lt.shape[0]
    st = ops.TraceState(L * samples * n, ref=p["st"].t)
    hp, grad, hi, w2b = p["res"].hit_points_padded[e, :n], p["grad"][e, :n], p["res"].hit_index[e, :n], p["w2b"][e]
    if mode == lib.OCCLUSION_BATCH_SHADOW:
        ops.trace_shadow_begin(st, hp, grad, n, lt, w2b, p["bias"])
    elif mode == lib.OCCLUSION_BATCH_CAP:
        ops.occlusion_light_begin(st, hp, grad, hi, n, lt, radius, samples, w2b, p["bias"], SEED)
    elif mode == lib.OCCLUSION_BATCH_HEMISPHERE:
        ops.occlusion_ambient_begin(st, hp, grad, hi, n, samples, p["bias"], AO_DISTANCE, SEED)
    else:
        ops.local_light_begin(st, hp, grad, hi, n, lt, samples, w2b, p["bias"], SEED)
    return st


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode", ["SHADOW", "CAP", "HEMISPHERE", "LOCAL"])
def test_begin_rays_are_the_single_view_entries(precision, mode):
    from oi_amd import lib, ops, trace
    p = primary(precision)
    code = getattr(lib, "OCCLUSION_BATCH_" + mode)
    dev = p["st"].t.device
    lt = trace._stack_lights(p["gen"], local_lights() if mode == "LOCAL" else G.lights()[:NL], dev, "test")
    radius = torch.full((NL,), RADIUS, device=dev) if mode == "CAP" else None
    samples = {"SHADOW": 1, "CAP": S, "HEMISPHERE": NA, "LOCAL": S}[mode]
    L, Sc = (1 if mode == "HEMISPHERE" else NL), (1 if mode == "SHADOW" else 2)
    E, n_pad, res = p["E"], p["n_pad"], p["res"]
    single = [_single_begin(code, p, e, lt, radius, samples) if res.n_hit[e] else None for e in range(E)]
    statuses = set()
    for j0 in range(0, samples, Sc):
        c = min(Sc, samples - j0)
        sb = ops.trace_batch_state_empty(E, L * c * n_pad, p["st"].t)
        ops.occlusion_batch_begin(sb, code, guarded_copy(res.hit_points_padded, "hit_points"), guarded_copy(p["grad"], "grad"),
                                  guarded_copy(res.hit_index, "hit_index"), guarded_copy(p["st"].counts, "counts"), n_pad, samples, j0, c,
                                  p["bias"], SEED, lights=None if mode == "HEMISPHERE" else lt, radius=radius,
                                  w2b=None if mode == "HEMISPHERE" else p["w2b"], distance=AO_DISTANCE if mode == "HEMISPHERE" else None)
        counts0, live0 = sb.counts[:, 0].tolist(), int(sb.live[0])
        assert live0 == max(counts0)
        for e in range(E):
            n = res.n_hit[e]
            v = lambda x, *tail: x[e].view(L, c, n_pad, *tail)
            status = v(sb.status)
            # the slots behind the view's hits: ended rays, MISS, never entered
            assert bool((status[:, :, n:] == T.MISS).all())
            assert not bool(v(sb.rays_o, 3)[:, :, n:].any()) and not bool(v(sb.far)[:, :, n:].any())
            entered = sb.active[e, 0, :counts0[e]].long()
            assert bool(((entered % n_pad) < n).all())
            marching = torch.nonzero(sb.status[e] == lib.TRACE_MARCH).view(-1)
            assert torch.equal(torch.sort(entered).values, marching) and counts0[e] == marching.numel()
            if n == 0:
                assert counts0[e] == 0
                continue
            ref = single[e]
            w = lambda x, *tail: x.view(L, samples, n, *tail)[:, j0:j0 + c]
            for what, got, want in (("origins", v(sb.rays_o, 3)[:, :, :n], w(ref.rays_o, 3)), ("directions", v(sb.rays_d, 3)[:, :, :n], w(ref.rays_d, 3)),
                                    ("far", v(sb.far)[:, :, :n], w(ref.far)), ("status", status[:, :, :n].float(), w(ref.status).float())):
                bad = got != want
                print(f"rays[{precision},{mode},view {e},j0={j0}] {what}: {int(bad.sum())} of {bad.numel()} elements differ, max |difference| "
                      f"{float((got - want).abs().nan_to_num().max()):.3e}, NaN {int(got.isnan().sum())}/{int(want.isnan().sum())}")
            assert torch.equal(v(sb.rays_o, 3)[:, :, :n], w(ref.rays_o, 3)), (mode, e, j0, "origins")
            assert torch.equal(v(sb.rays_d, 3)[:, :, :n], w(ref.rays_d, 3)), (mode, e, j0, "directions")
            assert torch.equal(v(sb.near)[:, :, :n], w(ref.near)) and torch.equal(v(sb.far)[:, :, :n], w(ref.far)), (mode, e, j0)
            assert torch.equal(status[:, :, :n], w(ref.status)), (mode, e, j0, "status")
            assert torch.equal(v(sb.t)[:, :, :n], w(ref.t))
            statuses |= set(status[:, :, :n].unique().tolist())
    assert lib.TRACE_MARCH in statuses and (mode not in ("SHADOW", "CAP") or lib.TRACE_BACKFACING in statuses)


# ---------------------------------------------------------------------------------------------------------------------
# states: the marched chunks against render_surface's shadow_trace / ao_trace
# ---------------------------------------------------------------------------------------------------------------------
def _recorded_chains(monkeypatch):
    """Every state oi_trace_batch_finish sees, in order: the primary batch, then the finished chunks of secondary rays.  The
    first entry is (the primary state, its hit_index (E, N)): the run's own hit order, which the compaction does not fix."""
    from oi_amd import ops
    seen, real = [], ops.trace_batch_finish

    def finish(st):
        out = real(st)
        seen.append(st if seen else (st, out[0]))
        return out

    monkeypatch.setattr(ops, "trace_batch_finish", finish)
    return seen


def _same_states(sb, e_local, e, hit_index, n, n_pad, ref_state, ref_trace, L, samples, j0, c):
    """Chunk [j0, j0 + c) of view e in the batch state sb against the single-view state of render_surface, whose own primary
    trace lists the hits in its own order: slot i of the batch is the slot of pixel hit_index[e][i] there."""
    assert n == ref_trace.hit_index.shape[0]
    perm = ref_trace.hit_slot[hit_index[e, :n].long()].long()
    assert int(perm.min()) >= 0
    for name in ("t", "status", "steps"):
        got = getattr(sb, name)[e_local].view(L, c, n_pad)[:, :, :n]
        want = getattr(ref_state, name).view(L, samples, n)[:, j0:j0 + c][:, :, perm]
        assert torch.equal(got, want), (name, e, j0)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("readback", [1, 16])
@pytest.mark.parametrize("name", ["hard", "soft", "local"])
def test_marched_states_are_the_single_view_states(precision, name, readback, monkeypatch):
    from oi_amd import trace
    p = primary(precision)
    E, n_pad = p["E"], p["n_pad"]
    samples = 1 if name == "hard" else S
    cap = E * NL * min(2, samples) * n_pad                                  # Sc = 2 for the shadow samples: chunks [0, 2) and [2, 3)
    seen = _recorded_chains(monkeypatch)
    outs = batched(precision, name, VIEWS4, batch_secondary=True, max_secondary_rays=cap, readback=readback)
    stages = [("shadow_trace", NL, samples)] + ([("ao_trace", 1, NA)] if name == "soft" else [])
    (first, hit_index), chains = seen[0], seen[1:]
    n_hit = first.counts[:, -1].tolist()
    assert n_hit == list(p["res"].n_hit)
    k = 0
    for key, L, n_samples in stages:
        groups, chunks = trace.plan_secondary(E, L, n_samples, n_pad, cap)
        assert groups == [(0, E)] and (key != "shadow_trace" or chunks == ([(0, 1)] if name == "hard" else [(0, 2), (2, 1)]))
        for j0, c in chunks:
            sb = chains[k]
            k += 1
            assert sb.N == L * c * n_pad and sb.E == E
            for e in range(3):
                ref = reference(precision, name, VIEWS4[e])
                _same_states(sb, e, e, hit_index, n_hit[e], n_pad, ref[key], ref["trace"], L, n_samples, j0, c)
            assert bool((sb.status[3] == T.MISS).all()) and not bool(sb.steps[3].any())        # the view without a hit: never marched
    assert k == len(chains)
    for e in range(4):
        assert outs[e]["shadow_trace"] is None and outs[e]["stats"]["secondary_batched"] is True
        same_maps(outs[e], reference(precision, name, VIEWS4[e]), (name, e, readback))


# ---------------------------------------------------------------------------------------------------------------------
# maps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["hard", "soft", "local"])
def test_maps_are_render_surface_bit_for_bit(precision, name):
    outs = batched(precision, name, VIEWS4, batch_secondary=True)
    loop = batched(precision, name, VIEWS4, batch_secondary=False)
    assert len(outs) == len(loop) == 4
    for e, view in enumerate(VIEWS4):
        ref = reference(precision, name, view)
        assert list(outs[e]) == list(loop[e]) == list(ref), (list(outs[e]), list(ref))               # the keys and their order
        same_maps(outs[e], ref, (name, e))
        same_maps(outs[e], loop[e], (name, e, "loop"))
        assert set(outs[e]["stats"]) == set(loop[e]["stats"]) | {"secondary_batched"}
        for k in loop[e]["stats"]:
            if k not in ("shadow_evals", "ao_evals"):
                assert outs[e]["stats"][k] == loop[e]["stats"][k], k
        assert outs[e]["shadow_trace"] is None and ("ao_trace" not in ref or outs[e]["ao_trace"] is None)
        assert torch.equal(outs[e]["trace"].t, ref["trace"].t)
        assert "secondary_batched" not in loop[e]["stats"]
    assert bool((outs[3]["visibility"] == 1).all()) and not bool(outs[3]["mask"].any())
    assert min(float(o["visibility"].min()) for o in outs[:3]) < 0.5                                 # something is in shadow
    if name != "hard":
        vis = torch.cat([o["visibility"].view(-1) for o in outs[:3]])
        assert bool(((vis > 0) & (vis < 1)).any())                                                    # a penumbra


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["hard", "soft", "local"])
def test_one_view_and_views_without_a_hit(precision, name, monkeypatch):
    one = batched(precision, name, B.BATCH_VIEWS[1:2], batch_secondary=True)
    assert len(one) == 1
    same_maps(one[0], reference(precision, name, B.BATCH_VIEWS[1]), (name, "E=1"))
    # no view has a hit: n_pad == 0, no secondary ray is launched, the visibility is all ones
    from oi_amd import ops
    for op in ("occlusion_batch_begin", "occlusion_batch_resolve", "trace_batch_state_empty"):
        monkeypatch.setattr(ops, op, lambda *a, **k: pytest.fail("a launch of secondary rays without a hit"))
    away = ((0, AWAY), (1, AWAY))
    none = batched(precision, name, away, batch_secondary=True, bg=(0.25, 0.5, 0.75))
    loop = batched(precision, name, away, bg=(0.25, 0.5, 0.75))
    for e in range(2):
        same_maps(none[e], loop[e], (name, "no hit", e))
        assert bool((none[e]["visibility"] == 1).all()) and none[e]["stats"]["hit"] == 0 and none[e]["stats"]["shadow_evals"] == 0
        assert name != "soft" or bool((none[e]["ambient_occlusion"] == 1).all())
        assert torch.equal(none[e]["image"], torch.tensor((0.25, 0.5, 0.75)).cuda()[None, :, None, None].expand_as(none[e]["image"]))


# ---------------------------------------------------------------------------------------------------------------------
# a split trace equals the unsplit one
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["soft", "local"])
def test_split_equals_unsplit(precision, name, monkeypatch):
    from oi_amd import trace
    n_pad = primary(precision)["n_pad"]
    whole = batched(precision, name, VIEWS4, batch_secondary=True)
    again = batched(precision, name, VIEWS4, batch_secondary=True)
    caps = {"one sample per chunk": 4 * NL * n_pad, "groups of two views": 2 * NL * n_pad, "groups of one view": NL * n_pad}
    assert trace.plan_secondary(4, NL, S, n_pad, caps["one sample per chunk"]) == ([(0, 4)], [(0, 1), (1, 1), (2, 1)])
    assert trace.plan_secondary(4, NL, S, n_pad, caps["groups of two views"])[0] == [(0, 2), (2, 4)]
    assert trace.plan_secondary(4, NL, S, n_pad, caps["groups of one view"])[0] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    runs = {"again": again}
    for what, cap in caps.items():
        runs[what] = batched(precision, name, VIEWS4, batch_secondary=True, max_secondary_rays=cap)
    for what, outs in runs.items():
        for e in range(4):
            for k in ("visibility", "ambient_occlusion", "image"):
                if k in whole[e]:
                    assert torch.equal(outs[e][k], whole[e][k]), (what, e, k)
    with pytest.raises(ValueError, match=rf"1 view x {NL} lights x {n_pad} hit slots = L \* n_pad = {NL * n_pad} rays per sample"):
        seen = _recorded_chains(monkeypatch)
        try:
            batched(precision, name, VIEWS4, batch_secondary=True, max_secondary_rays=NL * n_pad - 1)
        finally:
            assert len(seen) == 1                                            # the primary batch alone: no secondary chain began


# ---------------------------------------------------------------------------------------------------------------------
# one chain: what is launched
# ---------------------------------------------------------------------------------------------------------------------
def _logged(monkeypatch):
    """The names of the watched oi_amd.ops wrappers and of the library's MLP entries, in call order."""
    from oi_amd import lib, ops
    log, L = [], lib.load()

    def wrap(owner, name):
        real = getattr(owner, name)

        def call(*a, **k):
            log.append(name)
            return real(*a, **k)

        monkeypatch.setattr(owner, name, call)

    for name in SINGLE_OPS + BATCH_OPS + OTHER_OPS:
        wrap(ops, name)
    for name in MLP_ENTRIES:                      # the march calls the C entries directly (oi_amd.trace._march)
        wrap(L, name)
    return log


def _per_view_loop(precision, name, views):
    """The light-dependent stages as the per-view path runs them: render_surfaces' loop over the elements of the batch,
    restated on the package's own per-view parts (the code path of a call without the keyword)."""
    from oi_amd import ops, trace
    from oi_amd.fields import LatentField
    gen, cfg, dev = G.make_gen(precision), config(name), "cuda"
    kw, bias = trace._Surface.params(trace.DEFAULT_BIAS, {"max_steps": MAX_STEPS})
    zs = trace._latents(latents(views), gen.it.device)
    lt = trace._stack_lights(gen, cfg["lights"], gen.it.device, "render_surfaces")
    radii = trace._check_occlusion(True, cfg.get("shadow_samples", 1), cfg.get("light_radius", 0.0), cfg.get("ao_samples", 0),
                                   cfg.get("ao_distance", 0.5), cfg.get("seed", 0), lt.shape[0], "render_surfaces", trace._is_local(lt))
    field = LatentField(gen, zs, None, "render_surfaces", batch_ok=True)
    gen.eval()
    field.prepare(zs, None)
    rays = [trace._view_rays(gen, pose_of(p)) for _, p in views]
    ro, rd, near, far = (torch.stack([v[i] for v in rays]) for i in range(4))
    E = len(views)
    st = ops.TraceBatchState(E, ro.shape[1], ro, rd, near, far)
    res = trace._trace_batch(field, st, *kw)
    _, grad, rgb = field.full(res.hit_points_padded.view(E * res.n_pad, 3))
    grad, rgb = grad.view(E, res.n_pad, 3), rgb.view(E, res.n_pad, 3)
    out = []
    for e in range(E):
        one = copy.copy(field)
        one.B, one.gamma, one.beta = 1, field.gamma[e:e + 1], field.beta[e:e + 1]
        n = res.n_hit[e]
        s = trace._Surface.from_batch(one, kw, bias, st.rays_o[e], st.rays_d[e], rays[e][4], gen.resolution, res[e],
                                      grad[e, :n] if n else None, rgb[e, :n] if n else None)
        out.append(trace._lit(s, lt, radii, True, cfg.get("shadow_samples", 1), cfg.get("ao_samples", 0), cfg.get("ao_distance", 0.5),
                              cfg.get("seed", 0), None, gen.it.device))
    return out


MAX_STEPS = 32


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["hard", "soft", "local"])
def test_one_chain_per_stage(precision, name, monkeypatch):
    log = _logged(monkeypatch)
    per_chunk = {}
    for views in (VIEWS4, B.BATCH_VIEWS[1:2]):
        del log[:]
        batched(precision, name, views, batch_secondary=True, max_steps=MAX_STEPS)
        calls = list(log)
        assert not set(calls) & set(SINGLE_OPS), set(calls) & set(SINGLE_OPS)                   # no single-view begin, resolve or shade
        assert calls.count("surface_shade_batch") == 1 and calls[-1] == "surface_shade_batch"
        n_stages = 2 if name == "soft" else 1
        assert calls.count("occlusion_batch_begin") == calls.count("occlusion_batch_resolve") == n_stages      # one chunk each
        assert calls.count("trace_batch_finish") == 1 + n_stages and "oi_sdf_mlp_fwd" in calls                    # (the full pass)
        chunks, at = [], None
        for c in calls:
            if c == "occlusion_batch_begin":
                at = 0
            elif c == "oi_sdf_mlp_fwd_segments" and at is not None:
                at += 1
            elif c == "occlusion_batch_resolve":
                chunks.append(at)
                at = None
        assert len(chunks) == n_stages and all(1 <= n <= MAX_STEPS for n in chunks), chunks
        per_chunk[len(views)] = chunks
    print(f"one_chain[{precision},{name}] sdf passes per chunk: E=4 {per_chunk[4]}, E=1 {per_chunk[1]} (at most max_steps={MAX_STEPS})")
    # with the keyword off: the call list of the per-view code path, and nothing of the new entries
    del log[:]
    off = batched(precision, name, VIEWS4, max_steps=MAX_STEPS)
    calls_off = list(log)
    del log[:]
    loop = _per_view_loop(precision, name, VIEWS4)
    assert calls_off == list(log) and not set(calls_off) & set(BATCH_OPS)
    assert sum(c in SINGLE_OPS for c in calls_off) > 0
    for e in range(4):
        same_maps(off[e], loop[e], (name, e, "off"))


# ---------------------------------------------------------------------------------------------------------------------
# work
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["hard", "soft"])
def test_work_of_the_shared_chain(precision, name, monkeypatch):
    """With a count read every step the chain evaluates E * sum_k live[k] points: the bound of step k is live[k], the largest
    number of rays any view still has in flight.  The ratio to the per-view chains' evaluations is recorded, not bounded: it
    is the padding the views with fewer rays in flight ride along with."""
    seen = _recorded_chains(monkeypatch)
    outs = batched(precision, name, VIEWS4, batch_secondary=True, readback=1)
    chains = seen[1:]
    assert len(chains) == (2 if name == "soft" else 1)
    for key, sb in zip(("shadow_evals", "ao_evals"), chains):
        live = sb.live.cpu().numpy()
        per_view = int(live[:T.MAX_STEPS].sum())
        assert per_view > 0 and all(o["stats"][key] == per_view for o in outs), key
        chain = 4 * per_view
        loop = sum(reference(precision, name, v)["stats"][key] for v in VIEWS4)
        assert loop > 0
        print(f"work[{precision},{name}] {key}: the shared chain {chain} sdf evaluations = 4 x sum_k live[k], the per-view chains {loop}, "
              f"ratio {chain / loop:.3f}")
        record_margin(f"occlusion_batch_work[{precision},{name}]", key + "_over_loop", chain / loop)


# ---------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_surface_frames_batched_secondary_equals_the_loop(precision):
    from oi_amd import inference
    gen = G.make_gen(precision)
    zs = [A.latent(s)[0] for s, _ in B.FRAME_VIEWS]
    b2ws = [T.pose(p) for _, p in B.FRAME_VIEWS]
    keys = ("image", "visibility", "ambient_occlusion")
    kw = dict(keys=keys, shadows=True, shadow_samples=S, light_radius=RADIUS, ao_samples=NA)
    loop = inference.surface_frames(gen, zs, b2ws, batch=1, **kw)
    frames = inference.surface_frames(gen, zs, b2ws, batch=3, batch_secondary=True, **kw)        # a group of 3 and a group of 2
    for k in keys:
        assert frames[k].shape[0] == 5 and biteq(frames[k], loop[k]), k
    assert bool(((frames["visibility"] > 0) & (frames["visibility"] < 1)).any())
