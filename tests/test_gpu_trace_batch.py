"""Batched sphere tracing on the MI355X (include/oi_trace_batch.h; oi_amd.trace.sphere_trace_batch / render_surfaces;
oi_amd.inference.surface_frames(batch=E)).  The reference of every per-ray result is the library's own single-latent trace
(oi_amd.trace.sphere_trace / render_surface, tested against the fp64 oracle by tests/test_gpu_trace.py) on each element
alone, bit for bit: per-ray results depend neither on the slot nor on the bound, and the sdf-only
pass's arithmetic per point does not depend on blockIdx.y.  The cost is stated on the fp64 oracle's tracer through the
rehearsal of tests/helpers/trace_batch_ref.py (tests/test_trace_batch_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_trace as G
from helpers import mesh_attr_ref as A
from helpers import trace_batch_ref as B
from helpers import trace_ref as T
from helpers.guarded import POISON_WORD, guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)
from test_trace_batch_cpu import invalid_argument_cases

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS = G.PRECISIONS
_RAYS, _SINGLE = {}, {}


def biteq(a, b):
    """Equal bit for bit (NaN included: the depth off the mask)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def view_rays(precision, views=B.BATCH_VIEWS):
    """The library's rays of the views, stacked (E, N, ...), and the latents (E, 64); computed once, never modified."""
    key = (precision, views)
    if key not in _RAYS:
        from oi_amd import trace
        gen = G.make_gen(precision)
        r = [trace._view_rays(gen, T.pose(p)) for _, p in views]
        _RAYS[key] = tuple(torch.stack([v[i] for v in r]).contiguous() for i in range(4)) + (B.latents(views).cuda(),)
    return _RAYS[key]


def singles(precision):
    """sphere_trace on each element of the batch alone: the reference, computed once."""
    if precision not in _SINGLE:
        from oi_amd import trace
        ro, rd, near, far, z = view_rays(precision)
        gen = G.make_gen(precision)
        _SINGLE[precision] = [trace.sphere_trace(gen, ro[e], rd[e], near[e], far[e], z=z[e:e + 1]) for e in range(len(z))]
    return _SINGLE[precision]


def same_rays(one, ref):
    """One element of a batch against the single trace of that element: per ray bit-equal, the hit lists as sets."""
    assert torch.equal(one.t, ref.t) and torch.equal(one.status, ref.status) and torch.equal(one.steps, ref.steps)
    a, b = one.hit_index.long(), ref.hit_index.long()
    assert len(a) == len(b)
    pa, pb = torch.argsort(a), torch.argsort(b)
    assert torch.equal(a[pa], b[pb])
    assert torch.equal(one.hit_points[pa], ref.hit_points[pb])
    # hit_slot: the ray's position in the element's own hit_index, or -1
    assert torch.equal(one.hit_slot >= 0, ref.hit_slot >= 0)
    assert torch.equal(a[one.hit_slot[a].long()], a) and torch.equal(one.hit_slot[a].long(), torch.arange(len(a), device=a.device))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_batched_equals_single_bit_for_bit(precision):
    from oi_amd import trace
    ro, rd, near, far, z = view_rays(precision)
    gen = G.make_gen(precision)
    res = trace.sphere_trace_batch(gen, guarded_copy(ro, "rays_o"), guarded_copy(rd, "rays_d"), near, far, z=z)
    ref = singles(precision)
    assert len(res) == 3 and res.n_pad == max(res.n_hit) == max(len(r.hit_index) for r in ref)
    for e in range(3):
        same_rays(res[e], ref[e])
        assert res[e].hit_slot.shape == (T.R_VIEW ** 2,) and res.n_hit[e] == len(ref[e].hit_index) > 0
        pad = res.hit_points_padded[e, res.n_hit[e]:]
        assert not bool(pad.any())                                   # the padding: the coordinate origin
        assert torch.equal(res.counts[e, -1].cpu(), torch.tensor(res.n_hit[e], dtype=torch.int32))
    counts = res.counts.cpu().numpy()
    assert np.array_equal(res.live.cpu().numpy(), counts.max(0))      # live[k] = max_e counts[e][k], the hit word included
    assert np.array_equal(counts[:, 0], [T.R_VIEW ** 2] * 3)
    assert res.n_evals == 3 * res[0].n_evals and res.n_steps == res[0].n_steps <= T.MAX_STEPS
    for e in range(3):                                                # counts[e][k] = the element's rays that took more than k steps
        steps = res[e].steps.cpu().numpy()
        assert counts[e, :res.n_steps].tolist() == [int((steps > k).sum()) for k in range(res.n_steps)]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_stale_bound_changes_the_cost_and_not_the_rays(precision):
    from oi_amd import trace
    ro, rd, near, far, z = view_rays(precision)
    gen = G.make_gen(precision)
    every = trace.sphere_trace_batch(gen, ro, rd, near, far, z=z, readback=1)
    stale = trace.sphere_trace_batch(gen, ro, rd, near, far, z=z, readback=16)
    ref = singles(precision)
    for e in range(3):
        same_rays(every[e], ref[e])
        same_rays(stale[e], ref[e])
    live = every.live.cpu().numpy()
    assert every.n_evals == 3 * int(live[:every.n_steps].sum()) < stale.n_evals
    print("n_evals: read every step", every.n_evals, "every 16th", stale.n_evals)


def _bundle(n, seed):
    ro, rd = G._bundle(n, seed)
    near, far = T.O.near_far_from_sphere(ro, rd)
    return ro, rd, near.reshape(-1), far.reshape(-1)


def _away(n):
    return tuple(torch.from_numpy(x).float().cuda() for x in B.away_rays(n))


def _stack(bundles):
    return tuple(torch.stack([b[i] for b in bundles]).contiguous() for i in range(4))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N,E", [(130, 2), (1, 3), (65, 1)])
def test_ragged_and_limit_shapes(precision, N, E):
    """N = 130: the stride is no multiple of the 128-point tile and the last tile has 2 points; N = 1; E = 1."""
    from oi_amd import trace
    gen = G.make_gen(precision)
    z = B.latents()[:E].cuda()
    bundles = [_bundle(N, 10 * N + e) for e in range(E)]
    ro, rd, near, far = _stack(bundles)
    res = trace.sphere_trace_batch(gen, guarded_copy(ro, "rays_o"), guarded_copy(rd, "rays_d"), near, far, z=z)
    assert len(res) == E
    for e in range(E):
        same_rays(res[e], trace.sphere_trace(gen, *bundles[e], z=z[e:e + 1]))
        assert res[e].t.shape == (N,) and res[e].hit_points.shape == (res.n_hit[e], 3)
    one = trace.sphere_trace_batch(gen, ro, rd, near, far, z=z, max_steps=1)
    assert one.n_steps == 1 and one.n_evals == E * N
    for e in range(E):
        assert set(np.unique(one[e].status.cpu().numpy())) <= {T.LIMIT, T.HIT} and int(one[e].steps.max()) == 1
    empty = trace.sphere_trace_batch(gen, ro[:, :0], rd[:, :0], z=z)
    assert len(empty) == E and empty.n_evals == 0 and empty[0].t.shape == (0,) and empty.n_pad == 0


def _shade_off(res_e, ro, rd, bg):
    """oi_surface_shade on an element without a hit: mask and image."""
    from oi_amd import ops
    lt = torch.tensor([T.light_block(T.LIGHT_DIRS[0])]).cuda()
    return ops.surface_shade(ro, rd, res_e.t, res_e.status, res_e.hit_slot, ro, ro, ro, 0, torch.eye(4).cuda(), lt,
                             torch.tensor(bg).cuda(), outputs=("mask", "depth", "albedo", "image"))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_element_that_ends_at_once_and_a_batch_without_a_hit(precision):
    from oi_amd import trace
    gen = G.make_gen(precision)
    N = 130
    z = B.latents().cuda()
    b0, b2, away = _bundle(N, 21), _bundle(N, 23), _away(N)
    ro, rd, near, far = _stack([b0, away, b2])
    res = trace.sphere_trace_batch(gen, ro, rd, near, far, z=z, readback=1)
    counts = res.counts.cpu().numpy()
    # the away element: every ray misses on its first sample (rehearsed on the oracle), so its count is 0 from step 1 on
    assert counts[1, 0] == N and not counts[1, 1:].any() and counts[0, 1] > 0 and counts[2, 1] > 0 and res.n_steps > 1
    assert bool((res[1].status == T.MISS).all()) and bool((res[1].steps == 1).all())
    assert res.n_hit[1] == 0 and res[1].hit_index.shape == (0,) and bool((res[1].hit_slot == -1).all())
    assert not bool(res.hit_points_padded[1].any()) and res.n_pad == max(res.n_hit) > 0
    bg = (0.25, 0.5, 0.75)
    maps = _shade_off(res[1], ro[1], rd[1], bg)
    assert not bool(maps["mask"].any()) and bool(torch.isnan(maps["depth"]).all()) and not bool(maps["albedo"].any())
    assert torch.equal(maps["image"], torch.tensor(bg).cuda()[None, :, None].expand(1, 3, N))
    # its neighbours are what they are alone
    same_rays(res[0], trace.sphere_trace(gen, *b0, z=z[0:1]))
    same_rays(res[2], trace.sphere_trace(gen, *b2, z=z[2:3]))
    # no element has a hit: n_pad == 0, nothing is gathered, no full pass
    ro, rd, near, far = _stack([away] * 3)
    none = trace.sphere_trace_batch(gen, ro, rd, near, far, z=z)
    assert none.n_pad == 0 and none.n_hit == (0, 0, 0) and none.hit_points_padded.shape == (3, 0, 3) and none.n_steps <= 4
    for e in range(3):
        assert bool((none[e].status == T.MISS).all()) and bool((none[e].hit_slot == -1).all())
        maps = _shade_off(none[e], ro[e], rd[e], bg)
        assert not bool(maps["mask"].any()) and torch.equal(maps["image"], torch.tensor(bg).cuda()[None, :, None].expand(1, 3, N))


MAPS = ("mask", "depth", "position", "normal_object", "normal_map", "albedo", "image", "visibility")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_render_surfaces_against_render_surface(precision):
    """Every map of every view is render_surface's, bit for bit: the trace by test_batched_equals_single, and the full
    kernels' arithmetic per point has no term in the tile position or in B (mlp_fwd3.hip / mlp.hip: a point's row of the
    tile is contracted with the layer's weights and its element's FiLM rows, nothing else)."""
    from oi_amd import trace
    gen = G.make_gen(precision)
    zs = [A.latent(s)[0] for s, _ in B.BATCH_VIEWS]
    outs = trace.render_surfaces(gen, zs, [T.pose(p) for _, p in B.BATCH_VIEWS], lights=G.lights(), shadows=True)
    assert len(outs) == 3
    for (seed, pose), out in zip(B.BATCH_VIEWS, outs):
        ref = G.run_view(precision, seed, pose)["out"]            # render_surface(..., lights=lights(), shadows=True)
        for k in MAPS:
            diff = float((out[k] - ref[k]).nan_to_num().abs().max())
            print(f"render_surfaces[{precision},seed={seed},{pose}] {k}: max |difference| {diff}")
        for k in MAPS:
            assert biteq(out[k], ref[k]), (seed, pose, k)
        assert out["stats"]["hit"] == ref["stats"]["hit"] and out["stats"]["shadow_evals"] == ref["stats"]["shadow_evals"]
        assert torch.equal(out["trace"].t, ref["trace"].t)
    plain = trace.render_surfaces(gen, zs[:2], [T.pose(p) for _, p in B.BATCH_VIEWS[:2]], lights=G.lights())
    assert "visibility" not in plain[0] and biteq(plain[1]["depth"], outs[1]["depth"]) and biteq(plain[1]["albedo"], outs[1]["albedo"])
    assert bool((plain[1]["image"] >= outs[1]["image"]).all())       # a shadow only darkens


@pytest.mark.parametrize("precision", PRECISIONS)
def test_cost_against_the_oracle_tracer(precision):
    """n_evals <= 2 x E * sum_k max_e in_flight_e[k] of the fp64 oracle tracer for the same views (the factor of
    test_gpu_trace.py::test_primary_rays)."""
    from oi_amd import trace
    ro, rd, near, far, z = view_rays(precision)
    res = trace.sphere_trace_batch(G.make_gen(precision), ro, rd, near, far, z=z)
    r = B.rehearse()
    flights = [x[3] for x in r["rays"]]
    fresh = 3 * sum(max((f[k] if k < len(f) else 0) for f in flights) for k in range(T.MAX_STEPS))
    assert fresh == r["fresh_evals"]
    G.record_margin(f"trace_batch_cost[{precision}]", "evals_over_oracle", res.n_evals / fresh)
    print(f"trace_batch_cost[{precision}] n_evals", res.n_evals, "oracle E * sum_k max_e in_flight", fresh, "ratio", res.n_evals / fresh,
          "per ray", res.n_evals / (3 * T.R_VIEW ** 2))
    assert res.n_evals <= 2 * fresh


@pytest.mark.parametrize("precision", PRECISIONS)
def test_surface_frames_batched_equals_the_loop(precision):
    from oi_amd import inference
    gen = G.make_gen(precision)
    zs = [A.latent(s)[0] for s, _ in B.FRAME_VIEWS]
    b2ws = [T.pose(p) for _, p in B.FRAME_VIEWS]
    keys = ("image", "mask", "normal_map", "depth", "albedo")
    loop = inference.surface_frames(gen, zs, b2ws, keys=keys)
    batched = inference.surface_frames(gen, zs, b2ws, keys=keys, batch=3)      # a group of 3 and a group of 2
    whole = inference.surface_frames(gen, zs, b2ws, keys=keys, batch=8)        # one partial group
    for k in keys:
        assert loop[k].shape[0] == 5
        assert biteq(batched[k], loop[k]) and biteq(whole[k], loop[k]), k
    sh = inference.surface_frames(gen, zs[:2], b2ws[:2], keys=("image", "visibility"), shadows=True, batch=2)
    sl = inference.surface_frames(gen, zs[:2], b2ws[:2], keys=("image", "visibility"), shadows=True)
    assert biteq(sh["image"], sl["image"]) and biteq(sh["visibility"], sl["visibility"])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [1, 128, 129, 300])
def test_segmented_mlp_pass_alone(precision, n):
    """B = 3 segments of stride 300: the first n points of each are evaluated as by oi_sdf_mlp_fwd with B = 1, nothing is
    written behind them."""
    from oi_amd import lib, ops
    from oi_amd.fields import LatentField
    gen = G.make_gen(precision)
    z = B.latents().cuda()
    f = LatentField(gen, z, None, "test", batch_ok=True).prepare(z, None)
    Bn, stride = 3, 300
    pts = guarded_copy(0.5 * torch.randn(Bn, stride, 3, generator=torch.Generator().manual_seed(n)).cuda(), "pts")
    sdf = guarded_empty((Bn, stride), what="sdf segments", must_write=False)
    ops.sdf_mlp_fwd_segments(pts, f.packed, f.gamma, f.beta, sdf, Bn, n, f.prec, f.fast)
    poison = sdf.view(torch.int32) == int(POISON_WORD)
    assert not bool(poison[:, :n].any()) and bool(poison[:, n:].all())
    for e in range(Bn):
        ref = ops.sdf_mlp_fwd(pts[e, :n].contiguous(), f.packed, f.gamma[e:e + 1], f.beta[e:e + 1], 1, f.prec, f.fast)[0]
        assert torch.equal(sdf[e, :n], ref), e
    with pytest.raises(lib.OiHipError, match="stride"):
        ops.sdf_mlp_fwd_segments(pts, f.packed, f.gamma, f.beta, sdf, Bn, stride + 1, f.prec, f.fast)


def test_c_abi_rejects_invalid_arguments_and_launches_nothing():
    """The refusals of tests/test_trace_batch_cpu.py on real, poisoned device arrays: each returns a negative status with its
    text, and no array is touched."""
    from oi_amd import lib, ops
    L = lib.load()
    E, N = 3, 5
    g = lambda sh, dt=torch.float32: guarded_empty(sh, dt, what="untouched", must_write=False)
    shapes = dict(rays_o=(E, N, 3), rays_d=(E, N, 3), near_=(E, N), far_=(E, N), t=(E, N), bracket=(E, N, 4), points=(E, N, 3))
    arr = {k: g(sh) for k, sh in shapes.items()}
    arr.update(status=g((E, N), torch.uint8), side=g((E, N), torch.uint8), steps=g((E, N), torch.int16),
               active=g((E, 2, N), torch.int32), counts=g((E, lib.TRACE_COUNT_WORDS), torch.int32))
    other = g((1024 * 8,))                                  # live, sdf, hit lists, the packed image ...: never dereferenced
    p = lambda t_: ctypes.c_void_p(t_.data_ptr())
    cases = invalid_argument_cases(lib, L, p(other), {k: p(v) for k, v in arr.items()})
    wanted = {"stride=8", "E=0", "E=1025", "bound=6", "null pointer"}          # stride < n_per_elem, E, bound > N, a NULL array
    assert wanted <= {text for _, _, text in cases}
    for call, entry, text in cases:
        rc = call()
        msg = L.oi_last_error().decode()
        assert rc < 0 and msg.startswith(entry) and text in msg, (entry, text, rc, msg)
    torch.cuda.synchronize()
    for k, v in list(arr.items()) + [("other", other)]:
        fresh = guarded_empty(tuple(v.shape), v.dtype, what="pattern", must_write=False)
        assert torch.equal(v.view(torch.uint8), fresh.view(torch.uint8)), k                 # still poison: nothing ran
