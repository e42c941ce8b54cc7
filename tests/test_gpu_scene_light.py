"""Soft shadows, ambient occlusion and environment lighting between the instances of a scene on the MI355X
(include/oi_scene_light.h; oi_amd.scene; oi_amd.inference.scene_env_walk / scene_light_walk).

Exact properties are checked bit for bit against the library's own single-instance paths, which tests/test_gpu_occlusion.py
and tests/test_gpu_envlight.py hold against the fp64 oracle: for E = 1 the statuses and evaluation counts against
oi_occlusion_light_begin / oi_occlusion_ambient_begin + the single any-hit march, the any-hit step per element against
oi_occlusion_step on that element's state alone, a split trace against the unsplit one, the default keywords against the
parent's launches.  The layer's own decisions -- the construction of the rays in every element, the cull, the combination
across elements, the accumulation over chunks -- are checked against the float64 restatement of
tests/helpers/scene_light_ref.py, which touches no code under test.

Bars (eps = 2^-24):
  DIRECTIONS    1e-6 against the restatement fed the kernel's own float32 points and gradients: the bar DESIGN section 4.19
                measured for the shared shadow-ray function, for the same reason (the compiler contracts the shared
                __device__ function's sums of products differently per kernel).
  CULL          the entered set of every other element is the restatement's cull of the KERNEL'S OWN float32 ray, except
                where |c2 - 1| <= 4 eps (|o|^2 + 1) (test_gpu_scene.py's edge) or, in the ambient form, |near - distance| <=
                1e-5 (near carries the chord's cancellation, test_gpu_scene.py's 1e-5 / sqrt(1 - c2) capped at the rim).
  COUNTS        exact: integers.
  TRANSFER      per pixel and coefficient c, with n the number of escaped samples and A_c the sum of |y_c| over them:
                  eps ((n + 1) A_c + 16 * 1.1 n) / S
                n rounded additions of partial sums each at most A_c and one division ((n + 1) eps A_c); each term's own
                evaluation -- the rotation into the world (3 products, 2 sums), the normalisation (3 products, 2 sums, a
                square root, 3 divisions) and the basis polynomial (at most 4 roundings) -- is within 16 eps of the largest
                basis value 1.1, the figure tests/test_gpu_envlight.py uses for the same expressions.  The reference is fed
                the kernel's own float32 directions and statuses.
  CLOSED FORM   oi_scene_transfer_normal against env_ref.closed_form of the world normal map: 32 eps, oi_transfer_normal's bar.
  CONSTANT ENV  under EnvLight.constant(1) the shading is L_0 T_0 = (2 sqrt(pi)) (n / S) 0.28209479 against ambient's n / S:
                the float32 L_0, the basis constant, their product with the sum, and the division each round once: 4 eps
                (section 4.18's identity and bar).
  ANALYTIC      two fields |x| - 0.5.  Per ray "escaped every instance" against ray-against-sphere in float64 on the kernel's
                own rays taken to the world, outside the band |closest approach - 0.5| < 1e-3 (scene_ref.AN_SHADOW_EDGE); at
                most 1 % of the rays may lie in the band (occlusion_ref.EXCLUDED_CAP; tests/test_scene_light_cpu.py rehearses
                that on float64 alone).  The transfer vector of every pixel without a ray in the band against the mean of
                basis(d) over the closed form's escaped samples: TRANSFER's bar.  The soft-shadow share: exact."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_scene as GS
import test_gpu_trace as G
import test_scene_light_cpu as C
from conftest import record_margin
from helpers import env_ref as EV
from helpers import occlusion_ref as R
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T
from helpers.guarded import guarded_empty, guarded_ops  # noqa: F401  (fixture)
from test_gpu_trace_batch import biteq

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS, npd = G.PRECISIONS, G.npd
EPS = 2.0 ** -24
SEED = SL.SEED
RADII = {1: [0.1], 2: [0.1, 0.0]}                 # one radius 0 among non-zero ones
INF = float("inf")
GOLDEN_W = 16                                    # window of the golden two-instance scene (test_scene_cpu.GOLDEN_W)
# kind, W, samples, L; every case runs the lights' caps and the hemisphere
CASES = [("pair", 9, 4, 2), ("triple", 12, 4, 1), ("single", 9, 1, 2), ("twice", 12, 4, 1), ("pair", 12, 1, 1)]


def lights_t(L):
    from oi_amd.relight import stack_lights
    return stack_lights(GS.lights(L), "cuda")


def radius_t(L):
    return torch.tensor(RADII[L], dtype=torch.float32, device="cuda")


def cuts_of(S):
    """The splits of S samples the tests run: whole, one sample per chunk, an uneven one."""
    return {1: [[1]], 4: [[4], [1, 1, 1, 1], [1, 3]], 16: [[16], [5, 11]], 64: [[64], [24, 40]]}[S]


def sampled(s, S, cuts, lt=None, radius=None, distance=None, transfer=False, march=None, seed=SEED):
    """The sequence of include/oi_scene_light.h through the ops wrappers, chunk by chunk.  -> dict: chunks (the finished
    batch states), count, out, transfer."""
    from oi_amd import ops, trace
    pos, nrm, elem = s.world_points()
    pixel = s.point_pixels()
    n_vis, L, M = sum(s.n_vis), 1 if lt is None else lt.shape[0], s.S * s.S
    count, out = ops._new(pos, L, M).view(torch.int32), ops._new(pos, L, M)
    tr = ops._new(pos, 9, M) if transfer else None
    chunks, j0 = [], 0
    for c in cuts:
        sb = ops.trace_batch_state_empty(s.E, L * c * n_vis, pos)
        ops.scene_occlusion_begin(sb, s.points, s.grad, s.n_pad, s.offset, elem, pixel, pos, nrm, n_vis, s.w2b, s.bias, S, j0, c, seed,
                                  lt, radius, distance)
        bound = int(sb.live[0].item())
        if bound:
            if march is None:
                trace._march_batch(s.field, sb, *s.kw, bound=bound, anyhit=True)
            else:
                march(sb)
            ops.trace_batch_finish(sb)
        last = j0 + c == S
        ops.scene_occlusion_resolve(sb.status, s.owner, s.owner_ray, s.vis_slot, s.offset, s.E, s.N, L, S, j0, c, n_vis, s.S, count, out,
                                    last)
        if transfer:
            ops.scene_transfer_resolve(sb.status, sb.rays_d, s.owner, s.owner_ray, s.vis_slot, s.offset, s.w2b, s.E, s.N, S, j0, c,
                                       n_vis, s.S, tr, last)
        chunks.append(sb)
        j0 += c
    return dict(chunks=chunks, count=count, out=out, transfer=tr)


def shaped(sb, E, L, c, n):
    return sb.status.cpu().numpy().reshape(E, L, c, n)


def scene_arrays(s):
    return dict(owner=s.owner.cpu().numpy(), owner_ray=s.owner_ray.cpu().numpy(), vis_slot=s.vis_slot.cpu().numpy(),
                offset=s.offset.cpu().numpy(), w2b=npd(s.w2b))


def transfer_bar(status_chunks, mag, a, S):
    """TRANSFER's bar (9, M) of the file's docstring; status_chunks: (E, 1, Sc, n_vis) each."""
    n = np.zeros(len(a["owner"]))
    on, g = SL.pixel_points(a["owner"], a["owner_ray"], a["vis_slot"], a["offset"])
    for st in status_chunks:
        n[on] += SL.escaped(st)[0][:, g].sum(0)
    return EPS * ((n[None] + 1) * mag + 16 * 1.1 * n[None]) / S


# ---------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ambient", [False, True], ids=["lights", "ambient"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W,S,L", CASES)
def test_rays_in_every_element(precision, kind, W, S, L, ambient):
    """One chunk of oi_scene_occlusion_begin (an uneven one where S allows) against the restatement: the owner's directions
    drawn from the kernel's float32 points and gradients, then every element's ray, cull and state from the kernel's own
    directions; the compaction within each element."""
    from oi_amd import lib
    s = GS.traced(precision, kind, W)
    j0, c = (1, 3) if S == 4 else (0, 1)
    distance = 2.0 if kind != "triple" else INF
    Lr = 1 if ambient else L
    kw = dict(distance=distance) if ambient else dict(lt=lights_t(L), radius=radius_t(L))
    from oi_amd import ops
    pos, nrm, elem = s.world_points()
    pixel = s.point_pixels()
    n, E = sum(s.n_vis), s.E
    sb = ops.trace_batch_state_empty(E, Lr * c * n, pos)
    ops.scene_occlusion_begin(sb, s.points, s.grad, s.n_pad, s.offset, elem, pixel, pos, nrm, n, s.w2b, s.bias, S, j0, c, SEED,
                              kw.get("lt"), kw.get("radius"), kw.get("distance"))
    a = scene_arrays(s)
    vis_index = s.vis_index.cpu().numpy()
    window = s.window.cpu().numpy()
    pix_ref = SL.point_pixels(vis_index, window, s.W, s.S, a["offset"], s.n_vis)
    assert np.array_equal(pixel.cpu().numpy(), pix_ref) and pixel.dtype == torch.int32
    on, g = SL.pixel_points(a["owner"], a["owner_ray"], a["vis_slot"], a["offset"])
    assert np.array_equal(pix_ref[g], on)                                # the point of a pixel is keyed by that pixel
    elem_np = elem.cpu().numpy()
    common = (npd(s.points), npd(s.grad), a["offset"], elem_np, pix_ref, npd(pos), npd(nrm), a["w2b"], s.bias, S, j0, c, SEED)
    rkw = dict(distance=distance) if ambient else dict(light_dirs=[l.direction for l in GS.lights(L)], radius=RADII[L])
    drawn = SL.rays(*common, **rkw)
    o, d = npd(sb.rays_o).reshape(E, Lr, c, n, 3), npd(sb.rays_d).reshape(E, Lr, c, n, 3)
    near, far = npd(sb.near).reshape(E, Lr, c, n), npd(sb.far).reshape(E, Lr, c, n)
    status = sb.status.cpu().numpy().reshape(E, Lr, c, n)
    d_own = d[elem_np, :, :, np.arange(n)].transpose(1, 2, 0, 3)          # the owner's element holds the drawn direction
    err = float(np.abs(d_own - drawn["d_owner"]).max())
    record_margin(f"scene_light_directions[{precision},{kind},W={W},S={S},{'ambient' if ambient else 'lights'}]", "error_over_bar", err / 1e-6)
    assert err <= 1e-6
    assert np.abs(np.linalg.norm(d_own, axis=-1) - 1).max() < 1e-6
    if not ambient and L == 2:                                            # radius 0: every sample is the light's direction
        assert np.abs(d_own[1] - d_own[1][:1]).max() == 0
    # every element's ray from the kernel's own directions
    r = SL.rays(*common, d_owner=d_own, **rkw)
    ndd = (SL.unit(npd(s.grad))[elem_np, np.arange(n) - a["offset"][elem_np]][None, None] * d_own).sum(-1)
    sure = np.abs(ndd) > 1e-6                                             # n . d decided in float32 as in float64
    back = status == T.BACKFACING
    assert np.array_equal(back.all(0), back.any(0))                       # facing away: BACKFACING in every element
    assert np.array_equal(back[0][sure], ~r["traced"][sure])
    assert set(np.unique(status)) <= {T.MARCH, T.MISS, T.BACKFACING} and not sb.steps.any()
    edge = np.abs(r["c2"] - 1) <= 4 * EPS * ((r["o"] ** 2).sum(-1) + 1)
    if ambient and np.isfinite(distance):
        edge |= np.abs(r["near"] - distance) <= 1e-5
    cmp_ = sure[None] & ~edge
    entered = status == T.MARCH
    assert np.array_equal(entered[cmp_], (r["status"] == SL.MARCH)[cmp_])
    n_edge = int((edge & sure[None] & ~back).sum())
    assert n_edge <= 0.001 * status.size
    assert float(np.abs(o - r["o"])[cmp_].max()) <= 2e-5                  # origins at |o| up to ~12: 12 ulp(8) / 2 per component
    assert float(np.abs(d - r["d"])[cmp_].max()) <= 1e-6
    both = cmp_ & entered
    tol = 1e-5 / np.sqrt(np.maximum(1 - r["c2"][both], 1e-4))
    assert (np.abs(near[both] - r["near"][both]) <= tol).all() and (np.abs(far[both] - r["far"][both]) <= tol).all()
    assert not near[~entered].any() and not far[~entered].any()
    mine = np.broadcast_to((elem_np[None] == np.arange(E)[:, None])[:, None, None, :], status.shape)
    assert not near[mine].any() and entered[mine & ~back].all()           # the owner's own ray: near 0, always entered
    if E > 1 and kind != "twice":
        assert (entered & ~mine).any() and ((status == T.MISS) & ~mine).any()
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
        expect = npd(sb.rays_o[e])[act] + npd(sb.near[e])[act, None] * npd(sb.rays_d[e])[act]
        assert np.abs(pts[:n_ent] - expect).max(initial=0.0) <= 1e-6 and not pts[n_ent:].any()
    assert live[0] == counts[:, 0].max() and not live[1:].any() and len(live) == lib.TRACE_COUNT_WORDS
    print(f"scene_light rays[{precision},{kind},W={W},S={S},L={Lr},{'ambient' if ambient else 'lights'}] n_vis {n} (mod 256: {n % 256}) "
          f"entered {counts[:, 0].tolist()} of {Lr * c * n} worst direction error {err:.3g} rays on an edge {n_edge}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("W,S,L", [(9, 4, 2), (12, 1, 1)])
def test_one_instance_equals_the_single_view_paths(precision, W, S, L):
    """E = 1: statuses and evaluation counts are oi_occlusion_light_begin's / oi_occlusion_ambient_begin's followed by the
    single any-hit march on the owner's slices with hit_index = pixel; the resolves agree with oi_occlusion_resolve's and
    (to TRANSFER's bar) oi_transfer_resolve's on those states."""
    from oi_amd import ops, trace
    s = GS.traced(precision, "single", W)
    n = s.n_vis[0]
    assert s.E == 1 and n > 0
    pixel = s.point_pixels()
    pts, grad = s.points[0, :n].contiguous(), s.grad[0, :n].contiguous()
    lt, rad = lights_t(L), radius_t(L)
    hit_slot = torch.full((s.S * s.S,), -1, dtype=torch.int32, device="cuda")
    hit_slot[pixel.long()] = torch.arange(n, dtype=torch.int32, device="cuda")

    def single(begin):
        one = ops.TraceState(begin[0] * n, ref=s.points)
        begin[1](one)
        trace._march(s.field, one, int(one.counts[0].item()), *s.kw, anyhit=True)
        ops.trace_finish(one)
        return one

    soft = sampled(s, S, [S], lt=lt, radius=rad)
    one = single((L * S, lambda st: ops.occlusion_light_begin(st, pts, grad, pixel, n, lt, rad, S, s.w2b[0], s.bias, SEED)))
    sb = soft["chunks"][0]
    assert torch.equal(sb.status[0], one.status) and torch.equal(sb.steps[0], one.steps)
    traced_ = one.status != T.BACKFACING
    close = lambda x, y: float((x - y).abs().max()) <= 1e-6
    assert close(sb.rays_o[0], one.rays_o) and close(sb.rays_d[0], one.rays_d) and close(sb.far[0][traced_], one.far[traced_])
    assert biteq(soft["out"], ops.occlusion_resolve(one.status, hit_slot, s.S * s.S, n, L, S))
    amb = sampled(s, S, [S], distance=R.AO_DISTANCE, transfer=True)
    one = single((S, lambda st: ops.occlusion_ambient_begin(st, pts, grad, pixel, n, S, s.bias, R.AO_DISTANCE, SEED)))
    sb = amb["chunks"][0]
    assert torch.equal(sb.status[0], one.status) and torch.equal(sb.steps[0], one.steps)
    assert close(sb.rays_d[0], one.rays_d) and close(sb.far[0], one.far) and int((one.status == T.MISS).sum()) > 0
    assert biteq(amb["out"], ops.occlusion_resolve(one.status, hit_slot, s.S * s.S, n, 1, S))
    ref = ops.transfer_resolve(one.status, one.rays_d, hit_slot, s.S * s.S, n, S, s.w2b[0])
    assert float((amb["transfer"] - ref).abs().max()) <= 2 * (S + 16) * EPS * 1.1      # both within test_gpu_envlight.py's bar


# ---------------------------------------------------------------------------------------------------------------------
# the any-hit step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W", [("pair", 9), ("triple", 12)])
def test_anyhit_step_per_element_is_the_single_step(precision, kind, W):
    """Per element, status / t / steps after the batched any-hit march equal oi_occlusion_step's march on that element's
    state alone (its rays, its counters, its FiLM rows)."""
    from oi_amd import ops, trace
    s = GS.traced(precision, kind, W)
    pos, nrm, elem = s.world_points()
    n, S = sum(s.n_vis), 4
    sb = ops.trace_batch_state_empty(s.E, S * n, pos)
    ops.scene_occlusion_begin(sb, s.points, s.grad, s.n_pad, s.offset, elem, s.point_pixels(), pos, nrm, n, s.w2b, s.bias, S, 0, S, SEED,
                              distance=INF)
    ones = []
    for e in range(s.E):
        one = ops.TraceState(S * n, sb.rays_o[e].clone(), sb.rays_d[e].clone(), sb.near[e].clone(), sb.far[e].clone())
        for k in ("t", "status", "steps", "bracket", "side", "active", "points", "counts"):
            getattr(one, k).copy_(getattr(sb, k)[e])
        ones.append(one)
    trace._march_batch(s.field, sb, *s.kw, bound=int(sb.live[0].item()), anyhit=True)
    seen = set()
    for e, one in enumerate(ones):
        f = copy.copy(s.field)
        f.B, f.gamma, f.beta = 1, s.field.gamma[e:e + 1], s.field.beta[e:e + 1]
        bound = int(one.counts[0].item())
        if bound:
            trace._march(f, one, bound, *s.kw, anyhit=True)
        assert torch.equal(sb.status[e], one.status) and torch.equal(sb.steps[e], one.steps) and torch.equal(sb.t[e], one.t), e
        seen |= set(np.unique(one.status.cpu().numpy()).tolist())
    assert {T.MISS, T.HIT} <= seen and T.REFINE not in seen               # the any-hit form has no refinement


# ---------------------------------------------------------------------------------------------------------------------
# resolves and chunks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W,S,L", CASES)
def test_resolves_and_chunks(precision, kind, W, S, L):
    """Counts exactly and transfer to its bar against the restatement fed the library's own statuses and directions; a split
    trace equals the unsplit one byte for byte in visibility, ambient occlusion and transfer; off-mask values; the closed form."""
    from oi_amd import ops
    s = GS.traced(precision, kind, W)
    a = scene_arrays(s)
    E, n, M = s.E, sum(s.n_vis), s.S * s.S
    off = a["owner"] < 0
    lt, rad = lights_t(L), radius_t(L)
    whole_soft = whole_amb = None
    for cuts in cuts_of(S):
        soft = sampled(s, S, cuts, lt=lt, radius=rad)
        amb = sampled(s, S, cuts, distance=INF, transfer=True)
        count, out = SL.counts([shaped(sb, E, L, c, n) for sb, c in zip(soft["chunks"], cuts)], a["owner"], a["owner_ray"], a["vis_slot"],
                               a["offset"], S)
        assert np.array_equal(soft["count"].cpu().numpy(), count) and np.array_equal(npd(soft["out"]), out)
        st_chunks = [shaped(sb, E, 1, c, n) for sb, c in zip(amb["chunks"], cuts)]
        count, out = SL.counts(st_chunks, a["owner"], a["owner_ray"], a["vis_slot"], a["offset"], S)
        assert np.array_equal(amb["count"].cpu().numpy(), count) and np.array_equal(npd(amb["out"]), out)
        elem_np = s.world_points()[2].cpu().numpy()
        d_chunks = [npd(sb.rays_d).reshape(E, 1, c, n, 3)[elem_np, :, :, np.arange(n)].transpose(1, 2, 0, 3) for sb, c in zip(amb["chunks"], cuts)]
        ref, mag = SL.transfer(list(zip(st_chunks, d_chunks)), a["owner"], a["owner_ray"], a["vis_slot"], a["offset"], a["w2b"], S)
        bar = transfer_bar(st_chunks, mag, a, S)
        err = np.abs(npd(amb["transfer"]) - ref)
        ratio = float((err[bar > 0] / bar[bar > 0]).max())                 # (no escaped sample: the sum and the bar are 0)
        record_margin(f"scene_transfer[{precision},{kind},W={W},S={S},cuts={len(cuts)}]", "error_over_bar", ratio)
        assert (err <= bar).all()
        # off the mask: 1, count 0, nine zeros -- exactly
        assert (npd(soft["out"])[:, off] == 1).all() and (npd(amb["out"])[:, off] == 1).all() and not npd(amb["transfer"])[:, off].any()
        assert not soft["count"].cpu().numpy()[:, off].any()
        if whole_soft is None:
            whole_soft, whole_amb = soft, amb
            print(f"scene_light resolves[{precision},{kind},W={W},S={S},L={L}] worst transfer error / bar {ratio:.3f}; lit share "
                  f"{float(npd(soft['out'])[:, ~off].mean()):.3f}, escaped share {float(npd(amb['out'])[:, ~off].mean()):.3f}")
        else:
            assert biteq(soft["out"], whole_soft["out"]) and torch.equal(soft["count"], whole_soft["count"]), cuts
            assert biteq(amb["out"], whole_amb["out"]) and biteq(amb["transfer"], whole_amb["transfer"]), cuts
    vals = np.unique(npd(whole_soft["out"]))
    assert set(vals) <= {k / S for k in range(S + 1)} | {float(np.float32(k) / np.float32(S)) for k in range(S + 1)}
    # the host layer: the same bytes, whole and split by max_shadow_rays
    vis = s.visibility(lt, RADII[L], S, SEED)
    assert biteq(vis, whole_soft["out"])
    assert biteq(s.ambient(S, INF, SEED), whole_amb["out"].view(-1)) and biteq(s.transfer(S, SEED), whole_amb["transfer"])
    if S > 1:
        limit = E * L * n * (S - 1)                                       # S - 1 samples fit: chunks of S - 1 and 1
        assert biteq(s.visibility(lt, RADII[L], S, SEED, max_shadow_rays=limit), vis)
        assert biteq(s.transfer(S, SEED, max_shadow_rays=E * n), whole_amb["transfer"])
    # the unshadowed closed form
    t0 = s.transfer(0)
    nw = npd(s._shade(None, None, None, ("normal_world",))["normal_world"])
    want = EV.closed_form(nw).T
    assert np.abs(npd(t0)[:, ~off] - want[:, ~off]).max() <= 32 * EPS and not npd(t0)[:, off].any()
    assert biteq(t0, ops.scene_transfer_normal(s.grad, s.n_pad, s.owner, s.owner_ray, s.vis_slot, s.w2b, E, s.N, s.S))


# ---------------------------------------------------------------------------------------------------------------------
# bitwise properties of the host layer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W,L", [("pair", 9, 2), ("triple", 12, 1), ("twice", 12, 1)])
def test_defaults_are_the_parents_launches_and_shade_ao(precision, kind, W, L):
    from oi_amd import ops, trace
    s = GS.traced(precision, kind, W)
    S, M = s.S, s.S * s.S
    bg = (0.25, 0.5, 0.75)
    lt, bgt = lights_t(L), torch.tensor(bg).cuda()
    # the parent's sequence, spelled out: one hard ray per light and point, oi_scene_visibility, oi_scene_shade
    pos, nrm, elem = s.world_points()
    n = sum(s.n_vis)
    sb = ops.trace_batch_state_empty(s.E, L * n, pos)
    ops.scene_shadow_begin(sb, s.points, s.grad, s.n_pad, s.offset, elem, pos, nrm, n, lt, s.w2b, s.bias)
    trace._march_batch(s.field, sb, *s.kw, bound=int(sb.live[0].item()))
    ops.trace_batch_finish(sb)
    vis = ops.scene_visibility(sb.status, s.owner, s.owner_ray, s.vis_slot, s.offset, s.E, s.N, L, n, S)
    args = (s.state, s.W, S, s.owner, s.owner_ray, s.vis_slot, s.points, s.grad, s.rgb, s.n_pad, s.w2b, s.b2w, lt, bgt, vis)
    ref = ops.scene_shade(*args)
    for kw in ({}, dict(shadow_samples=1, light_radius=0.0, ao_samples=0), dict(light_radius=[0.0] * L, seed=5)):
        before = s.occlusion_evals
        out = s.shade(GS.lights(L), shadows=True, bg=bg, **kw)
        assert biteq(out["image"].view(L, 3, M), ref["image"]) and biteq(out["visibility"].view(L, M), vis)
        assert biteq(out["depth"].view(-1), ref["depth"]) and "ambient_occlusion" not in out and s.occlusion_evals == before
        assert s.shadow.N == L * n and torch.equal(s.shadow.status, sb.status) and torch.equal(s.shadow.steps, sb.steps)
    # oi_scene_shade_ao: NULL and an all-ones factor give oi_scene_shade's bytes; a factor scales the ambient term only
    for ao in (None, torch.ones(M, device="cuda")):
        got = ops.scene_shade_ao(*args, ao)
        for k, v in ref.items():
            assert biteq(got[k], v), (k, ao is None)
    half = ops.scene_shade_ao(*args, torch.full((M,), 0.5, device="cuda"))
    zero = ops.scene_shade_ao(*args, torch.zeros(M, device="cuda"))
    on = (s.owner >= 0)[None, None, :].expand(L, 3, M)
    assert bool((half["image"][on] <= ref["image"][on]).all()) and bool((zero["image"][on] <= half["image"][on]).all())
    assert bool((zero["image"][on] < ref["image"][on]).any()) and biteq(zero["image"][~on], ref["image"][~on])
    mid = 0.5 * (zero["image"].double() + ref["image"].double())
    assert float((half["image"].double() - mid)[on].abs().max()) <= 4 * EPS * float(ref["image"][on].abs().max())
    # per element: oi_surface_shade_ao on the owner's slices, bit for bit
    ao = s.ambient(4, 2.0, SEED)
    got = ops.scene_shade_ao(*args, ao)
    owner, owner_ray = s.owner.long(), s.owner_ray.long()
    for e in range(s.E):
        q = torch.nonzero(owner == e).flatten()
        if len(q) == 0:
            continue
        r = owner_ray[q]
        vis_e, ao_e = torch.ones(L, s.N).cuda(), torch.ones(s.N).cuda()
        vis_e[:, r], ao_e[r] = vis[:, q], ao[q]
        one = ops.surface_shade_ao(s.state.rays_o[e], s.state.rays_d[e], s.state.t[e], GS._owner_status(s, e), s.vis_slot[e], s.points[e],
                                   s.grad[e], s.rgb[e], s.n_pad, s.w2b[e], lt, bgt, vis_e, ao_e)
        assert biteq(got["image"][:, :, q], one["image"][:, :, r]), e
    full = s.shade(GS.lights(L), shadows=True, bg=bg, ao_samples=4, ao_distance=2.0, seed=SEED)
    assert biteq(full["image"].view(L, 3, M), got["image"]) and biteq(full["ambient_occlusion"].view(-1), ao)
    assert full["ambient_occlusion"].shape == (1, 1, S, S) and full["stats"][0]["occlusion_evals"] > 0
    if kind == "twice":                                                   # deterministic across two runs
        again = s.shade(GS.lights(L), shadows=True, bg=bg, shadow_samples=4, light_radius=0.1, ao_samples=4, ao_distance=2.0, seed=SEED)
        once = s.shade(GS.lights(L), shadows=True, bg=bg, shadow_samples=4, light_radius=0.1, ao_samples=4, ao_distance=2.0, seed=SEED)
        for k in ("image", "visibility", "ambient_occlusion"):
            assert biteq(again[k], once[k]), k
        assert biteq(s.transfer(4, SEED), s.transfer(4, SEED))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W,S", [("pair", 9, 4), ("triple", 12, 16)])
def test_environments(precision, kind, W, S):
    """Under the constant environment the shading is ambient(samples, inf) to 4 eps; environment f of an F-launch is the
    1-launch; more than 256 environments are split; the image is max(shading, 0) albedo on the mask and bg off it."""
    from oi_amd import scene
    from oi_amd.envlight import EnvLight
    s = GS.traced(precision, kind, W)
    M = s.S * s.S
    cap = s.capture_transfer(S, SEED)
    assert isinstance(cap, scene.SceneTransfer) and cap.transfer.shape == (1, 9, s.S, s.S) and cap.samples == S
    on = s.owner >= 0
    rs = np.random.RandomState(2)
    envs = [EnvLight.constant(1.0), EnvLight(rs.randn(9, 3) * 0.5), EnvLight.constant((0.2, 0.5, 1.0)).rotated(EV.random_rotation(rs))]
    bg = (0.1, 0.2, 0.3)
    out = cap.shade(envs, bg=bg)
    assert out["image"].shape == out["shading"].shape == (3, 3, s.S, s.S) and out["instance"].dtype == torch.int32
    ao = s.ambient(S, INF, SEED)
    worst = float((out["shading"][0].reshape(3, M)[:, on] - ao[on][None]).abs().max())
    record_margin(f"scene_constant_env[{precision},{kind},S={S}]", "error_over_bar", worst / (4 * EPS))
    assert worst <= 4 * EPS
    for f, env in enumerate(envs):
        alone = cap.shade(env, bg=bg)
        assert biteq(alone["image"][0], out["image"][f]) and biteq(alone["shading"][0], out["shading"][f]), f
    sh, img, mag = EV.shade(npd(cap.transfer.view(9, M)), np.stack([e.coeffs for e in envs]), on.cpu().numpy(),
                            npd(out["albedo"][0].reshape(3, M).t()), bg)
    assert (np.abs(npd(out["shading"].view(3, 3, M)) - sh) <= 16 * EPS * mag + 1e-30).all()
    got, onn = npd(out["image"].view(3, 3, M)), on.cpu().numpy()
    assert (np.abs(got - img)[:, :, onn] <= (16 * EPS * mag)[:, :, onn] + 1e-30).all()
    assert np.array_equal(got[:, :, ~onn], np.broadcast_to(np.float32(bg).astype(np.float64)[None, :, None], (3, 3, int((~onn).sum()))))
    assert not bool(out["shading"].view(3, 3, M)[:, :, ~on].any())
    many = cap.shade([envs[f % 3] for f in range(258)], bg=bg)            # two launches
    assert biteq(many["image"][257], out["image"][257 % 3]) and biteq(many["image"][255], out["image"][255 % 3])
    assert out["stats"][0]["transfer_evals"] > 0
    with pytest.raises(ValueError, match="EnvLight objects only"):
        cap.shade(["sky"])
    # render_scene_env: the same capture through the public entry
    zs, b2ws = GS.instances(kind)
    res = scene.render_scene_env(GS.make_gen(precision), zs, b2ws, envs, transfer_samples=S, seed=SEED, bg=bg, window=W)
    assert biteq(res["image"], out["image"]) and biteq(res["transfer"], cap.transfer) and res["scene"].E == s.E


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mutual_occlusion_on_the_golden_pair(precision):
    """With instance 1 between instance 0 and a light of angular radius 0.1, pixels of instance 0 lie in a penumbra that is
    not there when instance 1 is left out; adding an instance never brightens a pixel."""
    from oi_amd import scene
    from oi_amd.relight import Light
    W = GOLDEN_W
    s = GS.traced(precision, "pair", W)
    zs, b2ws = GS.instances("pair")
    lt = [Light(direction=tuple((b2ws[1][:3, 3] - b2ws[0][:3, 3]).tolist()))]
    kw = dict(shadows=True, shadow_samples=4, light_radius=0.1, ao_samples=4, ao_distance=4.0, seed=SEED)
    both = s.shade(lt, **kw)
    alone = scene.render_scene(GS.make_gen(precision), zs[:1], b2ws[:1], lights=lt, window=W, **kw)
    mine = (both["instance"] == 0) & (alone["instance"] == 0)
    vb, va = both["visibility"][mine[:, :1].expand_as(both["visibility"])], alone["visibility"][mine[:, :1].expand_as(alone["visibility"])]
    penumbra = (vb > 0) & (vb < 1) & (va == 1)
    ab, aa = both["ambient_occlusion"][mine], alone["ambient_occlusion"][mine]
    print(f"scene_light golden pair[{precision}]: pixels of instance 0 {int(mine.sum())}, in instance 1's penumbra only {int(penumbra.sum())}, "
          f"fully shadowed by it only {int(((vb == 0) & (va == 1)).sum())}, with less ambient light {int((ab < aa).sum())}")
    assert int(penumbra.sum()) > 0 and int((vb > va).sum()) == 0
    assert int((ab < aa).sum()) > 0 and int((ab > aa).sum()) == 0



# ---------------------------------------------------------------------------------------------------------------------
# the analytic two-sphere scene
# ---------------------------------------------------------------------------------------------------------------------
class _AnalyticScene:
    """The analytic scene traced as test_gpu_scene._analytic traces it, holding what `sampled` reads of a SceneSurface."""

    def __init__(self):
        from oi_amd import ops
        sc = SR.analytic_scene()
        E, W, S = 2, sc["W"], sc["S"]
        f32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32).cuda().contiguous()
        c2b, self.b2w, kinv = f32(sc["c2b"]), f32(sc["b2w"]), f32(sc["K_inv"])
        self.w2b = f32(np.stack([SR.rigid_inverse(m) for m in sc["b2w"]]))
        self.window = torch.tensor(sc["origins"], dtype=torch.int32).cuda()
        self.sc, self.E, self.W, self.S, self.N, self.bias = sc, E, W, S, W * W, T.BIAS
        st = self.state = ops.trace_batch_state_empty(E, W * W, c2b)
        ops.scene_begin(st, c2b, kinv, self.window, W, S)
        self.march(st, anyhit=False)
        ops.trace_batch_finish(st)
        self.owner, self.owner_ray = ops.scene_resolve(st, self.window, W, S)
        self.vis_index, self.vis_slot = ops.scene_visible(st, self.owner, self.window, W, S)
        self.n_pad, self.n_vis = int(st.live[-1].item()), st.counts[:, -1].tolist()
        self.points = ops.trace_batch_gather(st, self.vis_index, self.n_pad)
        self.grad = (2.0 * self.points).contiguous()
        self.offset = torch.tensor(SR.offsets(self.n_vis), dtype=torch.int32).cuda()
        self._world = ops.scene_points(st, self.points, self.grad, self.n_pad, self.offset, sum(self.n_vis), self.b2w, self.w2b)
        self._pixel = ops.scene_point_pixels(st, self.vis_index, self.window, W, S, self.offset, sum(self.n_vis))

    def world_points(self):
        return self._world

    def point_pixels(self):
        return self._pixel

    def march(self, st, anyhit=True):
        """The field |x| - 0.5 evaluated by torch between the steps (up to OI_TRACE_MAX_STEPS: test_gpu_scene._analytic)."""
        from oi_amd import ops
        step = ops.trace_batch_step_anyhit if anyhit else ops.trace_batch_step
        sdf = torch.zeros(self.E, st.N).cuda()
        bound, k = int(st.live[0].item()), 0
        while bound > 0 and k < T.MAX_MAX_STEPS:
            sdf[:, :bound] = st.points[:, :bound].norm(dim=-1) - SR.RADIUS
            step(st, sdf, bound, k, T.TOL, T.OMEGA)
            k += 1
            bound = int(st.live[k].item())


def test_analytic_two_sphere_scene():
    s = _AnalyticScene()
    sc = s.sc
    cf = SR.analytic_closed_form(sc)
    a = scene_arrays(s)
    E, n, M = 2, sum(s.n_vis), s.S * s.S
    pos, nrm, elem = s.world_points()
    elem_np, b2w = elem.cpu().numpy(), np.asarray(sc["b2w"], dtype=np.float64)
    on, g = SL.pixel_points(a["owner"], a["owner_ray"], a["vis_slot"], a["offset"])
    keep_px = np.zeros(M, dtype=bool)
    keep_px[on] = ~cf["excluded"][on] & (cf["owner"][on] == a["owner"][on])   # the pixels test_gpu_scene.py's analytic test compares
    lt = torch.tensor([T.light_block(tuple(float(x) for x in sc["light"]))], dtype=torch.float32).cuda()
    runs = {"ambient16": (SL.AN_AO_S, dict(distance=INF, transfer=True)), "ambient64": (SL.AN_TRANSFER_S, dict(distance=INF, transfer=True)),
            "soft": (SL.AN_SOFT_S, dict(lt=lt, radius=torch.tensor([SL.AN_SOFT_RADIUS], device="cuda")))}
    for name, (S, kw) in runs.items():
        res = sampled(s, S, [S], march=s.march, **kw)
        sb = res["chunks"][0]
        status = shaped(sb, E, 1, S, n)
        assert set(np.unique(status)) <= {T.MISS, T.HIT, T.BACKFACING}
        # the kernel's own rays, taken to the world in float64: the owner's element holds origin and direction in its frame
        o_own = npd(sb.rays_o).reshape(E, 1, S, n, 3)[elem_np, 0, :, np.arange(n)].transpose(1, 0, 2)      # (S, n, 3)
        d_own = npd(sb.rays_d).reshape(E, 1, S, n, 3)[elem_np, 0, :, np.arange(n)].transpose(1, 0, 2)
        o_w = np.einsum("nab,snb->sna", b2w[elem_np][:, :3, :3], o_own) + b2w[elem_np][None, :, :3, 3]
        d_w = np.einsum("nab,snb->sna", b2w[elem_np][:, :3, :3], d_own)
        blocked, band = SL.sphere_blocks(o_w, d_w)
        facing = status[elem_np, 0, :, np.arange(n)].T != T.BACKFACING                                       # (S, n)
        nw = npd(nrm)
        ndd = (nw[None] * d_w).sum(-1)
        assert np.array_equal(facing[np.abs(ndd) > 1e-5], (ndd > 0)[np.abs(ndd) > 1e-5])
        free_cf = facing & ~blocked.any(0)
        in_band = band.any(0) & facing
        free = SL.escaped(status)[0]
        cmp_ = np.broadcast_to(keep_px[on][None], (S, len(on))) & ~in_band[:, g]
        share_excluded = float(in_band[:, g][:, keep_px[on]].mean())
        assert share_excluded <= R.EXCLUDED_CAP                          # a condition on the scene (rehearsed on the CPU)
        assert np.array_equal(free[:, g][cmp_], free_cf[:, g][cmp_])
        clean = keep_px[on] & ~in_band[:, g].any(0)                      # pixels none of whose rays is in the band
        q = on[clean]
        by_other = blocked[1][:, g][:, clean & (a["owner"][on] == 0)]
        print(f"scene_light analytic[{name}]: points {n}, pixels compared {int(clean.sum())}, rays in the band {int(in_band[:, g].sum())} "
              f"({share_excluded:.5f}), sphere-0 rays blocked by sphere 1 {int(by_other.sum())} of {by_other.size}")
        if "transfer" in kw:
            assert by_other.mean() > SL.BLOCKED_FLOOR
            y = EV.basis(d_w[:, g][:, clean] / np.linalg.norm(d_w[:, g][:, clean], axis=-1, keepdims=True))
            esc = free_cf[:, g][:, clean]
            ref = (esc[..., None] * y).sum(0).T / S
            mag = (esc[..., None] * np.abs(y)).sum(0).T
            bar = EPS * ((esc.sum(0)[None] + 1) * mag + 16 * 1.1 * esc.sum(0)[None]) / S
            err = np.abs(npd(res["transfer"])[:, q] - ref)
            record_margin(f"scene_analytic_transfer[{name}]", "error_over_bar", float((err[bar > 0] / bar[bar > 0]).max()))
            assert (err <= bar).all()
            assert np.array_equal(npd(res["out"])[0, q], (esc.sum(0).astype(np.float32) / np.float32(S)).astype(np.float64))
        else:
            share = (free_cf[:, g][:, clean].sum(0).astype(np.float32) / np.float32(S)).astype(np.float64)
            assert np.array_equal(npd(res["out"])[0, q], share)
            on0 = a["owner"][q] == 0
            assert ((share[on0] > 0) & (share[on0] < 1)).any() and (share[on0] == 0).any()      # sphere 1's penumbra and umbra on sphere 0


# ---------------------------------------------------------------------------------------------------------------------
# ragged scenes, the walks, the refusals on device memory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_scenes(precision):
    """An instance wholly off screen changes nothing; a scene without any hit launches nothing and returns the off-mask
    values; a window half outside the image and E = 1 are among CASES."""
    from oi_amd import scene
    from oi_amd.envlight import EnvLight
    gen = GS.make_gen(precision)
    bg, W = (0.25, 0.5, 0.75), 12
    S = gen.scene_resolution
    kw = dict(lights=GS.lights(2), shadows=True, bg=bg, window=W, shadow_samples=4, light_radius=[0.1, 0.0], ao_samples=4, ao_distance=1.0,
              seed=SEED)
    zs, b2ws = GS.instances("offscreen")
    off = scene.render_scene(gen, zs, b2ws, **kw)
    alone = scene.render_scene(gen, zs[:1], b2ws[:1], **kw)
    for k in ("image", "visibility", "ambient_occlusion", "depth", "instance"):
        assert biteq(off[k], alone[k]), k
    so = off["scene"]
    assert so.n_vis[1] == 0 and so.shadow.E == 2 and not bool(so.shadow.steps[1].any())       # nothing entered the far instance
    envs = [EnvLight.constant(1.0)]
    assert biteq(so.capture_transfer(4, SEED).shade(envs, bg)["image"], alone["scene"].capture_transfer(4, SEED).shade(envs, bg)["image"])
    zs, b2ws = GS.instances("nothing")
    none = scene.render_scene(gen, zs, b2ws, **kw)
    sn = none["scene"]
    assert sn.n_pad == 0 and sn.shadow is None and sn.ao is None and sn.shadow_evals == sn.occlusion_evals == 0
    assert bool((none["visibility"] == 1).all()) and bool((none["ambient_occlusion"] == 1).all())
    assert torch.equal(none["image"], torch.tensor(bg).cuda()[None, :, None, None].expand(2, 3, S, S))
    cap = sn.capture_transfer(4, SEED)
    assert not bool(cap.transfer.any()) and sn.transfer_state is None and sn.transfer_evals == 0
    res = cap.shade(envs, bg)
    assert torch.equal(res["image"], torch.tensor(bg).cuda()[None, :, None, None].expand(1, 3, S, S)) and not bool(res["shading"].any())
    assert bool((res["instance"] == -1).all())
    tri = GS.traced(precision, "triple", W)                              # the third window lies half outside the image
    out = tri.shade(GS.lights(1), shadows=True, shadow_samples=4, light_radius=0.1, ao_samples=4)
    assert int(tri.window[2, 0]) < 0 and tri.n_vis[2] > 0 and bool(torch.isfinite(out["image"]).all())
    assert float(out["visibility"].min()) >= 0 and float(out["visibility"].max()) <= 1


@pytest.mark.parametrize("precision", PRECISIONS)
def test_walks(precision):
    from oi_amd import inference, scene
    from oi_amd.envlight import EnvLight
    gen = GS.make_gen(precision)
    zs, b2ws = GS.instances("pair")
    s = GS.traced(precision, "pair", 12)
    env = EnvLight(np.random.RandomState(4).randn(9, 3) * 0.4 + np.eye(9, 3))
    walk = inference.scene_env_walk(gen, zs, b2ws, env, n_frames=5, transfer_samples=4, seed=SEED, window=12, bg=(0.1, 0.1, 0.1))
    S = gen.scene_resolution
    assert walk["image"].shape == walk["shading"].shape == (5, 3, S, S) and walk["transfer"].shape == (1, 9, S, S)
    cap = s.capture_transfer(4, SEED)
    assert biteq(walk["transfer"], cap.transfer)
    for f, Rm in enumerate(inference.env_walk_rotations(5, (0, 0, 1))):
        one = cap.shade(env.rotated(Rm), bg=(0.1, 0.1, 0.1))
        assert biteq(one["image"][0], walk["image"][f]) and biteq(one["shading"][0], walk["shading"][f]), f
    assert biteq(cap.shade(env, bg=(0.1, 0.1, 0.1))["image"][0], walk["image"][0]) and walk["stats"][0]["transfer_evals"] > 0
    # the light walk with soft shadows and ambient occlusion: the split by max_shadow_rays changes no byte
    kw = dict(n_frames=5, window=12, shadow_samples=4, light_radius=0.1, ao_samples=4, ao_distance=1.0, seed=SEED)
    whole = inference.scene_light_walk(gen, zs, b2ws, **kw)
    split = inference.scene_light_walk(gen, zs, b2ws, max_shadow_rays=2 * 4 * s.E * sum(s.n_vis), **kw)
    finer = inference.scene_light_walk(gen, zs, b2ws, max_shadow_rays=3 * s.E * sum(s.n_vis), **kw)          # one light, chunks of 3 + 1
    for k in ("image", "visibility", "ambient_occlusion", "mask", "depth"):
        assert biteq(whole[k], split[k]) and biteq(whole[k], finer[k]), k
    assert whole["ambient_occlusion"].shape == (1, 1, S, S)
    vals = np.unique(whole["visibility"].cpu().numpy())
    assert set(vals) <= {0.0, 0.25, 0.5, 0.75, 1.0} and len(vals) > 2
    from oi_amd.relight import Light
    one = scene.render_scene(gen, zs, b2ws, lights=[Light.from_module(gen.light)], shadows=True, window=12, shadow_samples=4, light_radius=0.1,
                             ao_samples=4, ao_distance=1.0, seed=SEED)
    assert biteq(one["image"][0], whole["image"][0])


def test_c_abi_rejects_invalid_arguments_and_launches_nothing():
    """The refusals of tests/test_scene_light_cpu.py on real, poisoned device arrays: each returns a negative status with its
    text, and no array is touched."""
    from oi_amd import lib
    L = lib.load()
    E, N = 3, 48
    g = lambda sh, dt=torch.float32: guarded_empty(sh, dt, what="untouched", must_write=False)
    shapes = dict(rays_o=(E, N, 3), rays_d=(E, N, 3), near_=(E, N), far_=(E, N), t=(E, N), bracket=(E, N, 4), points=(E, N, 3))
    arr = {k: g(sh) for k, sh in shapes.items()}
    arr.update(status=g((E, N), torch.uint8), side=g((E, N), torch.uint8), steps=g((E, N), torch.int16),
               active=g((E, 2, N), torch.int32), counts=g((E, lib.TRACE_COUNT_WORDS), torch.int32))
    other = g((1024 * 8,))
    p = lambda t_: ctypes.c_void_p(t_.data_ptr())
    for call, entry, text in C.invalid_argument_cases(lib, L, p(other), {k: p(v) for k, v in arr.items()}):
        rc = call()
        msg = L.oi_last_error().decode()
        assert rc < 0 and msg.startswith(entry) and text in msg, (entry, text, rc, msg)
    torch.cuda.synchronize()
    for k, v in list(arr.items()) + [("other", other)]:
        fresh = guarded_empty(tuple(v.shape), v.dtype, what="pattern", must_write=False)
        assert torch.equal(v.view(torch.uint8), fresh.view(torch.uint8)), k
