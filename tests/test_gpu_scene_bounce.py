"""The diffuse interreflection bounce between the instances of a scene on the MI355X (include/oi_scene_bounce.h; oi_amd.scene;
oi_amd.inference.scene_env_walk): the winner of every transfer ray among the instances, the per-element
lists of the rays won, the bounce transfer resolved over chunks of samples, and the host layer around them.

Exact properties are checked bit for bit: the winners and the lists against the float64 restatement of
tests/helpers/scene_bounce_ref.py (integers), chunked against unchunked, a one-instance scene against oi_bounce_resolve (the
per-sample term is one __device__ function), the direct transfer of a bounce capture against the plain capture's, bounces=0
against the parent's launches.  The restatement touches no code under test.

Bars (EPS = 2^-24), each one a neighbouring file derives:
  RESOLVE    section 4.22's (K_band + S + 2) EPS mag per output, K = 1 / 14 / 40 by band (helpers.bounce_ref.resolve_bar), against the
             restatement fed the kernel's own float32 inputs.
  FURNACE    section 4.22's (S + 16) EPS on |shading - 1| for every pixel whose samples are all free or front-face winners.
  ANALYTIC   two fields |x| - 0.5.  Winners exact against ray-against-sphere in float64 on the kernel's own rays, outside the band
             |closest approach - 0.5| < 1e-3 and |n . d| < 1e-3 at the hit (at most 1 % of the facing rays; tests/test_scene_bounce_cpu.py
             rehearses that on float64 alone); hit points within tol + 8 EPS of the winning sphere; T1 per pixel within 5 standard
             errors of the per-sample bound 0.5 rho A_c |y_c|max / sqrt(S) of the restatement on the exact intersections."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_envbounce as GB
import test_gpu_scene as GS
import test_gpu_scene_light as GL
import test_gpu_trace as G
import test_scene_bounce_cpu as C
from conftest import record_margin
from helpers import bounce_ref as B
from helpers import env_ref as EV
from helpers import scene_bounce_ref as SB
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)
from test_gpu_trace_batch import biteq

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS, npd = G.PRECISIONS, G.npd
EPS = B.EPS
SEED = SL.SEED
INF = float("inf")
BG = (0.1, 0.2, 0.3)
SCENE_OPS = {"trace_batch_state_empty", "scene_occlusion_begin", "trace_batch_finish", "scene_transfer_resolve", "scene_transfer_normal",
             "scene_bounce_nearest", "scene_bounce_visible", "trace_batch_gather", "sdf_mlp_fwd", "scene_bounce_resolve", "scene_shade",
             "scene_lobe_begin", "scene_occlusion_resolve", "scene_reflect", "env_shade", "env_shade_bounce", "env_shade_glossy_dirs"}

p_ = lambda t_: None if t_ is None else ctypes.c_void_p(t_.data_ptr())


def dev(a, dtype, what="input"):
    return guarded_copy(torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda(), what)


# ---------------------------------------------------------------------------------------------------------------------
# oi_scene_bounce_nearest and oi_scene_bounce_visible on synthetic states
# ---------------------------------------------------------------------------------------------------------------------
def _synthetic_states(rs, E, Nr):
    """(name, status (E, Nr) uint8, t (E, Nr) float32): every final status with equal t in two elements and an element that wins
    nothing; an element that wins everything; all MISS."""
    st = rs.choice(C.FINAL, size=(E, Nr), p=[0.3, 0.5, 0.05, 0.05, 0.05, 0.05]).astype(np.uint8)
    t = (rs.rand(E, Nr) * 3 + 0.1).astype(np.float32)
    if E > 1:
        st[0] = np.where(st[0] == T.HIT, T.MISS, st[0])                       # element 0 wins nothing
        same = rs.rand(Nr) < 0.5
        t[E - 1] = np.where(same, t[E // 2], t[E - 1])                        # equal t in two elements (E = 2: no HIT in element 0)
        if E > 2:
            t[1] = np.where(rs.rand(Nr) < 0.5, t[E - 1], t[1])
    yield "mixed", st, t
    st2 = np.where(rs.rand(E, Nr) < 0.5, T.HIT, T.MISS).astype(np.uint8)
    st2[E - 1] = T.HIT
    t2 = t.copy()
    t2[E - 1] = 0.01                                                          # the last element is nearest everywhere
    yield "one_wins_all", st2, t2
    yield "all_miss", np.full((E, Nr), T.MISS, dtype=np.uint8), t


@pytest.mark.parametrize("Nr", [1, 63, 65, 257, 1025])
@pytest.mark.parametrize("E", [1, 2, 3, 5])
def test_nearest_and_visible(E, Nr):
    from oi_amd import lib
    L = lib.load()
    rs = np.random.RandomState(100 * E + Nr)
    WORDS = lib.TRACE_COUNT_WORDS
    for name, st, t in _synthetic_states(rs, E, Nr):
        status, td = dev(st, torch.uint8, "status"), dev(t, torch.float32, "t")
        winner = guarded_empty((Nr,), torch.int32, what="winner")
        assert L.oi_scene_bounce_nearest(p_(status), p_(td), E, Nr, p_(winner), None) == 0, L.oi_last_error()
        want = SB.winners(st, t)
        got = winner.cpu().numpy()
        assert np.array_equal(got, want), name
        if name == "mixed" and Nr >= 63:
            assert (want < 0).any() and (want >= 0).any()
            if E > 1:
                assert not (want == 0).any()
            tied = (want >= 0) & (((t == t[want.clip(0), np.arange(Nr)][None]) & (st == T.HIT)).sum(0) > 1)
            assert tied.any() or E < 3                                        # equal t among the nearest hits: the lowest index won
            assert (want[tied] == ((t == t[want.clip(0), np.arange(Nr)][None]) & (st == T.HIT)).argmax(0)[tied]).all()
        if name == "one_wins_all":
            assert (want == E - 1).all()
        # the lists: only the hit words of counts and live are written
        counts = guarded_empty((E, WORDS), torch.int32, what="counts", must_write=False).fill_(77)
        live = guarded_empty((WORDS,), torch.int32, what="live", must_write=False).fill_(55)
        b = lib.TraceBatch()
        b.s.N, b.E, b.live = Nr, E, p_(live)
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(b.s, n, p_(status))                                       # never dereferenced, but for counts
        b.s.counts = p_(counts)
        sel_index = guarded_empty((E, Nr), torch.int32, what="sel_index", must_write=False)
        sel_slot = guarded_empty((E, Nr), torch.int32, what="sel_slot")
        assert L.oi_scene_bounce_visible(ctypes.byref(b), p_(winner), p_(sel_index), p_(sel_slot), None) == 0, L.oi_last_error()
        c, lv = counts.cpu().numpy(), live.cpu().numpy()
        n_sel = [int((want == e).sum()) for e in range(E)]
        assert c[:, -1].tolist() == n_sel and (c[:, :-1] == 77).all() and lv[-1] == max(n_sel) and (lv[:-1] == 55).all(), name
        idx, slot = sel_index.cpu().numpy(), sel_slot.cpu().numpy()
        assert SB.slots_consistent(want, idx, slot, n_sel) is None, (name, SB.slots_consistent(want, idx, slot, n_sel))
        poison = guarded_empty((E, Nr), torch.int32, what="pattern", must_write=False).cpu().numpy()
        for e in range(E):
            assert np.array_equal(idx[e, n_sel[e]:], poison[e, n_sel[e]:]), (name, e)   # behind n_sel_e nothing is written
        if name == "all_miss":
            assert max(n_sel) == 0 and (slot == -1).all()
        assert torch.equal(status.cpu(), torch.as_tensor(st))


# ---------------------------------------------------------------------------------------------------------------------
# oi_scene_bounce_resolve against the restatement fed the kernel's own float32 inputs
# ---------------------------------------------------------------------------------------------------------------------
def _upload(c):
    d = dict(owner=dev(c["owner"], torch.int32, "owner"), owner_ray=dev(c["owner_ray"], torch.int32, "owner_ray"),
             vis_slot=dev(c["vis_slot"], torch.int32, "vis_slot"), offset=dev(c["offset"], torch.int32, "offset"),
             w2b=dev(c["w2b"], torch.float32, "w2b"))
    if c["n_pad2"]:
        d.update(grad2=dev(c["grad2"], torch.float32, "grad2"), rgb2=dev(c["rgb2"], torch.float32, "rgb2"))
    else:
        d.update(grad2=None, rgb2=None)
    return d


def _chunk_lists(c, j0, k):
    """Chunk [j0, j0 + k) of the case as the sequence would present it: its own selection -- per element the rays won in this
    chunk, densely numbered -- and the rows of the case's gathered gradients and albedo in that numbering, padded with zeros to
    the chunk's own n_pad2.  A ray whose slot lies behind the case's rows keeps no slot: it is skipped either way."""
    E, n, pad = c["E"], c["n"], c["n_pad2"]
    w = c["winner"][j0:j0 + k].reshape(-1)
    old = c["sel_slot"][:, j0:j0 + k].reshape(E, -1)
    rows = [np.nonzero((w == e) & (old[e] >= 0) & (old[e] < pad))[0] for e in range(E)]
    n_pad2 = max(len(r) for r in rows)
    slot = np.full((E, k * n), -1, dtype=np.int32)
    grad2, rgb2 = np.zeros((E, max(n_pad2, 1), 3), dtype=np.float32), np.zeros((E, max(n_pad2, 1), 3), dtype=np.float32)
    for e, r in enumerate(rows):
        slot[e, r] = np.arange(len(r))
        if len(r):
            grad2[e, :len(r)], rgb2[e, :len(r)] = c["grad2"][e, old[e, r]], c["rgb2"][e, old[e, r]]
    return slot.reshape(E, k, n), n_pad2, grad2[:, :n_pad2], rgb2[:, :n_pad2]


def _resolve_gpu(L, c, d, cuts, scene_S):
    """The case resolved in chunks of samples through the C ABI on guarded buffers -> bounce (3, 9, M).  One chunk: the case's
    own lists and rows; several: each chunk's own (_chunk_lists), so n_pad2 differs from chunk to chunk as it does in a trace."""
    E, S, n, M = c["E"], c["S"], c["n"], c["M"]
    out = guarded_empty((3, 9, M), what="bounce")
    j0 = 0
    for k in cuts:
        if len(cuts) == 1:
            slots, n_pad2, g2, c2 = c["sel_slot"], c["n_pad2"], d["grad2"], d["rgb2"]
        else:
            slots, n_pad2, g2, c2 = _chunk_lists(c, j0, k)
            g2, c2 = (dev(g2, torch.float32, "grad2"), dev(c2, torch.float32, "rgb2")) if n_pad2 else (None, None)
        w = dev(c["winner"][j0:j0 + k], torch.int32, "winner")
        sl = dev(slots, torch.int32, "sel_slot")
        rd = dev(c["rays_d"][:, j0:j0 + k], torch.float32, "rays_d")
        rc = L.oi_scene_bounce_resolve(p_(w), p_(sl), p_(rd), p_(g2), p_(c2), n_pad2, p_(d["owner"]), p_(d["owner_ray"]),
                                       p_(d["vis_slot"]), p_(d["offset"]), p_(d["w2b"]), E, c["N"], S, j0, k, n, scene_S, int(j0 + k == S),
                                       p_(out), None)
        assert rc == 0, L.oi_last_error()
        j0 += k
    return out


def _shapes(scene_S, E):
    """Visible points per element for a scene of scene_S^2 pixels: most pixels on the mask, some off it."""
    M = scene_S * scene_S
    if M == 1:
        return [1] + [0] * (E - 1), 4
    n = (M * 3) // 4
    per = [n // E + (1 if e < n % E else 0) for e in range(E)]
    return per, max(per) + 3


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("E", [1, 2, 3])
@pytest.mark.parametrize("scene_S", [1, 9, 12])
def test_bounce_resolve(scene_S, E, S):
    _run_resolve(scene_S, E, S)


def test_bounce_resolve_256_samples():
    _run_resolve(1, 2, 256)


def _run_resolve(scene_S, E, S):
    from oi_amd import lib
    L = lib.load()
    rs = np.random.RandomState(1000 * scene_S + 10 * E + S)
    n_vis, N = _shapes(scene_S, E)
    M = scene_S * scene_S
    worst, seen = 0.0, set()
    for pad in ("full", "half", 1, 0):
        c = C.random_case(rs, E, S, n_vis, M, N=N)
        full = c["n_pad2"]
        n_pad2 = {"full": full, "half": min(full, max(1, full // 2)), 1: min(full, 1), 0: 0}[pad]
        c = dict(c, n_pad2=n_pad2, grad2=c["grad2"][:, :n_pad2] if n_pad2 else None, rgb2=c["rgb2"][:, :n_pad2] if n_pad2 else None)
        d = _upload(c)
        got = _resolve_gpu(L, c, d, [S], scene_S)
        ref, mag, ndds, fronts = C.resolved(c)
        bar = SB.resolve_bar(mag, S)
        err = np.abs(npd(got) - ref)
        assert (err <= bar).all(), (pad, float((err - bar).max()))
        if (bar > 0).any():
            worst = max(worst, float((err[bar > 0] / bar[bar > 0]).max()))
        off = c["owner"] < 0
        assert not got[:, :, torch.as_tensor(off).cuda()].view(torch.int32).any()              # off the mask: exact zeros
        on, g = SL.pixel_points(c["owner"], c["owner_ray"], c["vis_slot"], c["offset"])
        w = c["winner"][:, g]
        if n_pad2:
            seen |= {"front"} if fronts[0].any() else set()
            seen |= {"back"} if ((w >= 0) & ~fronts[0] & (ndds[0] > 0)).any() else set()
            seen |= {"other"} if (fronts[0] & (w != c["owner"][on][None])).any() else set()
            k = np.where(w >= 0, c["sel_slot"][w.clip(0), np.arange(S)[:, None], g[None]], -1)
            tiny = np.linalg.norm(c["grad2"], axis=-1) < 1e-6
            seen |= {"tiny"} if ((w >= 0) & (k >= 0) & (k < n_pad2) & tiny[w.clip(0), k.clip(0, n_pad2 - 1)]).any() else set()
        else:
            assert not got.view(torch.int32).any()
        seen |= {"off"} if off.any() else set()
        # chunks: one sample per chunk and an uneven split, byte for byte
        for cuts in ([1] * S, [S - 1, 1], [1, S - 1]) if S > 1 else ():
            assert biteq(_resolve_gpu(L, c, d, cuts, scene_S), got), (pad, cuts)
    case = f"scene_bounce_resolve[M={M},E={E},S={S}]"
    print(case, "worst error / bar", worst, "seen", sorted(seen))
    record_margin(case, "err_over_bar", worst)
    if M > 1 and S > 1:
        assert {"front", "back", "off", "tiny"} <= seen and (E == 1 or "other" in seen), seen


@pytest.mark.parametrize("S", [1, 4])
def test_one_element_is_the_single_view_resolve(S):
    """E = 1: the same statuses, directions, gradients and albedo through oi_bounce_resolve (hit_slot2 = the selection's slots)
    and through oi_scene_bounce_resolve: byte-equal, the per-sample term being one __device__ function."""
    from oi_amd import lib, ops
    L = lib.load()
    rs = np.random.RandomState(40 + S)
    scene_S = 12
    c = C.random_case(rs, 1, S, [100], scene_S * scene_S, N=110)
    d = _upload(c)
    scene = _resolve_gpu(L, c, d, [S], scene_S)
    on, g = SL.pixel_points(c["owner"], c["owner_ray"], c["vis_slot"], c["offset"])
    hit_slot = np.full(c["M"], -1)
    hit_slot[on] = g
    slot2 = np.where(c["winner"] == 0, c["sel_slot"][0], -1).reshape(-1)
    one = ops.bounce_resolve(dev(c["status"][0].reshape(-1), torch.uint8, "status"), dev(c["rays_d"][0].reshape(-1, 3), torch.float32, "d"),
                             dev(slot2, torch.int32, "slot2"), d["grad2"][0], d["rgb2"][0], c["n_pad2"], dev(hit_slot, torch.int32, "slot"),
                             c["M"], c["n"], S, d["w2b"][0])
    assert bool(scene.abs().max() > 0) and biteq(one, scene)


# ---------------------------------------------------------------------------------------------------------------------
# the furnace through the kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 256])
@pytest.mark.parametrize("E", [1, 3])
def test_furnace(E, S):
    """White albedo at the secondary points under the constant environment: oi_scene_transfer_resolve + oi_scene_bounce_resolve +
    oi_env_shade_bounce shade every pixel whose S samples are all free or front-face winners 1 within (S + 16) EPS."""
    from oi_amd import ops
    from oi_amd.envlight import EnvLight, stack_envs
    rs = np.random.RandomState(7 * E + S)
    scene_S = 9
    n_vis, N = _shapes(scene_S, E)
    M = scene_S * scene_S
    c = C.random_case(rs, E, S, n_vis, M, N=N, statuses=(T.MISS, T.HIT), p_hit=0.3, front=True, tiny_grad=0.0)
    dead = rs.rand(E, S, c["n"]) < (0.02 if S < 16 else 0.0005)              # a few samples that bounce nothing
    c["status"] = np.where(dead, T.LIMIT, c["status"]).astype(np.uint8)
    c["winner"] = SB.winners(c["status"], c["t"])
    keep = c["winner"][None] == np.arange(E)[:, None, None]
    c["sel_slot"] = np.where(keep, c["sel_slot"], -1)                         # (slots of rays no longer won are never read)
    c["rgb2"] = np.ones_like(c["rgb2"])
    d = _upload(c)
    n = c["n"]
    st = dev(c["status"].reshape(E, -1), torch.uint8, "status")
    rd = dev(c["rays_d"].reshape(E, -1, 3), torch.float32, "rays_d")
    transfer = ops._new(rd, 9, M)
    ops.scene_transfer_resolve(st, rd, d["owner"], d["owner_ray"], d["vis_slot"], d["offset"], d["w2b"], E, c["N"], S, 0, S, n, scene_S,
                               transfer, True)
    bounce = ops._new(rd, 3, 9, M)
    ops.scene_bounce_resolve(dev(c["winner"], torch.int32, "winner"), dev(c["sel_slot"], torch.int32, "sel_slot"), rd, d["grad2"], d["rgb2"],
                             c["n_pad2"], d["owner"], d["owner_ray"], d["vis_slot"], d["offset"], d["w2b"], E, c["N"], S, 0, S, n, scene_S,
                             bounce, True)
    mask = c["owner"] >= 0
    prim = dev(np.where(mask, T.HIT, T.MISS), torch.uint8, "status1")
    slot = dev(np.where(mask, np.arange(M), -1), torch.int32, "slot1")
    out = ops.env_shade_bounce(prim, slot, torch.ones(M, 3).cuda(), M, transfer, bounce, stack_envs([EnvLight.constant(1)]), None)
    _, _, _, fronts = C.resolved(c)
    on, g = SL.pixel_points(c["owner"], c["owner_ray"], c["vis_slot"], c["offset"])
    full = np.zeros(M, dtype=bool)
    full[on] = (SL.escaped(c["status"])[:, g] | fronts[0]).all(0)
    sh = npd(out["shading"])[0]
    err, bar = float(np.abs(sh[:, full] - 1.0).max()), (S + 16) * EPS
    print(f"scene_bounce_furnace[E={E},S={S}] pixels on the mask {int(mask.sum())}, with every sample free or a front-face winner "
          f"{int(full.sum())}; |shading - 1| {err:.3g} bar {bar:.3g}; indirect share {float(npd(out['indirect'])[0][:, full].mean()):.3f}")
    record_margin(f"scene_bounce_furnace[E={E},S={S}]", "err_over_bar", err / bar)
    assert full.sum() > 10 and (mask & ~full).sum() > 0 and err <= bar
    assert (sh[:, mask & ~full] < 1.0 - 0.5 / S).all() and not sh[:, ~mask].any()


# ---------------------------------------------------------------------------------------------------------------------
# the sequence on traced scenes
# ---------------------------------------------------------------------------------------------------------------------
def bounced(s, S, cuts, march=None, grad_rgb=None, seed=SEED):
    """The sequence of include/oi_scene_bounce.h through the ops wrappers, chunk by chunk.  march(sb): the closest-hit march
    (default the field's); grad_rgb(points (E, n_pad2, 3)) -> grad2, rgb2 (default the field's full pass).  -> dict: chunks (per
    chunk the state and what the resolve read), transfer, bounce."""
    from oi_amd import ops, trace
    pos, nrm, elem = s.world_points()
    pixel = s.point_pixels()
    n_vis, M, E = sum(s.n_vis), s.S * s.S, s.E
    tr, bo = ops._new(pos, 9, M), ops._new(pos, 3, 9, M)
    chunks, j0 = [], 0
    for c in cuts:
        sb = ops.trace_batch_state_empty(E, c * n_vis, pos)
        ops.scene_occlusion_begin(sb, s.points, s.grad, s.n_pad, s.offset, elem, pixel, pos, nrm, n_vis, s.w2b, s.bias, S, j0, c, seed,
                                  distance=INF)
        bound = int(sb.live[0].item())
        if bound:
            if march is None:
                trace._march_batch(s.field, sb, *s.kw, bound=bound, anyhit=False)
            else:
                march(sb)
            ops.trace_batch_finish(sb)
        last = j0 + c == S
        ops.scene_transfer_resolve(sb.status, sb.rays_d, s.owner, s.owner_ray, s.vis_slot, s.offset, s.w2b, E, s.N, S, j0, c, n_vis, s.S, tr,
                                   last)
        winner = ops.scene_bounce_nearest(sb.status, sb.t, E, sb.N)
        sel_index, sel_slot = ops.scene_bounce_visible(sb, winner)
        n_pad2 = int(sb.live[-1].item())
        n_sel = sb.counts[:, -1].tolist()
        points2 = grad2 = rgb2 = None
        if n_pad2:
            points2 = ops.trace_batch_gather(sb, sel_index, n_pad2)
            if grad_rgb is None:
                _, grad2, rgb2 = s.field.full(points2.view(E * n_pad2, 3))
                grad2, rgb2 = grad2.view(E, n_pad2, 3), rgb2.view(E, n_pad2, 3)
            else:
                grad2, rgb2 = grad_rgb(points2)
        ops.scene_bounce_resolve(winner, sel_slot, sb.rays_d, grad2, rgb2, n_pad2, s.owner, s.owner_ray, s.vis_slot, s.offset, s.w2b, E, s.N,
                                 S, j0, c, n_vis, s.S, bo, last)
        chunks.append(dict(sb=sb, c=c, winner=winner, sel_index=sel_index, sel_slot=sel_slot, n_pad2=n_pad2, n_sel=n_sel, points=points2,
                           grad=grad2, rgb=rgb2))
        j0 += c
    return dict(chunks=chunks, transfer=tr, bounce=bo)


def ref_chunks(chunks, E, n):
    """The chunks of `bounced` as scene_bounce_ref.resolve takes them: the kernel's own float32 inputs."""
    out = []
    for ch in chunks:
        c = ch["c"]
        out.append(dict(winner=ch["winner"].cpu().numpy().reshape(c, n), sel_slot=ch["sel_slot"].cpu().numpy().reshape(E, c, n),
                        rays_d=npd(ch["sb"].rays_d).reshape(E, c, n, 3), grad2=None if ch["grad"] is None else npd(ch["grad"]),
                        rgb2=None if ch["rgb"] is None else npd(ch["rgb"])))
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W,S", [("pair", 9, 4), ("triple", 12, 4), ("pair", 12, 1), ("triple", 9, 1)])
def test_chunks_and_the_direct_transfer(precision, kind, W, S):
    """On traced scenes: winners and lists exact against the restatement on the library's own states; the bounce within its bar;
    Sc = S, Sc = 1 and an uneven split byte-equal, through the ops and through max_shadow_rays (the MLP pass is per point: padding
    to another n_pad2 changes no value); the direct transfer of the closest-hit march byte-equal to the any-hit one's, because per
    element the rays ending MISS are the same; per element the batched closest-hit march equals oi_trace_step on that element."""
    from oi_amd import ops, trace
    s = GS.traced(precision, kind, W)
    a = GL.scene_arrays(s)
    E, n, M = s.E, sum(s.n_vis), s.S * s.S
    whole = None
    for cuts in GL.cuts_of(S):
        res = bounced(s, S, cuts)
        for ch in res["chunks"]:
            st, t = ch["sb"].status.cpu().numpy(), ch["sb"].t.cpu().numpy()
            want = SB.winners(st, t)
            assert np.array_equal(ch["winner"].cpu().numpy(), want) and int(st.max()) <= T.BACKFACING
            n_sel = [int((want == e).sum()) for e in range(E)]
            assert ch["n_sel"] == n_sel and ch["n_pad2"] == max(n_sel)
            assert SB.slots_consistent(want, ch["sel_index"].cpu().numpy(), ch["sel_slot"].cpu().numpy(), n_sel) is None
        ref, mag, _, fronts = SB.resolve(ref_chunks(res["chunks"], E, n), a["owner"], a["owner_ray"], a["vis_slot"], a["offset"], a["w2b"], S)
        bar = SB.resolve_bar(mag, S)
        err = np.abs(npd(res["bounce"]) - ref)
        assert (err <= bar).all()
        if (bar > 0).any():
            record_margin(f"scene_bounce[{precision},{kind},W={W},S={S},cuts={len(cuts)}]", "err_over_bar", float((err[bar > 0] / bar[bar > 0]).max()))
        assert not npd(res["bounce"])[:, :, a["owner"] < 0].any()
        if whole is None:
            whole = res
            print(f"scene_bounce[{precision},{kind},W={W},S={S}] rays {S * n}, won per element {res['chunks'][0]['n_sel']}, front-face winners "
                  f"{int(sum(f.sum() for f in fronts))}")
        else:
            assert biteq(res["bounce"], whole["bounce"]) and biteq(res["transfer"], whole["transfer"]), cuts
    # T0 is untouched: the any-hit trace's transfer, byte for byte; per element the same rays end MISS under both steps
    any_ = GL.sampled(s, S, [S], distance=INF, transfer=True)
    assert biteq(any_["transfer"], whole["transfer"])
    sb_c, sb_a = whole["chunks"][0]["sb"], any_["chunks"][0]
    assert torch.equal(sb_c.status == T.MISS, sb_a.status == T.MISS) and torch.equal(sb_c.status == T.BACKFACING, sb_a.status == T.BACKFACING)
    assert bool((sb_c.status == T.HIT).any())
    # the host layer: the same bytes, whole and split by max_shadow_rays; the direct transfer is the plain capture's
    t1, b1 = s.transfer_bounce(S, SEED)
    assert biteq(t1, whole["transfer"]) and biteq(b1, whole["bounce"]) and biteq(s.transfer(S, SEED), t1)
    if S > 1:
        for limit in (E * n, E * n * (S - 1)):
            t2, b2 = s.transfer_bounce(S, SEED, max_shadow_rays=limit)
            assert biteq(t2, t1) and biteq(b2, b1), limit
    plain, cap = s.capture_transfer(S, SEED), s.capture_transfer(S, SEED, bounces=1)
    assert plain.bounce is None and cap.bounce.shape == (1, 3, 9, s.S, s.S) and biteq(cap.transfer, plain.transfer)
    assert biteq(cap.bounce.view(3, 9, M), b1)
    # per element: the batched closest-hit march is oi_trace_step's on that element's state alone
    pos, nrm, elem = s.world_points()
    sb = ops.trace_batch_state_empty(E, S * n, pos)
    ops.scene_occlusion_begin(sb, s.points, s.grad, s.n_pad, s.offset, elem, s.point_pixels(), pos, nrm, n, s.w2b, s.bias, S, 0, S, SEED,
                              distance=INF)
    ones = []
    for e in range(E):
        one = ops.TraceState(S * n, sb.rays_o[e].clone(), sb.rays_d[e].clone(), sb.near[e].clone(), sb.far[e].clone())
        for k in ("t", "status", "steps", "bracket", "side", "active", "points", "counts"):
            getattr(one, k).copy_(getattr(sb, k)[e])
        ones.append(one)
    trace._march_batch(s.field, sb, *s.kw, bound=int(sb.live[0].item()), anyhit=False)
    for e, one in enumerate(ones):
        f = copy.copy(s.field)
        f.B, f.gamma, f.beta = 1, s.field.gamma[e:e + 1], s.field.beta[e:e + 1]
        bound = int(one.counts[0].item())
        if bound:
            trace._march(f, one, bound, *s.kw, anyhit=False)
        assert torch.equal(sb.status[e], one.status) and torch.equal(sb.steps[e], one.steps) and torch.equal(sb.t[e], one.t), e


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W", [("pair", 9), ("triple", 12)])
def test_defaults_are_the_parents_launches(precision, kind, W, monkeypatch):
    """bounces=0: the recorded ops of capture_transfer are those of a call without the keyword -- the parent's sequence, spelled
    out -- and the bytes of the capture and of its shade are the parent's."""
    from oi_amd import ops
    from oi_amd.envlight import EnvLight, stack_envs
    s = GS.traced(precision, kind, W)
    S, M = 4, s.S * s.S
    s.world_points(), s.point_pixels()
    envs = [EnvLight(np.random.RandomState(2).randn(9, 3) * 0.5 + np.eye(9)[0][:, None] * 3.0), EnvLight.constant((1.0, 0.5, 0.25))]
    # the parent's sequence through the ops: the any-hit trace, oi_scene_transfer_resolve, oi_env_shade on the scene's planes
    par = GL.sampled(s, S, [S], distance=INF, transfer=True)
    planes = s._shade(None, None, None, ("albedo", "instance"))
    on = planes["instance"] >= 0
    view = (on.to(torch.uint8) * T.HIT, torch.where(on, torch.arange(M, dtype=torch.int32).cuda(), torch.full((M,), -1, dtype=torch.int32).cuda()),
            planes["albedo"], M, par["transfer"])
    want = ops.env_shade(*view, stack_envs(envs, "cuda"), torch.tensor(BG).cuda())
    calls = GB._record_ops(monkeypatch)
    without = s.capture_transfer(S, SEED)
    a = [c for c in calls if c in SCENE_OPS or isinstance(c, tuple)]
    del calls[:]
    zero = s.capture_transfer(S, SEED, bounces=0)
    b = [c for c in calls if c in SCENE_OPS or isinstance(c, tuple)]
    del calls[:]
    one = s.capture_transfer(S, SEED, bounces=1)
    c1 = [c for c in calls if c in SCENE_OPS or isinstance(c, tuple)]
    del calls[:]
    assert a == b == ["trace_batch_state_empty", "scene_occlusion_begin", ("march", True), "trace_batch_finish", "scene_transfer_resolve",
                      "scene_shade"]
    n_pad2 = s.bounce_hits["n_pad2"]
    assert c1 == ["trace_batch_state_empty", "scene_occlusion_begin", ("march", False), "trace_batch_finish", "scene_transfer_resolve",
                  "scene_bounce_nearest", "scene_bounce_visible"] + (["trace_batch_gather", "sdf_mlp_fwd"] if n_pad2 else []) + [
                      "scene_bounce_resolve", "scene_shade"]
    out0, outw = zero.shade(envs, BG), without.shade(envs, BG)
    assert [c for c in calls if c in SCENE_OPS] == ["env_shade", "env_shade"]
    del calls[:]
    out1 = one.shade(envs, BG)
    assert [c for c in calls if c in SCENE_OPS] == ["env_shade_bounce"]
    assert zero.bounce is None and biteq(zero.transfer.view(9, M), par["transfer"]) and biteq(without.transfer, zero.transfer)
    assert set(k for k in out0 if k in ops.ENV_BOUNCE_OUT) == {"shading", "image"} and "indirect" in out1
    for k in ("shading", "image"):
        assert biteq(out0[k].view(2, 3, M), want[k]) and biteq(outw[k], out0[k]), k
    assert zero.scene.stats()[0]["bounce_points"] == s.bounce_points and "bounce_points" in s.stats()[-1]


# ---------------------------------------------------------------------------------------------------------------------
# the analytic two-sphere scene through the C ABI's sequence, the analytic sdf in the march
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SB.AN_SAMPLES)
def test_analytic_two_sphere_scene(S):
    s = GL._AnalyticScene()
    s.field = None
    sc = s.sc
    cf = SR.analytic_closed_form(sc)
    a = GL.scene_arrays(s)
    E, n, M = 2, sum(s.n_vis), s.S * s.S
    pos, nrm, elem = s.world_points()
    elem_np, b2w = elem.cpu().numpy(), np.asarray(sc["b2w"], dtype=np.float64)
    albedo = torch.tensor(SB.AN_ALBEDO, dtype=torch.float32).cuda()

    def grad_rgb(points2):                                                    # the closed form at the library's own hit points
        return points2.contiguous(), albedo[:, None, :].expand(E, points2.shape[1], 3).contiguous()

    res = bounced(s, S, [S], march=lambda sb: s.march(sb, anyhit=False), grad_rgb=grad_rgb, seed=SB.AN_SEED)
    ch = res["chunks"][0]
    sb = ch["sb"]
    status = sb.status.cpu().numpy().reshape(E, S, n)
    assert set(np.unique(status)) <= {T.MISS, T.HIT, T.BACKFACING}
    # the kernel's own rays, taken to the world in float64
    o_own = npd(sb.rays_o).reshape(E, S, n, 3)[elem_np, :, np.arange(n)].transpose(1, 0, 2)
    d_own = npd(sb.rays_d).reshape(E, S, n, 3)[elem_np, :, np.arange(n)].transpose(1, 0, 2)
    o_w = np.einsum("nab,snb->sna", b2w[elem_np][:, :3, :3], o_own) + b2w[elem_np][None, :, :3, 3]
    d_w = np.einsum("nab,snb->sna", b2w[elem_np][:, :3, :3], d_own)
    facing = status[elem_np, :, np.arange(n)].T != T.BACKFACING
    t_cf = SB.sphere_hits(o_w, d_w)
    hit_cf = np.isfinite(t_cf).any(0) & facing
    w_cf = np.where(hit_cf, t_cf.argmin(0), -1)
    y = o_w + np.where(hit_cf, t_cf.min(0), 0.0)[..., None] * d_w
    ndd = np.where(hit_cf, (((y - SR.AN_CENTRES[w_cf.clip(0)]) / SR.RADIUS) * d_w).sum(-1), 0.0)
    _, band = SL.sphere_blocks(o_w, d_w)
    excluded = (band.any(0) & facing) | (hit_cf & (np.abs(ndd) < SB.NDD_EDGE))
    on, g = SL.pixel_points(a["owner"], a["owner_ray"], a["vis_slot"], a["offset"])
    keep_pt = np.zeros(n, dtype=bool)
    keep_pt[g] = ~cf["excluded"][on] & (cf["owner"][on] == a["owner"][on])
    share = float(excluded[facing].mean())
    assert share <= SB.EXCLUDED_CAP                                           # a condition on the scene (rehearsed on the CPU)
    winner = ch["winner"].cpu().numpy().reshape(S, n)
    cmp_ = keep_pt[None] & ~excluded & facing
    assert np.array_equal(winner[cmp_], w_cf[cmp_])
    assert (winner[~facing] == -1).all()
    # the hit points lie on the winning sphere
    tol_pt = T.TOL + 8 * EPS
    for e in range(E):
        r = np.linalg.norm(npd(ch["points"][e, :ch["n_sel"][e]]), axis=-1)
        assert np.abs(r - SR.RADIUS).max(initial=0.0) <= tol_pt, e
    # T1 against the restatement on the exact intersections of the closed form's points
    pts = SL.analytic_points(sc, cf)
    exact = SB.analytic_bounce(sc, pts, S, SB.AN_SEED)
    got = npd(res["bounce"])[:, :, pts["q"]]                                   # (3, 9, points)
    rho = SB.AN_ALBEDO[1 - pts["e"]]                                          # what a point can see is the other sphere (both are convex)
    bar = 5.0 * 0.5 * rho.T[:, None, :] * B.A_Y_MAX[None, :, None] / np.sqrt(S)
    err = np.abs(got - exact["T1"])
    worst = float((err / bar).max())
    won1 = (winner[:, elem_np == 0] == 1)
    print(f"scene_bounce analytic[S={S}]: points {n}, rays excluded {int(excluded.sum())} ({share:.5f}); sphere-0 rays won by sphere 1 "
          f"{int(won1.sum())} of {won1.size} ({won1.mean():.4f}); secondary points {ch['n_sel']}; worst T1 error / 5 standard errors {worst:.4f}")
    record_margin(f"scene_bounce_analytic[S={S}]", "T1_err_over_bar", worst)
    assert (err <= bar).all() and won1.mean() >= SL.BLOCKED_FLOOR
    # the red sphere colours the white one; nothing without a winner
    bo = npd(res["bounce"])
    has = np.zeros(M, dtype=bool)
    has[on] = (winner[:, g] >= 0).any(0)
    on0 = has & (a["owner"] == 0)
    assert on0.sum() > 10 and (bo[0, 0, on0] > bo[1, 0, on0]).all() and (bo[1, 0, on0] > 0).all()
    assert not res["bounce"][:, :, torch.as_tensor(~has).cuda()].view(torch.int32).any()


# ---------------------------------------------------------------------------------------------------------------------
# the golden pair
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_golden_pair(precision):
    from oi_amd import scene
    from oi_amd.envlight import EnvLight
    W, S = GL.GOLDEN_W, 16
    s = GS.traced(precision, "pair", W)
    a = GL.scene_arrays(s)
    E, n, M = s.E, sum(s.n_vis), s.S * s.S
    cap = s.capture_transfer(S, SEED, bounces=1)
    plain = s.capture_transfer(S, SEED)
    h, sb = s.bounce_hits, s.transfer_state
    assert h["chunk"] == S and sb.N == S * n                                  # one chunk holds the whole trace
    chunk = dict(winner=h["winner"].cpu().numpy().reshape(S, n), sel_slot=h["sel_slot"].cpu().numpy().reshape(E, S, n),
                 rays_d=npd(sb.rays_d).reshape(E, S, n, 3), grad2=npd(h["grad"]) if h["n_pad2"] else None,
                 rgb2=npd(h["rgb"]) if h["n_pad2"] else None)
    assert np.array_equal(chunk["winner"].reshape(-1), SB.winners(sb.status.cpu().numpy(), sb.t.cpu().numpy()))
    ref, mag, _, fronts = SB.resolve([chunk], a["owner"], a["owner_ray"], a["vis_slot"], a["offset"], a["w2b"], S)
    bar = SB.resolve_bar(mag, S)
    err = np.abs(npd(cap.bounce).reshape(3, 9, M) - ref)
    assert (err <= bar).all()
    if (bar > 0).any():
        record_margin(f"scene_bounce_golden_pair[{precision}]", "err_over_bar", float((err[bar > 0] / bar[bar > 0]).max()))
    # the field's own sdf at the secondary hit points
    n_sel = sb.counts[:, -1].tolist()
    assert h["n_pad2"] == max(n_sel) > 0 and s.stats()[0]["bounce_points"] >= sum(n_sel)
    sdf = s.field.full(h["points"].view(E * h["n_pad2"], 3))[0].view(E, h["n_pad2"])
    worst_sdf = max(float(sdf[e, :n_sel[e]].abs().max()) if n_sel[e] else 0.0 for e in range(E))
    print(f"scene_bounce golden pair[{precision}]: secondary points {n_sel}, largest |sdf| there {worst_sdf:.3g} (tol {s.kw[0]:.3g})")
    record_margin(f"scene_bounce_golden_pair[{precision}]", "sdf_over_tol", worst_sdf / s.kw[0])
    assert worst_sdf <= s.kw[0]
    # the shade: indirect >= 0, > 0 exactly where a front-face winner is; shading - indirect is the direct shade
    envs = [EnvLight.constant(1.0), EnvLight(np.random.RandomState(2).randn(9, 3) * 0.5 + np.eye(9)[0][:, None] * 3.0)]
    d0, d1 = plain.shade(envs, BG), cap.shade(envs, BG)
    D, I, Sh = npd(d0["shading"]), npd(d1["indirect"]), npd(d1["shading"])
    assert (np.abs((Sh - I) - D) <= EPS * (np.abs(D) + np.abs(I))).all()
    on, g = SL.pixel_points(a["owner"], a["owner_ray"], a["vis_slot"], a["offset"])
    lit = np.zeros(M, dtype=bool)
    lit[on] = fronts[0].any(0)
    ind = I[0].reshape(3, M)                                                  # the constant environment
    assert (ind >= 0).all() and (ind[:, lit] > 0).all() and not ind[:, ~lit].any()
    # each instance alone: what the other instance adds
    zs, b2ws = GS.instances("pair")
    pair_px = lit & (a["owner"] == 0)
    alone_s = scene.trace_scene(GS.make_gen(precision), zs[:1], b2ws[:1], window=W)
    alone = alone_s.capture_transfer(S, SEED, bounces=1)
    ia = npd(alone.shade(envs[:1], BG)["indirect"])[0].reshape(3, M)
    mine = (a["owner"] == 0) & (alone_s.owner.cpu().numpy() == 0)
    n_pair, n_alone = int((pair_px & mine).sum()), int(((ia > 0).any(0) & mine).sum())
    t_pair, t_alone = npd(plain.transfer).reshape(9, M)[0], npd(alone.transfer).reshape(9, M)[0]
    lost = int(((t_pair < t_alone) & mine).sum())
    one_s = scene.trace_scene(GS.make_gen(precision), zs[1:], b2ws[1:], window=W)
    i1 = npd(one_s.capture_transfer(S, SEED, bounces=1).shade(envs[:1], BG)["indirect"])[0].reshape(3, M)
    print(f"scene_bounce golden pair[{precision}]: pixels of instance 0 {int(mine.sum())}, with indirect light in the pair {n_pair}, alone "
          f"{n_alone}; losing direct transfer to instance 1 {lost}; instance 1 alone with indirect light {int((i1 > 0).any(0).sum())}")
    record_margin(f"scene_bounce_golden_pair[{precision}]", "instance0_pixels_with_indirect_pair", n_pair)
    record_margin(f"scene_bounce_golden_pair[{precision}]", "instance0_pixels_with_indirect_alone", n_alone)
    assert n_pair >= n_alone and (n_pair == 0 or lost > 0)


# ---------------------------------------------------------------------------------------------------------------------
# ragged scenes, walks, refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_scenes_and_walks(precision, monkeypatch):
    from oi_amd import inference, ops, scene
    from oi_amd import trace as tr
    from oi_amd.envlight import EnvLight
    gen = GS.make_gen(precision)
    W, S = 12, 4
    Sg = gen.scene_resolution
    M = Sg * Sg
    envs = [EnvLight.constant(1.0)]
    # an instance wholly outside the image changes nothing
    zs, b2ws = GS.instances("offscreen")
    off = scene.render_scene_env(gen, zs, b2ws, envs, transfer_samples=S, seed=SEED, bg=BG, window=W, bounces=1)
    alone = scene.render_scene_env(gen, zs[:1], b2ws[:1], envs, transfer_samples=S, seed=SEED, bg=BG, window=W, bounces=1)
    assert {"bounce", "indirect", "capture", "transfer", "scene"} <= set(off) and off["bounce"].shape == (1, 3, 9, Sg, Sg)
    assert off["indirect"].shape == (1, 3, Sg, Sg) and off["capture"].bounce is off["bounce"]
    for k in ("image", "shading", "indirect", "bounce", "transfer"):
        assert biteq(off[k], alone[k]), k
    assert off["scene"].n_vis[1] == 0
    # a scene without any hit: nothing launched, zeros
    zs0, b2ws0 = GS.instances("nothing")
    calls = GB._record_ops(monkeypatch)
    none = scene.render_scene_env(gen, zs0, b2ws0, envs, transfer_samples=S, seed=SEED, bg=BG, window=W, bounces=1)
    assert [c for c in calls if c in SCENE_OPS] == ["trace_batch_state_empty"]       # the primary batch; nothing after it
    sn = none["scene"]
    assert sn.n_pad == 0 and sn.transfer_state is None and sn.bounce_points == 0 and sn.transfer_evals == 0
    assert not bool(none["bounce"].any()) and not bool(none["indirect"].any()) and not bool(none["shading"].any())
    assert torch.equal(none["image"], torch.tensor(BG).cuda()[None, :, None, None].expand(1, 3, Sg, Sg))
    # a scene where nothing wins (one step of the march: no ray reaches a surface): n_pad2 = 0, no MLP pass, zeros
    s = copy.copy(GS.traced(precision, "pair", W))
    s.kw = (s.kw[0], s.kw[1], 1, s.kw[3])
    s.world_points()
    s.point_pixels()
    del calls[:]
    t0, b0 = s.transfer_bounce(S, SEED)
    seen = [c for c in calls if c in SCENE_OPS or isinstance(c, tuple)]
    assert seen == ["trace_batch_state_empty", "scene_occlusion_begin", ("march", False), "trace_batch_finish", "scene_transfer_resolve",
                    "scene_bounce_nearest", "scene_bounce_visible", "scene_bounce_resolve"]
    assert s.bounce_hits["n_pad2"] == 0 and s.bounce_hits["grad"] is None and not b0.view(torch.int32).any()
    assert not bool((s.transfer_state.status == T.HIT).any()) and bool((s.transfer_state.status == T.LIMIT).any())
    monkeypatch.undo()
    # the walk: three frames are three single shades
    zs, b2ws = GS.instances("pair")
    env = EnvLight(np.random.RandomState(4).randn(9, 3) * 0.4 + np.eye(9, 3))
    walk = inference.scene_env_walk(gen, zs, b2ws, env, n_frames=3, transfer_samples=S, seed=SEED, window=W, bg=BG, bounces=1)
    cap = GS.traced(precision, "pair", W).capture_transfer(S, SEED, bounces=1)
    assert walk["indirect"].shape == (3, 3, Sg, Sg) and biteq(walk["bounce"], cap.bounce) and biteq(walk["transfer"], cap.transfer)
    for f, Rm in enumerate(inference.env_walk_rotations(3, (0, 0, 1))):
        one = cap.shade(env.rotated(Rm), bg=BG)
        for k in ("image", "shading", "indirect"):
            assert biteq(one[k][0], walk[k][f]), (k, f)
    assert walk["stats"][0]["bounce_points"] > 0
    plainw = inference.scene_env_walk(gen, zs, b2ws, env, n_frames=3, transfer_samples=S, seed=SEED, window=W, bg=BG)
    assert "indirect" not in plainw and "bounce" not in plainw
    # 257 environments: split at 256, each part the unsplit launch of that part
    rs = np.random.RandomState(6)
    many = [EnvLight(rs.randn(9, 3) * 0.3 + np.eye(9, 3)) for _ in range(257)]
    launches = []
    shade = ops.env_shade_bounce

    def counting(*a_, **k_):
        launches.append(a_[6].shape[0])
        return shade(*a_, **k_)
    with monkeypatch.context() as m:
        m.setattr(ops, "env_shade_bounce", counting)
        allf = cap.shade(many, BG)
    assert launches == [256, 1]
    head, tail = cap.shade(many[:256], BG), cap.shade(many[256:], BG)
    for k in ("image", "shading", "indirect"):
        assert biteq(allf[k][:256], head[k]) and biteq(allf[k][256:], tail[k]), k


def test_c_abi_rejects_invalid_arguments_and_launches_nothing():
    """The refusals of tests/test_scene_bounce_cpu.py on real, poisoned device arrays: each returns a negative status with its
    text, and no array is touched."""
    from oi_amd import lib
    L = lib.load()
    E, N = 3, 24
    g = lambda sh, dt=torch.float32: guarded_empty(sh, dt, what="untouched", must_write=False)
    shapes = dict(rays_o=(E, N, 3), rays_d=(E, N, 3), near_=(E, N), far_=(E, N), t=(E, N), bracket=(E, N, 4), points=(E, N, 3))
    arr = {k: g(sh) for k, sh in shapes.items()}
    arr.update(status=g((E, N), torch.uint8), side=g((E, N), torch.uint8), steps=g((E, N), torch.int16),
               active=g((E, 2, N), torch.int32), counts=g((E, lib.TRACE_COUNT_WORDS), torch.int32))
    other = g((1024 * 8,))
    for call, entry, text in C.invalid_argument_cases(lib, L, p_(other), {k: p_(v) for k, v in arr.items()}):
        rc = call()
        msg = L.oi_last_error().decode()
        assert rc < 0 and msg.startswith(entry) and text in msg, (entry, text, rc, msg)
    torch.cuda.synchronize()
    for k, v in list(arr.items()) + [("other", other)]:
        fresh = guarded_empty(tuple(v.shape), v.dtype, what="pattern", must_write=False)
        assert torch.equal(v.view(torch.uint8), fresh.view(torch.uint8)), k
