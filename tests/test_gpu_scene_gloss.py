"""Glossy environment lighting in scenes on the MI355X (include/oi_scene_gloss.h; oi_amd.scene; oi_amd.inference.scene_env_walk;
DESIGN section 4.25): the reflection-lobe rays of every visible point against EVERY instance, the reflection plane and the
glossy shade along it.

Exact properties are checked bit for bit against the library's own single-view paths, which tests/test_gpu_envgloss.py holds
against the fp64 oracle: for E = 1 the statuses and evaluation counts against oi_occlusion_lobe_begin + the single any-hit
march, a split trace against the unsplit one, k_s = 0 against oi_env_shade, an F-launch against the 1-launches.  The layer's
own decisions -- the eye of every point, the rays in every element, the cull, the plane, the shade with given directions --
are checked against the float64 restatement of tests/helpers/scene_gloss_ref.py, which touches no code under test.

Bars (EPS = 2^-24), each one a neighbouring file derives:
  LOBE DIRECTIONS  64 EPS in the owner's frame against the restatement fed the kernel's own float32 points, gradients and eyes
                   (tests/test_gpu_envgloss.py's DIR_BAR for the same __device__ function); statuses and entered sets exact
                   outside |n . d| <= 64 EPS and outside the CULL edge; both exclusions together at most 2 % of a case's rays.
  MOVED RAYS       1e-6 for the origins and directions in the other elements, against the restatement fed the kernel's own
                   owner-frame directions (tests/test_gpu_scene_light.py's DIRECTIONS bar).
  CULL             tests/test_gpu_scene_light.py's edge: |c2 - 1| <= 4 EPS (|o|^2 + 1).
  PLANE            64 EPS against the restatement; unit length within 8 EPS on the mask; zeros off it.
  SHADE            tests/test_gpu_envgloss.py's bar with C = 64: |k_s V| (coordinate error x the map's largest adjacent-texel
                   difference + 8 EPS max |g|); shading 16 EPS x the diffuse magnitude.
  ANALYTIC         per ray "escaped every instance" against ray-against-sphere in float64 on the kernel's own rays taken to the
                   world, outside the band |closest approach - 0.5| < 1e-3: exact; at most 1 % of the facing rays in the band."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_scene as GS
import test_gpu_scene_light as GL
import test_gpu_trace as G
import test_scene_gloss_cpu as C
from conftest import record_margin
from helpers import env_ref as EV
from helpers import envgloss_ref as Q
from helpers import occlusion_ref as R
from helpers import scene_gloss_ref as SG
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T
from helpers.guarded import guarded_empty, guarded_ops  # noqa: F401  (fixture)
from test_gpu_trace_batch import biteq

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS, npd = G.PRECISIONS, G.npd
EPS = 2.0 ** -24
DIR_BAR = 64 * EPS
COORD_C = 64.0
SEED = SL.SEED
KS = (0.3, 0.2, 0.1)
BG = (0.1, 0.2, 0.3)
CUTS = {1: [[1]], 4: [[4], [1, 1, 1, 1], [1, 3]]}


def lobe_begin(s, sb, S, j0, c, shin, seed=SEED):
    from oi_amd import ops
    pos, nrm, elem = s.world_points()
    ops.scene_lobe_begin(sb, s.state.rays_o, s.vis_index, s.N, s.points, s.grad, s.n_pad, s.offset, elem, s.point_pixels(), pos, nrm,
                         sum(s.n_vis), s.w2b, s.bias, S, j0, c, shin, seed)


def lobe_sampled(s, S, cuts, shin, march=None, seed=SEED):
    """The sequence of include/oi_scene_gloss.h through the ops wrappers, chunk by chunk.  -> dict: chunks, count, out."""
    from oi_amd import ops, trace
    pos = s.world_points()[0]
    n_vis, M = sum(s.n_vis), s.S * s.S
    count, out = ops._new(pos, 1, M).view(torch.int32), ops._new(pos, 1, M)
    chunks, j0 = [], 0
    for c in cuts:
        sb = ops.trace_batch_state_empty(s.E, c * n_vis, pos)
        lobe_begin(s, sb, S, j0, c, shin, seed)
        bound = int(sb.live[0].item())
        if bound:
            if march is None:
                trace._march_batch(s.field, sb, *s.kw, bound=bound, anyhit=True)
            else:
                march(sb)
            ops.trace_batch_finish(sb)
        ops.scene_occlusion_resolve(sb.status, s.owner, s.owner_ray, s.vis_slot, s.offset, s.E, s.N, 1, S, j0, c, n_vis, s.S, count, out,
                                    j0 + c == S)
        chunks.append(sb)
        j0 += c
    return dict(chunks=chunks, count=count, out=out)


def point_eyes(s):
    a = GL.scene_arrays(s)
    return SG.point_eyes(npd(s.state.rays_o), s.vis_index.cpu().numpy(), a["offset"], s.world_points()[2].cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shin", [1.0, 10.0, 200.0])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W", [("pair", 9), ("triple", 12), ("single", 9), ("twice", 12)])
def test_rays_in_every_element(precision, kind, W, shin):
    """Every chunk of every cut of S = 1 and S = 4 samples of oi_scene_lobe_begin against the restatement: the owner's
    directions drawn from the kernel's float32 points, gradients and eyes, then every element's ray, cull and state from the
    kernel's own directions; the compaction within each element."""
    from oi_amd import lib, ops
    s = GS.traced(precision, kind, W)
    pos, nrm, elem = s.world_points()
    n, E = sum(s.n_vis), s.E
    a = GL.scene_arrays(s)
    elem_np, pix = elem.cpu().numpy(), s.point_pixels().cpu().numpy()
    eyes = point_eyes(s)
    pts64, grad64 = npd(s.points), npd(s.grad)
    nrm_own = SL.unit(grad64)[elem_np, np.arange(n) - a["offset"][elem_np]]
    worst = dict(d=0.0, o=0.0, dd=0.0, excluded=0.0)
    for S, cuts in CUTS.items():
        for cut in cuts:
            j0 = 0
            for c in cut:
                sb = ops.trace_batch_state_empty(E, c * n, pos)
                lobe_begin(s, sb, S, j0, c, shin)
                o, d = npd(sb.rays_o).reshape(E, 1, c, n, 3), npd(sb.rays_d).reshape(E, 1, c, n, 3)
                near, far = npd(sb.near).reshape(E, 1, c, n), npd(sb.far).reshape(E, 1, c, n)
                status = sb.status.cpu().numpy().reshape(E, 1, c, n)
                d_own = d[elem_np, :, :, np.arange(n)].transpose(1, 2, 0, 3)      # the owner's element holds the drawn direction
                drawn, _, refl = SG.owner_lobe_directions(pts64, grad64, eyes, a["offset"], elem_np, pix, S, j0, c, shin, SEED)
                worst["d"] = max(worst["d"], float(np.abs(d_own - drawn).max()))
                assert np.abs(np.linalg.norm(d_own, axis=-1) - 1).max() <= DIR_BAR
                # every element's ray from the kernel's own directions
                r = SG.lobe_rays(pts64, grad64, eyes, a["offset"], elem_np, pix, npd(pos), npd(nrm), a["w2b"], s.bias, S, j0, c, shin, SEED,
                                 d_owner=d_own)
                ndd = (nrm_own[None, None] * d_own).sum(-1)
                sure = np.abs(ndd) > DIR_BAR                                      # n . d decided in float32 as in float64
                back = status == T.BACKFACING
                assert np.array_equal(back.all(0), back.any(0))                   # facing away: BACKFACING in every element
                assert np.array_equal(back[0][sure], ~r["traced"][sure])
                assert set(np.unique(status)) <= {T.MARCH, T.MISS, T.BACKFACING} and not sb.steps.any()
                edge = np.abs(r["c2"] - 1) <= 4 * EPS * ((r["o"] ** 2).sum(-1) + 1)
                mine = np.broadcast_to((elem_np[None] == np.arange(E)[:, None])[:, None, None, :], status.shape)
                edge &= ~mine                                                     # the owner's ray is never culled
                cmp_ = sure[None] & ~edge
                entered = status == T.MARCH
                assert np.array_equal(entered[cmp_], (r["status"] == SL.MARCH)[cmp_])
                worst["excluded"] = max(worst["excluded"], float((~cmp_).mean()))
                other = cmp_ & ~mine & ~back
                worst["o"] = max(worst["o"], float(np.abs(o - r["o"])[other].max(initial=0.0)))
                worst["dd"] = max(worst["dd"], float(np.abs(d - r["d"])[other].max(initial=0.0)))
                own = cmp_ & mine
                assert float(np.abs(o - r["o"])[own].max()) <= 1e-6 and float(np.abs(d - r["d"])[own].max()) == 0
                both = cmp_ & entered
                tol = 1e-5 / np.sqrt(np.maximum(1 - r["c2"][both], 1e-4))
                assert (np.abs(near[both] - r["near"][both]) <= tol).all() and (np.abs(far[both] - r["far"][both]) <= tol).all()
                assert not near[~entered].any() and not far[~entered].any()
                assert not near[mine].any() and entered[mine & ~back].all()       # the owner's own ray: near 0, always entered
                # the state: oi_scene_occlusion_begin's
                counts, live = sb.counts.cpu().numpy(), sb.live.cpu().numpy()
                flat = entered.reshape(E, -1)
                t, br = npd(sb.t), npd(sb.bracket)
                assert np.array_equal(t, npd(sb.near)) and np.array_equal(br[..., 0], t) and not br[..., 1].any() and not sb.side.any()
                for e in range(E):
                    n_ent = int(flat[e].sum())
                    assert counts[e, 0] == n_ent and not counts[e, 1:].any()
                    act = sb.active[e, 0, :n_ent].cpu().numpy()
                    assert sorted(act.tolist()) == np.nonzero(flat[e])[0].tolist()
                    p = npd(sb.points[e])
                    expect = npd(sb.rays_o[e])[act] + npd(sb.near[e])[act, None] * npd(sb.rays_d[e])[act]
                    assert np.abs(p[:n_ent] - expect).max(initial=0.0) <= 1e-6 and not p[n_ent:].any()
                assert live[0] == counts[:, 0].max() and not live[1:].any() and len(live) == lib.TRACE_COUNT_WORDS
                j0 += c
    case = f"scene_lobe_rays[{precision},{kind},W={W},s={shin:g}]"
    print(case, f"n_vis {n}: owner directions {worst['d']:.3g} (bar {DIR_BAR:.3g}), moved origins {worst['o']:.3g}, moved directions "
          f"{worst['dd']:.3g} (bar 1e-6), largest share of a chunk's rays inside an exclusion {worst['excluded']:.4f}")
    record_margin(case, "direction_err_over_bar", worst["d"] / DIR_BAR)
    record_margin(case, "moved_origin_err_over_bar", worst["o"] / 1e-6)
    record_margin(case, "moved_direction_err_over_bar", worst["dd"] / 1e-6)
    record_margin(case, "excluded_share", worst["excluded"])
    assert worst["d"] <= DIR_BAR and worst["o"] <= 1e-6 and worst["dd"] <= 1e-6
    assert worst["excluded"] <= 0.02


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("W", [9, 12])
def test_one_instance_equals_the_single_view_path(precision, W):
    """E = 1: statuses and evaluation counts are oi_occlusion_lobe_begin's followed by the single any-hit march on the owner's
    slices with hit_index = pixel and the eyes listed by scene pixel; V_spec is oi_occlusion_resolve's."""
    from oi_amd import ops, trace
    s = GS.traced(precision, "single", W)
    n, S, shin, M = s.n_vis[0], 4, 10.0, s.S * s.S
    assert s.E == 1 and n > 0
    pixel = s.point_pixels()
    pts, grad = s.points[0, :n].contiguous(), s.grad[0, :n].contiguous()
    eyes = torch.zeros(M, 3, device="cuda")
    eyes[pixel.long()] = s.state.rays_o[0][s.vis_index[0, :n].long()]
    hit_slot = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    hit_slot[pixel.long()] = torch.arange(n, dtype=torch.int32, device="cuda")
    lob = lobe_sampled(s, S, [S], shin)
    one = ops.TraceState(S * n, ref=s.points)
    ops.occlusion_lobe_begin(one, eyes, pts, grad, pixel, n, S, shin, s.bias, SEED)
    trace._march(s.field, one, int(one.counts[0].item()), *s.kw, anyhit=True)
    ops.trace_finish(one)
    sb = lob["chunks"][0]
    assert torch.equal(sb.status[0], one.status) and torch.equal(sb.steps[0], one.steps)
    close = lambda x, y: float((x - y).abs().max()) <= 1e-6
    traced_ = one.status != T.BACKFACING                                   # (a ray facing away keeps far = 0 in a scene)
    assert close(sb.rays_o[0], one.rays_o) and close(sb.rays_d[0], one.rays_d) and close(sb.far[0][traced_], one.far[traced_])
    seen = set(np.unique(one.status.cpu().numpy()).tolist())
    assert {T.MISS, T.BACKFACING} <= seen
    assert biteq(lob["out"], ops.occlusion_resolve(one.status, hit_slot, M, n, 1, S))


# ---------------------------------------------------------------------------------------------------------------------
# chunks, the plane
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,W", [("pair", 9), ("triple", 12)])
def test_chunks_and_the_reflection_plane(precision, kind, W):
    from oi_amd import ops
    s = GS.traced(precision, kind, W)
    a = GL.scene_arrays(s)
    E, n, M, S, shin = s.E, sum(s.n_vis), s.S * s.S, 4, 10.0
    off = a["owner"] < 0
    whole = None
    for cuts in CUTS[S]:
        res = lobe_sampled(s, S, cuts, shin)
        count, out = SL.counts([GL.shaped(sb, E, 1, c, n) for sb, c in zip(res["chunks"], cuts)], a["owner"], a["owner_ray"], a["vis_slot"],
                               a["offset"], S)
        assert np.array_equal(res["count"].cpu().numpy(), count) and np.array_equal(npd(res["out"]), out)
        assert (npd(res["out"])[:, off] == 1).all() and not res["count"].cpu().numpy()[:, off].any()
        if whole is None:
            whole = res
        else:
            assert biteq(res["out"], whole["out"]) and torch.equal(res["count"], whole["count"]), cuts
    v = npd(whole["out"])[0, ~off]
    assert 0 < v.mean() < 1 and set(np.unique(v)) <= {float(np.float32(k) / np.float32(S)) for k in range(S + 1)}
    before = s.glossy_evals
    vis = s.lobe_visibility(S, shin, SEED)
    assert biteq(vis, whole["out"].view(-1)) and s.glossy_evals > before and s.glossy_state.N == S * n
    assert biteq(s.lobe_visibility(S, shin, SEED, max_shadow_rays=E * n * (S - 1)), vis)      # chunks of S - 1 and 1
    assert biteq(s.lobe_visibility(S, shin, SEED, max_shadow_rays=E * n), vis)                # one sample per chunk
    # the plane
    plane = s.reflection()
    assert plane is s.reflection() and plane.shape == (M, 3)
    assert biteq(plane, ops.scene_reflect(s.state.rays_o, s.points, s.grad, s.n_pad, s.owner, s.owner_ray, s.vis_slot, s.w2b, E, s.N, s.S))
    ref = SG.reflection(npd(s.state.rays_o), npd(s.points), npd(s.grad), a["owner"], a["owner_ray"], a["vis_slot"], a["w2b"])
    got = npd(plane)
    err = float(np.abs(got - ref).max())
    length = float(np.abs(np.linalg.norm(got[~off], axis=-1) - 1).max())
    case = f"scene_reflect[{precision},{kind},W={W}]"
    print(case, "error", err, "bar", DIR_BAR, "unit length", length, "bar", 8 * EPS)
    record_margin(case, "err_over_bar", err / DIR_BAR)
    record_margin(case, "length_err_over_bar", length / (8 * EPS))
    assert err <= DIR_BAR and not got[off].any() and length <= 8 * EPS


# ---------------------------------------------------------------------------------------------------------------------
# the shade with given directions
# ---------------------------------------------------------------------------------------------------------------------
def _coordinate_error(d, mask, Hp, Wp):
    """tests/test_gpu_envgloss.py's bound (F, N) in texels for directions d (F, N, 3) within COORD_C EPS of the exact ones."""
    err = np.zeros(d.shape[:2])
    sin_t = np.sqrt(np.minimum(np.maximum(1.0 - np.clip(d[..., 2], -1, 1) ** 2, 0.0), d[..., 0] ** 2 + d[..., 1] ** 2))
    c = COORD_C * EPS
    with np.errstate(divide="ignore"):
        dth, dph = np.minimum(c / sin_t, np.sqrt(2 * c)), np.minimum(c / sin_t, np.pi)
    err[:, mask] = (Hp * dth / np.pi + Wp * dph / (2 * np.pi))[:, mask]
    return err


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 130])
def test_env_shade_glossy_dirs(N, F):
    from oi_amd import ops
    cu = lambda x, dt=torch.float32: torch.tensor(np.asarray(x), dtype=dt).cuda().contiguous()
    for n_hit in sorted({0, max(1, N // 2), N}):
        rs = np.random.RandomState(N * 100 + F * 10 + n_hit)
        mask = np.zeros(N, dtype=bool)
        mask[rs.permutation(N)[:n_hit]] = True
        slot = np.where(mask, np.arange(N), -1)                               # a scene's planes: a pixel is its own hit
        tr, env = rs.randn(9, N).astype(np.float32), (rs.randn(F, 9, 3) * 0.5).astype(np.float32)
        alb, vis = rs.rand(N, 3).astype(np.float32), rs.rand(N).astype(np.float32)
        dirs = rs.randn(N, 3)
        dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
        dirs[~mask] = 0
        maps = rs.randn(2, 3, 5, 9).astype(np.float32)
        index = [int(v) for v in rs.randint(0, 2, F)]
        rot = np.stack([EV.random_rotation(rs) for _ in range(F)]).astype(np.float32)
        ks, bg = np.float32(KS), np.float32(BG)
        d = dict(status=cu(mask * T.HIT, torch.uint8), slot=cu(slot, torch.int32), rgb=cu(alb), tr=cu(tr), dirs=cu(dirs), vis=cu(vis),
                 maps=cu(maps), ks=cu(ks), bg=cu(bg))
        run = lambda envs=env, rot_=rot, idx=index, ks_=d["ks"], vis_=d["vis"], **kw: ops.env_shade_glossy_dirs(
            d["status"], d["slot"], d["rgb"], N, d["tr"], cu(envs), d["dirs"], vis_, d["maps"], idx, cu(rot_), ks_, d["bg"], **kw)
        out = run()
        f64 = lambda x: np.asarray(x, dtype=np.float64)
        sh, img, spec, mag, look, dd = SG.shade_dirs(f64(tr), f64(env), mask, f64(alb), f64(dirs), f64(vis), f64(maps), index, f64(rot),
                                                     f64(ks), f64(bg))
        delta = np.array([Q.adjacent_difference(maps[m]).max() for m in index])
        gmax = np.array([np.abs(maps[m]).max() for m in index])
        kv = np.abs(f64(ks))[None, :, None] * f64(vis)[None, None, :]
        bar_spec = kv * (_coordinate_error(dd, mask, 5, 9)[:, None, :] * delta[:, None, None] + 8 * EPS * gmax[:, None, None])
        bar_sh = 16 * EPS * mag
        e_spec, e_sh, e_img = np.abs(npd(out["specular"]) - spec), np.abs(npd(out["shading"]) - sh), np.abs(npd(out["image"]) - img)
        if n_hit:
            record_margin(f"env_shade_glossy_dirs[N={N},F={F}]", "specular_err_over_bar", float((e_spec / bar_spec)[:, :, mask].max()))
        assert (e_spec[:, :, mask] <= bar_spec[:, :, mask]).all() and (e_sh <= bar_sh).all()
        assert (e_img[:, :, mask] <= (bar_spec + bar_sh + 2 * EPS * np.abs(img))[:, :, mask]).all()
        off = ~mask
        assert not npd(out["shading"])[:, :, off].any() and not npd(out["specular"])[:, :, off].any()
        assert np.array_equal(npd(out["image"])[:, :, off], np.broadcast_to(f64(bg)[None, :, None], (F, 3, int(off.sum()))))
        for k in ("shading", "image", "specular"):                             # any output may be absent
            assert biteq(run(outputs=(k,))[k], out[k]), k
        for f in range(F):                                                     # result f is the 1-launch of environment f
            one = run(envs=env[f:f + 1], rot_=rot[f:f + 1], idx=index[f:f + 1])
            for k in out:
                assert biteq(one[k][0], out[k][f]), (k, f)
        zero = run(ks_=cu(np.zeros(3)))                                        # k_s = 0: oi_env_shade's bytes
        plain = ops.env_shade(d["status"], d["slot"], d["rgb"], N, d["tr"], cu(env), d["bg"])
        assert biteq(zero["image"], plain["image"]) and biteq(zero["shading"], plain["shading"]) and biteq(out["shading"], plain["shading"])
        assert not bool(zero["specular"].any())
        ones = run(vis_=torch.ones(N, device="cuda"))
        none = run(vis_=None)                                                  # spec_vis = NULL is a map of ones
        for k in out:
            assert biteq(ones[k], none[k]), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_scene_shade_under_maps(precision):
    """SceneTransfer.shade with EnvMaps: environment f of an F-launch is the 1-launch; 258 environments are two launches; bg off
    the mask and no specular there; under a constant map the specular is (k_s V_spec) g formed in float32, bit for bit; with
    k_s = 0 and with EnvLights the bytes are the diffuse path's."""
    from oi_amd import scene
    from oi_amd.envlight import EnvMap, stack_maps
    s = GS.traced(precision, "pair", 9)
    S, M, shin = s.S, s.S * s.S, 10.0
    cap = s.capture_transfer(4, SEED, glossy_samples=4, shininess=shin)
    assert isinstance(cap, scene.SceneTransfer) and cap.glossy_samples == 4 and cap.shininess == shin
    assert cap.spec_visibility.shape == (1, 1, S, S) and cap.reflection.shape == (1, 3, S, S)
    assert biteq(cap.spec_visibility.reshape(-1), s.lobe_visibility(4, shin, SEED))
    assert torch.equal(cap.reflection[0].permute(1, 2, 0).reshape(M, 3), s.reflection())
    rs = np.random.RandomState(3)
    img = (rs.rand(3, 8, 16) * 2.0).astype(np.float32)
    img[:, 2:4, 3:6] += 20.0
    m = EnvMap.from_equirect(img, shin, size=(6, 12))
    envs = [m, m.rotated(EV.random_rotation(rs)), m.rotated(EV.random_rotation(rs))]
    on = s.owner >= 0
    out = cap.shade(envs, bg=BG, specular=KS)
    assert out["image"].shape == out["shading"].shape == out["specular"].shape == (3, 3, S, S) and out["instance"].dtype == torch.int32
    for f, env in enumerate(envs):
        alone = cap.shade(env, bg=BG, specular=KS)
        for k in ("image", "shading", "specular"):
            assert biteq(alone[k][0], out[k][f]), (k, f)
    many = cap.shade([envs[f % 3] for f in range(258)], bg=BG, specular=KS)           # two launches
    for k in ("image", "specular"):
        assert biteq(many[k][257], out[k][257 % 3]) and biteq(many[k][255], out[k][255 % 3]), k
    assert not bool(out["specular"].view(3, 3, M)[:, :, ~on].any()) and bool(out["specular"].view(3, 3, M)[:, :, on].any())
    assert torch.equal(out["image"].view(3, 3, M)[:, :, ~on], torch.tensor(BG).cuda()[None, :, None].expand(3, 3, int((~on).sum())))
    # the diffuse half is the EnvLight path's, and k_s = 0 gives its image
    plain = cap.shade([e.sh for e in envs], bg=BG)
    zero = cap.shade(envs, bg=BG, specular=0.0)
    assert biteq(plain["shading"], out["shading"]) and biteq(zero["image"], plain["image"]) and "specular" not in plain
    assert biteq(plain["image"], s.capture_transfer(4, SEED).shade([e.sh for e in envs], bg=BG)["image"])
    # against the restatement fed the kernel's own plane and V_spec
    _, maps, index, rot, _ = stack_maps(envs)
    sh, im, spec, mag, look, dd = SG.shade_dirs(npd(cap.transfer.view(9, M)), np.stack([e.sh.coeffs for e in envs]), on.cpu().numpy(),
                                                npd(out["albedo"][0].reshape(3, M).t()), npd(s.reflection()),
                                                npd(cap.spec_visibility.reshape(-1)), npd(maps), index, npd(rot), np.float32(KS), BG)
    onn = on.cpu().numpy()
    delta, gmax = Q.adjacent_difference(npd(maps[0])).max(), np.abs(npd(maps[0])).max()
    kv = np.abs(np.float32(KS).astype(np.float64))[None, :, None] * npd(cap.spec_visibility.reshape(-1))[None, None, :]
    bar = kv * (_coordinate_error(dd, onn, 6, 12)[:, None, :] * delta + 8 * EPS * gmax)
    e_spec = np.abs(npd(out["specular"].view(3, 3, M)) - spec)
    record_margin(f"scene_shade_glossy[{precision}]", "specular_err_over_bar", float((e_spec / bar)[:, :, onn].max()))
    assert (e_spec[:, :, onn] <= bar[:, :, onn]).all()
    # a constant map: a bilinear lerp of equal texels is exact
    c = EnvMap.constant((0.2, 0.5, 1.0), shin)
    got = cap.shade([c], bg=BG, specular=KS)["specular"][0].view(3, M)
    g = c.map.view(3).cuda()
    want = (torch.tensor(KS).cuda()[:, None] * cap.spec_visibility.reshape(1, M)) * g[:, None]
    assert biteq(got[:, on], want[:, on])


# ---------------------------------------------------------------------------------------------------------------------
# between instances
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_reflection_occlusion_on_the_golden_pair(precision):
    """Adding instance 1 never raises the reflection-lobe visibility of a pixel instance 0 owns in both renders (exact: the
    owner's own rays are the same rays, and an instance can only block).  How many pixels it lowers is recorded, not asserted."""
    from oi_amd import scene
    from oi_amd.envlight import EnvMap
    W = GL.GOLDEN_W
    gen = GS.make_gen(precision)
    zs, b2ws = GS.instances("pair")
    env = [EnvMap.constant(1.0, 1.0)]
    kw = dict(transfer_samples=4, seed=SEED, window=W, glossy_samples=16, shininess=1.0)
    both = scene.render_scene_env(gen, zs, b2ws, env, **kw)
    alone = scene.render_scene_env(gen, zs[:1], b2ws[:1], env, **kw)
    mine = (both["instance"] == 0) & (alone["instance"] == 0)
    vb, va = both["spec_visibility"][mine], alone["spec_visibility"][mine]
    lower = int((vb < va).sum())
    print(f"scene_gloss golden pair[{precision}]: pixels of instance 0 {int(mine.sum())}, with a lower reflection-lobe visibility beside "
          f"instance 1: {lower}")
    record_margin(f"scene_gloss_golden_pair[{precision}]", "pixels_lowered", lower)
    assert int(mine.sum()) > 0 and int((vb > va).sum()) == 0


class _AnalyticLobeScene(GL._AnalyticScene):
    """tests/test_gpu_scene_light.py's analytic two-sphere scene; lobe_sampled reads the same attributes."""


@pytest.mark.parametrize("shin", SG.AN_SHININESS)
def test_analytic_two_sphere_scene(shin):
    s = _AnalyticLobeScene()
    sc = s.sc
    cf = SR.analytic_closed_form(sc)
    a = GL.scene_arrays(s)
    E, n, M, S = 2, sum(s.n_vis), s.S * s.S, SG.AN_S
    pos, nrm, elem = s.world_points()
    elem_np, b2w = elem.cpu().numpy(), np.asarray(sc["b2w"], dtype=np.float64)
    on, g = SL.pixel_points(a["owner"], a["owner_ray"], a["vis_slot"], a["offset"])
    keep_px = np.zeros(M, dtype=bool)
    keep_px[on] = ~cf["excluded"][on] & (cf["owner"][on] == a["owner"][on])
    res = lobe_sampled(s, S, [S], shin, march=s.march)
    sb = res["chunks"][0]
    status = GL.shaped(sb, E, 1, S, n)
    assert set(np.unique(status)) <= {T.MISS, T.HIT, T.BACKFACING}
    o_own = npd(sb.rays_o).reshape(E, 1, S, n, 3)[elem_np, 0, :, np.arange(n)].transpose(1, 0, 2)      # (S, n, 3)
    d_own = npd(sb.rays_d).reshape(E, 1, S, n, 3)[elem_np, 0, :, np.arange(n)].transpose(1, 0, 2)
    o_w = np.einsum("nab,snb->sna", b2w[elem_np][:, :3, :3], o_own) + b2w[elem_np][None, :, :3, 3]
    d_w = np.einsum("nab,snb->sna", b2w[elem_np][:, :3, :3], d_own)
    blocked, band = SL.sphere_blocks(o_w, d_w)
    facing = status[elem_np, 0, :, np.arange(n)].T != T.BACKFACING                                       # (S, n)
    ndd = (npd(nrm)[None] * d_w).sum(-1)
    sure = np.abs(ndd) > SG.NDD_EDGE
    assert np.array_equal(facing[sure], (ndd > 0)[sure])
    free_cf = facing & ~blocked.any(0)
    in_band = band.any(0) & facing
    free = SL.escaped(status)[0]
    kept = np.broadcast_to(keep_px[on][None], (S, len(on)))
    cmp_ = kept & ~in_band[:, g]
    share_excluded = float(in_band[:, g][kept].sum() / max(1, facing[:, g][kept].sum()))
    assert share_excluded <= R.EXCLUDED_CAP                                  # a condition on the scene (rehearsed on the CPU)
    assert np.array_equal(free[:, g][cmp_], free_cf[:, g][cmp_])
    clean = keep_px[on] & ~in_band[:, g].any(0)                              # pixels none of whose rays is in the band
    q = on[clean]
    on0 = clean & (a["owner"][on] == 0)
    by_other = (blocked[1] & facing)[:, g][:, on0]
    f0 = facing[:, g][:, on0]
    print(f"scene_gloss analytic[s={shin:g}]: points {n}, pixels compared {int(clean.sum())}, facing rays in the band "
          f"{int(in_band[:, g][kept].sum())} ({share_excluded:.5f}), sphere-0 facing rays blocked by sphere 1 {int(by_other.sum())} of "
          f"{int(f0.sum())}")
    record_margin(f"scene_gloss_analytic[s={shin:g}]", "band_share", share_excluded)
    assert by_other.sum() / f0.sum() >= SG.BLOCKED_FLOOR
    share = (free_cf[:, g][:, clean].sum(0).astype(np.float32) / np.float32(S)).astype(np.float64)
    assert np.array_equal(npd(res["out"])[0, q], share)
    alone = (facing & ~blocked[0])[:, g][:, clean].sum(0) / S                # with sphere 1 removed
    assert (share[a["owner"][q] == 0] < alone[a["owner"][q] == 0]).any()
    # the plane of the analytic scene: the mirror direction of the camera ray about the sphere's normal
    from oi_amd import ops
    plane = npd(ops.scene_reflect(s.state.rays_o, s.points, s.grad, s.n_pad, s.owner, s.owner_ray, s.vis_slot, s.w2b, E, s.N, s.S))
    _, eye_w = SG.analytic_eyes(sc, dict(w2b=np.stack([SR.rigid_inverse(m) for m in sc["b2w"]]), e=elem_np))
    p_w, n_w = npd(pos)[g], npd(nrm)[g]
    v = SL.unit(eye_w[None] - p_w)
    want = 2.0 * (n_w * v).sum(-1, keepdims=True) * n_w - v
    assert np.abs(plane[on] - want).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# ragged scenes, the public entries, the refusals on device memory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_and_empty_scenes(precision, monkeypatch):
    from oi_amd import ops, scene
    from oi_amd.envlight import EnvMap
    gen = GS.make_gen(precision)
    W, S, shin = 12, gen.scene_resolution, 10.0
    envs = [EnvMap.constant((0.2, 0.5, 1.0), shin)]
    kw = dict(transfer_samples=4, seed=SEED, bg=BG, window=W, glossy_samples=4, shininess=shin, specular=KS)
    zs, b2ws = GS.instances("offscreen")
    off = scene.render_scene_env(gen, zs, b2ws, envs, **kw)
    alone = scene.render_scene_env(gen, zs[:1], b2ws[:1], envs, **kw)
    for k in ("image", "shading", "specular", "spec_visibility", "reflection", "instance"):
        assert biteq(off[k].contiguous(), alone[k].contiguous()), k
    so = off["scene"]
    assert so.n_vis[1] == 0 and so.glossy_state.E == 2 and not bool(so.glossy_state.steps[1].any())
    zs, b2ws = GS.instances("nothing")
    none = scene.render_scene_env(gen, zs, b2ws, envs, **kw)
    sn = none["scene"]
    assert sn.n_pad == 0 and sn.glossy_state is None and sn.glossy_evals == 0
    assert torch.equal(none["image"], torch.tensor(BG).cuda()[None, :, None, None].expand(1, 3, S, S))
    assert not bool(none["specular"].any()) and not bool(none["shading"].any()) and bool((none["spec_visibility"] == 1).all())
    assert not bool(none["reflection"].any()) and bool((none["instance"] == -1).all())
    # glossy_samples = 0: no lobe trace, V_spec = 1

    def refuse(*a_, **k_):
        raise AssertionError("a reflection-lobe trace ran without glossy samples")
    monkeypatch.setattr(ops, "scene_lobe_begin", refuse)
    s = GS.traced(precision, "pair", W)
    before = s.glossy_evals
    zero = s.capture_transfer(4, SEED, glossy_samples=0, shininess=shin)
    old = s.capture_transfer(4, SEED)
    monkeypatch.undo()
    assert zero.spec_visibility is None and zero.glossy_samples == 0 and s.glossy_evals == before and old.glossy_samples is None
    assert biteq(zero.transfer, old.transfer)
    flat = zero.shade(envs, specular=KS)["specular"][0].view(3, -1)
    want = torch.tensor(KS).cuda()[:, None] * envs[0].map.view(3, 1).cuda()
    on = s.owner >= 0
    assert biteq(flat[:, on], want.expand(3, int(on.sum())).contiguous()) and not bool(flat[:, ~on].any())
    with pytest.raises(ValueError, match="no reflection-lobe trace"):
        old.shade(envs)
    with pytest.raises(ValueError, match="shininess"):
        zero.shade([EnvMap.constant(1.0, 20.0)])
    with pytest.raises(ValueError, match="EnvLight objects only"):
        zero.shade(["sky"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_public_entries(precision, monkeypatch):
    from oi_amd import inference, ops, scene
    from oi_amd.envlight import EnvMap
    gen = GS.make_gen(precision)
    zs, b2ws = GS.instances("pair")
    s = GS.traced(precision, "pair", 12)
    S, shin = gen.scene_resolution, 10.0
    rs = np.random.RandomState(2)
    img = (rs.rand(3, 16, 32) * 2.0).astype(np.float32)
    img[:, 4:7, 5:9] += 20.0                                                  # a bright window: the walk is not symmetric
    env = EnvMap.from_equirect(img, shin, size=(8, 16))
    cap = s.capture_transfer(4, SEED, glossy_samples=4, shininess=shin)
    one = cap.shade([env], bg=BG, specular=KS)
    res = scene.render_scene_env(gen, zs, b2ws, [env], transfer_samples=4, seed=SEED, bg=BG, window=12, glossy_samples=4, shininess=shin,
                                 specular=KS)
    for k in ("image", "shading", "specular"):
        assert biteq(res[k], one[k]), k
    assert biteq(res["spec_visibility"], cap.spec_visibility) and biteq(res["transfer"], cap.transfer)
    assert torch.equal(res["reflection"], cap.reflection) and res["stats"][0]["glossy_evals"] > 0

    def refuse(*a_, **k_):
        raise AssertionError("the walk prefiltered a map")
    monkeypatch.setattr(ops, "env_prefilter", refuse)
    launches = []
    shade = ops.env_shade_glossy_dirs

    def counting(*a_, **k_):
        launches.append((a_[5].shape[0], a_[8].shape[0]))
        return shade(*a_, **k_)
    monkeypatch.setattr(ops, "env_shade_glossy_dirs", counting)
    kw = dict(n_frames=5, axis=(0.2, -0.1, 1.0), transfer_samples=4, seed=SEED, bg=BG, window=12, glossy_samples=4, shininess=shin,
              specular=KS)
    walk = inference.scene_env_walk(gen, zs, b2ws, env, **kw)
    monkeypatch.undo()
    assert launches == [(5, 1)]                                               # one launch, rotations of ONE prefiltered map
    assert walk["image"].shape == walk["shading"].shape == walk["specular"].shape == (5, 3, S, S)
    assert biteq(walk["spec_visibility"], cap.spec_visibility) and walk["stats"][0]["glossy_evals"] > 0
    for f, Rm in enumerate(inference.env_walk_rotations(5, kw["axis"])):
        fr = cap.shade([env.rotated(Rm)], bg=BG, specular=KS)
        for k in ("image", "shading", "specular"):
            assert biteq(fr[k][0], walk[k][f]), (k, f)
    assert biteq(one["image"][0], walk["image"][0]) and not torch.equal(walk["specular"][0], walk["specular"][2])
    # the default keywords: the parent's walk and render, byte for byte, and no glossy keys
    plain = inference.scene_env_walk(gen, zs, b2ws, env.sh, n_frames=2, transfer_samples=4, seed=SEED, bg=BG, window=12)
    assert set(plain) == {"image", "shading", "mask", "depth", "instance", "transfer", "stats"}
    assert biteq(plain["image"][0], s.capture_transfer(4, SEED).shade(env.sh, bg=BG)["image"][0])


def test_c_abi_rejects_invalid_arguments_and_launches_nothing():
    """The refusals of tests/test_scene_gloss_cpu.py on real, poisoned device arrays: each returns a negative status with its
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
    p = lambda t_: ctypes.c_void_p(t_.data_ptr())
    for call, entry, text in C.invalid_argument_cases(lib, L, p(other), {k: p(v) for k, v in arr.items()}):
        rc = call()
        msg = L.oi_last_error().decode()
        assert rc < 0 and msg.startswith(entry) and text in msg, (entry, text, rc, msg)
    torch.cuda.synchronize()
    for k, v in list(arr.items()) + [("other", other)]:
        fresh = guarded_empty(tuple(v.shape), v.dtype, what="pattern", must_write=False)
        assert torch.equal(v.view(torch.uint8), fresh.view(torch.uint8)), k
