"""Adaptive anti-aliasing of scenes on the MI355X (include/oi_scene_aa.h; oi_amd.scene.trace_scene / render_scene(aa_samples=...);
oi_amd.inference.scene_light_walk / scene_light_orbit).

The references are tests/helpers/scene_aa_ref.py -- the classification restated in numpy fp32 in the header's operation order
(the flagged SET is the kernel's), the sub-pixel rays, the window rule and the cull in float64 -- tests/helpers/aa_ref.py for
the resolve (bit for bit), the closed form of the analytic two-sphere scene for an answer that owes the library nothing, and
the library's own entries where the stage claims to add nothing new: oi_scene_begin for a zero offset, sphere_trace per
instance for the sub-samples' march, render_scene under one light for a frame of a walk.

Bars: the project's ray bars (origins 1e-5, directions 2e-6; near and far test_gpu_scene.py::test_rays_and_cull's 1e-5 /
sqrt(1 - c2)); everything else is exact.  The analytic scene's exclusions and their 3 % cap are scene_ref's own
(tests/test_scene_aa_cpu.py rehearses them on the closed form alone)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import test_gpu_aa as GA
import test_gpu_occlusion as OC
import test_gpu_scene as TS
import test_gpu_scene_local_light as SLL
import test_gpu_trace as G
from conftest import record_margin
from helpers import aa_ref as AR
from helpers import scene_aa_ref as SAR
from helpers import scene_ref as SR
from helpers import trace_ref as T
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

PRECISIONS, npd = G.PRECISIONS, G.npd
_p, _cuda, _bits = OC._p, OC._cuda, OC._bits
_same_bits, _f32 = GA._same_bits, GA._f32
ORIGIN_BAR, DIRECTION_BAR = GA.ORIGIN_BAR, GA.DIRECTION_BAR
BG = (0.1, 0.2, 0.3)
AA_OPS = ("scene_aa_classify", "scene_aa_begin", "aa_resolve_strided")
UNCHANGED = ("depth", "position", "normal_map", "albedo", "mask", "instance", "visibility", "ambient_occlusion")
SEED = SLL.SEED


def _np(t):
    return t.detach().cpu().numpy()


def recorded(monkeypatch, fn):
    """fn() with every public function of oi_amd.ops recording its name.  -> (the names in call order, fn's result)."""
    from oi_amd import ops
    calls = []
    for name, f in list(vars(ops).items()):
        if isinstance(f, types.FunctionType) and f.__module__ == ops.__name__ and not name.startswith("_"):
            monkeypatch.setattr(ops, name, (lambda f_, n_: lambda *a, **k: (calls.append(n_), f_(*a, **k))[1])(f, name))
    try:
        return calls, fn()
    finally:
        monkeypatch.undo()


class Spy:
    """Records what the three ops of include/oi_scene_aa.h were given and returned while they run unchanged."""

    def __init__(self, monkeypatch):
        from oi_amd import ops
        self.classify, self.begin, self.resolve = [], [], []
        classify, begin, resolve = ops.scene_aa_classify, ops.scene_aa_begin, ops.aa_resolve_strided

        def scene_aa_classify(*a, **k):
            out = classify(*a, **k)
            self.classify.append(out)
            return out

        def scene_aa_begin(st, c2b, kinv, window, W, S, edge_index, n_edge, offsets):
            begin(st, c2b, kinv, window, W, S, edge_index, n_edge, offsets)
            self.begin.append(dict(st=st, edge_index=edge_index, n_edge=n_edge, offsets=offsets))

        def aa_resolve_strided(centre, sub, edge_slot, n_edge, S, out=None):
            res = resolve(centre, sub, edge_slot, n_edge, S, out=out)
            self.resolve.append(dict(centre=centre, sub=sub, edge_slot=edge_slot, n_edge=n_edge, S=S, out=res))
            return res
        for name, fn in zip(AA_OPS, (scene_aa_classify, scene_aa_begin, aa_resolve_strided)):
            monkeypatch.setattr(ops, name, fn)


def scene_args(kind, W):
    zs, b2ws = TS.instances(kind)
    return zs, b2ws, dict(window=W)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the default path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_sample_is_the_call_without_the_keywords(precision, monkeypatch):
    from oi_amd import inference, scene
    gen = TS.make_gen(precision)
    zs, b2ws, win = scene_args("pair", 9)
    kw = dict(lights=TS.lights(3), shadows=True, bg=BG, **win)
    off = dict(aa_samples=1, aa_adaptive=False, aa_plane=0.25, aa_cos=0.75, aa_pattern=[[0.0, 0.0]])
    scene.render_scene(gen, zs, b2ws, **kw)                                         # (the first call packs the weights)
    calls, plain = recorded(monkeypatch, lambda: scene.render_scene(gen, zs, b2ws, **kw))
    calls1, same = recorded(monkeypatch, lambda: scene.render_scene(gen, zs, b2ws, **kw, **off))
    assert calls == calls1 and len(calls) > 10 and not set(calls) & set(AA_OPS)
    assert set(plain) == set(same) and "coverage" not in same and "aa_pixels" not in same["stats"][0] and same["scene"].aa is None
    for k, v in plain.items():
        if torch.is_tensor(v):
            assert _same_bits(v, same[k]), k
    wcalls, walk = recorded(monkeypatch, lambda: inference.scene_light_walk(gen, zs, b2ws, n_frames=3, bg=BG, **win))
    wcalls1, walk1 = recorded(monkeypatch, lambda: inference.scene_light_walk(gen, zs, b2ws, n_frames=3, bg=BG, **win, **off))
    assert wcalls == wcalls1 and not set(wcalls) & set(AA_OPS) and set(walk) == set(walk1)
    for k, v in walk.items():
        if torch.is_tensor(v):
            assert _same_bits(v, walk1[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 2. the classification
# ---------------------------------------------------------------------------------------------------------------------
def classified(s, plane=0.5, cos=0.5, parts=False):
    """oi_scene_aa_classify on a traced scene, checked against the restatement.  -> the flagged set (and the restatement's parts)."""
    from oi_amd import ops
    out = ops.scene_aa_classify(s.owner, s.owner_ray, s.vis_slot, s.points, s.grad, s.n_pad, s.S, plane, cos)
    ref = SAR.classify(_np(s.owner), _np(s.owner_ray), _np(s.vis_slot), _np(s.points), _np(s.grad), s.S, plane, cos, parts=True)
    got = GA._check_classify(*out, ref[0] | ref[1] | ref[2] | ref[3])
    return (got, ref) if parts else got


@pytest.mark.parametrize("kind,W", [("pair", 9), ("triple", 12), ("single", 9)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_classification_is_the_restatement(precision, kind, W):
    s = TS.traced(precision, kind, W)
    first, (mask, inst, plane, normal) = classified(s, parts=True)
    assert first == classified(s)                                                  # two calls: the same set, whatever the slots
    share = len(first) / (s.S * s.S)
    record_margin(f"scene_aa_classify[{precision},{kind},W={W}]", "flagged_share", share)
    print(f"scene_aa_classify[{precision},{kind},W={W}]: flagged {len(first)} of {s.S * s.S} ({share:.4f}), mask {int(mask.sum())}, instance "
          f"{int(inst.sum())} ({int((inst & ~mask).sum())} alone), plane only {int((plane & ~mask & ~inst).sum())}, normal only "
          f"{int((normal & ~mask & ~inst & ~plane).sum())}")
    assert 0 < len(first) and mask.sum() > 0
    assert (inst.sum() > 0) == (kind != "single")                                  # instances overlap in the pair and the triple
    for pl, co in ((0.1, 0.5), (0.5, 0.95), (0.0, 0.0)):                           # other thresholds: the plane and normal criteria fire
        more = classified(s, pl, co)
        assert first <= more or (pl, co) == (0.0, 0.0)                              # a lower plane or a higher cos bar flags no less
    assert len(classified(s, 0.0, 0.0)) > len(first)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_twice_flags_what_one_instance_flags(precision):
    """One instance entered twice at one pose: every tie goes to element 0, so the scene is the one-instance scene and no
    pixel is flagged by (instance)."""
    from oi_amd import scene
    s = TS.traced(precision, "twice", 12)
    zs, b2ws = TS.instances("twice")
    one = scene.trace_scene(TS.make_gen(precision), zs[:1], b2ws[:1], window=12)
    got, (mask, inst, plane, normal) = classified(s, parts=True)
    assert set(np.unique(_np(s.owner))) == {-1, 0} and not inst.any()
    assert got == classified(one) and len(got) > 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_is_the_single_view_classifier(precision):
    from oi_amd import ops
    s = TS.traced(precision, "single", 9)
    status, hit_slot = SAR.dense(_np(s.owner), _np(s.owner_ray), _np(s.vis_slot), s.n_pad)
    for plane, cos in ((0.5, 0.5), (0.1, 0.9)):
        ei, es, count = ops.aa_classify(_cuda(status, torch.uint8), _cuda(hit_slot, torch.int32), s.points[0].contiguous(),
                                        s.grad[0].contiguous(), s.n_pad, s.S, s.S, plane, cos)
        n = int(count.item())
        assert set(ei[:n].tolist()) == classified(s, plane, cos)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the sub-pixel rays
# ---------------------------------------------------------------------------------------------------------------------
def _test_pixels(origins, W, S, seed):
    """Scene pixels in and about the windows, some outside every window, in ascending order."""
    rs = np.random.RandomState(seed)
    lo, hi = origins.min(0) - 2, origins.max(0) + W + 2
    X, Y = np.meshgrid(np.arange(max(lo[0], 0), min(hi[0], S)), np.arange(max(lo[1], 0), min(hi[1], S)))
    pix = (Y * S + X).reshape(-1)
    pix = np.union1d(rs.permutation(pix)[:150], [0, S - 1, S * S - 1, pix[0], pix[-1]])
    return pix.astype(np.int32)


@pytest.mark.parametrize("kind,W", [("pair", 9), ("triple", 12), ("offscreen", 12)])
def test_begin(kind, W):
    from oi_amd import lib, ops
    st, c2b, kinv, window, origins, S = TS.begun(kind, W)
    E = st.E
    pix = _test_pixels(origins, W, S, W)
    n = len(pix)
    d_pix = _cuda(pix, torch.int32)
    X, Y = pix % S, pix // S
    # an all-zero pattern: oi_scene_begin's ray, near, far and status of that pixel and element, bit for bit, for every sample
    Sa = 3
    n_sub = (Sa - 1) * n
    Q = SAR.virtual_size(n_sub)
    assert Q * Q > n_sub                                                           # padding rays behind the sub-samples
    zb = ops.trace_batch_state_empty(E, Q * Q, c2b)
    ops.scene_aa_begin(zb, c2b, kinv, window, W, S, d_pix, n, torch.zeros(Sa, 2).cuda())
    for e in range(E):
        i, j = X - origins[e][0], Y - origins[e][1]
        cov = (i >= 0) & (i < W) & (j >= 0) & (j < W)
        r = torch.from_numpy((j * W + i)[cov]).cuda()
        for smp in range(Sa - 1):
            q = torch.from_numpy(smp * n + np.nonzero(cov)[0]).cuda()
            for name in ("rays_o", "rays_d", "near", "far", "t", "status", "bracket"):
                assert _same_bits(getattr(zb, name)[e][q], getattr(st, name)[e][r]), (name, e, smp)
            out = torch.from_numpy(smp * n + np.nonzero(~cov)[0]).cuda()
            assert bool((zb.status[e][out] == T.MISS).all()) and not bool(zb.near[e][out].any()) and not bool(zb.far[e][out].any())
        assert int(zb.counts[e, 0]) == (Sa - 1) * int((st.status[e][r] == T.MARCH).sum())
    # the R2 pattern against the float64 restatement
    Sa = 4
    pat = AR.r2_pattern(Sa)
    n_sub = (Sa - 1) * n
    Q = SAR.virtual_size(n_sub)
    sb = ops.trace_batch_state_empty(E, Q * Q, c2b)
    ops.scene_aa_begin(sb, c2b, kinv, window, W, S, d_pix, n, torch.from_numpy(pat).cuda())
    o, d, cov, ent, near, far = SAR.sub_rays(npd(c2b), npd(kinv), S, W, origins, pix, pat)
    counts, live = _np(sb.counts), _np(sb.live)
    errs = dict(origins=0.0, directions=0.0, chord=0.0)
    edge_total = 0
    for e in range(E):
        ko, kd = npd(sb.rays_o[e]), npd(sb.rays_d[e])
        errs["origins"] = max(errs["origins"], np.abs(ko[:n_sub] - o[e]).max())
        errs["directions"] = max(errs["directions"], np.abs(kd[:n_sub] - d[e]).max())
        # the entered set: the restatement's cull of the kernel's own fp32 rays, under the window rule
        kent, knear, kfar, c2 = SR.cull(ko[:n_sub], kd[:n_sub])
        kent &= cov[e]
        status, steps = _np(sb.status[e]), _np(sb.steps[e])
        got = status == T.MARCH
        edge = np.abs(c2 - 1) <= 4 * 2.0 ** -24 * ((ko[:n_sub] ** 2).sum(-1) + 1)
        edge_total += int((edge & cov[e]).sum())
        assert np.array_equal(got[:n_sub][~edge], kent[~edge]) and set(np.unique(status)) <= {T.MARCH, T.MISS} and not steps.any()
        assert not got[:n_sub][~cov[e]].any() and not got[n_sub:].any()             # the window rule; padding is never traced
        nr, fr, t = npd(sb.near[e]), npd(sb.far[e]), npd(sb.t[e])
        assert np.array_equal(t, nr) and not nr[~got].any() and not fr[~got].any()
        both = got[:n_sub] & kent
        tol = 1e-5 / np.sqrt(np.maximum(1 - c2[both], 1e-4))
        chord = np.maximum(np.abs(nr[:n_sub][both] - knear[both]), np.abs(fr[:n_sub][both] - kfar[both])) / tol
        errs["chord"] = max(errs["chord"], chord.max(initial=0.0))
        n_ent = int(got.sum())
        assert counts[e, 0] == n_ent and not counts[e, 1:].any()
        act = _np(sb.active[e, 0, :n_ent])
        assert sorted(act.tolist()) == np.nonzero(got)[0].tolist()                  # compacted within the element, in no fixed order
        pts = npd(sb.points[e])
        assert np.abs(pts[:n_ent] - (ko[act] + nr[act, None] * kd[act])).max(initial=0.0) <= 1e-6 and not pts[n_ent:].any()
        br = npd(sb.bracket[e])
        assert np.array_equal(br[:, 0], nr) and np.array_equal(br[:, 2], nr) and not br[:, 1].any() and not br[:, 3].any()
        assert not bool(sb.side[e].any())
        # the padding rays hold pixel (0, 0)'s centre ray
        assert _same_bits(sb.rays_d[e][n_sub:], zb.rays_d[e][-1:].expand(Q * Q - n_sub, 3))
    for k, v in errs.items():
        record_margin(f"scene_aa_begin[{kind},W={W}]", k, v)
    print(f"scene_aa_begin[{kind},W={W}] pixels {n}, Q {Q}, entered {counts[:, 0].tolist()}, on the cull's edge {edge_total},", errs)
    assert errs["origins"] < ORIGIN_BAR and errs["directions"] < DIRECTION_BAR and errs["chord"] <= 1.0
    assert live[0] == counts[:, 0].max() and not live[1:].any() and len(live) == lib.TRACE_COUNT_WORDS
    assert counts[0, 0] > 0 and cov.any() and not cov.all()
    if kind == "offscreen":
        assert counts[1, 0] == 0
    assert not _same_bits(sb.rays_d[:, :n], zb.rays_d[:, :n])                      # the offsets do move the rays


# ---------------------------------------------------------------------------------------------------------------------
# 4. the march is the library's own
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sub_samples_are_sphere_trace_per_instance(precision, monkeypatch):
    from oi_amd import scene, trace
    gen = TS.make_gen(precision)
    zs, b2ws, win = scene_args("pair", 9)
    spy = Spy(monkeypatch)
    s = scene.trace_scene(gen, zs, b2ws, aa_samples=4, **win)
    monkeypatch.undo()
    (b,), sub = spy.begin, s.sub
    n_edge = b["n_edge"]
    assert sub is not None and sub.state is b["st"] and n_edge == s.n_edge > 0
    flagged = b["edge_index"][:n_edge]
    assert bool((flagged[1:] > flagged[:-1]).all())                                 # the host lists the flagged pixels in ascending order
    assert torch.equal(s.edge_slot[flagged.long()], torch.arange(n_edge, dtype=torch.int32).cuda())
    Q = SAR.virtual_size(3 * n_edge)
    assert (sub.W, sub.S, sub.N, sub.E) == (Q, Q, Q * Q, s.E) and not bool(sub.window.any())
    st = sub.state
    for e in range(s.E):
        ent = torch.nonzero(st.steps[e] > 0).flatten()
        assert len(ent) == sub.n_entered[e] > 0 and bool((st.status[e][st.steps[e] == 0] == T.MISS).all())
        ref = trace.sphere_trace(gen, st.rays_o[e][ent], st.rays_d[e][ent], st.near[e][ent], st.far[e][ent], z=zs[e:e + 1].cuda())
        assert torch.equal(st.t[e][ent], ref.t) and torch.equal(st.status[e][ent], ref.status) and torch.equal(st.steps[e][ent], ref.steps)
        assert sub.n_hit[e] == int((ref.status == T.HIT).sum())
    # the resolve over the virtual image: the restatement's arg-min with the tie rule, every window at the origin
    owner_ref, ray_ref = SR.resolve(_np(st.status), _np(st.t), np.zeros((s.E, 2), np.int64), Q, Q)
    assert np.array_equal(_np(sub.owner), owner_ref) and np.array_equal(_np(sub.owner_ray), ray_ref)
    assert (owner_ref[3 * n_edge:] == -1).all() and (owner_ref == 0).sum() > 0 and (owner_ref == 1).sum() > 0
    stats = s.stats()
    assert stats[0]["aa_pixels"] == n_edge and stats[0]["aa_rays"] == 3 * n_edge and stats[1]["aa_evals"] == sub.n_evals > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. an independent answer: the analytic two-sphere scene
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sa", [2, 8])
def test_analytic_two_sphere_scene(Sa):
    from oi_amd import ops
    a = TS._analytic()
    sc, st = a["sc"], a["st"]
    S, W, E = sc["S"], sc["W"], 2
    f32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32).cuda().contiguous()
    c2b, kinv = f32(sc["c2b"]), f32(sc["K_inv"])
    window = torch.tensor(sc["origins"], dtype=torch.int32).cuda()
    # the primary's owner map and visible hits, as _analytic made them
    owner, owner_ray = ops.scene_resolve(st, window, W, S)       # (resolve reads status and t, which scene_visible left alone)
    vis_index, vis_slot = ops.scene_visible(st, owner, window, W, S)
    n_pad = int(st.live[-1].item())
    pts = ops.trace_batch_gather(st, vis_index, n_pad)
    grad = (2.0 * pts).contiguous()
    ei, es, count = ops.scene_aa_classify(owner, owner_ray, vis_slot, pts, grad, n_pad, S)
    ref = SAR.classify(_np(owner), _np(owner_ray), _np(vis_slot), _np(pts), _np(grad), S)
    GA._check_classify(ei, es, count, ref)
    n_edge = int(count.item())
    pix = torch.sort(ei[:n_edge]).values
    es[pix.long()] = torch.arange(n_edge, dtype=torch.int32).cuda()
    pat = AR.r2_pattern(Sa)
    n_sub = (Sa - 1) * n_edge
    Q = SAR.virtual_size(n_sub)
    sb = ops.trace_batch_state_empty(E, Q * Q, c2b)
    ops.scene_aa_begin(sb, c2b, kinv, window, W, S, pix, n_edge, torch.from_numpy(pat).cuda())
    sdf = torch.zeros(E, sb.N).cuda()
    bound, k = int(sb.live[0].item()), 0
    while bound > 0 and k < T.MAX_MAX_STEPS:
        sdf[:, :bound] = sb.points[:, :bound].norm(dim=-1) - SR.RADIUS
        ops.trace_batch_step(sb, sdf, bound, k, T.TOL, T.OMEGA)
        k += 1
        bound = int(sb.live[k].item())
    ops.trace_batch_finish(sb)
    zero = torch.zeros(E, 2, dtype=torch.int32).cuda()
    sub_owner, _ = ops.scene_resolve(sb, zero, Q, Q)
    got = _np(sub_owner)
    cf_owner, excluded = SAR.analytic_sub(sc, _np(pix), pat)
    keep = ~excluded
    print(f"analytic scene Sa={Sa}: flagged {n_edge} of {S * S}, sub-samples {n_sub}, Q {Q}, excluded {int(excluded.sum())} "
          f"({excluded.mean():.4f}), owners {[int((got[:n_sub] == e).sum()) for e in (-1, 0, 1)]}, disagreeing among the excluded "
          f"{int((got[:n_sub] != cf_owner)[excluded].sum())}")
    assert excluded.mean() <= SR.AN_CAP                                            # a condition on the scene, rehearsed on the CPU
    assert np.array_equal(got[:n_sub][keep], cf_owner[keep]) and (got[n_sub:] == -1).all()
    # coverage: the mean of the mask over a pixel's samples, against the closed form's, within its excluded samples / Sa
    centre_mask = (owner >= 0).float().view(1, -1)
    sub_mask = (sub_owner >= 0).float().view(1, -1)
    cov = _f32(ops.aa_resolve_strided(centre_mask, sub_mask, es, n_edge, Sa))[0]
    cf = SR.analytic_closed_form(sc)
    p = _np(pix)
    cf_cov = ((cf["owner"][p] >= 0).astype(np.float64) + (cf_owner >= 0).reshape(Sa - 1, n_edge).sum(0)) / Sa
    slack = (cf["excluded"][p].astype(np.float64) + excluded.reshape(Sa - 1, n_edge).sum(0)) / Sa
    err = np.abs(cov[p] - cf_cov)
    record_margin(f"scene_aa_analytic[Sa={Sa}]", "coverage_error", err.max())
    assert (err <= slack + 1e-6).all()
    off = np.ones(S * S, bool)
    off[p] = False
    assert np.array_equal(cov[off], _f32(centre_mask)[0][off])
    # what the sub-samples buy: the error of the coverage against the closed form's at 64 samples per flagged pixel
    o64, _ = SAR.analytic_sub(sc, p, AR.r2_pattern(64))
    cov64 = ((cf["owner"][p] >= 0).astype(np.float64) + (o64 >= 0).reshape(63, n_edge).sum(0)) / 64
    e1, eS = np.abs((cf["owner"][p] >= 0) - cov64).mean(), np.abs(cov[p] - cov64).mean()
    record_margin(f"scene_aa_analytic[Sa={Sa}]", "coverage_error_ratio", eS / e1)
    print(f"analytic scene Sa={Sa}: mean |coverage - coverage(64)| one sample {e1:.4f}, {Sa} samples {eS:.4f}, ratio {eS / e1:.3f}")
    assert Sa < 8 or eS < e1


# ---------------------------------------------------------------------------------------------------------------------
# 6. the resolve, the unchanged maps, adaptive against full
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_resolve_and_the_unchanged_maps(precision, monkeypatch):
    from oi_amd import scene
    gen = TS.make_gen(precision)
    zs, b2ws, win = scene_args("pair", 9)
    Sa, L = 4, 3
    kw = dict(lights=TS.lights(L), bg=BG, shadows=True, **win)
    one = scene.render_scene(gen, zs, b2ws, **kw)
    spy = Spy(monkeypatch)
    out = scene.render_scene(gen, zs, b2ws, aa_samples=Sa, **kw)
    monkeypatch.undo()
    img, cov = spy.resolve
    S = gen.scene_resolution
    M = S * S
    slot = _np(img["edge_slot"])
    flagged = slot >= 0
    n_edge, sub = int(flagged.sum()), out["scene"].sub
    n_sub, Q = (Sa - 1) * n_edge, sub.S
    assert img["S"] == cov["S"] == Sa and img["n_edge"] == n_edge == out["stats"][0]["aa_pixels"] and Q == SAR.virtual_size(n_sub)
    assert img["sub"].shape == (3 * L, Q * Q) and cov["sub"].shape == (1, Q * Q) and Q * Q > n_sub
    assert np.array_equal(_f32(out["aa_mask"]).reshape(-1), flagged.astype(np.float32))
    # the centre planes are the one-sample call's, and the results are the fp32 restatement of (centre, sub-samples)
    assert _same_bits(img["centre"].view(L, 3, S, S), one["image"]) and _same_bits(cov["centre"].view(1, 1, S, S), one["mask"])
    ref_img = AR.resolve(_f32(one["image"]).reshape(3 * L, M), _f32(img["sub"])[:, :n_sub], slot, Sa)
    ref_cov = AR.resolve(_f32(one["mask"]).reshape(1, M), _f32(cov["sub"])[:, :n_sub], slot, Sa)
    image, coverage = _f32(out["image"]).reshape(3 * L, M), _f32(out["coverage"]).reshape(1, M)
    assert np.array_equal(image.view(np.uint32), ref_img.view(np.uint32))
    assert np.array_equal(coverage.view(np.uint32), ref_cov.view(np.uint32))
    assert (image[:, flagged] != _f32(one["image"]).reshape(3 * L, M)[:, flagged]).any()
    k = coverage[0] * Sa
    assert np.array_equal(k, np.round(k)) and k.min() >= 0 and k.max() <= Sa
    assert ((coverage[0] > 0) & (coverage[0] < 1)).any()                             # the outlines blend
    # off-surface samples carry bg; the sub-samples' mask is the virtual image's owner map
    sub_mask = _f32(cov["sub"])[0]
    assert np.array_equal(sub_mask, (_np(sub.owner) >= 0).astype(np.float32)) and not sub_mask[n_sub:].any()
    bgs = _f32(img["sub"]).reshape(L, 3, Q * Q)[:, :, sub_mask == 0]
    assert np.array_equal(bgs, np.broadcast_to(np.asarray(BG, np.float32)[None, :, None], bgs.shape))
    for name in UNCHANGED[:-1]:                                                      # the centre sample's, byte for byte
        assert _same_bits(out[name], one[name]), name
    assert set(out) - set(one) == {"coverage", "aa_mask"}
    with pytest.raises(ValueError, match="aa_samples"):
        out["scene"].capture_transfer(4)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_adaptive_is_full_at_the_flagged_pixels(precision, monkeypatch):
    from oi_amd import ops, scene
    gen = TS.make_gen(precision)
    zs, b2ws, win = scene_args("pair", 9)
    kw = dict(lights=TS.lights(3), bg=BG, shadows=True, aa_samples=4, **win)
    adaptive = scene.render_scene(gen, zs, b2ws, **kw)

    def refuse(*a, **k):
        raise AssertionError("oi_scene_aa_classify ran with aa_adaptive=False")
    monkeypatch.setattr(ops, "scene_aa_classify", refuse)
    full = scene.render_scene(gen, zs, b2ws, aa_adaptive=False, **kw)
    monkeypatch.undo()
    M = gen.scene_resolution ** 2
    st = full["stats"][0]
    assert st["aa_pixels"] == M and bool((full["aa_mask"] == 1).all()) and st["aa_rays"] == 3 * M
    on = adaptive["aa_mask"].view(-1) > 0
    assert 0 < int(on.sum()) == adaptive["stats"][0]["aa_pixels"] < M
    assert _same_bits(adaptive["image"].view(9, M)[:, on], full["image"].view(9, M)[:, on])
    assert _same_bits(adaptive["coverage"].view(M)[on], full["coverage"].view(M)[on])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_scenes_without_a_hit_or_a_flagged_pixel(precision, monkeypatch):
    from oi_amd import ops, scene
    gen = TS.make_gen(precision)
    zs, b2ws = TS.instances("nothing")

    def refuse(*a, **k):
        raise AssertionError("an entry of include/oi_scene_aa.h's first two ran without a primary hit")
    monkeypatch.setattr(ops, "scene_aa_classify", refuse)
    monkeypatch.setattr(ops, "scene_aa_begin", refuse)
    for adaptive in (True, False):
        none = scene.render_scene(gen, zs, b2ws, lights=TS.lights(2), shadows=True, bg=BG, window=12, aa_samples=4, aa_adaptive=adaptive)
        S = gen.scene_resolution
        assert none["scene"].sub is None and none["stats"][0]["aa_pixels"] == 0 and none["stats"][0]["aa_evals"] == 0
        assert torch.equal(none["image"], torch.tensor(BG).cuda()[None, :, None, None].expand(2, 3, S, S))
        assert not bool(none["coverage"].any()) and not bool(none["aa_mask"].any())
    monkeypatch.undo()
    # an instance wholly off screen: its element enters no sub-sample ray, the frame is the one-instance scene's
    zs, b2ws = TS.instances("offscreen")
    kw = dict(lights=TS.lights(1), shadows=True, bg=BG, window=12, aa_samples=2)
    off = scene.render_scene(gen, zs, b2ws, **kw)
    alone = scene.render_scene(gen, zs[:1], b2ws[:1], **kw)
    assert off["scene"].sub.n_entered[1] == 0 and off["scene"].sub.n_entered[0] > 0
    for k in ("image", "coverage", "aa_mask", "depth", "instance"):
        assert _same_bits(off[k], alone[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 7. every shading path runs on the sub-samples
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("local", [False, True], ids=["directional", "local"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_soft_shadows_occlusion_and_local_lights(precision, local):
    from oi_amd import scene
    gen = TS.make_gen(precision)
    zs, b2ws, win = scene_args("pair", 9)
    kw = dict(shadows=True, shadow_samples=4, ao_samples=4, seed=SEED, bg=BG, **win)
    kw.update(dict(lights=SLL.scene_lights("pair")) if local else dict(lights=TS.lights(2), light_radius=0.05))
    one = scene.render_scene(gen, zs, b2ws, **kw)
    out = scene.render_scene(gen, zs, b2ws, aa_samples=4, **kw)
    L, M = out["image"].shape[0], gen.scene_resolution ** 2
    assert bool(torch.isfinite(out["image"]).all()) and out["image"].shape == one["image"].shape
    off = out["aa_mask"].view(-1) == 0
    assert 0 < int(off.sum()) < M
    assert _same_bits(out["image"].view(3 * L, M)[:, off], one["image"].view(3 * L, M)[:, off])
    assert not _same_bits(out["image"].view(3 * L, M)[:, ~off], one["image"].view(3 * L, M)[:, ~off])
    for name in UNCHANGED:
        assert _same_bits(out[name], one[name]), name
    s = out["scene"]
    st = out["stats"][0]
    assert s.sub.shadow_evals > 0 and s.sub.occlusion_evals > 0
    assert st["aa_evals"] == s.sub.n_evals + s.sub.shadow_evals + s.sub.occlusion_evals and st["aa_rays"] == 3 * st["aa_pixels"]
    # split by a small max_shadow_rays (chunks of two samples on the larger of the two surfaces) and unsplit: the same bytes
    per = s.E * L * max(sum(s.n_vis), sum(s.sub.n_vis))
    split = scene.render_scene(gen, zs, b2ws, aa_samples=4, max_shadow_rays=2 * per, **kw)
    for name in ("image", "coverage", "visibility", "ambient_occlusion"):
        assert _same_bits(out[name], split[name]), name
    assert split["stats"][0]["aa_evals"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. it anti-aliases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_adaptive_samples_approach_the_converged_image(precision):
    from oi_amd import scene
    gen = TS.make_gen(precision)
    zs, b2ws, win = scene_args("pair", 12)
    kw = dict(lights=TS.lights(3), bg=BG, **win)
    one = scene.render_scene(gen, zs, b2ws, **kw)
    eight = scene.render_scene(gen, zs, b2ws, aa_samples=8, **kw)
    ref = scene.render_scene(gen, zs, b2ws, aa_samples=64, aa_adaptive=False, **kw)
    on = _np(eight["aa_mask"].view(-1) > 0)
    M = gen.scene_resolution ** 2
    err = lambda o: float(np.abs(npd(o["image"]) - npd(ref["image"])).reshape(9, M)[:, on].mean())
    e1, e8 = err(one), err(eight)
    case = f"scene_aa_converges[{precision}]"
    record_margin(case, "one_sample", e1)
    record_margin(case, "adaptive_8", e8)
    record_margin(case, "ratio", e8 / e1)
    print(case, "flagged", int(on.sum()), "of", M, "mean |image - S64|: one sample", e1, "adaptive 8", e8, "ratio", e8 / e1)
    assert on.sum() > 0 and e8 < e1


# ---------------------------------------------------------------------------------------------------------------------
# 9. the light walk and the orbit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_light_walk_traces_the_sub_samples_once(precision, monkeypatch):
    from oi_amd import inference, scene
    from oi_amd.relight import Light
    gen = TS.make_gen(precision)
    zs, b2ws, win = scene_args("pair", 9)
    spy = Spy(monkeypatch)
    walk = inference.scene_light_walk(gen, zs, b2ws, n_frames=4, aa_samples=4, bg=BG, ao_samples=2, seed=SEED, **win)
    monkeypatch.undo()
    S = gen.scene_resolution
    assert len(spy.begin) == 1 and len(spy.classify) == 1
    assert walk["image"].shape == (4, 3, S, S) and walk["stats"][0]["aa_pixels"] == spy.begin[0]["n_edge"] > 0
    base = Light.from_module(gen.light)
    dirs = inference.light_walk_directions(base.direction, 4)
    for i in range(4):
        lt = base if i == 0 else base.replace(direction=tuple(dirs[i]))
        one = scene.render_scene(gen, zs, b2ws, lights=[lt], shadows=True, bg=BG, aa_samples=4, ao_samples=2, seed=SEED, **win)
        assert torch.equal(walk["image"][i], one["image"][0]), i
        assert torch.equal(walk["visibility"][i], one["visibility"][0]), i
    for name in ("mask", "coverage", "aa_mask", "instance", "ambient_occlusion"):
        assert torch.equal(walk[name], one[name]), name
    # split into two lights per shadow batch, sized by the larger of the two surfaces: the same frames
    s = one["scene"]
    split = inference.scene_light_walk(gen, zs, b2ws, n_frames=4, aa_samples=4, bg=BG, ao_samples=2, seed=SEED,
                                       max_shadow_rays=2 * s.E * max(sum(s.n_vis), sum(s.sub.n_vis)), **win)
    assert torch.equal(split["image"], walk["image"]) and torch.equal(split["coverage"], walk["coverage"])
    plain = inference.scene_light_walk(gen, zs, b2ws, n_frames=4, bg=BG, ao_samples=2, seed=SEED, **win)
    off = walk["aa_mask"].view(-1) == 0
    assert torch.equal(plain["image"].view(12, -1)[:, off], walk["image"].view(12, -1)[:, off]) and "coverage" not in plain


@pytest.mark.parametrize("precision", PRECISIONS)
def test_light_orbit_traces_the_sub_samples_once(precision, monkeypatch):
    from oi_amd import inference, scene
    gen = TS.make_gen(precision)
    zs, b2ws, win = scene_args("pair", 9)
    light = SLL.scene_lights("pair")[0]                                              # a point light: one hard shadow ray
    c = SLL.centres("pair")
    kw = dict(shadows=True, bg=BG, aa_samples=4, **win)
    spy = Spy(monkeypatch)
    orbit = inference.scene_light_orbit(gen, zs, b2ws, light, n_frames=3, centre=tuple((c[0] + c[1]) / 2), radius=1.9, height=0.5, **kw)
    monkeypatch.undo()
    S = gen.scene_resolution
    assert len(spy.begin) == 1 and orbit["image"].shape == (3, 3, S, S)
    for f in range(3):
        one = scene.render_scene(gen, zs, b2ws, lights=[light.replace(position=tuple(orbit["positions"][f]))], **kw)
        assert torch.equal(orbit["image"][f], one["image"][0]) and torch.equal(orbit["visibility"][f], one["visibility"][0]), f
    assert torch.equal(orbit["coverage"], one["coverage"]) and torch.equal(orbit["aa_mask"], one["aa_mask"])


@pytest.mark.parametrize("ground", [False, True], ids=["aa", "ground"])
@pytest.mark.parametrize("entry", ["walk", "orbit"])
def test_walk_frames_are_the_single_renders(entry, ground):
    """test_gpu_aa's check of the walk loop on the two scene walks; with a ground plane (which has no anti-aliasing stage:
    aa_samples=1) also its mask and the shadow matte of every frame."""
    from oi_amd import inference, scene
    from oi_amd.relight import Light
    import test_gpu_ground as GG
    gen = TS.make_gen("f16x3")
    zs, b2ws, win = scene_args("pair", 9)
    kw = dict(GA.WALK_KW, seed=SEED, **win)
    maps = ("image", "visibility", "instance") + GA.WALK_MAPS
    if ground:
        kw.update(aa_samples=1, ground=GG.golden_ground(TS.traced("f16x3", "pair", 9)))
        maps = tuple(k for k in maps if k not in ("coverage", "aa_mask")) + ("ground_mask", "shadow_matte")
    if entry == "walk":
        base = Light.from_module(gen.light)
        lights = [base] + [base.replace(direction=tuple(d)) for d in inference.light_walk_directions(base.direction, 3)[1:]]
        walk = inference.scene_light_walk(gen, zs, b2ws, n_frames=3, **kw)
    else:
        c = SLL.centres("pair")
        walk = inference.scene_light_orbit(gen, zs, b2ws, SLL.scene_lights("pair")[1], n_frames=3, centre=tuple((c[0] + c[1]) / 2),
                                           radius=1.9, height=0.5, **kw)
        lights = [SLL.scene_lights("pair")[1].replace(position=tuple(p)) for p in walk["positions"]]
    stats = walk["stats"][0]
    assert stats["shadow_evals"] > 0 and stats["occlusion_evals"] > 0 and (stats["ground_pixels"] if ground else stats["aa_pixels"]) > 0
    GA.walk_frames_are_single_renders(walk, lambda lt: scene.render_scene(gen, zs, b2ws, lights=[lt], **kw), lights, maps)


# ---------------------------------------------------------------------------------------------------------------------
# 10. guarded shapes through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _guarded_batch(E, N, tag, must_write=True):
    """An oi_trace_batch of E elements x N rays on guarded, poisoned buffers."""
    from oi_amd import lib
    g = lambda sh, dt=torch.float32, what="?", mw=True: guarded_empty(sh, dt, what=f"{tag}_{what}", must_write=mw and must_write)
    arr = dict(rays_o=g((E, N, 3), what="rays_o"), rays_d=g((E, N, 3), what="rays_d"), near_=g((E, N), what="near"), far_=g((E, N), what="far"),
               t=g((E, N), what="t"), status=g((E, N), torch.uint8, "status"), steps=g((E, N), torch.int16, "steps", False),
               bracket=g((E, N, 4), what="bracket"), side=g((E, N), torch.uint8, "side"), active=g((E, 2, N), torch.int32, "active", False),
               points=g((E, N, 3), what="points"), counts=g((E, lib.TRACE_COUNT_WORDS), torch.int32, "counts"))
    live = g((lib.TRACE_COUNT_WORDS,), torch.int32, "live")
    B = lib.TraceBatch()
    B.s.N, B.E, B.live = N, E, _p(live)
    for k_, v_ in arr.items():
        setattr(B.s, k_, _p(v_))
    return arr, live, B


@pytest.mark.parametrize("n_edge,Sa", [(1, 2), (257, 64), (257, 2)])
def test_guarded_begin(n_edge, Sa):
    from oi_amd import lib, ops
    _, c2b, kinv, window, origins, S = TS.begun("triple", 12)
    W, E = 12, 3
    rs = np.random.RandomState(n_edge + Sa)
    X0, Y0 = origins[0]
    near0 = [(Y0 + 6) * S + X0 + 6] if n_edge == 1 else []                           # the single pixel lies in a window
    pix = np.asarray(near0 + rs.permutation(S * S)[:n_edge - len(near0)].tolist(), np.int32)
    pat = AR.r2_pattern(Sa)
    n_sub = (Sa - 1) * n_edge
    Q = SAR.virtual_size(n_sub)
    N = Q * Q if n_edge > 1 else 5                                                   # ragged: N above n_sub, not a square
    assert N > n_sub
    g_c2b, g_kinv, g_win = guarded_copy(c2b, "c2b"), guarded_copy(kinv, "kinv"), guarded_copy(window, "window")
    edge_index, offsets = guarded_copy(_cuda(pix, torch.int32), "edge_index"), guarded_copy(_cuda(pat), "offsets")
    arr, live, B = _guarded_batch(E, N, "sa")
    assert lib.load().oi_scene_aa_begin(ctypes.byref(B), _p(g_c2b), _p(g_kinv), _p(g_win), W, S, _p(edge_index), n_edge, _p(offsets), Sa,
                                        ops._stream()) == 0
    o, d, cov, ent, near, far = SAR.sub_rays(npd(c2b), npd(kinv), S, W, origins, pix, pat)
    status = _np(arr["status"])
    got = status == T.MARCH
    assert set(np.unique(status)) <= {T.MARCH, T.MISS} and not got[:, n_sub:].any() and not got[:, :n_sub][~cov].any()
    assert np.abs(npd(arr["rays_o"])[:, :n_sub] - o).max() < ORIGIN_BAR and np.abs(npd(arr["rays_d"])[:, :n_sub] - d).max() < DIRECTION_BAR
    # away from the cull's edge the entered set is the restatement's
    _, _, _, c2 = SR.cull(o, d)
    sure = np.abs(c2 - 1) > 1e-5
    assert np.array_equal(got[:, :n_sub][sure], ent[sure])
    counts = _np(arr["counts"])
    assert np.array_equal(counts[:, 0], got.sum(1)) and not counts[:, 1:].any()
    assert int(live[0]) == counts[:, 0].max() and not bool(live[1:].any())
    assert torch.equal(arr["t"], arr["near_"]) and not bool(arr["near_"][torch.from_numpy(~got).cuda()].any())
    assert not bool(arr["steps"].any()) and not bool(_bits(arr["side"]).any())
    for e in range(E):
        n_ent = int(counts[e, 0])
        assert sorted(arr["active"][e, 0, :n_ent].tolist()) == np.nonzero(got[e])[0].tolist() and not bool(arr["points"][e, n_ent:].any())
    if n_edge == 1:
        assert got[0, 0] and counts[0, 0] == 1


@pytest.mark.parametrize("P,n_edge,Sa,extra", [(1, 40, 2, 1), (9, 100, 64, 25), (9, 257, 3, 0), (1, 0, 4, 0)])
def test_guarded_strided_resolve(P, n_edge, Sa, extra):
    from oi_amd import lib, ops
    N = 17 * 16
    rs = np.random.RandomState(P * 1000 + n_edge + Sa)
    slot = np.full(N, -1, np.int32)
    slot[rs.permutation(N)[:n_edge]] = rs.permutation(n_edge).astype(np.int32)
    n_sub = (Sa - 1) * n_edge
    stride = n_sub + extra
    centre, sub = rs.rand(P, N).astype(np.float32), rs.rand(P, stride).astype(np.float32)
    d_centre, d_slot = guarded_copy(_cuda(centre), "centre"), guarded_copy(_cuda(slot, torch.int32), "edge_slot")
    d_sub = guarded_copy(_cuda(sub), "sub") if n_edge else None
    out = guarded_empty((P, N), what="out")
    L_ = lib.load()
    assert L_.oi_aa_resolve_strided(_p(d_centre), _p(d_sub) if n_edge else None, stride, _p(d_slot), N, n_edge, Sa, P, _p(out),
                                    ops._stream()) == 0
    ref = AR.resolve(centre, sub[:, :n_sub], slot, Sa)
    assert np.array_equal(_f32(out).view(np.uint32), ref.view(np.uint32))
    if n_edge == 0:
        assert _same_bits(out, d_centre)
    if extra == 0 and n_edge:                                                        # oi_aa_resolve is the call at the dense stride
        dense = guarded_empty((P, N), what="dense")
        assert L_.oi_aa_resolve(_p(d_centre), _p(d_sub), _p(d_slot), N, n_edge, Sa, P, _p(dense), ops._stream()) == 0
        assert _same_bits(out, dense)
    # the wrapper: the stride is the width of `sub`
    assert _same_bits(ops.aa_resolve_strided(d_centre, d_sub, d_slot, n_edge, Sa), out)


def test_refused_arguments_launch_nothing():
    from oi_amd import lib, ops
    L_, st = lib.load(), ops._stream()
    buf = torch.zeros(4096, device="cuda")
    p = _p(buf)
    E, N = 2, 16
    arr, live, B = _guarded_batch(E, N, "refused", must_write=False)
    ref = ctypes.byref(B)
    bad = [
        L_.oi_scene_aa_classify(p, p, p, p, p, E, N, 4, 8, 1.0, 0.5, p, p, p, st),      # plane_threshold outside [0, 1)
        L_.oi_scene_aa_classify(p, p, p, p, p, E, N, 4, 8, 0.5, float("nan"), p, p, p, st),
        L_.oi_scene_aa_classify(p, p, p, p, p, E, N, N + 1, 8, 0.5, 0.5, p, p, p, st),  # more visible hits than rays
        L_.oi_scene_aa_classify(p, p, p, None, p, E, N, 4, 8, 0.5, 0.5, p, p, p, st),   # null hit arrays with n_pad > 0
        L_.oi_scene_aa_classify(p, None, p, p, p, E, N, 4, 8, 0.5, 0.5, p, p, p, st),
        L_.oi_scene_aa_classify(p, p, p, p, p, 0, N, 4, 8, 0.5, 0.5, p, p, p, st),      # E = 0
        L_.oi_scene_aa_classify(p, p, p, p, p, E, N, 4, 0, 0.5, 0.5, p, p, p, st),      # S = 0
        L_.oi_scene_aa_begin(ref, p, p, p, 4, 8, p, 17, p, 2, st),                      # N = 16 < (Sa - 1) * n_edge = 17
        L_.oi_scene_aa_begin(ref, p, p, p, 4, 8, p, 6, p, 4, st),                       # N = 16 < 18
        L_.oi_scene_aa_begin(ref, p, p, p, 4, 1, p, 1, p, 2, st),                       # S = 1
        L_.oi_scene_aa_begin(ref, p, p, p, 4, 8, p, 4, p, 1, st),                       # Sa = 1
        L_.oi_scene_aa_begin(ref, p, p, p, 4, 8, p, 1, p, 65, st),
        L_.oi_scene_aa_begin(ref, p, p, p, 4, 8, p, 0, p, 2, st),                       # n_edge = 0
        L_.oi_scene_aa_begin(ref, p, p, p, 0, 8, p, 4, p, 2, st),                       # W = 0
        L_.oi_scene_aa_begin(ref, p, p, None, 4, 8, p, 4, p, 2, st),                    # null window
        L_.oi_scene_aa_begin(None, p, p, p, 4, 8, p, 4, p, 2, st),
        L_.oi_aa_resolve_strided(p, p, 5, p, 4, 2, 4, 1, p, st),                        # stride 5 < (Sa - 1) * n_edge = 6
        L_.oi_aa_resolve_strided(p, p, 6, p, 4, 2, 1, 1, p, st),                        # Sa = 1
        L_.oi_aa_resolve_strided(p, None, 6, p, 4, 2, 4, 1, p, st),                     # sub missing with flagged pixels
        L_.oi_aa_resolve_strided(p, p, 20, p, 4, 5, 4, 1, p, st),                       # more flagged pixels than pixels
        L_.oi_aa_resolve_strided(p, p, 6, p, 4, 2, 4, 0, p, st),                        # P = 0
    ]
    assert all(rc < 0 for rc in bad), bad
    torch.cuda.synchronize()
    assert not bool(buf.any())
    for k, v in list(arr.items()) + [("live", live)]:
        fresh = guarded_empty(tuple(v.shape), v.dtype, what="pattern", must_write=False)
        assert torch.equal(v.view(torch.uint8), fresh.view(torch.uint8)), k               # still poison: nothing ran
