"""CPU checks of the ground plane of a scene (include/oi_ground.h; oi_amd.scene.Ground): header <=>
library <=> binding, the C ABI's refusals (checked on the host before any launch, the pointers never dereferenced), the Python
refusals, the self-consistency of the restatement the GPU tests compare against (tests/helpers/ground_ref.py: against per-ray
loops, chunked == unchunked), and the CONDITIONS the GPU test's analytic two-sphere scene must satisfy on float64 alone: the
number of ground pixels, that none hides an instance, no depth tie, enough shadowed pixels per sphere, the exclusion caps of its
shadow and ambient rays with the real sampler, and the plane that cuts sphere 0."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import cabi
from helpers import env_ref as EV
from helpers import ground_ref as GR
from helpers import local_light_ref as LL
from helpers import occlusion_ref as R
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T
from test_scene_cpu import fake_gen

ENTRIES = ["oi_ground_begin", "oi_ground_occlude", "oi_ground_rays_begin", "oi_ground_resolve", "oi_ground_shade"]

_lib = cabi.built_lib


def test_header_library_and_binding_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_ground.h", lib)
    assert sorted(names) == ENTRIES == lib.symbols("oi_ground.h")
    assert mirrors == []                                             # no struct of its own: oi_scene_light.h's parameters
    _, structs = cabi.parse(text := cabi.read("oi_ground.h"))
    assert structs == {}
    assert int(re.search(r"#define OI_GROUND_FLOATS (\d+)", text).group(1)) == lib.GROUND_FLOATS == GR.FLOATS == 12
    for name in ("CAP", "HEMISPHERE", "LOCAL"):
        assert int(re.search(rf"#define OI_GROUND_RAYS_{name} (\d+)", text).group(1)) == getattr(lib, f"GROUND_RAYS_{name}")
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"ground.hip"' in src and "include/oi_ground.h" in src
    # nothing was added to the headers whose entry lists other tests pin
    for header, n in (("oi_scene.h", 7), ("oi_scene_light.h", 7), ("oi_local_light.h", 4), ("oi_occlusion.h", 5),
                      ("oi_trace_batch.h", 5), ("oi_scene_aa.h", 3), ("oi_scene_gloss.h", 3), ("oi_scene_bounce.h", 3)):
        assert len(lib.symbols(header)) == n, header


def invalid_argument_cases(lib, L, f):
    """(call, entry, text of the message) of the refusals; f: a non-null pointer for every array (never dereferenced: each
    call returns before any launch)."""
    keep = []

    def batch(E=3, N=48, live=f, **kw):
        b = lib.TraceBatch()
        b.s.N, b.E, b.live = N, E, live
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(b.s, n, kw.get(n, f))
        keep.append(b)
        return ctypes.byref(b)

    def rays(b=None, mode=0, c2w=f, sS=8, rec=f, gt=f, **kw):
        """Defaults: E = 3 occluders, L = 2 lights, S = 4 strata, the chunk [1, 4), n_g = 8: N = 2 * 3 * 8 = 48."""
        P = lib.SceneOcclusionParams()
        P.L, P.S, P.j0, P.Sc = kw.get("L", 2), kw.get("S", 4), kw.get("j0", 1), kw.get("Sc", 3)
        P.ambient = kw.get("ambient", int(mode == 1))
        P.seed, P.bias, P.distance = 7, kw.get("bias", 1e-2), kw.get("distance", 0.5)
        P.n_pad, P.n_vis = 0, kw.get("n_g", 8)
        for n in ("pixel", "lights", "radius", "w2b"):                        # the other pointers are not read: left NULL
            setattr(P, n, kw.get(n, f))
        keep.append(P)
        return L.oi_ground_rays_begin(batch() if b is None else b, ctypes.byref(P), mode, c2w, f, sS, rec, gt, None)

    def shade(S=8, n_g=8, c2w=f, index=f, lights=f, Lt=1, local=0, image=f, matte=f):
        return L.oi_ground_shade(c2w, f, S, f, f, index, n_g, lights, Lt, local, f, f, image, f, f, f, f, f, f, f, matte, None)

    begin = lambda c2w=f, S=8, owner=f, owner_ray=f, t=f, W=4, E=3, out=f, count=f: L.oi_ground_begin(
        c2w, f, S, f, owner, owner_ray, t, f, W, E, out, f, count, None)
    res = lambda st=f, E=3, n_g=8, Lt=2, S=4, j0=1, Sc=3, last=1, count=f, out=f: L.oi_ground_resolve(st, E, n_g, Lt, S, j0, Sc, last,
                                                                                                 count, out, None)
    occ = lambda b=None, rec=f, elem=f, b2w=f, n_vis=8, limit=0.5: L.oi_ground_occlude(batch() if b is None else b, rec, elem, b2w,
                                                                                       n_vis, limit, None)
    inf, nan = float("inf"), float("nan")
    return [(lambda: begin(S=0), "oi_ground_begin", "S=0"),
            (lambda: begin(S=32769), "oi_ground_begin", "S=32769"),
            (lambda: begin(E=0), "oi_ground_begin", "E=0"),
            (lambda: begin(E=1025), "oi_ground_begin", "E=1025"),
            (lambda: begin(W=0), "oi_ground_begin", "W=0"),
            (lambda: begin(E=1024, W=1 << 11), "oi_ground_begin", "2^31"),
            (lambda: begin(c2w=None), "oi_ground_begin", "null pointer"),
            (lambda: begin(out=None), "oi_ground_begin", "null pointer"),
            (lambda: begin(count=None), "oi_ground_begin", "null pointer"),
            (lambda: begin(owner_ray=None), "oi_ground_begin", "null owner_ray"),
            (lambda: begin(t=None), "oi_ground_begin", "null owner_ray"),
            (lambda: L.oi_ground_rays_begin(None, None, 0, f, f, 8, f, f, None), "oi_ground_rays_begin", "null batch"),
            (lambda: L.oi_ground_rays_begin(batch(), None, 0, f, f, 8, f, f, None), "oi_ground_rays_begin", "null params"),
            (lambda: rays(batch(E=0)), "oi_ground_rays_begin", "E=0"),
            (lambda: rays(batch(live=None)), "oi_ground_rays_begin", "null live"),
            (lambda: rays(batch(status=None)), "oi_ground_rays_begin", "null pointer in the state"),
            (lambda: rays(sS=0), "oi_ground_rays_begin", "S=0"),
            (lambda: rays(n_g=0), "oi_ground_rays_begin", "n_g=0"),
            (lambda: rays(n_g=65), "oi_ground_rays_begin", "n_g=65"),
            (lambda: rays(gt=None), "oi_ground_rays_begin", "null pointer among the ground"),
            (lambda: rays(pixel=None), "oi_ground_rays_begin", "null pointer among the ground"),
            (lambda: rays(rec=None), "oi_ground_rays_begin", "null pointer among the ground"),
            (lambda: rays(L=0), "oi_ground_rays_begin", "L=0"),
            (lambda: rays(L=257), "oi_ground_rays_begin", "L=257"),
            (lambda: rays(S=0), "oi_ground_rays_begin", "S=0"),
            (lambda: rays(S=257), "oi_ground_rays_begin", "S=257"),
            (lambda: rays(j0=-1), "oi_ground_rays_begin", "j0=-1"),
            (lambda: rays(Sc=0), "oi_ground_rays_begin", "Sc=0"),
            (lambda: rays(j0=2), "oi_ground_rays_begin", "j0=2, Sc=3, S=4"),
            (lambda: rays(mode=3), "oi_ground_rays_begin", "mode=3"),
            (lambda: rays(mode=-1), "oi_ground_rays_begin", "mode=-1"),
            (lambda: rays(mode=1), "oi_ground_rays_begin", "L=2 with the hemisphere"),
            (lambda: rays(mode=0, ambient=1), "oi_ground_rays_begin", "ambient=1 with mode=0"),
            (lambda: rays(batch(N=24), mode=1, L=1, ambient=0), "oi_ground_rays_begin", "ambient=0 with mode=1"),
            (lambda: rays(Sc=2), "oi_ground_rays_begin", "N must be L * Sc * n_g"),
            (lambda: rays(bias=-1.0), "oi_ground_rays_begin", "bias"),
            (lambda: rays(bias=inf), "oi_ground_rays_begin", "bias"),
            (lambda: rays(bias=nan), "oi_ground_rays_begin", "bias"),
            (lambda: rays(batch(N=24), L=1, mode=1, distance=0.0), "oi_ground_rays_begin", "distance"),
            (lambda: rays(batch(N=24), L=1, mode=1, distance=nan), "oi_ground_rays_begin", "distance"),
            (lambda: rays(w2b=None), "oi_ground_rays_begin", "null input"),
            (lambda: rays(lights=None), "oi_ground_rays_begin", "null input"),
            (lambda: rays(radius=None), "oi_ground_rays_begin", "null input"),
            (lambda: rays(mode=2, lights=None), "oi_ground_rays_begin", "null input"),
            (lambda: res(E=0), "oi_ground_resolve", "E=0"),
            (lambda: res(Lt=257), "oi_ground_resolve", "L=257"),
            (lambda: res(S=257), "oi_ground_resolve", "S=257"),
            (lambda: res(j0=2), "oi_ground_resolve", "j0=2"),
            (lambda: res(Sc=0), "oi_ground_resolve", "Sc=0"),
            (lambda: res(n_g=0), "oi_ground_resolve", "n_g=0"),
            (lambda: res(E=1024, Lt=256, S=256, j0=0, Sc=256, n_g=1 << 10), "oi_ground_resolve", "2^31"),
            (lambda: res(st=None), "oi_ground_resolve", "null pointer"),
            (lambda: res(count=None), "oi_ground_resolve", "null pointer"),
            (lambda: res(out=None), "oi_ground_resolve", "null pointer"),
            (lambda: shade(S=0), "oi_ground_shade", "S=0"),
            (lambda: shade(n_g=0), "oi_ground_shade", "n_g=0"),
            (lambda: shade(n_g=65), "oi_ground_shade", "n_g=65"),
            (lambda: shade(c2w=None), "oi_ground_shade", "null pointer among the ground"),
            (lambda: shade(index=None), "oi_ground_shade", "null pointer among the ground"),
            (lambda: shade(Lt=0), "oi_ground_shade", "L=0"),
            (lambda: shade(Lt=257), "oi_ground_shade", "L=257"),
            (lambda: shade(Lt=0, image=None), "oi_ground_shade", "L=0"),         # a matte alone needs the lights too
            (lambda: shade(lights=None), "oi_ground_shade", "null lights"),
            (lambda: L.oi_ground_occlude(None, f, f, f, 8, 0.5, None), "oi_ground_occlude", "null batch"),
            (lambda: occ(batch(E=1025)), "oi_ground_occlude", "E=1025"),
            (lambda: occ(n_vis=0), "oi_ground_occlude", "n_vis=0"),
            (lambda: occ(n_vis=7), "oi_ground_occlude", "multiple of n_vis"),
            (lambda: occ(n_vis=96), "oi_ground_occlude", "n_vis=96"),
            (lambda: occ(limit=0.0), "oi_ground_occlude", "limit"),
            (lambda: occ(limit=-1.0), "oi_ground_occlude", "limit"),
            (lambda: occ(limit=nan), "oi_ground_occlude", "limit"),
            (lambda: occ(rec=None), "oi_ground_occlude", "null pointer"),
            (lambda: occ(elem=None), "oi_ground_occlude", "null pointer"),
            (lambda: occ(b2w=None), "oi_ground_occlude", "null pointer")]


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)
    cases = invalid_argument_cases(lib, L, f)
    assert {e for _, e, _ in cases} == set(ENTRIES)
    for call, entry, text in cases:
        assert call() == -1, (entry, text)
        msg = L.oi_last_error().decode()
        assert msg.startswith(entry) and text in msg, (entry, text, msg)


def test_python_refusals():
    from oi_amd import inference, scene
    from oi_amd.relight import LocalLight
    up = (0.0, -1.0, 0.0)
    for bad in ((0.0, -1.1, 0.0), (0.0, 0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, -1.0)):
        with pytest.raises(ValueError, match="normal"):
            scene.Ground(bad, 0.0)
    scene.Ground((0.0, -1.00005, 0.0), 0.0)                       # unit to 1e-4
    for bad in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="offset"):
            scene.Ground(up, bad)
        with pytest.raises(ValueError, match="centre"):
            scene.Ground(up, 0.0, centre=(0.0, bad, 0.0))
    for bad in ((0.5, 1.1, 0.5), (-0.1, 0.5, 0.5), (0.5, float("nan"), 0.5)):
        with pytest.raises(ValueError, match="albedo"):
            scene.Ground(up, 0.0, albedo=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="extent"):
            scene.Ground(up, 0.0, extent=bad)
    with pytest.raises(ValueError, match="points"):
        scene.Ground.below(np.zeros((0, 3)), up)
    g = scene.Ground(up, -0.6, extent=4.0)
    assert g.packed().dtype == np.float32 and g.packed().tolist() == pytest.approx([0, -1, 0, -0.6, 0.8, 0.8, 0.8, 4, 0, 0, 0, 0])
    assert scene.Ground.through((1.0, 2.0, 3.0), up).offset == -2.0
    pts = np.array([[0.0, 0.5, 0.0], [0.0, -0.25, 1.0]])
    assert scene.Ground.below(pts, up, gap=0.02).offset == pytest.approx(-0.52)
    assert scene.Ground.below(torch.tensor(pts), up).offset == pytest.approx(-0.5) and np.isinf(scene.Ground(up, 0.0).packed()[7])
    gen = fake_gen()
    z, centre = torch.zeros(64), T.pose("centre")
    with pytest.raises(ValueError, match="ground with aa_samples=4"):
        scene.render_scene(gen, [z], [centre], ground=g, aa_samples=4)
    with pytest.raises(ValueError, match="an oi_amd.scene.Ground"):
        scene.render_scene(gen, [z], [centre], ground=(0, -1, 0, 0))
    with pytest.raises(ValueError, match="ground with aa_samples=2"):
        inference.scene_light_walk(gen, [z], [centre], n_frames=2, ground=g, aa_samples=2)
    with pytest.raises(ValueError, match="ground with aa_samples=2"):
        inference.scene_light_orbit(gen, [z], [centre], LocalLight(position=(0.0, -2.0, 0.0)), n_frames=2, ground=g, aa_samples=2)
    with pytest.raises(ValueError, match="environment paths"):
        scene.render_scene_env(gen, [z], [centre], [], ground=g)
    s = scene.SceneSurface.__new__(scene.SceneSurface)
    s.E, s.S, s.N, s.W, s.n_vis, s.n_pad, s.aa, s._grounds = 2, 9, 16, 4, [100, 50], 100, None, {}
    with pytest.raises(ValueError, match="environment paths"):
        from oi_amd.envlight import EnvLight
        inference.scene_env_walk(gen, [z], [centre], EnvLight.constant(1.0), n_frames=2, ground=g)
    # the camera must be above the plane: n . eye > offset
    s.b2w, s.c2w = torch.zeros(2, 4, 4), torch.eye(4)
    s.c2w[2, 3] = -6.0
    for bad in (scene.Ground(up, 0.0), scene.Ground(up, 0.5), scene.Ground((0.0, 0.0, 1.0), -6.0)):
        with pytest.raises(ValueError, match="on or below the plane"):
            s.ground(bad)
    with pytest.raises(ValueError, match="an oi_amd.scene.Ground"):
        s.ground("floor")
    s.aa = type("AA", (), {"S": 4})()
    with pytest.raises(ValueError, match="aa_samples=4"):
        s.ground(g)
    with pytest.raises(ValueError, match="shadow_matte"):
        scene.composite_over({"image": torch.zeros(1, 3, 2, 2)}, torch.zeros(3, 2, 2))
    # a chunk of one sample that does not fit: refused naming the counts E * L * n_g, before anything is launched
    gs = scene.GroundSurface.__new__(scene.GroundSurface)
    s.aa = None
    gs.scene, gs.n_g, gs.record = s, 150, torch.zeros(12)
    with pytest.raises(ValueError, match=r"2 instances x 2 lights x 150 ground points = E \* L \* n_g = 600 rays per sample"):
        gs.visibility(torch.zeros(2, 16), [0.1, 0.0], samples=4, max_shadow_rays=599)
    with pytest.raises(ValueError, match=r"E \* L \* n_g = 300 rays per sample"):
        gs.ambient(16, 0.5, max_shadow_rays=299)
    with pytest.raises(ValueError, match=r"E \* L \* n_g = 300 rays per sample"):
        gs.local_visibility(torch.zeros(1, 20), 4, max_shadow_rays=299)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against per-ray loops
# ---------------------------------------------------------------------------------------------------------------------
def _random_case(rs, E=3, n=11, S=9):
    w2b = []
    for e in range(E):
        m = np.eye(4)
        m[:3, :3] = EV.random_rotation(rs)
        m[:3, 3] = rs.randn(3) * 0.8
        w2b.append(m)
    nrm = EV.random_rotation(rs)[0]
    rec = GR.record(nrm, 0.3, (0.7, 0.6, 0.5), 5.0, (0.1, 0.2, 0.3))
    # points on the plane
    t1, t2 = R.frame(nrm)
    p = 0.3 * nrm + rs.randn(n, 1) * t1 + rs.randn(n, 1) * t2
    pixel = rs.permutation(S * S)[:n]
    return np.stack(w2b), rec, p, pixel


def _one_ray(rec, p, w2b_e, d_world, limit, bias):
    """One element's ray by the header's words, scalar by scalar."""
    o = w2b_e[:3, :3] @ (p + bias * rec[:3]) + w2b_e[:3, 3]
    d = w2b_e[:3, :3] @ d_world
    dd, od = d @ d, o @ d
    mid = -od / dd
    c = o + mid * d
    c2 = c @ c
    if not c2 < 1.0:
        return o, d, 0.0, 0.0, MISS_
    h = np.sqrt((1.0 - c2) / dd)
    near, far = max(mid - h, 0.0), mid + h
    if not far > 0 or not near < limit:
        return o, d, 0.0, 0.0, MISS_
    return o, d, near, min(far, limit), GR.MARCH


MISS_ = GR.MISS


@pytest.mark.parametrize("mode", ["caps", "hemisphere", "local"])
def test_restated_rays_against_per_ray_loops(mode):
    rs = np.random.RandomState(5)
    w2b, rec, p, pixel = _random_case(rs)
    S, j0, Sc, bias, n = 4, 1, 3, 1e-2, len(p)
    lights = [tuple(rec[:3] + 0.3 * rs.randn(3)), tuple(-rec[:3] + 0.1 * rs.randn(3))]      # the second from below: BACKFACING
    local = np.array([LL.record(tuple(p[0] + 0.8 * rec[:3]), 0.05), LL.record(tuple(p[1] + 0.005 * rec[:3]), 0.1)])
    kw = {"caps": dict(light_dirs=lights, radius=[0.1, 0.0]), "hemisphere": dict(distance=0.7), "local": dict(local=local)}[mode]
    r = GR.rays(rec, p, pixel, w2b, bias, S, j0, Sc, GR.SEED, **kw)
    L = r["d_world"].shape[0]
    assert r["status"].shape == (3, L, Sc, n)
    u1, u2 = R.sample_numbers(pixel, GR.SEED, S)
    seen = set()
    for l in range(L):
        for jj in range(Sc):
            for g in range(n):
                j = j0 + jj
                limit, inside = np.inf, False
                if mode == "hemisphere":
                    d = R.directions(rec[:3], np.sqrt(u1[j]), np.sqrt(1 - u1[j]), u2[j, g])
                    limit = 0.7
                elif mode == "caps":
                    ax = T.light_object_dir(lights[l], np.eye(4))
                    ca = 1.0 - u1[j] * (1.0 - np.cos([0.1, 0.0][l]))
                    d = R.directions(ax, np.sqrt(max(0.0, 1 - ca * ca)), ca, u2[j, g])
                else:
                    o = p[g] + bias * rec[:3]
                    a = LL.aimed(o[None], rec[None, :3], pixel[g:g + 1], local[l][:3], local[l][3], S, GR.SEED, j, 1)
                    d, limit, inside = a["d"][0, 0], a["t_light"][0, 0], bool(a["inside"][0])
                    if inside:
                        d = np.zeros(3)
                assert np.abs(r["d_world"][l, jj, g] - d).max() < 1e-12
                facing = d @ rec[:3] > 0
                for e in range(3):
                    if inside:
                        o_e, d_e = w2b[e][:3, :3] @ (p[g] + bias * rec[:3]) + w2b[e][:3, 3], np.zeros(3)
                        near, far, st = 0.0, 0.0, GR.MISS
                    else:
                        o_e, d_e, near, far, st = _one_ray(rec, p[g], w2b[e], d, limit, bias)
                        if not facing:
                            near, far, st = 0.0, 0.0, GR.BACKFACING
                    seen.add((mode, st))
                    assert r["status"][e, l, jj, g] == st
                    assert abs(r["near"][e, l, jj, g] - near) < 1e-12 and abs(r["far"][e, l, jj, g] - far) < 1e-12
                    assert np.abs(r["o"][e, l, jj, g] - o_e).max() < 1e-12 and np.abs(r["d"][e, l, jj, g] - d_e).max() < 1e-12
    assert {s for _, s in seen} >= {GR.MARCH, GR.MISS} and (mode == "hemisphere" or (mode, GR.BACKFACING) in seen)
    if mode == "local":
        assert r["limit"].min() < 0.1 and (r["status"][:, 1, :, 1] == GR.MISS).all()        # the origin inside light 1: lit


def test_chunked_equals_unchunked_and_resolve():
    rs = np.random.RandomState(6)
    w2b, rec, p, pixel = _random_case(rs)
    S, n = 4, len(p)
    whole = GR.rays(rec, p, pixel, w2b, 1e-2, S, 0, S, GR.SEED, distance=1.5)
    status = rs.choice([GR.MISS, GR.HIT, GR.BACKFACING, T.LIMIT], size=whole["status"].shape, p=[0.7, 0.1, 0.1, 0.1]).astype(np.uint8)
    for cuts in ([4], [1, 1, 1, 1], [1, 3]):
        j0, parts, sts = 0, [], []
        for c in cuts:
            parts.append(GR.rays(rec, p, pixel, w2b, 1e-2, S, j0, c, GR.SEED, distance=1.5))
            sts.append(status[:, :, j0:j0 + c])
            j0 += c
        for k in ("o", "d", "near", "far", "status"):
            assert np.array_equal(np.concatenate([x[k] for x in parts], 2), whole[k]), (cuts, k)
        count, out = GR.counts(sts, S)
        loop = np.zeros((1, n), dtype=np.int64)
        for g in range(n):
            for j in range(S):
                loop[0, g] += all(status[e, 0, j, g] == GR.MISS for e in range(3))
        assert np.array_equal(count, loop) and np.array_equal(out, loop / 4.0)


def test_restated_classification_shade_and_occlude_against_loops():
    rs = np.random.RandomState(7)
    sc = SR.analytic_scene()
    rec = GR.analytic_record()
    S = sc["S"]
    owner = np.where(rs.rand(S * S) < 0.3, rs.randint(0, 2, S * S), -1)
    t_owner = rs.uniform(3.0, 12.0, S * S)
    g = GR.classify(sc["c2w"], sc["K_inv"], S, rec, owner, t_owner)
    o, d = SR.scene_rays(sc["c2w"], sc["K_inv"], S)
    d = d.reshape(-1, 3)
    for q in rs.permutation(S * S)[:200]:
        nd = d[q] @ rec[:3]
        t = (rec[3] - rec[:3] @ o) / nd
        pt = o + t * d[q]
        expect = nd < -1e-6 and t > 0 and np.linalg.norm(pt - rec[8:11]) <= rec[7] and (owner[q] < 0 or t < t_owner[q])
        assert bool(g["ground"][q]) == bool(expect) and (np.isnan(g["t"][q]) != bool(expect))
    assert 0 < (g["front"] & ~g["ground"]).sum() and g["ground"].sum() > 100          # owners hide some of it
    tie = GR.classify(sc["c2w"], sc["K_inv"], S, rec, np.zeros(S * S, dtype=int), g["t_all"])
    assert not tie["ground"].any()                                                       # an equal depth goes to the instance
    # shade: per point, light and channel
    q = np.nonzero(g["ground"])[0][::40]
    pts = g["p"][q]
    lights = np.array([T.light_block(GR.AN_GROUND_LIGHT), T.light_block((0.2, 0.9, -0.4), 0.2, 0.5)])
    vis, ao = rs.rand(2, len(q)), rs.rand(len(q))
    img, matte, bar, bar_m = GR.shade(rec, pts, lights, False, vis, ao)
    assert (bar > 0).all() and (bar < 1e-6).all() and (bar_m < 1e-5).all()
    for l in range(2):
        ndl = max(T.light_object_dir(lights[l][:3], np.eye(4)) @ rec[:3], 0.0)
        for c in range(3):
            full = (lights[l][4 + c] + lights[l][8 + c] * ndl) * rec[4 + c]
            val = (lights[l][4 + c] * ao + lights[l][8 + c] * ndl * vis[l]) * rec[4 + c]
            assert np.allclose(img[l, c], val, rtol=0, atol=1e-15) and np.allclose(matte[l, c], val / full, rtol=0, atol=1e-15)
    assert (matte[1] == ao[None]).all() or np.allclose(matte[1], ao[None])               # a light from below: the ambient term alone
    black, m0, _, _ = GR.shade(GR.record(rec[:3], rec[3], (0.0, 0.5, 1.0)), pts, lights[:1])
    assert not black[0, 0].any() and (m0[0, 0] == 1).all() and (m0[0, 1] == 1).all()      # denominator 0: matte 1; nothing occluded: 1
    above = tuple(pts[len(pts) // 2] + 1.0 * rec[:3])                                    # the cone's edge falls among the points
    loc = np.array([LL.record(above, 0.05, reference_distance=1.2, cone_axis=(0.0, 1.0, 0.1), cone_inner=0.3, cone_outer=1.0)])
    img, matte, bar, _ = GR.shade(rec, pts, loc, True, vis[:1], ao)
    assert (bar >= 0).all() and (bar < 1e-5).all()
    l, att, spot = LL.factors(pts, loc[0], np.eye(4))
    for i in range(len(q)):
        k = att[i] * spot[i]
        val = (loc[0][4] * ao[i] + loc[0][8] * max(l[i] @ rec[:3], 0.0) * k * vis[0, i]) * rec[4]
        assert abs(img[0, 0, i] - val) < 1e-15
    assert spot.min() < 1 and spot.max() > 0
    # occlude: per ray
    E, n_vis, Q = 2, 5, 15
    b2w = np.stack([SR.rigid_inverse(m) for m in _random_case(rs, E)[0]])
    elem = np.array([0, 0, 1, 1, 0])
    ob, db = rs.randn(E, Q, 3) * 0.3, rs.randn(E, Q, 3)
    db /= np.linalg.norm(db, axis=-1, keepdims=True)
    status = rs.choice([GR.MISS, GR.HIT, GR.BACKFACING], size=(E, Q), p=[0.7, 0.15, 0.15]).astype(np.uint8)
    plane = GR.record((0.0, -1.0, 0.0), -0.4, extent=3.0)
    for limit in (np.inf, 0.8):
        out, t, rim = GR.occlude(status, ob, db, elem, b2w, plane, limit)
        changed = 0
        for qq in range(Q):
            e = elem[qq % n_vis]
            ow, dw = b2w[e][:3, :3] @ ob[e, qq] + b2w[e][:3, 3], b2w[e][:3, :3] @ db[e, qq]
            tt = (plane[3] - plane[:3] @ ow) / (plane[:3] @ dw)
            hit = 0 < tt < limit and np.linalg.norm(ow + tt * dw - plane[8:11]) <= plane[7]
            assert out[e, qq] == (GR.HIT if (status[e, qq] == GR.MISS and hit) else status[e, qq])
            assert np.array_equal(out[1 - e, qq], status[1 - e, qq])                     # only the owner's row
            changed += out[e, qq] != status[e, qq]
        assert changed > 0


# ---------------------------------------------------------------------------------------------------------------------
# the conditions of the analytic scene, on float64 alone
# ---------------------------------------------------------------------------------------------------------------------
def test_analytic_scene_conditions():
    sc = SR.analytic_scene()
    cf = SR.analytic_closed_form(sc)
    rec = GR.analytic_record()
    g = GR.analytic_ground(sc, cf, rec)
    owned = cf["owner"] >= 0
    assert int(g["ground"].sum()) == 358 and not (g["ground"] & owned).any()              # none hides an instance
    assert not ((np.abs(g["nd"] + GR.FRONT) < GR.ND_BAND) | (np.abs(g["rim"]) < GR.RIM_BAND)).any()
    assert (~g["front"] & (g["nd"] < -GR.FRONT) & (g["t_all"] > 0)).any()                 # the rim of the disc is in the picture
    sh = GR.analytic_shadows(g)
    assert sh["blocked"].sum(1).tolist() == [14, 18] and int(sh["band"].sum()) == 0
    assert (sh["blocked"].sum(1) >= 10).all()
    # the ambient rays with the real sampler
    q = sh["q"]
    d = GR.world_directions(rec, q, GR.SEED, GR.AN_AO_S, 0, GR.AN_AO_S)["d"][0]
    o = np.broadcast_to(g["p"][q] + T.BIAS * rec[:3], d.shape)
    assert (d @ rec[:3] > 0).all()                                                        # the cosine hemisphere: every ray is traced
    blocked, band = SL.sphere_blocks(o, d, GR.AN_AO_DISTANCE)
    share, excluded = float(blocked.any(0).mean()), float(band.any(0).mean())
    print("analytic ground: ambient rays", d.shape[0] * d.shape[1], "blocked", share, "in the band", excluded)
    assert excluded <= R.EXCLUDED_CAP and share >= 0.05
    # the plane that cuts sphere 0
    cut = GR.analytic_record(GR.AN_CUT_OFFSET)
    gc = GR.analytic_ground(sc, cf, cut)
    hides = gc["ground"] & owned
    assert int(hides.sum()) >= 10 and (cf["owner"][hides] == 0).all()
    both = gc["front"] & owned
    ties = np.abs(gc["t_all"][both] - cf["depth"][both]) < SR.AN_DEPTH_GAP
    assert ties.sum() <= SR.AN_CAP * both.sum()      # (the silhouette pixels of the closed form are its own exclusion, under its own cap)
    assert (both & ~gc["ground"]).sum() >= 10                                             # and the sphere hides the ground too
