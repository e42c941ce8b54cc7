"""CPU checks of glossy environment lighting in scenes (include/oi_scene_gloss.h; oi_amd.scene): header
<=> library <=> binding, the C ABI's refusals (checked on the host before any launch), the Python refusals, the
self-consistency of the restatement the GPU tests compare against (tests/helpers/scene_gloss_ref.py: against per-ray loops,
chunked == unchunked), and the CONDITIONS the GPU test's analytic two-sphere scene must satisfy on float64 alone: the
exclusion cap of its lobe rays, and that the other sphere blocks enough of them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import cabi
from helpers import envgloss_ref as Q
from helpers import occlusion_ref as R
from helpers import scene_gloss_ref as SG
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T
from test_scene_cpu import fake_gen
from test_scene_light_cpu import _random_scene, _stub_scene

ENTRIES = ["oi_env_shade_glossy_dirs", "oi_scene_lobe_begin", "oi_scene_reflect"]
# the headers this one was not allowed to grow, and the number of entries other tests pin for them
PINNED = (("oi_scene_light.h", 7), ("oi_envgloss.h", 4), ("oi_scene.h", 7), ("oi_occlusion.h", 5), ("oi_envlight.h", 5),
          ("oi_trace_batch.h", 5))

_lib = cabi.built_lib


def test_header_library_and_binding_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_scene_gloss.h", lib)
    # no struct of its own: the lobe's begin takes oi_scene_light.h's parameters (bound as POINTER of their mirror) and its four
    # own arguments as plain ones, so the set of struct mirrors in oi_amd.lib is the parent's
    assert sorted(names) == ENTRIES == lib.symbols("oi_scene_gloss.h") and mirrors == []
    _, structs = cabi.parse(cabi.read("oi_scene_gloss.h"))
    assert sorted(structs) == []
    assert lib.SIGS["oi_scene_gloss.h"]["oi_scene_lobe_begin"][1][1] == ctypes.POINTER(lib.SceneOcclusionParams)
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"scene_gloss.hip"' in src and "include/oi_scene_gloss.h" in src
    for header, n in PINNED:
        assert len(lib.symbols(header)) == n, header
    text = cabi.read("oi_scene_gloss.h")
    assert not re.search(r"#\s*define\s+OI_", re.sub(r"#define OI_SCENE_GLOSS_H_", "", text))      # it borrows every limit


def invalid_argument_cases(lib, L, f, arrays=None):
    """(call, entry, text of the message) of the refusals; f: a non-null pointer for every array (never dereferenced: each
    call returns before any launch), arrays: {field: pointer} to use instead for the state."""
    arrays = arrays or {}
    keep = []

    def batch(E=3, N=24, live=f, **kw):
        b = lib.TraceBatch()
        b.s.N, b.E, b.live = N, E, live
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(b.s, n, kw.get(n, arrays.get(n, f)))
        keep.append(b)
        return ctypes.byref(b)

    def begin(b=None, **kw):
        """Defaults: E = 3 occluders, S = 4 strata, the chunk [1, 4), n_vis = 8: N = 3 * 8 = 24; 16 primary rays per element."""
        P = lib.SceneOcclusionParams()
        P.L, P.S, P.j0, P.Sc, P.ambient = kw.get("L", 1), kw.get("S", 4), kw.get("j0", 1), kw.get("Sc", 3), 1
        P.seed, P.bias, P.distance = 7, kw.get("bias", 1e-2), float("inf")
        P.n_pad, P.n_vis = kw.get("n_pad", 5), kw.get("n_vis", 8)
        for n, _ in lib.SceneOcclusionParams._fields_[10:]:
            setattr(P, n, kw.get(n, None if n in ("lights", "radius") else f))
        keep.append(P)
        return L.oi_scene_lobe_begin(batch() if b is None else b, ctypes.byref(P), kw.get("rays_o", f), kw.get("vis_index", f),
                                     kw.get("N", 16), kw.get("shininess", 10.0), None)

    refl = lambda ro=f, grad=f, n_pad=5, E=3, N=16, sS=8, out=f: L.oi_scene_reflect(ro, f, grad, n_pad, f, f, f, f, E, N, sS, out, None)

    def shade(dirs=f, glossy=f, M=2, Hp=4, Wp=8, index=(0, 1), rot=f, ks=f, spec=f, **kw):
        P = lib.EnvShadeParams()
        P.N, P.n_hit, P.F = kw.get("N", 32), kw.get("n_hit", 20), kw.get("F", 2)
        for n, _ in lib.EnvShadeParams._fields_[3:]:
            setattr(P, n, kw.get(n, f))
        idx = None if index is None else (ctypes.c_int * len(index))(*index)
        keep.append((P, idx))
        return L.oi_env_shade_glossy_dirs(ctypes.byref(P), dirs, f, glossy, M, Hp, Wp, idx, rot, ks, spec, None)

    inf, nan = float("inf"), float("nan")
    return [(lambda: L.oi_scene_lobe_begin(None, None, f, f, 16, 10.0, None), "oi_scene_lobe_begin", "null batch"),
            (lambda: L.oi_scene_lobe_begin(batch(), None, f, f, 16, 10.0, None), "oi_scene_lobe_begin", "null params"),
            (lambda: begin(batch(E=0)), "oi_scene_lobe_begin", "E=0"),
            (lambda: begin(batch(live=None)), "oi_scene_lobe_begin", "null live"),
            (lambda: begin(batch(counts=None)), "oi_scene_lobe_begin", "null pointer"),
            (lambda: begin(S=0), "oi_scene_lobe_begin", "S=0"),
            (lambda: begin(S=257), "oi_scene_lobe_begin", "S=257"),
            (lambda: begin(j0=-1), "oi_scene_lobe_begin", "j0=-1"),
            (lambda: begin(Sc=0), "oi_scene_lobe_begin", "Sc=0"),
            (lambda: begin(j0=2), "oi_scene_lobe_begin", "j0=2, Sc=3, S=4"),
            (lambda: begin(batch(N=48), L=2), "oi_scene_lobe_begin", "L=2"),
            (lambda: begin(L=0), "oi_scene_lobe_begin", "L=0"),
            (lambda: begin(Sc=2), "oi_scene_lobe_begin", "N must be L * Sc * n_vis"),
            (lambda: begin(n_vis=0), "oi_scene_lobe_begin", "n_vis=0"),
            (lambda: begin(batch(N=48), n_vis=16), "oi_scene_lobe_begin", "n_vis=16"),
            (lambda: begin(n_pad=0), "oi_scene_lobe_begin", "n_pad=0"),
            (lambda: begin(batch(N=144), n_pad=17, n_vis=48), "oi_scene_lobe_begin", "n_pad=17"),
            (lambda: begin(N=0), "oi_scene_lobe_begin", "N=0"),
            (lambda: begin(shininess=0.5), "oi_scene_lobe_begin", "shininess"),
            (lambda: begin(shininess=4097.0), "oi_scene_lobe_begin", "shininess"),
            (lambda: begin(shininess=nan), "oi_scene_lobe_begin", "shininess"),
            (lambda: begin(shininess=inf), "oi_scene_lobe_begin", "shininess"),
            (lambda: begin(bias=-1.0), "oi_scene_lobe_begin", "bias"),
            (lambda: begin(bias=inf), "oi_scene_lobe_begin", "bias"),
            (lambda: begin(bias=nan), "oi_scene_lobe_begin", "bias"),
            (lambda: begin(elem=None), "oi_scene_lobe_begin", "null input"),
            (lambda: begin(pixel=None), "oi_scene_lobe_begin", "null input"),
            (lambda: begin(rays_o=None), "oi_scene_lobe_begin", "null input"),
            (lambda: begin(vis_index=None), "oi_scene_lobe_begin", "null input"),
            (lambda: refl(E=0), "oi_scene_reflect", "E=0"),
            (lambda: refl(E=1025), "oi_scene_reflect", "E=1025"),
            (lambda: refl(N=0), "oi_scene_reflect", "N=0"),
            (lambda: refl(n_pad=0), "oi_scene_reflect", "n_pad=0"),
            (lambda: refl(n_pad=17), "oi_scene_reflect", "n_pad=17"),
            (lambda: refl(sS=0), "oi_scene_reflect", "S=0"),
            (lambda: refl(sS=32769), "oi_scene_reflect", "S=32769"),
            (lambda: refl(ro=None), "oi_scene_reflect", "null pointer"),
            (lambda: refl(grad=None), "oi_scene_reflect", "null pointer"),
            (lambda: refl(out=None), "oi_scene_reflect", "null pointer"),
            (lambda: L.oi_env_shade_glossy_dirs(None, f, f, f, 1, 4, 8, None, f, f, f, None), "oi_env_shade_glossy_dirs", "null params"),
            (lambda: shade(N=0), "oi_env_shade_glossy_dirs", "N=0"),
            (lambda: shade(n_hit=33), "oi_env_shade_glossy_dirs", "n_hit=33"),
            (lambda: shade(F=0), "oi_env_shade_glossy_dirs", "F=0"),
            (lambda: shade(F=257), "oi_env_shade_glossy_dirs", "F=257"),
            (lambda: shade(transfer=None), "oi_env_shade_glossy_dirs", "null input"),
            (lambda: shade(shading=None, image=None, spec=None), "oi_env_shade_glossy_dirs", "no output"),
            (lambda: shade(rgb=None), "oi_env_shade_glossy_dirs", "null rgb"),
            (lambda: shade(M=0), "oi_env_shade_glossy_dirs", "M=0"),
            (lambda: shade(M=257), "oi_env_shade_glossy_dirs", "M=257"),
            (lambda: shade(Hp=0), "oi_env_shade_glossy_dirs", "Hp=0"),
            (lambda: shade(glossy=None), "oi_env_shade_glossy_dirs", "null glossy input"),
            (lambda: shade(index=None), "oi_env_shade_glossy_dirs", "null glossy input"),
            (lambda: shade(rot=None), "oi_env_shade_glossy_dirs", "null glossy input"),
            (lambda: shade(ks=None), "oi_env_shade_glossy_dirs", "null glossy input"),
            (lambda: shade(dirs=None), "oi_env_shade_glossy_dirs", "null dirs"),
            (lambda: shade(index=(0, 2)), "oi_env_shade_glossy_dirs", "map_index[1]=2"),
            (lambda: shade(index=(-1, 0)), "oi_env_shade_glossy_dirs", "map_index[0]=-1")]


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


def _stub_capture(glossy_samples=None, shininess=None):
    """A SceneTransfer that holds only what shade's refusals read."""
    from oi_amd import scene
    c = scene.SceneTransfer.__new__(scene.SceneTransfer)
    c.scene, c.S, c.glossy_samples, c.shininess, c.specular = _stub_scene(), 9, glossy_samples, shininess, (0.1, 0.1, 0.1)
    return c


def test_python_refusals():
    from oi_amd import inference, scene
    from oi_amd.envlight import EnvLight, EnvMap
    gen = fake_gen()
    z, centre = torch.zeros(64), T.pose("centre")
    for entry in (lambda **kw: scene.render_scene_env(gen, [z], [centre], [], **kw),
                  lambda **kw: inference.scene_env_walk(gen, [z], [centre], EnvLight.constant(1.0), **kw),
                  lambda **kw: _stub_scene().capture_transfer(4, **kw)):
        with pytest.raises(ValueError, match="shininess=10.0 without glossy_samples"):
            entry(shininess=10.0)
        for bad in (-1, 257, 1.5, True):
            with pytest.raises(ValueError, match="glossy_samples"):
                entry(glossy_samples=bad, shininess=10.0)
        for bad in (0.5, 4097, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="shininess"):
                entry(glossy_samples=4, shininess=bad)
    with pytest.raises(TypeError, match="EnvLight"):
        inference.scene_env_walk(gen, [z], [centre], env="sky", glossy_samples=4, shininess=10.0)
    # EnvMap objects whose maps are never read: the refusals come before anything is stacked or launched
    env = lambda s=10.0: EnvMap.__new__(EnvMap)
    m10, m20 = env(), env()
    m10.shininess, m20.shininess = 10.0, 20.0
    with pytest.raises(ValueError, match="no reflection-lobe trace"):
        _stub_capture().shade([m10])
    with pytest.raises(ValueError, match="EnvMap and EnvLight objects in one list"):
        _stub_capture(4, 10.0).shade([m10, EnvLight.constant(1.0)])
    with pytest.raises(ValueError, match="specular= needs EnvMap"):
        _stub_capture(4, 10.0).shade([EnvLight.constant(1.0)], specular=0.3)
    with pytest.raises(ValueError, match=r"shininess \[10.0, 20.0\], the capture's lobe is 10"):
        _stub_capture(4, 10.0).shade([m10, m20])
    for bad in (["sky"], [], [m10, "sky"]):
        with pytest.raises(ValueError, match="EnvLight objects only"):
            _stub_capture(4, 10.0).shade(bad)
    # a chunk of one sample that does not fit: refused naming the counts, before anything is launched
    with pytest.raises(ValueError, match=r"2 instances x 1 lights x 150 visible points = 300 rays per sample"):
        _stub_scene()._sampled("SceneSurface.lobe_visibility", 16, 0, 299, None, lobe=10.0)
    # the positional signature of _sampled is the parent's
    with pytest.raises(ValueError, match="300 rays per sample"):
        _stub_scene()._sampled("SceneSurface.ambient", 16, 0, 299, None, None, None, 0.5)


def test_restated_rays_against_a_per_ray_loop_and_chunked_equals_unchunked():
    rs = np.random.RandomState(17)
    sc = _random_scene(rs, E=3, n_pad=7)
    E, N, n = sc["E"], sc["W"] * sc["W"], len(sc["elem"])
    S, seed, bias, s = 5, 11, 1e-2, 10.0
    rays_o = rs.randn(E, N, 3) * 0.3 + np.array([0.0, 0.0, 3.0])
    vis_index = np.stack([rs.permutation(N) for _ in range(E)])
    eyes = SG.point_eyes(rays_o, vis_index, sc["offset"], sc["elem"])
    common = (sc["points"], sc["grad"], eyes, sc["offset"], sc["elem"], sc["pixel"], sc["position"], sc["normal_world"], sc["w2b"], bias, S)
    whole = SG.lobe_rays(*common, 0, S, s, seed)
    assert whole["status"].shape == (E, 1, S, n)
    seen = set()
    for g in range(n):
        e, k = sc["elem"][g], sc["slot"][g]
        assert np.array_equal(eyes[g], rays_o[e, vis_index[e, k]])
        nrm = SL.unit(sc["grad"][e, k])
        v = SL.unit(eyes[g] - sc["points"][e, k])
        r = 2.0 * (nrm @ v) * nrm - v
        u1, u2 = R.sample_numbers(np.array([sc["pixel"][g]]), seed, S)
        for j in range(S):
            c, sn = Q.lobe_angles(u1[j:j + 1], s)
            d = R.directions(r[None, None], sn[:, None], c[:, None], u2[j:j + 1])[0, 0]
            assert np.abs(d - whole["d_owner"][0, j, g]).max() < 1e-14 and abs(np.linalg.norm(d) - 1) < 1e-12
            assert abs(d @ r - c[0]) < 1e-12                                  # the polar angle is about r
            traced = nrm @ d > 0
            dw = sc["w2b"][e][:3, :3].T @ d
            for eo in range(E):
                st = whole["status"][eo, 0, j, g]
                if not traced:
                    assert st == SL.BACKFACING and whole["near"][eo, 0, j, g] == whole["far"][eo, 0, j, g] == 0
                    seen.add("back")
                elif eo == e:
                    o = sc["points"][e, k] + bias * nrm
                    assert st == SL.MARCH and whole["near"][eo, 0, j, g] == 0
                    assert abs(whole["far"][eo, 0, j, g] - float(R.unit_sphere_exit(o, d))) < 1e-14
                    assert np.abs(whole["o"][eo, 0, j, g] - o).max() < 1e-15 and np.abs(whole["d"][eo, 0, j, g] - d).max() < 1e-15
                    seen.add("own")
                else:
                    o = SR.transform(sc["w2b"][eo], (sc["position"][g] + bias * sc["normal_world"][g])[None])[0]
                    de = sc["w2b"][eo][:3, :3] @ dw
                    ent, near, far, _ = SR.cull(o, de)
                    assert st == (SL.MARCH if ent else SL.MISS)
                    if ent:
                        assert abs(whole["near"][eo, 0, j, g] - near) < 1e-14 and abs(whole["far"][eo, 0, j, g] - far) < 1e-14
                        assert np.abs(whole["o"][eo, 0, j, g] - o).max() < 1e-14 and np.abs(whole["d"][eo, 0, j, g] - de).max() < 1e-14
                    seen.add("entered" if ent else "culled")
    assert seen == {"own", "entered", "culled", "back"}
    for cuts in ([1] * S, [2, 3], [4, 1]):
        j0 = 0
        for c in cuts:
            part = SG.lobe_rays(*common, j0, c, s, seed)
            for key in ("d_owner", "o", "d", "near", "far", "status"):
                ax = 1 if key == "d_owner" else 2
                assert np.array_equal(part[key], np.take(whole[key], range(j0, j0 + c), axis=ax)), (key, cuts)
            j0 += c
    # the reflection plane and the shade with given directions, against per-pixel loops
    M = 30
    owner, owner_ray = np.full(M, -1), np.full(M, -1)
    vis_slot = np.full((E, N), -1)
    for e, nv in enumerate(sc["n_vis"]):
        q = rs.permutation(np.nonzero(owner < 0)[0])[:nv]
        owner[q], owner_ray[q] = e, vis_index[e, :nv]
        vis_slot[e, vis_index[e, :nv]] = np.arange(nv)
    plane = SG.reflection(rays_o, sc["points"], sc["grad"], owner, owner_ray, vis_slot, sc["w2b"])
    for q in range(M):
        if owner[q] < 0:
            assert not plane[q].any()
            continue
        e, k = owner[q], vis_slot[owner[q], owner_ray[q]]
        nrm, v = SL.unit(sc["grad"][e, k]), SL.unit(rays_o[e, owner_ray[q]] - sc["points"][e, k])
        want = sc["w2b"][e][:3, :3].T @ (2.0 * (nrm @ v) * nrm - v)
        assert np.abs(plane[q] - want).max() < 1e-14 and abs(np.linalg.norm(plane[q]) - 1) < 1e-12
    F, mask = 2, owner >= 0
    maps, rot = rs.randn(2, 3, 5, 9), np.stack([np.eye(3), sc["w2b"][0][:3, :3]])
    tr, envs, alb, vis, ks = rs.randn(9, M), rs.randn(F, 9, 3), rs.rand(M, 3), rs.rand(M), np.array([0.3, 0.2, 0.1])
    sh, img, spec, mag, look, d = SG.shade_dirs(tr, envs, mask, alb, plane, vis, maps, [1, 0], rot, ks, bg=(0.1, 0.2, 0.3))
    for f in range(F):
        for q in np.nonzero(mask)[0]:
            want = ks * vis[q] * Q.lookup(maps[[1, 0][f]], (rot[f].T @ plane[q])[None])[0]
            assert np.abs(spec[f, :, q] - want).max() < 1e-14
            assert np.abs(img[f, :, q] - (np.maximum(sh[f, :, q], 0) * alb[q] + want)).max() < 1e-14
    assert not spec[:, :, ~mask].any() and np.array_equal(img[0][:, ~mask], np.broadcast_to(np.array([[0.1], [0.2], [0.3]]), (3, int((~mask).sum()))))


def test_analytic_scene_rehearsal():
    """The GPU test's analytic two-sphere scene on float64 ALONE, seed 7, eye at the camera centre, 64 lobe rays per point at
    shininess 1 and 10: the facing rays excluded because float32 may decide them either way (closest approach within
    AN_SHADOW_EDGE of the radius) stay within occlusion_ref.EXCLUDED_CAP, and sphere 1 blocks at least 1 % of sphere 0's facing
    rays, so the scene pins the reflection of one instance in another."""
    sc = SR.analytic_scene()
    cf = SR.analytic_closed_form(sc)
    pts = SL.analytic_points(sc, cf)
    on0 = pts["e"] == 0
    for s in SG.AN_SHININESS:
        a = SG.analytic_lobe(sc, pts, SG.AN_S, s, SL.SEED)
        facing = a["facing"][:, on0]
        by1 = a["blocked_by"][1][:, on0] & facing
        band = a["in_band"][a["facing"]]
        share = a["free"][:, on0].mean(0)
        alone = (a["facing"] & ~a["blocked_by"][0])[:, on0].mean(0)
        print(f"analytic rehearsal: lobe s={s:g} S={SG.AN_S}: facing rays {int(a['facing'].sum())} of {a['facing'].size}, in the band "
              f"{int(band.sum())} ({band.mean():.5f}); sphere 0: facing {int(facing.sum())}, blocked by sphere 1 {int(by1.sum())} "
              f"({by1.sum() / facing.sum():.4f}), pixels lowered {int((share < alone).sum())}, rays with |n . d| < {SG.NDD_EDGE} "
              f"{int((np.abs(a['ndd']) < SG.NDD_EDGE).sum())}")
        assert band.mean() <= R.EXCLUDED_CAP
        assert by1.sum() / facing.sum() >= SG.BLOCKED_FLOOR
        assert not (a["blocked_by"][0][:, on0] & facing).any()               # a convex sphere never blocks its own biased points
        assert (share < alone).any()
