"""CPU checks of the sampled secondary rays between the instances of a scene (include/oi_scene_light.h; oi_amd.scene; DESIGN
section 4.21): header <=> library <=> binding, the C ABI's refusals (checked on the host before any launch), the Python
refusals, the self-consistency of the restatement the GPU tests compare against (tests/helpers/scene_light_ref.py: against
per-ray loops, chunked == unchunked), and the CONDITIONS the GPU test's analytic two-sphere scene must satisfy on float64
alone: the exclusion caps of its ambient, transfer and soft-shadow rays, and that the other sphere blocks enough of them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import cabi
from helpers import env_ref as EV
from helpers import occlusion_ref as R
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T
from test_scene_cpu import fake_gen

ENTRIES = ["oi_scene_occlusion_begin", "oi_scene_occlusion_resolve", "oi_scene_point_pixels", "oi_scene_shade_ao",
           "oi_scene_transfer_normal", "oi_scene_transfer_resolve", "oi_trace_batch_step_anyhit"]

_lib = cabi.built_lib


def test_header_library_and_binding_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_scene_light.h", lib)
    # the header's two parameter structs, in its order: check_header held each mirror against it field by field
    assert sorted(names) == ENTRIES == lib.symbols("oi_scene_light.h") and mirrors == ["SceneOcclusionParams", "SceneShadeAoParams"]
    _, structs = cabi.parse(cabi.read("oi_scene_light.h"))
    assert sorted(structs) == ["oi_scene_occlusion_params", "oi_scene_shade_ao_params"]
    assert lib.SceneShadeAoParams._fields_[0][1] is lib.SceneShadeParams
    assert ctypes.sizeof(lib.SceneShadeAoParams) == ctypes.sizeof(lib.SceneShadeParams) + ctypes.sizeof(ctypes.c_void_p)
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"scene_light.hip"' in src and "include/oi_scene_light.h" in src
    # nothing was added to the headers whose entry lists other tests pin
    for header, n in (("oi_scene.h", 7), ("oi_occlusion.h", 5), ("oi_envlight.h", 5), ("oi_trace_batch.h", 5)):
        assert len(lib.symbols(header)) == n, header
    text = cabi.read("oi_scene_light.h")
    assert not re.search(r"#\s*define\s+OI_", re.sub(r"#define OI_SCENE_LIGHT_H_", "", text))      # it borrows every limit


def invalid_argument_cases(lib, L, f, arrays=None):
    """(call, entry, text of the message) of the refusals; f: a non-null pointer for every array (never dereferenced: each
    call returns before any launch), arrays: {field: pointer} to use instead for the state."""
    arrays = arrays or {}
    keep = []

    def batch(E=3, N=48, live=f, **kw):
        b = lib.TraceBatch()
        b.s.N, b.E, b.live = N, E, live
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(b.s, n, kw.get(n, arrays.get(n, f)))
        keep.append(b)
        return ctypes.byref(b)

    def begin(b=None, **kw):
        """Defaults: E = 3 occluders, L = 2 lights, S = 4 strata, the chunk [1, 4), n_vis = 8: N = 2 * 3 * 8 = 48."""
        P = lib.SceneOcclusionParams()
        P.L, P.S, P.j0, P.Sc, P.ambient = kw.get("L", 2), kw.get("S", 4), kw.get("j0", 1), kw.get("Sc", 3), kw.get("ambient", 0)
        P.seed, P.bias, P.distance = 7, kw.get("bias", 1e-2), kw.get("distance", 0.5)
        P.n_pad, P.n_vis = kw.get("n_pad", 5), kw.get("n_vis", 8)
        for n, _ in lib.SceneOcclusionParams._fields_[10:]:
            setattr(P, n, kw.get(n, f))
        keep.append(P)
        return L.oi_scene_occlusion_begin(batch() if b is None else b, ctypes.byref(P), None)

    def shade(ao=f, **kw):
        A = lib.SceneShadeAoParams()
        P = A.s
        P.E, P.W, P.S, P.L, P.n_pad = kw.get("E", 3), kw.get("W", 4), kw.get("S", 8), kw.get("L", 1), kw.get("n_pad", 5)
        for n, _ in lib.SceneShadeParams._fields_[5:]:
            setattr(P, n, kw.get(n, f))
        A.ambient_occlusion = ao
        keep.append(A)
        return L.oi_scene_shade_ao(ctypes.byref(A), None)

    pixels = lambda b=None, W=4, S=8, n_vis=9, out=f: L.oi_scene_point_pixels(batch(N=16) if b is None else b, f, f, W, S, f, n_vis, out,
                                                                             None)
    step = lambda b=None, sdf=f, bound=5, k=0, tol=1e-5, omega=1.0: L.oi_trace_batch_step_anyhit(batch() if b is None else b, sdf, bound,
                                                                                                  k, tol, omega, None)
    occ = lambda st=f, E=3, N=16, Lt=2, S=4, j0=1, Sc=3, n_vis=8, sS=8, last=1, count=f, out=f: L.oi_scene_occlusion_resolve(
        st, f, f, f, f, E, N, Lt, S, j0, Sc, n_vis, sS, last, count, out, None)
    tra = lambda st=f, E=3, N=16, S=4, j0=1, Sc=3, n_vis=8, sS=8, last=1, out=f, d=f: L.oi_scene_transfer_resolve(
        st, d, f, f, f, f, f, E, N, S, j0, Sc, n_vis, sS, last, out, None)
    nrm = lambda grad=f, n_pad=5, E=3, N=16, sS=8, out=f: L.oi_scene_transfer_normal(grad, n_pad, f, f, f, f, E, N, sS, out, None)
    inf, nan = float("inf"), float("nan")
    return [(lambda: pixels(batch(E=0, N=16)), "oi_scene_point_pixels", "E=0"),
            (lambda: pixels(W=5), "oi_scene_point_pixels", "W=5"),
            (lambda: pixels(S=0), "oi_scene_point_pixels", "S=0"),
            (lambda: pixels(n_vis=0), "oi_scene_point_pixels", "n_vis=0"),
            (lambda: pixels(n_vis=49), "oi_scene_point_pixels", "n_vis=49"),
            (lambda: pixels(out=None), "oi_scene_point_pixels", "null pointer"),
            (lambda: L.oi_scene_occlusion_begin(None, None, None), "oi_scene_occlusion_begin", "null batch"),
            (lambda: L.oi_scene_occlusion_begin(batch(), None, None), "oi_scene_occlusion_begin", "null params"),
            (lambda: begin(batch(E=0)), "oi_scene_occlusion_begin", "E=0"),
            (lambda: begin(batch(live=None)), "oi_scene_occlusion_begin", "null live"),
            (lambda: begin(L=0), "oi_scene_occlusion_begin", "L=0"),
            (lambda: begin(L=257), "oi_scene_occlusion_begin", "L=257"),
            (lambda: begin(S=0), "oi_scene_occlusion_begin", "S=0"),
            (lambda: begin(S=257), "oi_scene_occlusion_begin", "S=257"),
            (lambda: begin(j0=-1), "oi_scene_occlusion_begin", "j0=-1"),
            (lambda: begin(Sc=0), "oi_scene_occlusion_begin", "Sc=0"),
            (lambda: begin(j0=2), "oi_scene_occlusion_begin", "j0=2, Sc=3, S=4"),
            (lambda: begin(L=2, ambient=1), "oi_scene_occlusion_begin", "L=2 with ambient"),
            (lambda: begin(Sc=2), "oi_scene_occlusion_begin", "N must be L * Sc * n_vis"),
            (lambda: begin(n_vis=0), "oi_scene_occlusion_begin", "n_vis=0"),
            (lambda: begin(batch(N=96), n_vis=16), "oi_scene_occlusion_begin", "n_vis=16"),
            (lambda: begin(n_pad=0), "oi_scene_occlusion_begin", "n_pad=0"),
            (lambda: begin(bias=-1.0), "oi_scene_occlusion_begin", "bias"),
            (lambda: begin(bias=inf), "oi_scene_occlusion_begin", "bias"),
            (lambda: begin(bias=nan), "oi_scene_occlusion_begin", "bias"),
            (lambda: begin(batch(N=24), L=1, ambient=1, distance=0.0), "oi_scene_occlusion_begin", "distance"),
            (lambda: begin(batch(N=24), L=1, ambient=1, distance=-1.0), "oi_scene_occlusion_begin", "distance"),
            (lambda: begin(batch(N=24), L=1, ambient=1, distance=nan), "oi_scene_occlusion_begin", "distance"),
            (lambda: begin(elem=None), "oi_scene_occlusion_begin", "null input"),
            (lambda: begin(pixel=None), "oi_scene_occlusion_begin", "null input"),
            (lambda: begin(radius=None), "oi_scene_occlusion_begin", "null input"),
            (lambda: begin(lights=None), "oi_scene_occlusion_begin", "null input"),
            (lambda: step(batch(E=1025)), "oi_trace_batch_step_anyhit", "E=1025"),
            (lambda: step(k=-1), "oi_trace_batch_step_anyhit", "k=-1"),
            (lambda: step(k=1024), "oi_trace_batch_step_anyhit", "k=1024"),
            (lambda: step(bound=49), "oi_trace_batch_step_anyhit", "bound=49"),
            (lambda: step(bound=-1), "oi_trace_batch_step_anyhit", "bound=-1"),
            (lambda: step(tol=0.0), "oi_trace_batch_step_anyhit", "tol"),
            (lambda: step(omega=inf), "oi_trace_batch_step_anyhit", "omega"),
            (lambda: step(sdf=None), "oi_trace_batch_step_anyhit", "null sdf"),
            (lambda: step(batch(counts=None)), "oi_trace_batch_step_anyhit", "null pointer"),
            (lambda: occ(E=0), "oi_scene_occlusion_resolve", "E=0"),
            (lambda: occ(N=0), "oi_scene_occlusion_resolve", "N=0"),
            (lambda: occ(Lt=257), "oi_scene_occlusion_resolve", "L=257"),
            (lambda: occ(S=257), "oi_scene_occlusion_resolve", "S=257"),
            (lambda: occ(j0=2), "oi_scene_occlusion_resolve", "j0=2"),
            (lambda: occ(Sc=0), "oi_scene_occlusion_resolve", "Sc=0"),
            (lambda: occ(sS=0), "oi_scene_occlusion_resolve", "S=0"),
            (lambda: occ(n_vis=0), "oi_scene_occlusion_resolve", "n_vis=0"),
            (lambda: occ(n_vis=49), "oi_scene_occlusion_resolve", "n_vis=49"),
            (lambda: occ(E=1024, N=1 << 20, Lt=256, S=256, j0=0, Sc=256, n_vis=1 << 10), "oi_scene_occlusion_resolve", "2^31"),
            (lambda: occ(st=None), "oi_scene_occlusion_resolve", "null pointer"),
            (lambda: occ(count=None), "oi_scene_occlusion_resolve", "null pointer"),
            (lambda: occ(out=None), "oi_scene_occlusion_resolve", "null pointer"),
            (lambda: tra(E=1025), "oi_scene_transfer_resolve", "E=1025"),
            (lambda: tra(S=0), "oi_scene_transfer_resolve", "S=0"),
            (lambda: tra(j0=-1), "oi_scene_transfer_resolve", "j0=-1"),
            (lambda: tra(j0=2), "oi_scene_transfer_resolve", "j0=2"),
            (lambda: tra(n_vis=49), "oi_scene_transfer_resolve", "n_vis=49"),
            (lambda: tra(sS=32769), "oi_scene_transfer_resolve", "S=32769"),
            (lambda: tra(d=None), "oi_scene_transfer_resolve", "null pointer"),
            (lambda: tra(out=None), "oi_scene_transfer_resolve", "null pointer"),
            (lambda: nrm(E=0), "oi_scene_transfer_normal", "E=0"),
            (lambda: nrm(n_pad=0), "oi_scene_transfer_normal", "n_pad=0"),
            (lambda: nrm(n_pad=17), "oi_scene_transfer_normal", "n_pad=17"),
            (lambda: nrm(sS=0), "oi_scene_transfer_normal", "S=0"),
            (lambda: nrm(grad=None), "oi_scene_transfer_normal", "null pointer"),
            (lambda: nrm(out=None), "oi_scene_transfer_normal", "null pointer"),
            (lambda: L.oi_scene_shade_ao(None, None), "oi_scene_shade_ao", "null params"),
            (lambda: shade(E=0), "oi_scene_shade_ao", "E=0"),
            (lambda: shade(W=0), "oi_scene_shade_ao", "W=0"),
            (lambda: shade(S=0), "oi_scene_shade_ao", "S=0"),
            (lambda: shade(n_pad=17), "oi_scene_shade_ao", "n_pad=17"),
            (lambda: shade(L=257), "oi_scene_shade_ao", "L=257"),
            (lambda: shade(owner=None), "oi_scene_shade_ao", "null owner"),
            (lambda: shade(grad=None), "oi_scene_shade_ao", "null input")]


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


def _stub_scene(E=2, n_vis=(100, 50), S=9):
    """A SceneSurface that holds only what the refusals read: nothing was traced."""
    from oi_amd import scene
    s = scene.SceneSurface.__new__(scene.SceneSurface)
    s.E, s.S, s.N, s.W, s.n_vis, s.n_pad = E, S, 16, 4, list(n_vis), max(n_vis)
    return s


def test_python_refusals():
    from oi_amd import inference, scene
    gen = fake_gen()
    z, centre = torch.zeros(64), T.pose("centre")
    one = lambda **kw: scene.render_scene(gen, [z], [centre], **kw)
    for bad in (0, 257, 2.0, True):
        with pytest.raises(ValueError, match="shadow_samples"):
            one(shadows=True, shadow_samples=bad)
    for bad in (-1, 257, 1.5):
        with pytest.raises(ValueError, match="ao_samples"):
            one(ao_samples=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ao_distance"):
            one(ao_samples=4, ao_distance=bad)
    for bad in (-0.1, 1.6, float("nan"), [[0.1]]):
        with pytest.raises(ValueError, match="light_radius"):
            one(shadows=True, light_radius=bad)
    with pytest.raises(ValueError, match="need shadows=True"):
        one(shadow_samples=4)
    with pytest.raises(ValueError, match="need shadows=True"):
        one(light_radius=0.1)
    with pytest.raises(ValueError, match="seed"):
        one(ao_samples=4, seed=-1)
    for bad in (-1, 257, 1.5, True):
        with pytest.raises(ValueError, match="transfer_samples"):
            scene.render_scene_env(gen, [z], [centre], [], transfer_samples=bad)
    with pytest.raises(ValueError, match="seed"):
        scene.render_scene_env(gen, [z], [centre], [], seed=1 << 32)
    with pytest.raises(TypeError, match="EnvLight"):
        inference.scene_env_walk(gen, [z], [centre], env="sky")
    with pytest.raises(ValueError, match="n_frames"):
        from oi_amd.envlight import EnvLight
        inference.scene_env_walk(gen, [z], [centre], EnvLight.constant(1.0), n_frames=0)
    # a chunk of one sample that does not fit: refused naming the counts, before anything is launched
    s = _stub_scene()
    lights = torch.zeros(2, 16)
    with pytest.raises(ValueError, match=r"2 instances x 2 lights x 150 visible points = 600 rays per sample"):
        s.visibility(lights, [0.1, 0.0], samples=4, max_shadow_rays=599)
    with pytest.raises(ValueError, match=r"2 instances x 1 lights x 150 visible points = 300 rays per sample"):
        s._sampled("SceneSurface.ambient", 16, 0, 299, None, distance=0.5)
    with pytest.raises(ValueError, match="300 rays per sample"):
        s._sampled("SceneSurface.capture_transfer", 64, 0, 299, None, distance=float("inf"))
    with pytest.raises(ValueError, match="transfer_samples"):
        s.capture_transfer(transfer_samples=300)
    # one hard ray per light keeps the parent's refusal and its text
    with pytest.raises(ValueError, match="600 shadow rays"):
        s.visibility(lights, max_shadow_rays=599)
    with pytest.raises(ValueError, match="600 shadow rays"):
        s.visibility(lights, [0.0, 0.0], samples=1, max_shadow_rays=599)


def _random_scene(rs, E=3, n_pad=7, W=5, S=9):
    """Random inputs of the ray construction: rigid poses, visible lists, points inside the unit spheres."""
    w2b = []
    for e in range(E):
        m = np.eye(4)
        m[:3, :3] = EV.random_rotation(rs)
        m[:3, 3] = rs.randn(3) * 0.8
        w2b.append(m)
    w2b = np.stack(w2b)
    b2w = np.stack([SR.rigid_inverse(m) for m in w2b])
    n_vis = [n_pad, 3, n_pad - 2][:E]
    offset = SR.offsets(n_vis)
    points = rs.randn(E, n_pad, 3) * 0.3
    grad = rs.randn(E, n_pad, 3)
    elem = np.concatenate([[e] * n for e, n in enumerate(n_vis)])
    slot = np.arange(len(elem)) - offset[elem]
    position = np.stack([SR.transform(b2w[e], points[e, k]) for e, k in zip(elem, slot)])
    normal_world = np.stack([b2w[e][:3, :3] @ SL.unit(grad[e, k]) for e, k in zip(elem, slot)])
    pixel = rs.permutation(S * S)[:len(elem)]
    return dict(w2b=w2b, b2w=b2w, n_vis=n_vis, offset=offset, points=points, grad=grad, elem=elem, slot=slot, position=position,
                normal_world=normal_world, pixel=pixel, E=E, n_pad=n_pad, W=W, S=S)


@pytest.mark.parametrize("ambient", [False, True])
def test_restated_rays_against_a_per_ray_loop(ambient):
    rs = np.random.RandomState(3 + ambient)
    sc = _random_scene(rs)
    S, j0, Sc, seed, bias = 5, 1, 3, 11, 1e-2
    dirs, radius, distance = [(0.3, -0.8, -0.5), (-0.7, -0.3, 0.6)], [0.2, 0.0], 1.3
    kw = dict(distance=distance) if ambient else dict(light_dirs=dirs, radius=radius)
    r = SL.rays(sc["points"], sc["grad"], sc["offset"], sc["elem"], sc["pixel"], sc["position"], sc["normal_world"], sc["w2b"], bias,
                S, j0, Sc, seed, **kw)
    L = 1 if ambient else 2
    n = len(sc["elem"])
    assert r["status"].shape == (sc["E"], L, Sc, n)
    seen = set()
    for g in range(n):
        e, k = sc["elem"][g], sc["slot"][g]
        nrm = SL.unit(sc["grad"][e, k])
        u1, u2 = R.sample_numbers(np.array([sc["pixel"][g]]), seed, S)
        for l in range(L):
            for jj in range(Sc):
                j = j0 + jj
                if ambient:
                    d = R.hemisphere_directions(nrm[None], u1[j:j + 1], u2[j:j + 1])[0, 0]
                else:
                    d = R.cap_directions(T.light_object_dir(dirs[l], sc["w2b"][e]), radius[l], u1[j:j + 1], u2[j:j + 1])[0, 0]
                assert np.abs(d - r["d_owner"][l, jj, g]).max() < 1e-15 and abs(np.linalg.norm(d) - 1) < 1e-12
                traced = nrm @ d > 0
                dw = sc["w2b"][e][:3, :3].T @ d
                for eo in range(sc["E"]):
                    st = r["status"][eo, l, jj, g]
                    if not traced:
                        assert st == SL.BACKFACING and r["near"][eo, l, jj, g] == r["far"][eo, l, jj, g] == 0
                        seen.add("back")
                        continue
                    if eo == e:
                        o = sc["points"][e, k] + bias * nrm
                        far = float(R.unit_sphere_exit(o, d))
                        far = min(far, distance) if ambient else far
                        assert st == SL.MARCH and r["near"][eo, l, jj, g] == 0 and abs(r["far"][eo, l, jj, g] - far) < 1e-14
                        assert np.abs(r["o"][eo, l, jj, g] - o).max() < 1e-15 and np.abs(r["d"][eo, l, jj, g] - d).max() < 1e-15
                        seen.add("own")
                        continue
                    o = SR.transform(sc["w2b"][eo], (sc["position"][g] + bias * sc["normal_world"][g])[None])[0]
                    de = sc["w2b"][eo][:3, :3] @ dw
                    ent, near, far, _ = SR.cull(o, de)
                    if ambient:
                        ent, far = ent and near < distance, min(float(far), distance)
                    assert st == (SL.MARCH if ent else SL.MISS)
                    if ent:
                        assert abs(r["near"][eo, l, jj, g] - near) < 1e-14 and abs(r["far"][eo, l, jj, g] - far) < 1e-14
                        assert np.abs(r["o"][eo, l, jj, g] - o).max() < 1e-14 and np.abs(r["d"][eo, l, jj, g] - de).max() < 1e-14
                        # the same ray in the world: the point and direction of the owner's own ray, moved rigidly
                        back = SR.transform(sc["b2w"][eo], o[None])[0]
                        own = SR.transform(sc["b2w"][e], (sc["points"][e, k] + bias * nrm)[None])[0]
                        assert np.abs(back - own).max() < 1e-12
                    seen.add("entered" if ent else "culled")
    assert seen >= {"own", "entered", "culled"} and (ambient or "back" in seen)
    # the radius-0 light: every sample is the light's own direction
    if not ambient:
        assert np.abs(r["d_owner"][1] - r["d_owner"][1][:1]).max() < 1e-15


def test_restated_resolves_against_per_pixel_loops_and_chunked_equals_unchunked():
    rs = np.random.RandomState(5)
    E, W, M, L, S = 3, 4, 30, 2, 7
    n_vis = [6, 0, 5]
    offset = SR.offsets(n_vis)
    owner, owner_ray = np.full(M, -1), np.full(M, -1)
    vis_slot = np.full((E, W * W), -1)
    for e, n in enumerate(n_vis):
        q = rs.permutation(np.nonzero(owner < 0)[0])[:n]
        r = rs.permutation(W * W)[:n]
        owner[q], owner_ray[q] = e, r
        vis_slot[e, r] = rs.permutation(n)
    nv = sum(n_vis)
    status = rs.choice([SL.MISS, SL.HIT, SL.BACKFACING, T.LIMIT], size=(E, L, S, nv), p=[0.85, 0.07, 0.04, 0.04]).astype(np.uint8)
    d = SL.unit(rs.randn(1, S, nv, 3))
    w2b = np.stack([np.eye(4)] * E)
    for e in range(E):
        w2b[e, :3, :3] = EV.random_rotation(rs)
    count, out = SL.counts([status], owner, owner_ray, vis_slot, offset, S)
    tr, mag = SL.transfer([(status[:, :1], d)], owner, owner_ray, vis_slot, offset, w2b, S)
    for q in range(M):
        if owner[q] < 0:
            assert (out[:, q] == 1).all() and not count[:, q].any() and not tr[:, q].any()
            continue
        e = owner[q]
        g = offset[e] + vis_slot[e, owner_ray[q]]
        for l in range(L):
            c = sum(all(status[eo, l, j, g] == SL.MISS for eo in range(E)) for j in range(S))
            assert count[l, q] == c and out[l, q] == float(np.float32(c) / np.float32(S))
        acc = np.zeros(9)
        for j in range(S):
            if all(status[eo, 0, j, g] == SL.MISS for eo in range(E)):
                v = w2b[e][:3, :3].T @ d[0, j, g]
                acc += EV.basis(v / np.linalg.norm(v))
        assert np.abs(acc / S - tr[:, q]).max() < 1e-14
    assert 0 < out[:, owner >= 0].mean() < 1
    for cuts in ([1] * S, [3, 4], [5, 1, 1]):
        edges = np.concatenate([[0], np.cumsum(cuts)])
        c2, o2 = SL.counts([status[:, :, a:b] for a, b in zip(edges[:-1], edges[1:])], owner, owner_ray, vis_slot, offset, S)
        t2, _ = SL.transfer([(status[:, :1, a:b], d[:, a:b]) for a, b in zip(edges[:-1], edges[1:])], owner, owner_ray, vis_slot, offset,
                            w2b, S)
        assert np.array_equal(c2, count) and np.array_equal(o2, out) and np.abs(t2 - tr).max() < 1e-15
    # the pixels of the visible points
    vis_index = np.full((E, W * W), -7)
    for e in range(E):
        r = np.nonzero(vis_slot[e] >= 0)[0]
        vis_index[e, vis_slot[e, r]] = r
    window = np.array([[1, 2], [0, 0], [-1, 3]])
    pix = SL.point_pixels(vis_index, window, W, 9, offset, n_vis)
    for e in range(E):
        for k in range(n_vis[e]):
            j, i = divmod(vis_index[e, k], W)
            assert pix[offset[e] + k] == (window[e, 1] + j) * 9 + window[e, 0] + i


def test_analytic_scene_rehearsal():
    """The GPU test's analytic two-sphere scene on float64 ALONE, seed 7: the rays excluded because float32 may decide them
    either way (closest approach within AN_SHADOW_EDGE of the radius) stay within occlusion_ref.EXCLUDED_CAP for the ambient
    / transfer rays at 16 and 64 samples and for the soft shadow of radius 0.1 at 4 samples; no soft-shadow ray is within
    1e-3 of n . d = 0; and the other sphere blocks more than 5 % of sphere 0's ambient rays, so the scene pins occlusion
    between instances."""
    sc = SR.analytic_scene()
    cf = SR.analytic_closed_form(sc)
    pts = SL.analytic_points(sc, cf)
    on = [pts["e"] == e for e in (0, 1)]
    assert [int(m.sum()) for m in on] == [77, 172]
    for S in (SL.AN_AO_S, SL.AN_TRANSFER_S):
        a = SL.analytic_secondary(sc, pts, S, SL.SEED)
        assert a["facing"].all()
        for e in (0, 1):
            other = a["blocked_by"][1 - e][:, on[e]]
            band = a["in_band"][:, on[e]]
            print(f"analytic rehearsal: ambient S={S} sphere {e}: pixels {int(on[e].sum())} rays {other.size} blocked by the other sphere "
                  f"{int(other.sum())} ({other.mean():.4f}) in the band {int(band.sum())} ({band.mean():.5f}) pixels with a blocked "
                  f"sample {int(other.any(0).sum())} lowest escaped share {a['free'][:, on[e]].mean(0).min():.4f}")
            assert band.mean() <= R.EXCLUDED_CAP
            assert not a["blocked_by"][e][:, on[e]].any()               # a convex sphere never blocks its own biased points
        assert a["blocked_by"][1][:, on[0]].mean() > SL.BLOCKED_FLOOR
        assert not a["blocked_by"][0][:, on[1]].any()                   # sphere 1 stands between sphere 0 and the camera's side
    a = SL.analytic_secondary(sc, pts, SL.AN_SOFT_S, SL.SEED, light=SR.AN_LIGHT, radius=SL.AN_SOFT_RADIUS)
    band, ndd = a["in_band"][:, on[0]], a["ndd"][:, on[0]]
    share = a["free"][:, on[0]].mean(0)
    print(f"analytic rehearsal: soft shadow S={SL.AN_SOFT_S} radius {SL.AN_SOFT_RADIUS}: rays {band.size} in the band {int(band.sum())} "
          f"smallest |n . d| {np.abs(ndd).min():.5f} pixels in penumbra {int(((share > 0) & (share < 1)).sum())} lit {int((share == 1).sum())}")
    assert band.size == 308 and band.mean() <= R.EXCLUDED_CAP and np.abs(ndd).min() > 1e-3
    assert (share == 0).any() and ((share > 0) & (share < 1)).any()       # an umbra and a penumbra
