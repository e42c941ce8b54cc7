"""CPU checks of soft shadows and ambient occlusion (include/oi_occlusion.h): header <=> library <=>
binding <=> helper, the argument refusals that need no GPU, the properties of the fp64 restatement
(tests/helpers/occlusion_ref.py) that hold exactly or by derivation, the any-hit machine against the full one on the oracle,
and the REHEARSAL on the oracle alone of exactly the configurations tests/test_gpu_occlusion.py runs.

Rehearsal results (oracle alone, float64, golden weights, 24 x 24 rays, two lights of radius 0.1 rad x 4 samples, 4 ambient
samples to distance 0.5, seed 7, defaults tol 1e-5, omega 1, 64 steps, bias 1e-2):

    seed 0 / centre: 113 hits; 702 of 904 light rays traced, 3 LIMIT (0.43 %), 1 occluded; 452 ambient rays, none LIMIT
    seed 1 / off:    127 hits; 728 of 1016 light rays traced, 1 LIMIT (0.14 %), 0 occluded; 508 ambient rays, none LIMIT
    no START_INSIDE anywhere; 8.1 .. 9.6 evaluations per traced light ray, 6.7 .. 7.0 per ambient ray
    analytic two-sphere scene (16 x 16 points x 64 samples, radius 0.15, 256 steps): 21 of 16384 rays (0.13 %) within 1e-4
    of tangency; outside that band every ray's state is the geometric one; 6 % of the patch in the umbra, 28 % in the penumbra"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from helpers import cabi
from helpers import occlusion_ref as R
from helpers import trace_ref as T


_lib = cabi.built_lib


def test_header_library_binding_and_helper_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_occlusion.h", lib)
    assert sorted(names) == ["oi_occlusion_ambient_begin", "oi_occlusion_light_begin", "oi_occlusion_resolve", "oi_occlusion_step",
                             "oi_surface_shade_ao"]
    assert mirrors == ["SurfaceAoParams"]
    text = cabi.read("oi_occlusion.h")
    assert int(re.search(r"#define OI_OCCLUSION_MAX_SAMPLES (\d+)", text).group(1)) == lib.OCCLUSION_MAX_SAMPLES == R.MAX_SAMPLES == 256
    fields = cabi.parse(text)[1]["oi_surface_ao_params"]
    assert [f for f, _ in fields] == [f[0] for f in lib.SurfaceAoParams._fields_]
    assert fields[:-1] == cabi.parse(cabi.read("oi_trace.h"))[1]["oi_surface_params"] and fields[-1][0] == "ambient_occlusion"
    assert lib.SurfaceAoParams._fields_[:-1] == lib.SurfaceParams._fields_
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"occlusion.hip"' in src
    from oi_amd import inference
    assert inference.TRACE_BYTES_PER_RAY == 100 and 1 <= inference.OCCLUSION_MAX_RAYS < 1 << 31


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)
    nan, inf = float("nan"), float("inf")

    def state(N=24, **kw):
        S = lib.TraceState()
        S.N = N
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(S, n, kw.get(n, f))
        return ctypes.byref(S)

    def surf(**kw):
        P = lib.SurfaceAoParams()
        P.N, P.n_hit, P.L = kw.pop("N", 5), kw.pop("n_hit", 2), kw.pop("L", 1)
        for n, _ in lib.SurfaceAoParams._fields_[3:]:
            setattr(P, n, kw.get(n, f))
        return ctypes.byref(P)

    def light(s=None, hp=f, g=f, hi=f, n_hit=2, lt=f, rad=f, L_=3, S=4, w2b=f, bias=0.01):   # 3 lights x 4 samples x 2 hits = 24
        return L.oi_occlusion_light_begin(state() if s is None else s, hp, g, hi, n_hit, lt, rad, L_, S, w2b, bias, 0, None)

    def amb(s=None, hp=f, g=f, hi=f, n_hit=6, S=4, bias=0.01, dist=0.5):
        return L.oi_occlusion_ambient_begin(state() if s is None else s, hp, g, hi, n_hit, S, bias, dist, 0, None)

    lb, ab, stp, rs, sh = ("oi_occlusion_light_begin", "oi_occlusion_ambient_begin", "oi_occlusion_step", "oi_occlusion_resolve",
                           "oi_surface_shade_ao")
    cases = [(lambda: L.oi_occlusion_light_begin(None, f, f, f, 2, f, f, 3, 4, f, 0.01, 0, None), lb, "null state"),
             (lambda: light(state(N=0)), lb, "N=0"),
             (lambda: light(state(N=1 << 31)), lb, "N=2147483648"),
             (lambda: light(state(points=None)), lb, "null pointer"),
             (lambda: light(L_=0), lb, "L=0"),
             (lambda: light(L_=257), lb, "L=257"),
             (lambda: light(S=0), lb, "S=0"),
             (lambda: light(S=257), lb, "S=257"),
             (lambda: light(n_hit=0), lb, "n_hit=0"),
             (lambda: light(state(N=25)), lb, "L * S * n_hit"),
             (lambda: light(n_hit=1 << 31), lb, "below 2^31"),
             (lambda: light(bias=-1.0), lb, "bias"),
             (lambda: light(bias=nan), lb, "bias"),
             (lambda: light(bias=inf), lb, "bias"),
             (lambda: light(rad=None), lb, "null radius"),
             (lambda: light(hp=None), lb, "null input"),
             (lambda: light(g=None), lb, "null input"),
             (lambda: light(hi=None), lb, "null input"),
             (lambda: light(lt=None), lb, "null input"),
             (lambda: light(w2b=None), lb, "null input"),
             (lambda: L.oi_occlusion_ambient_begin(None, f, f, f, 6, 4, 0.01, 0.5, 0, None), ab, "null state"),
             (lambda: amb(state(side=None)), ab, "null pointer"),
             (lambda: amb(S=0), ab, "S=0"),
             (lambda: amb(S=257), ab, "S=257"),
             (lambda: amb(n_hit=5), ab, "L * S * n_hit"),
             (lambda: amb(bias=-0.5), ab, "bias"),
             (lambda: amb(bias=nan), ab, "bias"),
             (lambda: amb(dist=0.0), ab, "distance"),
             (lambda: amb(dist=-1.0), ab, "distance"),
             (lambda: amb(dist=inf), ab, "distance"),
             (lambda: amb(dist=nan), ab, "distance"),
             (lambda: amb(hp=None), ab, "null input"),
             (lambda: amb(g=None), ab, "null input"),
             (lambda: amb(hi=None), ab, "null input"),
             (lambda: L.oi_occlusion_step(None, f, 5, 0, 1e-5, 1.0, None), stp, "null state"),
             (lambda: L.oi_occlusion_step(state(), f, 5, -1, 1e-5, 1.0, None), stp, "k=-1"),
             (lambda: L.oi_occlusion_step(state(), f, 5, 1024, 1e-5, 1.0, None), stp, "k=1024"),
             (lambda: L.oi_occlusion_step(state(), f, 25, 0, 1e-5, 1.0, None), stp, "bound=25"),
             (lambda: L.oi_occlusion_step(state(), f, 5, 0, 0.0, 1.0, None), stp, "tol"),
             (lambda: L.oi_occlusion_step(state(), f, 5, 0, 1e-5, nan, None), stp, "omega"),
             (lambda: L.oi_occlusion_step(state(), None, 5, 0, 1e-5, 1.0, None), stp, "null sdf"),
             (lambda: L.oi_occlusion_step(state(active=None), f, 5, 0, 1e-5, 1.0, None), stp, "null pointer"),
             (lambda: L.oi_occlusion_resolve(f, f, 0, 0, 1, 1, f, None), rs, "N=0"),
             (lambda: L.oi_occlusion_resolve(f, f, 5, 6, 1, 1, f, None), rs, "n_hit=6"),
             (lambda: L.oi_occlusion_resolve(f, f, 5, 2, 0, 1, f, None), rs, "L=0"),
             (lambda: L.oi_occlusion_resolve(f, f, 5, 2, 300, 1, f, None), rs, "L=300"),
             (lambda: L.oi_occlusion_resolve(f, f, 5, 2, 1, 0, f, None), rs, "S=0"),
             (lambda: L.oi_occlusion_resolve(f, f, 5, 2, 1, 257, f, None), rs, "S=257"),
             (lambda: L.oi_occlusion_resolve(f, f, 1 << 20, 1 << 20, 256, 8, f, None), rs, "below 2^31"),
             (lambda: L.oi_occlusion_resolve(None, f, 5, 2, 1, 4, f, None), rs, "null"),
             (lambda: L.oi_occlusion_resolve(f, None, 5, 2, 1, 4, f, None), rs, "null"),
             (lambda: L.oi_occlusion_resolve(f, f, 5, 2, 1, 4, None, None), rs, "null"),
             (lambda: L.oi_surface_shade_ao(None, None), sh, "null params"),
             (lambda: L.oi_surface_shade_ao(surf(N=0), None), sh, "N=0"),
             (lambda: L.oi_surface_shade_ao(surf(L=0), None), sh, "L=0"),
             (lambda: L.oi_surface_shade_ao(surf(L=257), None), sh, "L=257"),
             (lambda: L.oi_surface_shade_ao(surf(status=None), None), sh, "null input"),
             (lambda: L.oi_surface_shade_ao(surf(grad=None), None), sh, "null hit arrays")]
    for call, entry, text in cases:
        assert call() == -1, (entry, text)
        msg = L.oi_last_error().decode()
        assert msg.startswith(entry) and text in msg, (entry, text, msg)
    assert L.oi_occlusion_step(state(), None, 0, 3, 1e-5, 1.0, None) == 0      # bound = 0: success, nothing launched


def test_python_argument_checks():
    from oi_amd import inference, trace
    ok = dict(shadows=True, shadow_samples=4, light_radius=0.1, ao_samples=0, ao_distance=0.5, seed=0, n_lights=3, what="t")
    assert trace._check_occlusion(**ok) == pytest.approx([0.1] * 3)
    assert trace._check_occlusion(**{**ok, "light_radius": [0.0, 0.1, 0.2]}) == pytest.approx([0.0, 0.1, 0.2])
    assert trace._check_occlusion(**{**ok, "shadow_samples": 1, "light_radius": 0.0}) is None          # the hard path
    assert trace._check_occlusion(**{**ok, "shadows": False, "shadow_samples": 1, "light_radius": 0.0, "ao_samples": 8}) is None
    for bad, match in ((dict(shadow_samples=0), "shadow_samples"), (dict(shadow_samples=257), "shadow_samples"),
                       (dict(shadow_samples=2.0), "shadow_samples"), (dict(shadow_samples=True), "shadow_samples"),
                       (dict(ao_samples=-1), "ao_samples"), (dict(ao_samples=257), "ao_samples"), (dict(ao_samples=None), "ao_samples"),
                       (dict(ao_distance=0.0), "ao_distance"), (dict(ao_distance=float("inf")), "ao_distance"),
                       (dict(seed=-1), "seed"), (dict(seed=1 << 32), "seed"), (dict(seed=0.5), "seed"),
                       (dict(light_radius=-0.1), "light_radius"), (dict(light_radius=1.6), "light_radius"),
                       (dict(light_radius=float("nan")), "light_radius"), (dict(light_radius=[0.1, 0.2]), "light_radius"),
                       (dict(shadows=False), "shadows=True")):
        with pytest.raises(ValueError, match=match):
            trace._check_occlusion(**{**ok, **bad})
    with pytest.raises(ValueError, match="ambient_occlusion"):
        inference.surface_frames(None, [], [], keys=("ambient_occlusion",))
    import torch
    from oi_amd import ops
    for radius in (torch.zeros(2), torch.zeros(3, 1), torch.zeros(3, dtype=torch.float64), [0.0, 0.0, 0.0]):   # 3 lights
        with pytest.raises(ValueError, match="radius"):
            ops.occlusion_light_begin(None, None, None, None, 1, torch.zeros(3, 16), radius, 1, None, 0.01)
    assert "ambient_occlusion" in inference.SURFACE_KEYS


def test_sample_numbers_are_the_headers():
    # the mix in plain Python integers
    for pix, seed in ((0, 0), (1, 0), (12345, 7), (2 ** 31 - 1, 2 ** 32 - 1)):
        x = (pix * 0x9E3779B9 + seed) % 2 ** 32
        x ^= x >> 16
        x = x * 0x7FEB352D % 2 ** 32
        x ^= x >> 15
        x = x * 0x846CA68B % 2 ** 32
        x ^= x >> 16
        assert int(R.mix(np.array([pix]), seed)[0]) == x
        u1, u2 = R.sample_numbers(np.array([pix]), seed, 5)
        assert [float(v) for v in u2[:, 0]] == [(((j * 2654435769 + x) % 2 ** 32) >> 8) / 2 ** 24 for j in range(5)]
    for S in (1, 3, 4, 16, 64, 255, 256):
        u1, u2 = R.sample_numbers(np.arange(50), 3, S)
        # exactly one sample in each of the S strata [j / S, (j + 1) / S)
        assert np.array_equal(np.floor(u1 * S).astype(int), np.arange(S))
        assert u1.astype(np.float32).astype(np.float64).tolist() == u1.tolist()           # float32 numbers
        assert (u2 >= 0).all() and (u2 < 1).all() and np.array_equal(u2 * 2 ** 24, np.floor(u2 * 2 ** 24))
    a, b = R.sample_numbers(np.arange(50), 3, 8)[1], R.sample_numbers(np.arange(50), 4, 8)[1]
    assert (a != b).mean() > 0.9                                                            # the seed matters


def test_directions_of_the_restatement():
    """Unit length, inside the cap / the hemisphere, radius 0 is the axis; and the hemisphere's mean cosine.

    Mean of cos(alpha) over the S hemisphere samples: cos(alpha_j) = f(u_j) with f(u) = sqrt(1 - u) and u_j = (j + 1/2) / S, the
    midpoint rule for the integral of f over [0, 1], which is 2/3.  f is concave and decreasing, so on each stratum the tangent
    at the midpoint lies above f (midpoint value >= stratum mean) and the chord below it (stratum mean >= the mean of the end
    values): 0 <= f(u_j) - S * int_stratum f <= f(u_j) - (f(j/S) + f((j+1)/S)) / 2 <= (f(j/S) - f((j+1)/S)) / 2, the last step
    because f(u_j) <= f(j/S).  Averaged over the strata the right side telescopes to (f(0) - f(1)) / (2 S) = 1 / (2 S).  So
    0 <= mean - 2/3 <= 1 / (2 S)."""
    rs = np.random.RandomState(0)
    axes = rs.randn(40, 3)
    axes = np.concatenate([axes / np.linalg.norm(axes, axis=-1, keepdims=True), np.eye(3), -np.eye(3),
                           [[0.0, 1e-9, -1.0]], [[6e-4, 0.0, -1.0]]])
    axes /= np.linalg.norm(axes, axis=-1, keepdims=True)
    t1, t2 = R.frame(axes)
    for m in ((t1 * t1).sum(-1) - 1, (t2 * t2).sum(-1) - 1, (t1 * t2).sum(-1), (t1 * axes).sum(-1), (t2 * axes).sum(-1)):
        assert np.abs(m).max() < 1e-12
    assert np.abs(np.cross(t1, t2) - axes).max() < 1e-12                                   # right-handed: t1 x t2 = a
    pix = np.arange(len(axes)) * 7 + 1
    for S in (1, 3, 16, 256):
        u1, u2 = R.sample_numbers(pix, 5, S)
        hemi = R.hemisphere_directions(axes, u1, u2)
        assert np.abs(np.linalg.norm(hemi, axis=-1) - 1).max() < 1e-12
        cos_n = (hemi * axes[None]).sum(-1)
        assert (cos_n > 0).all()
        mean = cos_n.mean(0)
        assert (mean - 2 / 3 > -1e-12).all() and (mean - 2 / 3 <= 1 / (2 * S) + 1e-12).all()
        for l in axes[:6]:
            for radius in (0.0, 1e-3, 0.15, 1.0, np.pi / 2):
                d = R.cap_directions(l, radius, u1, u2)
                assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-12
                assert ((d * l).sum(-1) >= np.cos(radius) - 1e-12).all()
                if radius == 0.0:
                    assert np.array_equal(d, np.broadcast_to(l, d.shape))
    # a radius outside [0, pi / 2] is clamped into it, NaN counts as 0
    assert (R.clamp_radius(-1.0), R.clamp_radius(2.0), R.clamp_radius(float("nan"))) == (0.0, np.pi / 2, 0.0)
    # S = 1 and radius 0 are oi_trace_shadow_begin's rays
    pts, g = rs.randn(9, 3) * 0.3, rs.randn(9, 3)
    l = T.light_object_dir((0.3, -0.8, -0.5), np.eye(4))
    o, d, far, traced = R.light_rays(pts, g, np.arange(9), l, 0.0, 1, 0)
    o0, far0, traced0 = T.shadow_rays(pts, g, l)
    assert np.array_equal(o[0], o0) and np.array_equal(traced[0], traced0)
    assert np.abs(far[0] - far0).max() < 1e-14                                             # (a dot product summed in another order)
    assert np.array_equal(d[0], np.broadcast_to(l, (9, 3)))
    oa, da, fa, ta = R.ambient_rays(pts, g, np.arange(9), 4, 0, distance=0.25)
    assert ta.all() and (fa <= 0.25).all() and np.array_equal(oa[0], o0)


def test_cap_sine_in_float32():
    """Why the kernel evaluates sin(alpha) as sqrt(m (2 - m)), m = u1 (1 - cos r), and not as the header's sqrt(1 - cos^2 alpha):
    in float32 the latter cancels.  At r = 0.15, S = 64 the innermost sample's sine (0.0132) is off by 1.2e-6 in that form --
    more than the 1e-6 the directions are held to -- and by 2.3e-9 in the kernel's."""
    f = np.float32
    u1 = (f(0) + f(0.5)) / f(64)
    m = f(u1 * (f(1) - np.cos(f(0.15), dtype=f)))
    ca = f(f(1) - m)
    naive = np.sqrt(np.maximum(f(0), f(f(1) - f(ca * ca))), dtype=f)
    stable = np.sqrt(f(m * f(f(2) - m)), dtype=f)
    ca64 = 1.0 - (0.5 / 64) * (1.0 - np.cos(0.15))
    exact = np.sqrt(1.0 - ca64 * ca64)
    print("sin(alpha)", exact, "float32 error: 1 - cos^2 form", abs(float(naive) - exact), "m (2 - m) form", abs(float(stable) - exact))
    assert abs(float(naive) - exact) > 1e-6 and abs(float(stable) - exact) < 1e-8


def test_resolve_and_shade_of_the_restatement():
    L_, S, n_hit = 2, 3, 4
    rs = np.random.RandomState(1)
    st = rs.choice([T.MISS, T.HIT, T.LIMIT, T.START_INSIDE, T.NONFINITE, T.BACKFACING], size=L_ * S * n_hit)
    slot = np.array([-1, 2, 0, -1, 3, 1])
    out = R.resolve(st, slot, n_hit, L_, S)
    for l in range(L_):
        for px, i in enumerate(slot):
            want = 1.0 if i < 0 else float(np.float32(sum(st[(l * S + j) * n_hit + i] == T.MISS for j in range(S))) / np.float32(S))
            assert out[l, px] == want
    # S = 1 is oi_trace_visibility's rule
    st1 = st[:L_ * n_hit]
    assert np.array_equal(R.resolve(st1, slot, n_hit, L_, 1)[:, slot >= 0], T.visibility_of(st1.reshape(L_, n_hit))[:, slot[slot >= 0]])
    # the shade expression: ao scales the ambient part, visibility the rest
    n = 5
    ro, rd = rs.randn(n, 3), rs.randn(n, 3)
    rd /= np.linalg.norm(rd, axis=-1, keepdims=True)
    t, g, c = rs.rand(n) + 1, rs.randn(n, 3), rs.rand(n, 3)
    lt = np.array([T.light_block(d) for d in T.LIGHT_DIRS[:2]])
    vis, ao = rs.rand(2, n), rs.rand(n)
    assert np.abs(R.shade(ro, rd, t, g, c, np.eye(4), lt, vis) - T.shade(ro, rd, t, g, c, np.eye(4), lt, visibility=vis)).max() < 1e-15
    assert np.abs(R.shade(ro, rd, t, g, c, np.eye(4), lt) - T.shade(ro, rd, t, g, c, np.eye(4), lt)).max() < 1e-15
    amb = 0.33 * c.T[None] * ao[None, None]
    assert np.abs(R.shade(ro, rd, t, g, c, np.eye(4), lt, np.zeros((2, n)), ao) - amb).max() < 1e-15


def test_anyhit_machine_on_analytic_fields():
    """The scene of the GPU test on the oracle alone: outside the tangency band every state is the geometric one."""
    p, nrm = R.analytic_patch()
    pix = np.arange(len(p)) * 3 + 5
    o, d, far, traced = R.light_rays(p, nrm, pix, np.array(R.ANALYTIC_AXIS), R.ANALYTIC_RADIUS, R.ANALYTIC_S, R.SEED)
    assert traced.all()
    _, st, steps, in_flight = R.trace_anyhit(R.two_spheres, o, d, np.zeros(traced.size), far, max_steps=256)
    ca = R.closest_approach(o, d, far).reshape(-1)
    band = np.abs(ca - R.R1) < R.TANGENCY_BAND
    print("excluded", int(band.sum()), "of", band.size, "states", np.bincount(st).tolist(), "steps", int(steps.max()))
    assert band.sum() < R.EXCLUDED_CAP * band.size
    assert np.array_equal(st[~band], np.where(ca < R.R1, T.HIT, T.MISS)[~band])
    vis = (st.reshape(R.ANALYTIC_S, -1) == T.MISS).mean(0)
    r_xy = np.linalg.norm(p[:, :2], axis=-1)
    assert (vis[r_xy < 0.03] == 0).all() and (vis[r_xy > 0.2] == 1).all()
    assert ((vis > 0) & (vis < 1)).mean() >= 0.10
    # a steep field does not change MARCH; START_INSIDE, NONFINITE and one step only
    z3 = np.zeros(3)
    assert (R.trace_anyhit(R.two_spheres, np.zeros((3, 3)), d.reshape(-1, 3)[:3], z3, np.ones(3))[1] == T.START_INSIDE).all()
    assert (R.trace_anyhit(lambda x: np.full(len(x), np.nan), o.reshape(-1, 3)[:3], d.reshape(-1, 3)[:3], z3, np.ones(3))[1] == T.NONFINITE).all()
    assert set(np.unique(R.trace_anyhit(R.two_spheres, o, d, np.zeros(traced.size), far, max_steps=1)[1])) <= {T.LIMIT, T.HIT, T.MISS}


@pytest.mark.parametrize("seed,pose", T.VIEWS)
def test_anyhit_equals_full_in_the_oracle(seed, pose):
    """Golden field, the rehearsed views and lights: the any-hit oracle's visibility bits are the full oracle's, ray by ray,
    and it never evaluates more."""
    r = T.rehearse_primary(seed, pose)
    fld, ro, rd, near, far, w2b, t, status, steps = r["_state"]
    hit = status == T.HIT
    pts = ro[hit] + t[hit, None] * rd[hit]
    _, g, _ = fld.full(pts)
    for dd in T.LIGHT_DIRS:
        l = T.light_object_dir(dd, w2b)
        o, sfar, traced = T.shadow_rays(pts, g, l)
        n = int(traced.sum())
        ld = np.broadcast_to(l, (n, 3))
        _, st_full, _, fl_full = T.trace(fld.sdf, o[traced], ld, np.zeros(n), sfar[traced])
        _, st_any, _, fl_any = R.trace_anyhit(fld.sdf, o[traced], ld, np.zeros(n), sfar[traced])
        print(seed, pose, dd, "rays", n, "evaluations any-hit", sum(fl_any), "full", sum(fl_full))
        assert np.array_equal(st_any == T.MISS, st_full == T.MISS)
        assert sum(fl_any) <= sum(fl_full) and all(a <= b for a, b in zip(fl_any, fl_full))
        assert not (st_any == T.REFINE).any()


@pytest.mark.parametrize("seed,pose", R.SOFT_VIEWS)
def test_rehearsal_of_the_gpu_configuration(seed, pose):
    """The exact views, lights, radius, S and ao_distance of tests/test_gpu_occlusion.py on the fp64 oracle alone: at most 1 %
    of the rays of each secondary trace run out of steps, none starts inside."""
    r = R.rehearse_soft(seed, pose)
    print(seed, pose, r)
    lights = [r[f"light{i}"] for i in range(len(R.SOFT_LIGHTS))]
    for sets in (lights, [r["ambient"]]):
        traced, limit = sum(s["traced"] for s in sets), sum(s["limit"] for s in sets)
        assert traced > 0.5 * sum(s["of"] for s in sets)
        assert limit <= R.REHEARSAL_LIMIT_CAP * traced
        assert all(s["start_inside"] == 0 for s in sets)
        assert all(s["traced"] == s["limit"] + s["occluded"] + s["lit"] for s in sets)
    assert r["ambient"]["traced"] == r["ambient"]["of"] == R.AO_S * r["n_hit"]
