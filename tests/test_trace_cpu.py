"""CPU checks of the sphere tracer (include/oi_trace.h, oi_amd.trace, oi_amd.inference.surface_*): the REHEARSAL of the
tracer on the fp64 oracle alone (tests/helpers/trace_ref.py) for exactly the views and lights tests/test_gpu_trace.py uses,
header <=> library <=> binding <=> helper, and the argument refusals that need no GPU.

Rehearsal results (oracle alone, float64, golden weights, 48 x 48 rays of the example camera, defaults tol 1e-5, omega 1,
64 steps, bias 1e-2; seeds 0, 1, 2 x poses centre / off):

    hits 464 .. 540 of 2304 (20 .. 23 %), LIMIT 4 .. 14 (0.2 .. 0.6 %), no START_INSIDE, no NONFINITE
    6.6 .. 7.5 sdf evaluations per ray, median 7 .. 9 on hit rays
    no hit with a negative sample before t - 2e-3, no miss with a negative sample
    shadow rays (three lights): 323 .. 434 traced per light and view, none starts inside, at most 4 run out of steps;
    the golden object is nearly convex: one occluded ray in all 18 (view, light) pairs"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import cabi
from helpers import trace_ref as T

KW = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)


@pytest.mark.parametrize("seed,pose", T.VIEWS)
def test_rehearsal_on_the_oracle_satisfies_every_cap(seed, pose):
    r = T.rehearse_primary(seed, pose)
    state = r.pop("_state")
    print(r)
    assert r["N"] == T.R_VIEW ** 2 and r["hit"] > 0.15 * r["N"]
    assert r["start_inside"] == 0 and r["nonfinite"] == 0
    assert r["limit"] <= T.LIMIT_CAP * r["N"]
    assert r["hits_with_earlier_negative"] == 0 and r["misses_with_negative"] == 0
    assert r["hit"] + r["miss"] + r["limit"] == r["N"]
    assert 4.0 < r["evals_per_ray"] < 12.0          # against 320 full evaluations per ray of the volume render
    sh = T.rehearse_shadows(state)
    print(sh)
    assert len(sh) == len(T.LIGHT_DIRS) == 3
    for s in sh:
        assert s["traced"] > 0.5 * r["hit"]
        assert s["start_inside"] <= T.SHADOW_START_INSIDE_CAP * s["traced"]
        assert s["traced"] == s["start_inside"] + s["limit"] + s["occluded"] + s["lit"]


def test_state_machine_on_analytic_fields():
    n = 64
    o = np.tile([[0.0, 0.0, -3.0]], (n, 1))
    x = np.linspace(-0.9, 0.9, n)
    d = np.stack([x, np.zeros(n), np.full(n, 3.0)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    mid = -(o * d).sum(-1)
    sphere = lambda p: np.linalg.norm(p, axis=-1) - 0.5
    t, st, steps, in_flight = T.trace(sphere, o, d, mid - 1, mid + 1)
    hits = np.abs(x) < 0.49
    assert np.array_equal(st[hits], np.full(hits.sum(), T.HIT)) and (st[np.abs(x) > 0.51] == T.MISS).all()
    assert np.abs(sphere(o + t[:, None] * d))[st == T.HIT].max() <= T.TOL
    assert in_flight[0] == n and all(a >= b for a, b in zip(in_flight, in_flight[1:])) and sum(in_flight) == steps.sum()
    # a field twice as steep as a distance: marching overshoots, the bracket recovers the first crossing
    steep = lambda p: 2.0 * sphere(p)
    t2, st2, _, _ = T.trace(steep, o, d, mid - 1, mid + 1)
    inner = np.abs(x) < 0.4                          # (a grazing ray can step through a field this steep: no bracket)
    assert (st2[inner] == T.HIT).all() and np.abs(t2 - t)[inner].max() < 1e-4
    # first sample inside, a NaN field, one step only
    assert (T.trace(sphere, np.zeros((3, 3)), d[:3], np.zeros(3), np.ones(3))[1] == T.START_INSIDE).all()
    assert (T.trace(lambda p: np.full(len(p), np.nan), o, d, mid - 1, mid + 1)[1] == T.NONFINITE).all()
    assert set(np.unique(T.trace(sphere, o, d, mid - 1, mid + 1, max_steps=1)[1])) <= {T.LIMIT, T.HIT}
    # shadow rays of a sphere: the exit of the unit sphere, and no ray of a convex body is occluded
    pts = (o + t[:, None] * d)[st == T.HIT]
    l = T.light_object_dir((0.3, -0.8, -0.5), np.eye(4))
    so, far, traced = T.shadow_rays(pts, pts, l)
    assert np.allclose(np.linalg.norm(so + far[:, None] * l, axis=-1), 1.0) and traced.any() and not traced.all()
    k = int(traced.sum())
    assert (T.trace(sphere, so[traced], np.broadcast_to(l, (k, 3)), np.zeros(k), far[traced])[1] == T.MISS).all()
    assert T.visibility_of([T.MISS, T.HIT, T.LIMIT, T.START_INSIDE, T.NONFINITE, T.BACKFACING]).tolist() == [1, 0, 0, 0, 0, 0]


_lib = cabi.built_lib


def test_header_library_binding_and_helper_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_trace.h", lib)
    assert sorted(names) == ["oi_surface_shade", "oi_trace_begin", "oi_trace_finish", "oi_trace_shadow_begin", "oi_trace_step",
                             "oi_trace_visibility"]
    assert mirrors == ["TraceState", "SurfaceParams"]   # the ctypes mirrors have the header's fields, in its order
    text = cabi.read("oi_trace.h")
    ints = {"OI_TRACE_MISS": (lib.TRACE_MISS, T.MISS), "OI_TRACE_HIT": (lib.TRACE_HIT, T.HIT), "OI_TRACE_LIMIT": (lib.TRACE_LIMIT, T.LIMIT),
            "OI_TRACE_START_INSIDE": (lib.TRACE_START_INSIDE, T.START_INSIDE), "OI_TRACE_NONFINITE": (lib.TRACE_NONFINITE, T.NONFINITE),
            "OI_TRACE_BACKFACING": (lib.TRACE_BACKFACING, T.BACKFACING), "OI_TRACE_MARCH": (lib.TRACE_MARCH, T.MARCH),
            "OI_TRACE_REFINE": (lib.TRACE_REFINE, T.REFINE), "OI_TRACE_DEFAULT_MAX_STEPS": (lib.TRACE_DEFAULT_MAX_STEPS, T.MAX_STEPS),
            "OI_TRACE_MAX_STEPS": (lib.TRACE_MAX_STEPS, T.MAX_MAX_STEPS), "OI_TRACE_COUNT_WORDS": (lib.TRACE_COUNT_WORDS, T.COUNT_WORDS)}
    for macro, (a, b) in ints.items():
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == a == b, macro
    assert (T.MISS, T.HIT, T.LIMIT, T.START_INSIDE, T.NONFINITE) == (0, 1, 2, 3, 4)
    floats = {"OI_TRACE_DEFAULT_TOL": (lib.TRACE_DEFAULT_TOL, T.TOL), "OI_TRACE_DEFAULT_OMEGA": (lib.TRACE_DEFAULT_OMEGA, T.OMEGA),
              "OI_TRACE_DEFAULT_BIAS": (lib.TRACE_DEFAULT_BIAS, T.BIAS)}
    for macro, (a, b) in floats.items():
        assert float(re.search(r"#define %s ([0-9.e+-]+)f" % macro, text).group(1)) == a == b, macro
    assert (T.TOL, T.OMEGA, T.MAX_STEPS, T.BIAS) == (1e-5, 1.0, 64, 1e-2)
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"trace.hip"' in src


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)

    def state(N=5, **kw):
        S = lib.TraceState()
        S.N = N
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(S, n, kw.get(n, f))
        return ctypes.byref(S)

    def surf(**kw):
        P = lib.SurfaceParams()
        P.N, P.n_hit, P.L = kw.pop("N", 5), kw.pop("n_hit", 2), kw.pop("L", 1)
        for n, _ in lib.SurfaceParams._fields_[3:]:
            setattr(P, n, kw.get(n, f))
        return ctypes.byref(P)

    cases = [(lambda: L.oi_trace_begin(None, None), "oi_trace_begin", "null state"),
             (lambda: L.oi_trace_begin(state(N=0), None), "oi_trace_begin", "N=0"),
             (lambda: L.oi_trace_begin(state(N=1 << 31), None), "oi_trace_begin", "N=2147483648"),
             (lambda: L.oi_trace_begin(state(counts=None), None), "oi_trace_begin", "null pointer"),
             (lambda: L.oi_trace_step(state(), f, 5, -1, 1e-5, 1.0, None), "oi_trace_step", "k=-1"),
             (lambda: L.oi_trace_step(state(), f, 5, 1024, 1e-5, 1.0, None), "oi_trace_step", "k=1024"),
             (lambda: L.oi_trace_step(state(), f, 6, 0, 1e-5, 1.0, None), "oi_trace_step", "bound=6"),
             (lambda: L.oi_trace_step(state(), f, 5, 0, 0.0, 1.0, None), "oi_trace_step", "tol"),
             (lambda: L.oi_trace_step(state(), f, 5, 0, 1e-5, float("nan"), None), "oi_trace_step", "omega"),
             (lambda: L.oi_trace_step(state(), None, 5, 0, 1e-5, 1.0, None), "oi_trace_step", "null sdf"),
             (lambda: L.oi_trace_step(state(active=None), f, 5, 0, 1e-5, 1.0, None), "oi_trace_step", "null pointer"),
             (lambda: L.oi_trace_finish(state(), None, f, f, None), "oi_trace_finish", "null"),
             (lambda: L.oi_trace_shadow_begin(state(N=6), f, f, 2, f, 0, f, 0.01, None), "oi_trace_shadow_begin", "L=0"),
             (lambda: L.oi_trace_shadow_begin(state(N=6), f, f, 2, f, 257, f, 0.01, None), "oi_trace_shadow_begin", "L=257"),
             (lambda: L.oi_trace_shadow_begin(state(N=7), f, f, 2, f, 3, f, 0.01, None), "oi_trace_shadow_begin", "L * n_hit"),
             (lambda: L.oi_trace_shadow_begin(state(N=6), f, f, 2, f, 3, f, -1.0, None), "oi_trace_shadow_begin", "bias"),
             (lambda: L.oi_trace_shadow_begin(state(N=6), f, None, 2, f, 3, f, 0.01, None), "oi_trace_shadow_begin", "null"),
             (lambda: L.oi_trace_visibility(f, f, 0, 0, 1, f, None), "oi_trace_visibility", "N=0"),
             (lambda: L.oi_trace_visibility(f, f, 5, 6, 1, f, None), "oi_trace_visibility", "n_hit=6"),
             (lambda: L.oi_trace_visibility(f, f, 5, 2, 300, f, None), "oi_trace_visibility", "L=300"),
             (lambda: L.oi_trace_visibility(f, None, 5, 2, 1, f, None), "oi_trace_visibility", "null"),
             (lambda: L.oi_surface_shade(None, None), "oi_surface_shade", "null params"),
             (lambda: L.oi_surface_shade(surf(N=0), None), "oi_surface_shade", "N=0"),
             (lambda: L.oi_surface_shade(surf(L=0), None), "oi_surface_shade", "L=0"),
             (lambda: L.oi_surface_shade(surf(L=257), None), "oi_surface_shade", "L=257"),
             (lambda: L.oi_surface_shade(surf(status=None), None), "oi_surface_shade", "null input"),
             (lambda: L.oi_surface_shade(surf(grad=None), None), "oi_surface_shade", "null hit arrays")]
    for call, entry, text in cases:
        assert call() == -1, (entry, text)
        msg = L.oi_last_error().decode()
        assert msg.startswith(entry) and text in msg, (entry, text, msg)
    assert L.oi_trace_step(state(), None, 0, 3, 1e-5, 1.0, None) == 0      # bound = 0: success, nothing launched


def test_python_argument_checks():
    from oi_amd import inference, lib, trace
    from oi_amd.fields import ShapeNetwork, ColorNetwork, FieldPack
    net = ShapeNetwork(None, **KW)
    pack = FieldPack(net, ColorNetwork(**KW))
    ro, rd, z = torch.zeros(5, 3), torch.ones(5, 3), torch.zeros(1, 64)
    for bad in (0, 1025, 2.0, True, None):
        with pytest.raises(ValueError, match="max_steps"):
            trace.sphere_trace(pack, ro, rd, z=z, max_steps=bad)
    for kw in (dict(tol=0.0), dict(omega=-1.0), dict(tol=float("nan"))):
        with pytest.raises(ValueError, match="tol"):
            trace.sphere_trace(pack, ro, rd, z=z, **kw)
    with pytest.raises(ValueError, match="readback"):
        trace.sphere_trace(pack, ro, rd, z=z, readback=0)
    with pytest.raises(NotImplementedError, match="siren_network"):
        trace.sphere_trace(pack, ro, rd, z=z, siren_network=net)
    with pytest.raises(ValueError, match="one latent"):
        trace.sphere_trace(pack, ro, rd, z=torch.zeros(2, 64))
    with pytest.raises(ValueError, match="latent"):
        trace.sphere_trace(pack, ro, rd)
    with pytest.raises(ValueError, match="colour head"):
        trace.sphere_trace(net, ro, rd, z=z)
    with pytest.raises(TypeError):
        trace.sphere_trace(object(), ro, rd, z=z)
    with pytest.raises(ValueError, match=r"\(\.\.\., 3\)"):
        trace.sphere_trace(pack, ro, torch.ones(5, 2), z=z)
    with pytest.raises(lib.OiHipError):   # no CPU path
        trace.sphere_trace(pack, ro, rd, z=z)
    with pytest.raises(ValueError, match="visibility"):
        inference.surface_frames(None, [], [], keys=("visibility",))
    with pytest.raises(ValueError, match="keys"):
        inference.surface_frames(None, [], [], keys=("shading_map",))
    assert (trace.DEFAULT_TOL, trace.DEFAULT_OMEGA, trace.DEFAULT_MAX_STEPS, trace.DEFAULT_BIAS) == (T.TOL, T.OMEGA, T.MAX_STEPS, T.BIAS)
