"""CPU checks of glossy environment lighting (include/oi_envgloss.h): the properties of the fp64
restatement (tests/helpers/envgloss_ref.py) that hold exactly or by derivation -- the furnace and where its quadrature fails,
the directional limit against the Phong term of the directional-light path, the lobe sampler's first moment, rotation and
lookup through oi_amd.envlight.EnvMap -- the expected visibilities of the analytic scene, the refusals that need no GPU, and
header <=> library <=> binding."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import cabi
from helpers import env_ref as E
from helpers import envgloss_ref as Q
from helpers import mesh_attr_ref as A
from helpers import occlusion_ref as R
from helpers import trace_ref as T

NAMES = ["oi_env_prefilter", "oi_env_prefilter_partial_floats", "oi_env_shade_glossy", "oi_occlusion_lobe_begin"]

_lib = cabi.built_lib


def test_furnace_and_where_the_quadrature_fails():
    """A constant map: G_s = 2 / (s + 1).  The midpoint rule over 32 x 64 pixels is within 5e-3 of it up to s = 200; 16 rows at
    s = 200 are too few (the lobe's half-width 1 / sqrt(s) = 0.07 rad against pixels of 0.2 rad), which is what
    EnvMap.from_equirect warns of."""
    from oi_amd.envlight import EnvMap
    from oi_amd.lib import OiHipError
    worst = 0.0
    for s in (1, 10, 50, 200):
        g, mag, _ = Q.prefilter(np.ones((1, 3, 32, 64)), s, 4, 8)
        rel = float(np.abs(g * (s + 1) / 2.0 - 1.0).max())
        worst = max(worst, rel)
        assert rel < 5e-3, (s, rel)
        assert np.array_equal(g, mag)
    print("furnace: worst relative error of a 32 x 64 map on a 4 x 8 grid", worst)
    # Where the bound does NOT hold, measured and stated: a lobe that reaches a pole, where the first band's
    # midpoint cannot stand for the band.  On the default 64 x 128 grid the rows 8 .. 55 (more than 0.4 rad from either pole)
    # are inside the bound at every s; nearer the poles the sum is off by up to 2 % at s = 50 and 9 % at s = 200.
    for s in (1, 10, 50, 200):
        g, _, _ = Q.prefilter(np.ones((1, 3, 32, 64)), s, 64, 128)
        rel = np.abs(g[0, 0] * (s + 1) / 2.0 - 1.0).max(1)
        print("furnace: s", s, "rows 8 .. 55", float(rel[8:56].max()), "polar rows", float(rel.max()))
        assert rel[8:56].max() < 5e-3 and rel.max() < 0.1
    g, _, _ = Q.prefilter(np.ones((1, 3, 16, 32)), 200, 8, 16)
    coarse = float(np.abs(g * 201 / 2.0 - 1.0).max())
    print("furnace: 16 x 32 at s = 200 is off by", coarse)
    assert 0.1 < coarse < 0.5
    # the warning fires for the coarse map, before any device work (there is no device here: the projection then refuses)
    with pytest.warns(UserWarning, match="too coarse"):
        with pytest.raises((OiHipError, RuntimeError, AssertionError)):
            EnvMap.from_equirect(np.ones((3, 16, 32), dtype=np.float32), 200, device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises((OiHipError, RuntimeError, AssertionError)):
            EnvMap.from_equirect(np.ones((3, 32, 64), dtype=np.float32), 200, device="cpu")


def test_directional_limit_is_the_phong_term():
    """One texel holding pi c / w_texel is the directional light of colour c from that texel's direction: G(d) =
    c relu(d . d_texel)^s, and k_s G(r) is the specular term of the directional-light path with specular colour k_s c, for
    random normals and eyes.  That term is taken from tests/helpers/trace_ref.py's shade, the fp64 restatement of
    oi_surface_shade: a test helper, not product code (oi_amd.lighting holds the parameters and has no host evaluation of the
    term), so this test compares two restatements and pins the model, not the library."""
    rs = np.random.RandomState(1)
    He, We, s = 9, 14, 10.0
    d_in, w = E.equirect(He, We)
    r0, c0 = 3, 5
    col = np.array([0.7, 1.1, 0.4])
    img = np.zeros((1, 3, He, We))
    img[0, :, r0, c0] = np.pi * col / w[r0]
    l = d_in[r0, c0]
    d = A.unit(rs.randn(200, 3))
    g, _, _ = Q.convolve(img, s, d)
    err = float(np.abs(g[0].T - col[None] * np.maximum(d @ l, 0.0)[:, None] ** s).max())
    print("directional limit: G against c relu(d . l)^s", err)
    assert err < 1e-12
    # against the Phong specular of the directional-light path: ambient = diffuse = 0, specular k_s c, w2b = identity
    n_pts = 64
    pos, grad = 0.3 * A.unit(rs.randn(n_pts, 3)), rs.randn(n_pts, 3) * rs.uniform(0.3, 2.0, (n_pts, 1))
    eye = pos + A.unit(grad + 0.7 * rs.randn(n_pts, 3)) * rs.uniform(1.0, 3.0, (n_pts, 1))
    rd = A.unit(pos - eye)
    t = np.linalg.norm(pos - eye, axis=-1)
    ks = np.array([0.35, 0.2, 0.5])
    n, v, r = Q.reflect(grad, pos, eye)
    lit = (n @ l) > 0
    assert lit.sum() > 10 and (~lit).sum() > 10
    g_r, _, _ = Q.convolve(img, s, A.unit(r))
    mine = ks[None] * g_r[0].T * lit[:, None]                                  # [n . l > 0] is V_spec's horizon for a delta
    ref = np.zeros((n_pts, 3))
    for ch in range(3):
        light = T.light_block(tuple(l), ambient=0.0, diffuse=0.0, specular=float(ks[ch] * col[ch]), shininess=s)
        ref[:, ch] = T.shade(eye, rd, t, grad, np.ones((n_pts, 3)), np.eye(4), [light])[0, ch]
    err = float(np.abs(mine - ref).max())
    print("directional limit: k_s G(r) against the Phong specular", err)
    assert np.abs(ref).max() > 0.05 and err < 1e-12


def test_sampler():
    pix = np.arange(64) * 13 + 5
    axes = A.unit(np.random.RandomState(2).randn(64, 3))
    axes[0], axes[1] = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    for s in (1.0, 10.0, 200.0, 4096.0):
        d = Q.lobe_directions(axes, pix, 256, s, seed=3)
        assert np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() < 1e-12
        mean = (d * axes[None]).sum(-1).mean(0)                                  # per pixel, over the 256 strata
        assert np.abs(mean - (s + 1.0) / (s + 2.0)).max() < 1e-3, (s, np.abs(mean - (s + 1.0) / (s + 2.0)).max())
        c, sn = Q.lobe_angles(R.sample_numbers(pix, 3, 256)[0], s)
        assert (c > 0).all() and (c <= 1).all() and (sn >= 0).all() and np.abs(c * c + sn * sn - 1).max() < 1e-15
    # sin(alpha) = 0 gives the axis itself
    same = R.directions(axes, np.zeros(64), np.ones(64), np.linspace(0, 1, 64, endpoint=False))
    assert np.array_equal(same, axes)
    assert Q.lobe_angles(np.array([1.0]), 7.0) == (1.0, 0.0)


def test_lobe_cases_of_the_gpu_test():
    """The GPU test's inputs, on the restatement alone: the sign of the axis' z (the tangent frame's branch) is not in doubt,
    at most 2 % of a case's rays are nearer the horizon than the bar (64 * 2^-24) that exempts a ray from the exact status
    check, and over the cases both outcomes are common."""
    bar = 64 * 2.0 ** -24
    traced_all = []
    for n_hit, S, s in Q.LOBE_CASES:
        pts, grad, pix, eyes = Q.lobe_case(n_hit, S, s)
        _, _, r = Q.reflect(grad, pts, eyes[pix])
        assert (np.abs(r[:, 2]) > 1e-4).all(), (n_hit, S, s)
        _, d, far, traced, nd = Q.lobe_rays(pts, grad, pix, eyes[pix], S, float(s), 11 + s, T.BIAS)
        assert (np.abs(nd) <= bar).mean() <= 0.02, (n_hit, S, s)
        assert (far > 0).all()
        traced_all.append(traced.reshape(-1))
    share = np.concatenate(traced_all).mean()
    print("lobe cases: traced share", share)
    assert 0.5 < share < 0.99


def _random_map(rs, Hp, Wp, s):
    from oi_amd.envlight import EnvLight, EnvMap
    return EnvMap(EnvLight(rs.randn(9, 3)), torch.from_numpy(rs.randn(3, Hp, Wp).astype(np.float32)), s)


def test_rotation_and_lookup():
    from oi_amd.envlight import EnvMap
    rs = np.random.RandomState(4)
    env = _random_map(rs, 6, 11, 10.0)
    g = env.map.numpy().astype(np.float64)
    d = A.unit(rs.randn(300, 3))
    assert np.abs(env.glossy(d) - Q.lookup(g, d)).max() < 1e-12                    # the library's host lookup is the header's
    R1, R2 = E.random_rotation(rs), E.axis_rotation((0.3, -0.2, 0.9), 1.1)
    rot = env.rotated(R1)
    assert rot.map is env.map and rot.shininess == env.shininess                   # shared, not copied
    assert np.abs(rot.glossy(d) - env.glossy(d @ R1)).max() < 1e-12                 # G'(d) = G(R^T d)
    assert np.abs(rot.sh.coeffs - env.sh.rotated(R1).coeffs).max() < 1e-12
    two = rot.rotated(R2)
    assert two.map is env.map and np.abs(two.rotation - R2 @ R1).max() < 1e-15
    assert np.abs(two.glossy(d) - env.glossy(d @ (R2 @ R1))).max() < 1e-12
    with pytest.raises(ValueError, match="rotation"):
        env.rotated(np.diag([1.0, 1.0, -1.0]))
    # the seam: phi just below 2 pi and just above 0 are neighbours, both between the last and the first column
    Hp, Wp = g.shape[1:]
    th = np.pi * (2 + 0.5) / Hp                                                    # on row 2 exactly
    for phi, f in ((1e-9, 0.5), (2 * np.pi - 1e-9, 0.5), (np.pi / Wp * 0.5, 0.75)):
        dd = np.array([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)])
        want = (1 - f) * g[:, 2, Wp - 1] + f * g[:, 2, 0]
        assert np.abs(env.glossy(dd) - want).max() < 1e-7 and np.abs(Q.lookup(g, dd) - want).max() < 1e-7
    # the poles: rows clamp, so at theta = 0 / pi the value is row 0 / Hp - 1 interpolated in phi alone
    for z, row in ((1.0, 0), (-1.0, Hp - 1)):
        dd = np.array([0.0, 0.0, z])                                               # atan2(0, 0) = 0: v = -1/2
        want = 0.5 * g[:, row, Wp - 1] + 0.5 * g[:, row, 0]
        assert np.abs(env.glossy(dd) - want).max() < 1e-12 and np.abs(Q.lookup(g, dd) - want).max() < 1e-12
    # the closed form of a constant environment, whatever the direction and the rotation
    c = EnvMap.constant((0.2, 0.5, 1.0), 10.0)
    assert tuple(c.map.shape) == (3, 1, 1) and np.abs(c.sh.coeffs[0] - 2 * np.sqrt(np.pi) * np.array([0.2, 0.5, 1.0])).max() < 1e-15
    assert np.abs(c.rotated(R1).glossy(d) - np.array([0.2, 0.5, 1.0]) * 2.0 / 11.0).max() < 1e-7   # (the map is float32)
    assert np.abs(EnvMap.constant(1.0, 1.0).glossy(d) - 1.0).max() == 0


def test_stacking():
    from oi_amd.envlight import EnvLight, stack_maps
    rs = np.random.RandomState(5)
    a, b = _random_map(rs, 4, 8, 10.0), _random_map(rs, 4, 8, 10.0)
    R1 = E.random_rotation(rs)
    sh, maps, index, rot, s = stack_maps([a, b.rotated(R1), a.rotated(R1), b], "cpu")
    assert sh.shape == (4, 9, 3) and maps.shape == (2, 3, 4, 8) and index == [0, 1, 0, 1] and rot.shape == (4, 3, 3) and s == 10.0
    assert torch.equal(maps[0], a.map) and torch.equal(maps[1], b.map)
    assert np.abs(rot[1].numpy() - R1).max() < 1e-7 and torch.equal(rot[0], torch.eye(3))
    with pytest.raises(ValueError, match="shininess"):
        stack_maps([a, _random_map(rs, 4, 8, 11.0)], "cpu")
    with pytest.raises(ValueError, match="sizes"):
        stack_maps([a, _random_map(rs, 4, 9, 10.0)], "cpu")
    with pytest.raises(TypeError):
        stack_maps([a, EnvLight.constant(1)], "cpu")


def test_analytic_scene_expectations():
    """The visibilities the GPU test expects, and the stratified estimator's spread against its bar."""
    cap = E.analytic_cap_angle(Q.ANALYTIC_BIAS)
    assert abs(cap - 0.7985) < 1e-4
    v0, v6 = Q.analytic_lobe_visibility(0.0, 10.0, n1=1000, n2=1000), Q.analytic_lobe_visibility(0.6, 10.0, n1=1000, n2=1000)
    print("analytic lobe visibility: beta = 0", v0, "beta = 0.6", v6)
    assert abs(v0 - np.cos(cap) ** 11) < 2e-3 and abs(v0 - 0.019) < 2e-3 and abs(v6 - 0.316) < 3e-3
    # the S = 256 estimator over many pixels: its standard deviation is far inside the bar 5 * 0.5 / sqrt(256)
    pix = np.arange(400) * 3 + 1
    pts = np.broadcast_to(np.array([0.0, 0.0, E.R0]), (400, 3))
    for beta, want in ((0.0, v0), (0.6, v6)):
        eyes = np.broadcast_to(Q.analytic_eye(beta), (400, 3))
        o, d, far, traced, _ = Q.lobe_rays(pts, pts, pix, eyes, 256, 10.0, 7, Q.ANALYTIC_BIAS)
        oc = E.C1 - o
        tc = (d * oc).sum(-1)
        blocked = (tc > 0) & ((oc * oc).sum(-1) - tc * tc < E.R1 ** 2)
        est = (traced & ~blocked).mean(0)
        print("beta", beta, "estimator mean", est.mean(), "std", est.std())
        assert abs(est.mean() - want) < 0.01 and est.std() < 0.05 < 5 * 0.5 / np.sqrt(256)


def test_refusals_without_a_gpu():
    from oi_amd import envlight, inference, ops, trace
    from oi_amd.envlight import EnvLight, EnvMap
    for bad in (0.5, 4097, float("nan"), float("inf"), -1, None, "x", True):
        with pytest.raises(ValueError, match="shininess"):
            EnvMap.constant(1.0, bad)
        with pytest.raises(ValueError, match="shininess"):
            ops.env_prefilter(torch.zeros(1, 3, 4, 8), bad, (2, 4))
    for bad in (0.5, 4097, float("nan")):
        with pytest.raises(ValueError, match="shininess"):
            trace.capture_transfer(None, None, None, glossy_samples=4, shininess=bad)
        with pytest.raises(ValueError, match="shininess"):
            EnvMap.from_equirect(np.zeros((3, 4, 8), dtype=np.float32), bad)
    for bad in (-1, 257, 2.0, True, "4"):
        with pytest.raises(ValueError, match="glossy_samples"):
            trace.capture_transfer(None, None, None, glossy_samples=bad, shininess=10.0)
        with pytest.raises(ValueError, match="glossy_samples"):
            trace.render_surface_env(None, None, None, [EnvMap.constant(1, 10)], glossy_samples=bad, shininess=10.0)
    assert trace._check_glossy(None, None, None, "x") == (None, None, None)
    with pytest.raises(ValueError, match="without glossy_samples"):                # 0 samples has to be said, not implied
        trace.capture_transfer(None, None, None, shininess=10.0)
    with pytest.raises(ValueError, match="env_prefilter"):
        ops.env_prefilter(torch.zeros(3, 4, 8), 10.0, (2, 4))
    with pytest.raises(ValueError, match="env_prefilter"):
        ops.env_prefilter(torch.zeros(1, 3, 4, 8), 10.0, (0, 4))
    for shape in ((8, 16), (1, 3, 8, 16), (8, 16, 4)):
        with pytest.raises(ValueError, match="from_equirect"):
            EnvMap.from_equirect(np.zeros(shape, dtype=np.float32), 10.0)
    with pytest.raises(TypeError, match="EnvLight"):
        EnvMap(np.zeros((9, 3)), torch.zeros(3, 1, 1), 10.0)
    with pytest.raises(ValueError, match="float32"):
        EnvMap(EnvLight.constant(1), torch.zeros(1, 1), 10.0)
    with pytest.raises(TypeError, match="EnvLight or an EnvMap"):
        inference.env_walk(None, None, None, "sky", 4)

    # shade's own refusals come before it touches the device: a capture needs only the fields they read
    class _S:
        ro = torch.zeros(4, 3)
        N, n_hit, H = 4, 0, 2
    m10, m20 = EnvMap.constant(1.0, 10.0), EnvMap.constant(1.0, 20.0)
    plain = trace.TransferCapture(_S(), torch.zeros(9, 4), {}, 0)
    with pytest.raises(ValueError, match="no reflection-lobe trace"):
        plain.shade([m10])
    with pytest.raises(ValueError, match="specular"):
        plain.shade([EnvLight.constant(1)], specular=0.5)
    glossy = trace.TransferCapture(_S(), torch.zeros(9, 4), {}, 0, glossy_samples=0, shininess=10.0, specular=(0.1,) * 3)
    with pytest.raises(ValueError, match="one list"):
        glossy.shade([m10, EnvLight.constant(1)])
    with pytest.raises(ValueError, match="shininess"):
        glossy.shade([m20])
    with pytest.raises(ValueError, match="shininess"):
        glossy.shade([m10, m20])
    # map indices are checked before anything is uploaded
    z = torch.zeros
    with pytest.raises(ValueError, match="map_index"):
        ops.env_shade_glossy(z(4, dtype=torch.uint8), z(4, dtype=torch.int32), None, 0, z(9, 4), z(2, 9, 3), z(4, 3), None, None,
                             z(4, 4), None, z(1, 3, 2, 4), [0, 1], z(2, 3, 3), z(3))
    with pytest.raises(ValueError, match="map_index"):
        ops.env_shade_glossy(z(4, dtype=torch.uint8), z(4, dtype=torch.int32), None, 0, z(9, 4), z(2, 9, 3), z(4, 3), None, None,
                             z(4, 4), None, z(1, 3, 2, 4), [0], z(2, 3, 3), z(3))


def test_header_library_and_binding_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_envgloss.h", lib)
    assert sorted(names) == NAMES == lib.symbols("oi_envgloss.h") and mirrors == []       # no struct of its own
    text = cabi.read("oi_envgloss.h")
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert define("OI_ENVGLOSS_MIN_SHININESS") == lib.ENVGLOSS_MIN_SHININESS == Q.MIN_SHININESS
    assert define("OI_ENVGLOSS_MAX_SHININESS") == lib.ENVGLOSS_MAX_SHININESS == Q.MAX_SHININESS
    assert define("OI_ENVGLOSS_CHUNK") == lib.ENVGLOSS_CHUNK == Q.CHUNK
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"envgloss.hip"' in src and "include/oi_envgloss.h" in src
    pf = L.oi_env_prefilter_partial_floats
    assert pf(1, 1, 1, 1, 1) == 3 and pf(3, 33, 65, 9, 17) == 3 * 2 * 3 * 9 * 17 and pf(1, 32, 64, 4, 8) == 3 * 32
    assert pf(1, 32, 65, 4, 8) == 2 * 3 * 32 and pf(2, 256, 512, 64, 128) == 2 * 64 * 3 * 64 * 128
    assert pf(0, 4, 4, 2, 2) == 0 and pf(257, 4, 4, 2, 2) == 0 and pf(1, 0, 4, 2, 2) == 0 and pf(1, 4, 4, 2, 0) == 0
    assert pf(2, 1 << 15, 1 << 15, 2, 2) == 0 and pf(1, 4, 4, 1 << 15, 1 << 15) == 0
    assert pf(1, 1 << 15, 1 << 15, 1 << 12, 1 << 13) == 0                          # 2^19 chunks x 2^17 tiles of workgroups
    assert pf(256, 256, 512, 64, 128) == 256 * 64 * 3 * 64 * 128                   # 2^19 workgroups
    assert pf(1, 2048, 4096, 64, 128) > 0 and pf(1, 2048, 4096, 128, 128) > 0      # 2^17 and 2^18 of them
    assert pf(4, 2048, 4096, 256, 512) == 4 * 4096 * 3 * 256 * 512                 # 2^2 x 2^12 chunks x 2^9 tiles = 2^23: the limit
    assert pf(5, 2048, 4096, 256, 512) == 0 and pf(16, 2048, 4096, 256, 512) == 0  # above it


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)
    pf, lb, sh = "oi_env_prefilter", "oi_occlusion_lobe_begin", "oi_env_shade_glossy"

    def state(N=12, **kw):
        S = lib.TraceState()
        S.N = N
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(S, n, kw.get(n, f))
        return ctypes.byref(S)

    def shade(index=(0,), M=1, Hp=2, Wp=4, spec=f, args=None, **kw):
        P = lib.EnvShadeParams()
        P.N, P.n_hit, P.F = kw.pop("N", 5), kw.pop("n_hit", 2), kw.pop("F", len(index or ()))
        for n, _ in lib.EnvShadeParams._fields_[3:]:
            setattr(P, n, kw.get(n, f))
        a = dict(rays_o=f, hit_points=f, grad=f, w2b=f, spec_vis=f, glossy=f, rot=f, k_s=f)
        a.update(args or {})
        idx = (ctypes.c_int * max(len(index), 1))(*index) if index is not None else None
        return L.oi_env_shade_glossy(ctypes.byref(P), a["rays_o"], a["hit_points"], a["grad"], a["w2b"], a["spec_vis"], a["glossy"],
                                     M, Hp, Wp, idx, a["rot"], a["k_s"], spec, None)

    nan, inf = float("nan"), float("inf")
    cases = [(lambda: L.oi_env_prefilter(f, 1, 4, 8, 0.5, 2, 4, f, f, None), pf, "shininess"),
             (lambda: L.oi_env_prefilter(f, 1, 4, 8, 4097.0, 2, 4, f, f, None), pf, "shininess"),
             (lambda: L.oi_env_prefilter(f, 1, 4, 8, nan, 2, 4, f, f, None), pf, "shininess"),
             (lambda: L.oi_env_prefilter(f, 1, 4, 8, inf, 2, 4, f, f, None), pf, "shininess"),
             (lambda: L.oi_env_prefilter(f, 0, 4, 8, 10.0, 2, 4, f, f, None), pf, "E=0"),
             (lambda: L.oi_env_prefilter(f, 257, 4, 8, 10.0, 2, 4, f, f, None), pf, "E=257"),
             (lambda: L.oi_env_prefilter(f, 1, 0, 8, 10.0, 2, 4, f, f, None), pf, "He=0"),
             (lambda: L.oi_env_prefilter(f, 1, 4, 0, 10.0, 2, 4, f, f, None), pf, "We=0"),
             (lambda: L.oi_env_prefilter(f, 1, 4, 8, 10.0, 0, 4, f, f, None), pf, "Hp=0"),
             (lambda: L.oi_env_prefilter(f, 1, 4, 8, 10.0, 2, 0, f, f, None), pf, "Wp=0"),
             (lambda: L.oi_env_prefilter(f, 2, 1 << 15, 1 << 15, 10.0, 2, 4, f, f, None), pf, "2^31"),
             (lambda: L.oi_env_prefilter(f, 1, 4, 8, 10.0, 1 << 15, 1 << 15, f, f, None), pf, "2^31"),
             (lambda: L.oi_env_prefilter(f, 5, 2048, 4096, 10.0, 256, 512, f, f, None), pf, "at most 2^23"),
             (lambda: L.oi_env_prefilter(None, 1, 4, 8, 10.0, 2, 4, f, f, None), pf, "null pointer"),
             (lambda: L.oi_env_prefilter(f, 1, 4, 8, 10.0, 2, 4, None, f, None), pf, "null pointer"),
             (lambda: L.oi_env_prefilter(f, 1, 4, 8, 10.0, 2, 4, f, None, None), pf, "null pointer"),
             (lambda: L.oi_occlusion_lobe_begin(None, f, f, f, f, 4, 3, 10.0, 0.01, 0, None), lb, "null state"),
             (lambda: L.oi_occlusion_lobe_begin(state(N=0), f, f, f, f, 4, 3, 10.0, 0.01, 0, None), lb, "N=0"),
             (lambda: L.oi_occlusion_lobe_begin(state(status=None), f, f, f, f, 4, 3, 10.0, 0.01, 0, None), lb, "null pointer in the state"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, f, f, 4, 0, 10.0, 0.01, 0, None), lb, "S=0"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, f, f, 4, 257, 10.0, 0.01, 0, None), lb, "S=257"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, f, f, 5, 3, 10.0, 0.01, 0, None), lb, "n_hit=5"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, f, f, 0, 3, 10.0, 0.01, 0, None), lb, "n_hit=0"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, f, f, 4, 3, 0.5, 0.01, 0, None), lb, "shininess"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, f, f, 4, 3, nan, 0.01, 0, None), lb, "shininess"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, f, f, 4, 3, 5000.0, 0.01, 0, None), lb, "shininess"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, f, f, 4, 3, 10.0, -1.0, 0, None), lb, "bias"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, f, f, 4, 3, 10.0, inf, 0, None), lb, "bias"),
             (lambda: L.oi_occlusion_lobe_begin(state(), None, f, f, f, 4, 3, 10.0, 0.01, 0, None), lb, "null input"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, None, f, f, 4, 3, 10.0, 0.01, 0, None), lb, "null input"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, None, f, 4, 3, 10.0, 0.01, 0, None), lb, "null input"),
             (lambda: L.oi_occlusion_lobe_begin(state(), f, f, f, None, 4, 3, 10.0, 0.01, 0, None), lb, "null input"),
             (lambda: L.oi_env_shade_glossy(None, f, f, f, f, f, f, 1, 2, 4, (ctypes.c_int * 1)(0), f, f, f, None), sh, "null params"),
             (lambda: shade(N=0, n_hit=0), sh, "N=0"),
             (lambda: shade(n_hit=6), sh, "n_hit=6"),
             (lambda: shade(F=0), sh, "F=0"),
             (lambda: shade(F=257), sh, "F=257"),
             (lambda: shade(M=0), sh, "M=0"),
             (lambda: shade(M=257), sh, "M=257"),
             (lambda: shade(Hp=0), sh, "Hp=0"),
             (lambda: shade(Wp=0), sh, "Wp=0"),
             (lambda: shade(M=256, Hp=1 << 12, Wp=1 << 12), sh, "2^31"),
             (lambda: shade(status=None), sh, "null input"),
             (lambda: shade(hit_slot=None), sh, "null input"),
             (lambda: shade(transfer=None), sh, "null input"),
             (lambda: shade(envs=None), sh, "null input"),
             (lambda: shade(args=dict(rays_o=None)), sh, "null glossy input"),
             (lambda: shade(args=dict(w2b=None)), sh, "null glossy input"),
             (lambda: shade(args=dict(glossy=None)), sh, "null glossy input"),
             (lambda: shade(args=dict(rot=None)), sh, "null glossy input"),
             (lambda: shade(args=dict(k_s=None)), sh, "null glossy input"),
             (lambda: shade(index=None, F=1), sh, "null glossy input"),
             (lambda: shade(args=dict(hit_points=None)), sh, "null hit arrays"),
             (lambda: shade(args=dict(grad=None)), sh, "null hit arrays"),
             (lambda: shade(shading=None, image=None, spec=None), sh, "no output"),
             (lambda: shade(rgb=None), sh, "null rgb"),
             (lambda: shade(index=(1,)), sh, "map_index[0]=1"),
             (lambda: shade(index=(0, -1), M=2), sh, "map_index[1]=-1"),
             (lambda: shade(index=(0, 1, 2), M=2), sh, "map_index[2]=2")]
    for call, entry, text in cases:
        rc = call()
        msg = L.oi_last_error().decode()
        assert rc < 0, (entry, text)
        assert msg.startswith(entry + ":") and text in msg, (entry, text, msg)
