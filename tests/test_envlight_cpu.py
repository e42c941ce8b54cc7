"""CPU checks of environment lighting (include/oi_envlight.h): the properties of the fp64 restatement
(tests/helpers/env_ref.py) that hold exactly or by derivation -- the furnace, the closed form against the Monte-Carlo
estimator, the SH rotation, directional lights as an environment -- the same properties of oi_amd.envlight's host code, the
argument refusals that need no GPU, and header <=> library <=> binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import cabi
from helpers import env_ref as E
from helpers import mesh_attr_ref as A
from helpers import trace_ref as T

NAMES = ["oi_env_project", "oi_env_project_partial_floats", "oi_env_shade", "oi_transfer_normal", "oi_transfer_resolve"]

# at least 8 normals, +z and -z among them: the tangent frame of the sample directions switches sign between the two
NORMALS = A.unit(np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.3, -0.5, 0.81], [-0.7, 0.2, -0.68],
                           [0.57, 0.58, 0.58], [-0.2, -0.9, 1e-3], [0.1, 0.05, -0.99]]))


_lib = cabi.built_lib


def test_furnace():
    from oi_amd.envlight import EnvLight
    env = EnvLight.constant(1.0)
    assert env.coeffs.shape == (9, 3) and np.abs(env.coeffs[0] - 2.0 * np.sqrt(np.pi)).max() < 1e-15 and not env.coeffs[1:].any()
    for He, We in ((1, 1), (5, 7), (33, 65)):
        _, w = E.equirect(He, We)
        assert abs(w.sum() * We - 4.0 * np.pi) < 1e-12
    # a constant map projects to the constant environment (bands 1, 2 integrate to zero up to the quadrature in phi / theta)
    c, _ = E.project(np.ones((1, 3, 64, 128)))
    assert np.abs(c[0, 0] - 2.0 * np.sqrt(np.pi)).max() < 1e-12 and np.abs(c[0, 1:]).max() < 1e-3
    # any all-escaped ray set: T_0 = y_0 exactly, so the shading under constant(1) is 1
    rs = np.random.RandomState(0)
    n_hit, S = 7, 5
    d = A.unit(rs.randn(S * n_hit, 3))
    t = E.transfer(np.full(S * n_hit, T.MISS), d, np.arange(n_hit), n_hit, S, np.eye(4))
    sh, img, _ = E.shade(t, env.coeffs[None], np.ones(n_hit, bool), np.full((n_hit, 3), 0.5))
    assert np.abs(sh - 1.0).max() < 1e-12 and np.abs(img - 0.5).max() < 1e-12
    # and with some rays occluded it is the escaped share
    status = rs.randint(0, 6, S * n_hit)
    t = E.transfer(status, d, np.arange(n_hit), n_hit, S, np.eye(4))
    sh, _, _ = E.shade(t, env.coeffs[None], np.ones(n_hit, bool), np.ones((n_hit, 3)))
    assert np.abs(sh[0, 0] - (status.reshape(S, n_hit) == T.MISS).mean(0)).max() < 1e-12


def test_closed_form_against_the_estimator():
    """Mean over 1024 slots (distinct pixels) of the S = 256 estimator, every ray escaped, against A_band y_c(n): the standard
    error is <= 0.5 / sqrt(256 * 1024) = 1e-3, the bar 5 sigma = 5e-3; a wrong band constant moves a coefficient by >= 0.08."""
    assert len(NORMALS) >= 8
    pix = np.arange(1024) * 7 + 3
    assert len(set(pix.tolist())) == 1024
    worst = 0.0
    for n in NORMALS:
        est = E.estimate_all_escaped(np.broadcast_to(n, (1024, 3)), pix, 256, seed=11).mean(0)
        err = np.abs(est - E.closed_form(n))
        worst = max(worst, float(err.max()))
        assert err.max() < 5e-3, (n, err)
    print("closed form against the estimator: worst", worst)
    # the check discriminates: the band constants are far apart on this scale
    assert abs(2.0 / 3.0 - 1.0) * E.Y_MAX_BAND1 > 0.08


@pytest.mark.parametrize("rotation", ["restatement", "library"])
def test_rotation(rotation):
    from oi_amd import envlight
    rot = E.rotation if rotation == "restatement" else envlight.sh_rotation
    rs = np.random.RandomState(3)
    R1, R2 = E.random_rotation(rs), E.axis_rotation((0.3, -0.2, 0.9), 1.1)
    M1, M2 = rot(R1), rot(R2)
    assert np.abs(M1 @ M1.T - np.eye(9)).max() < 1e-10 and np.abs(M2.T @ M2 - np.eye(9)).max() < 1e-10
    assert np.abs(rot(R1 @ R2) - M1 @ M2).max() < 1e-10
    assert np.abs(rot(np.eye(3)) - np.eye(9)).max() < 1e-10
    off = np.ones((9, 9), bool)
    for a, b in ((0, 1), (1, 4), (4, 9)):
        off[a:b, a:b] = False
    assert np.abs(M1[off]).max() < 1e-10                                       # block-diagonal: a band maps onto itself
    coeffs = rs.randn(9, 3)
    d = A.unit(rs.randn(50, 3))
    assert np.abs(E.basis(d) @ (M1 @ coeffs) - E.basis(d @ R1) @ coeffs).max() < 1e-10   # f'(d) = f(R^T d)
    assert np.abs(envlight.sh_rotation(R1) - E.rotation(R1)).max() < 1e-10
    env = envlight.EnvLight(coeffs)
    assert np.abs(env.rotated(R1).coeffs - M1 @ coeffs).max() < 1e-10
    assert np.abs(env.rotated(R1).radiance(d) - env.radiance(d @ R1)).max() < 1e-10
    assert np.abs(envlight.sh_basis(d) - E.basis(d)).max() < 1e-15
    with pytest.raises(ValueError, match="rotation"):
        envlight.sh_rotation(np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError, match="rotation"):
        envlight.sh_rotation(2.0 * np.eye(3))


def test_from_lights():
    """A unit white diffuse light under the closed-form transfer is relu(n . l) up to the band-2 truncation
    1/4 + cos / 2 + (5 / 16) (3 cos^2 - 1) / 2, whose largest error is 0.094 (at cos = 0): the bar is 0.1."""
    from oi_amd.envlight import EnvLight, stack_envs
    from oi_amd.relight import Light
    cos = np.linspace(-1, 1, 2001)
    trunc = 0.25 + cos / 2 + (5.0 / 16.0) * (3 * cos * cos - 1) / 2
    worst = np.abs(trunc - np.maximum(cos, 0)).max()
    assert 0.09 < worst < 0.095 and abs(cos[np.abs(trunc - np.maximum(cos, 0)).argmax()]) < 1e-9
    rs = np.random.RandomState(5)
    l = np.array([0.4, -0.3, 0.85])
    env = EnvLight.from_lights([Light(direction=tuple(3.0 * l), ambient=0.0, diffuse=1.0, specular=0.7)])   # specular: dropped
    n = A.unit(rs.randn(1000, 3))
    sh = E.closed_form(n) @ env.coeffs
    cosnl = n @ (l / np.linalg.norm(l))
    assert np.abs(sh - np.maximum(cosnl, 0)[:, None]).max() < 0.1
    assert np.abs(sh[:, 0] - (0.25 + cosnl / 2 + (5.0 / 16.0) * (3 * cosnl ** 2 - 1) / 2)).max() < 1e-12
    # the ambient term is a constant environment; lights add
    amb = EnvLight.from_lights([Light(direction=(0, 0, 1), ambient=(0.1, 0.2, 0.3), diffuse=0.0)])
    assert np.abs(amb.coeffs - EnvLight.constant((0.1, 0.2, 0.3)).coeffs).max() < 1e-15
    two = EnvLight.from_lights([Light(direction=tuple(l), ambient=0.0, diffuse=1.0), Light(direction=(0, 0, 1), ambient=(0.1, 0.2, 0.3), diffuse=0.0)])
    assert np.abs(two.coeffs - env.coeffs - amb.coeffs).max() < 1e-15
    st = stack_envs([env, amb], "cpu")
    assert st.shape == (2, 9, 3) and st.dtype == torch.float32
    with pytest.raises(TypeError):
        stack_envs([env, "x"], "cpu")
    with pytest.raises(ValueError):
        stack_envs([], "cpu")


def test_cap_integral_of_the_analytic_scene():
    """The quadrature of the helper against the closed forms, and the size of the effect the GPU test measures."""
    a = E.analytic_cap_angle()
    cap = E.cap_transfer(a)
    k0, k1 = 0.5 / np.sqrt(np.pi), E.Y_MAX_BAND1
    assert abs(cap[0] - k0 * np.sin(a) ** 2) < 1e-9                             # cosine-weighted share of the cap
    assert abs(cap[2] - k1 * (2.0 / 3.0) * (1 - np.cos(a) ** 3)) < 1e-9
    assert not cap[[1, 3, 4, 5, 7, 8]].any()
    assert np.abs(E.cap_transfer(np.pi / 2) - E.closed_form(np.array([0.0, 0.0, 1.0]))).max() < 1e-9   # the whole hemisphere
    # the cap removes >= 0.3 |y|max of the +axis lobe, twice the 0.16 |y|max bar of the S = 256 estimator
    assert cap[2] >= 0.3 * k1 and 5 * 0.5 / np.sqrt(256) < 0.16
    assert E.C1[2] + E.R1 < 1.0 and E.C1[2] - E.R1 - E.R0 > 5 * T.BIAS         # inside the unit ball, clear of the lower sphere


def test_argument_checks():
    from oi_amd import envlight, trace
    for bad in (-1, 257, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match="transfer_samples"):
            trace.capture_transfer(None, None, None, transfer_samples=bad)
        with pytest.raises(ValueError, match="transfer_samples"):
            trace.render_surface_env(None, None, None, [envlight.EnvLight.constant(1)], transfer_samples=bad)
    with pytest.raises(ValueError, match="seed"):
        trace.capture_transfer(None, None, None, transfer_samples=4, seed=-1)
    assert trace._check_transfer(0, 0, "x") == (0, 0) and trace._check_transfer(np.int64(256), 7, "x") == (256, 7)
    with pytest.raises(ValueError, match="at most 9"):
        envlight.EnvLight(np.zeros((10, 3)))
    with pytest.raises(ValueError):
        envlight.EnvLight(np.zeros((9, 4)))
    with pytest.raises(ValueError, match="finite"):
        envlight.EnvLight(np.full((9, 3), np.nan))
    assert envlight.EnvLight(np.ones((4, 3))).coeffs[4:].sum() == 0             # bands 0 .. 1 are padded
    for shape in ((8, 16), (1, 3, 8, 16), (8, 16, 4)):
        with pytest.raises(ValueError, match="from_equirect"):
            envlight.EnvLight.from_equirect(np.zeros(shape, dtype=np.float32))
    from oi_amd import inference
    with pytest.raises(TypeError, match="EnvLight"):
        inference.env_walk(None, None, None, "sky", 4)
    with pytest.raises(ValueError, match="n_frames"):
        inference.env_walk(None, None, None, envlight.EnvLight.constant(1), 0)
    rots = inference.env_walk_rotations(4, (0, 0, 2.0))
    assert np.array_equal(rots[0], np.eye(3)) and np.abs(rots[1] - E.axis_rotation((0, 0, 1), np.pi / 2)).max() < 1e-15


def test_header_library_and_binding_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_envlight.h", lib)
    assert sorted(names) == NAMES and mirrors == ["EnvShadeParams"]
    text = cabi.read("oi_envlight.h")
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert define("OI_ENV_FLOATS") == lib.ENV_FLOATS == 27 and define("OI_ENV_COEFFS") == lib.ENV_COEFFS == E.N_COEFFS == 9
    assert define("OI_ENV_MAX_ENVS") == lib.ENV_MAX_ENVS == E.MAX_ENVS == 256
    assert '"envlight.hip"' in open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    # the basis constants of the header are the rounded values of the restatement's
    k =[float(v) for v in re.findall(r"\*   y\d = (\d\.\d+)", text)]
    d = A.unit(np.array([[0.3, -0.5, 0.81]]))
    x, y, z = d[0]
    assert len(k) == 9
    mine = np.array([k[0], k[1] * y, k[2] * z, k[3] * x, k[4] * x * y, k[5] * y * z, k[6] * (3 * z * z - 1), k[7] * x * z, k[8] * (x * x - y * y)])
    assert np.abs(mine - E.basis(d)[0]).max() < 1e-8
    # the size of the partial buffer
    assert L.oi_env_project_partial_floats(1, 1, 1) == 27 and L.oi_env_project_partial_floats(3, 33, 65) == 81
    assert L.oi_env_project_partial_floats(2, 128, 64) == 54 and L.oi_env_project_partial_floats(2, 128, 65) == 2 * 2 * 27
    assert L.oi_env_project_partial_floats(0, 4, 4) == 0 and L.oi_env_project_partial_floats(257, 4, 4) == 0
    assert L.oi_env_project_partial_floats(2, 1 << 15, 1 << 15) == 0


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)

    def shade(**kw):
        P = lib.EnvShadeParams()
        P.N, P.n_hit, P.F = kw.pop("N", 5), kw.pop("n_hit", 2), kw.pop("F", 1)
        for n, _ in lib.EnvShadeParams._fields_[3:]:
            setattr(P, n, kw.get(n, f))
        return L.oi_env_shade(ctypes.byref(P), None)

    pj, rs, nm, sh = "oi_env_project", "oi_transfer_resolve", "oi_transfer_normal", "oi_env_shade"
    cases = [(lambda: L.oi_env_project(f, 0, 4, 8, f, f, None), pj, "E=0"),
             (lambda: L.oi_env_project(f, 257, 4, 8, f, f, None), pj, "E=257"),
             (lambda: L.oi_env_project(f, 1, 0, 8, f, f, None), pj, "He=0"),
             (lambda: L.oi_env_project(f, 1, 4, 0, f, f, None), pj, "We=0"),
             (lambda: L.oi_env_project(f, 2, 1 << 15, 1 << 15, f, f, None), pj, "2^31"),
             (lambda: L.oi_env_project(None, 1, 4, 8, f, f, None), pj, "null pointer"),
             (lambda: L.oi_env_project(f, 1, 4, 8, None, f, None), pj, "null pointer"),
             (lambda: L.oi_env_project(f, 1, 4, 8, f, None, None), pj, "null pointer"),
             (lambda: L.oi_transfer_resolve(f, f, f, 0, 0, 4, f, f, None), rs, "N=0"),
             (lambda: L.oi_transfer_resolve(f, f, f, 1 << 31, 1, 4, f, f, None), rs, "N=2147483648"),
             (lambda: L.oi_transfer_resolve(f, f, f, 5, 6, 4, f, f, None), rs, "n_hit=6"),
             (lambda: L.oi_transfer_resolve(f, f, f, 5, -1, 4, f, f, None), rs, "n_hit=-1"),
             (lambda: L.oi_transfer_resolve(f, f, f, 5, 2, 0, f, f, None), rs, "S=0"),
             (lambda: L.oi_transfer_resolve(f, f, f, 5, 2, 257, f, f, None), rs, "S=257"),
             (lambda: L.oi_transfer_resolve(f, f, f, 1 << 30, 1 << 29, 8, f, f, None), rs, "below 2^31"),
             (lambda: L.oi_transfer_resolve(None, f, f, 5, 2, 4, f, f, None), rs, "null pointer"),
             (lambda: L.oi_transfer_resolve(f, None, f, 5, 2, 4, f, f, None), rs, "null pointer"),
             (lambda: L.oi_transfer_resolve(f, f, None, 5, 2, 4, f, f, None), rs, "null pointer"),
             (lambda: L.oi_transfer_resolve(f, f, f, 5, 2, 4, None, f, None), rs, "null pointer"),
             (lambda: L.oi_transfer_resolve(f, f, f, 5, 2, 4, f, None, None), rs, "null pointer"),
             (lambda: L.oi_transfer_normal(f, f, 0, 0, f, f, None), nm, "N=0"),
             (lambda: L.oi_transfer_normal(f, f, 5, 6, f, f, None), nm, "n_hit=6"),
             (lambda: L.oi_transfer_normal(None, f, 5, 2, f, f, None), nm, "null pointer"),
             (lambda: L.oi_transfer_normal(f, None, 5, 2, f, f, None), nm, "null pointer"),
             (lambda: L.oi_transfer_normal(f, f, 5, 2, None, f, None), nm, "null pointer"),
             (lambda: L.oi_transfer_normal(f, f, 5, 2, f, None, None), nm, "null pointer"),
             (lambda: L.oi_env_shade(None, None), sh, "null params"),
             (lambda: shade(N=0, n_hit=0), sh, "N=0"),
             (lambda: shade(n_hit=6), sh, "n_hit=6"),
             (lambda: shade(F=0), sh, "F=0"),
             (lambda: shade(F=257), sh, "F=257"),
             (lambda: shade(status=None), sh, "null input"),
             (lambda: shade(hit_slot=None), sh, "null input"),
             (lambda: shade(transfer=None), sh, "null input"),
             (lambda: shade(envs=None), sh, "null input"),
             (lambda: shade(shading=None, image=None), sh, "no output"),
             (lambda: shade(rgb=None), sh, "null rgb")]
    for call, entry, text in cases:
        rc = call()
        msg = L.oi_last_error().decode()
        assert rc < 0, (entry, text)
        assert msg.startswith(entry + ":") and text in msg, (entry, text, msg)
