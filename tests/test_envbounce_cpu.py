"""CPU checks of the diffuse interreflection bounce (include/oi_envbounce.h): the properties of the fp64
restatement (tests/helpers/bounce_ref.py) that hold exactly or by derivation -- the furnace, a black albedo, the S = 256
estimator of the analytic two-sphere scene against its quadrature --, header <=> library <=> binding, and the refusals that
need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import bounce_ref as B
from helpers import cabi
from helpers import env_ref as E
from helpers import mesh_attr_ref as A
from helpers import occlusion_ref as R
from helpers import trace_ref as T

NAMES = ["oi_bounce_resolve", "oi_env_shade_bounce"]

_lib = cabi.built_lib


def _ray_set(rs, N, n_hit, S, codes, white=False):
    """Random final states of S * n_hit transfer rays, each HIT with a secondary hit of its own whose normal faces the ray
    (codes: the final states drawn from; HIT rays get front faces), a permuted hit_slot, a rotation."""
    Q = S * n_hit
    status = rs.choice(codes, size=Q).astype(np.uint8)
    hit = status == T.HIT
    n2 = int(hit.sum())
    slot2 = np.full(Q, -1)
    slot2[hit] = rs.permutation(n2)
    d = A.unit(rs.randn(Q, 3))
    nrm = A.unit(rs.randn(n2, 3))
    dn = d[hit][np.argsort(slot2[hit])]                                      # the ray that meets secondary hit k
    nrm = np.where(((nrm * dn).sum(-1) < 0)[:, None], nrm, -nrm)            # a front face
    grad2 = nrm * rs.uniform(0.3, 3.0, (n2, 1))
    rgb2 = np.ones((n2, 3)) if white else rs.rand(n2, 3)
    slot = np.full(N, -1)
    slot[rs.permutation(N)[:n_hit]] = np.arange(n_hit)
    w2b = np.eye(4)
    w2b[:3, :3] = E.random_rotation(rs)
    return status, d, slot2, grad2, rgb2, slot, w2b


def test_furnace():
    """rho = 1 under the constant environment: direct + indirect is 1 for every pixel whose rays all end MISS or on a front
    face (A_0 y_0 2 sqrt(pi) = 1, and every other coefficient of the environment is 0)."""
    from oi_amd.envlight import EnvLight
    env = EnvLight.constant(1).coeffs[None]
    for seed, (N, n_hit, S) in enumerate([(7, 5, 1), (40, 33, 16), (65, 65, 256)]):
        rs = np.random.RandomState(seed)
        status, d, slot2, grad2, rgb2, slot, w2b = _ray_set(rs, N, n_hit, S, [T.MISS, T.HIT], white=True)
        t0 = E.transfer(status, d, slot, n_hit, S, w2b)
        t1, _, _, front = B.resolve(status, d, slot2, grad2, rgb2, slot, n_hit, S, w2b)
        assert front.sum() == (status == T.HIT).sum() > 0
        sh, ind, _, _ = B.shade(t0, t1, env, slot >= 0, np.ones((N, 3)))
        on = slot >= 0
        assert np.abs(sh[0][:, on] - 1.0).max() <= 1e-12
        assert ind[0][:, on].max() > 0.2 and not sh[0][:, ~on].any()
        # the share that comes by way of the object is the share of rays that hit it
        share = (status.reshape(S, n_hit) == T.HIT).mean(0)
        assert np.abs(ind[0, 0, on] - share[slot[on]]).max() <= 1e-12
    # a ray that ends any other way, or on a back face, bounces nothing: the sum falls short of 1
    rs = np.random.RandomState(9)
    status, d, slot2, grad2, rgb2, slot, w2b = _ray_set(rs, 30, 30, 64, [T.MISS, T.HIT, T.LIMIT, T.START_INSIDE, T.NONFINITE,
                                                                           T.BACKFACING], white=True)
    grad2[::2] *= -1.0                                                       # every other hit is a back face
    t0 = E.transfer(status, d, slot, 30, 64, w2b)
    t1, _, nd, front = B.resolve(status, d, slot2, grad2, rgb2, slot, 30, 64, w2b)
    sh, _, _, _ = B.shade(t0, t1, env, slot >= 0, np.ones((30, 3)))
    ok = (status == T.MISS).reshape(64, 30) | front
    assert 0 < front.sum() < (status == T.HIT).sum() and (nd[(status == T.HIT).reshape(64, 30) & ~front] > 0).all()
    assert np.abs(sh[0, 0, slot >= 0] - ok.mean(0)[slot[slot >= 0]]).max() <= 1e-12 and sh.max() < 1.0


def test_black_albedo_is_the_direct_shade():
    rs = np.random.RandomState(3)
    N, n_hit, S = 50, 41, 16
    status, d, slot2, grad2, rgb2, slot, w2b = _ray_set(rs, N, n_hit, S, [T.MISS, T.HIT, T.LIMIT])
    t0 = E.transfer(status, d, slot, n_hit, S, w2b)
    t1, mag, _, _ = B.resolve(status, d, slot2, grad2, np.zeros_like(rgb2), slot, n_hit, S, w2b)
    assert not t1.any() and not mag.any()
    envs, alb, bg = rs.randn(4, 9, 3), rs.rand(N, 3), np.array([0.1, 0.2, 0.3])
    sh, ind, img, _ = B.shade(t0, t1, envs, slot >= 0, alb, bg)
    sh0, img0, _ = E.shade(t0, envs, slot >= 0, alb, bg)
    assert np.array_equal(sh, sh0) and np.array_equal(img, img0) and not ind.any()
    # and without secondary hits at all (grad2 / rgb2 absent)
    t1, _, _, _ = B.resolve(status, d, slot2, None, None, slot, n_hit, S, w2b)
    assert t1.shape == (3, 9, N) and not t1.any()


def test_estimator_against_the_quadrature():
    """The point on top of the lower sphere of env_ref's scene, under the upper one: the S = 256 estimator (the kernel's sample
    directions, analytic intersections and normals) against the quadrature of the same integral.  Bar: 5 standard errors from
    the per-sample bound 0.5 rho A_band |y_c|max.  Only c = 0, 2, 6 are non-zero in the quadrature; the others are held to the
    same bar about 0."""
    S, rho = 256, np.array([0.9, 0.5, 0.1])
    quad = B.top_quadrature()
    alpha = E.analytic_cap_angle()
    k0 = 0.5 / np.sqrt(np.pi)
    assert abs(quad[0] - k0 * np.sin(alpha) ** 2) <= 1e-9                    # c = 0: y_0 times the share of the cap
    assert not quad[[1, 3, 4, 5, 7, 8]].any() and quad[2] < 0                # the blocker's underside faces down: n_z < 0
    assert abs(quad[6]) > 0.01
    est, share = B.top_estimator(S, R.SEED, np.array([11, 4, 300, 77, 5000]), rho)
    assert abs(share - np.sin(alpha) ** 2) < 0.02
    worst = 0.0
    for ch in range(3):
        bar = B.standard_error_bar(S, rho[ch])
        err = np.abs(est[ch] - rho[ch] * quad[:, None])                      # (9, pixels)
        worst = max(worst, float((err / bar[:, None]).max()))
        assert (err <= bar[:, None]).all(), (ch, err.max(1), bar)
        assert (bar[[0, 2]] < 0.5 * rho[ch] * np.abs(quad[[0, 2]])).all()    # the bar is well below the effect
    print("bounce estimator against the quadrature: worst error over the bar", worst, "T1 / rho", quad[[0, 2, 6]], "hit share", share)
    # the channels differ by the albedo alone
    assert np.abs(est[0] / rho[0] - est[2] / rho[2]).max() <= 1e-12


def test_header_library_and_binding_agree():
    lib, L = _lib()
    from oi_amd import ops
    names, mirrors = cabi.check_header("oi_envbounce.h", lib)
    # the header's parameter struct: check_header held the mirror against it field by field
    assert sorted(names) == NAMES == lib.symbols("oi_envbounce.h") and mirrors == ["EnvShadeBounceParams"]
    _, structs = cabi.parse(cabi.read("oi_envbounce.h"))
    assert sorted(structs) == ["oi_env_shade_bounce_params"]
    cls = lib.EnvShadeBounceParams
    fields = structs["oi_env_shade_bounce_params"]
    # oi_env_shade_params' fields in its order, then two pointers
    _, base = cabi.parse(cabi.read("oi_envlight.h"))
    assert fields[:len(base["oi_env_shade_params"])] == base["oi_env_shade_params"]
    assert cls._fields_[:len(lib.EnvShadeParams._fields_)] == lib.EnvShadeParams._fields_
    assert [f for f, _ in fields[-2:]] == ["bounce", "indirect"]
    assert ctypes.sizeof(cls) == ctypes.sizeof(lib.EnvShadeParams) + 2 * ctypes.sizeof(ctypes.c_void_p)
    text = cabi.read("oi_envbounce.h")
    assert int(re.search(r"#define OI_BOUNCE_FLOATS (\d+)", text).group(1)) == lib.BOUNCE_FLOATS == 3 * lib.ENV_COEFFS
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"envbounce.hip"' in src and "include/oi_envbounce.h" in src
    # nothing was added to the headers whose entry lists other tests pin
    for header, n in (("oi_envlight.h", 5), ("oi_occlusion.h", 5), ("oi_trace.h", 6)):
        assert len(lib.symbols(header)) == n, header
    assert ops.ENV_BOUNCE_OUT == ("shading", "image", "indirect")


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)
    br, sh = "oi_bounce_resolve", "oi_env_shade_bounce"

    def resolve(N=8, n_hit=4, n_hit2=3, S=2, **kw):
        a = dict(status=f, rays_d=f, hit_slot2=f, grad2=f, rgb2=f, hit_slot=f, w2b=f, bounce=f)
        a.update(kw)
        return L.oi_bounce_resolve(a["status"], a["rays_d"], a["hit_slot2"], a["grad2"], a["rgb2"], a["hit_slot"], N, n_hit, n_hit2,
                                   S, a["w2b"], a["bounce"], None)

    def shade(**kw):
        P = lib.EnvShadeBounceParams()
        P.N, P.n_hit, P.F = kw.pop("N", 5), kw.pop("n_hit", 2), kw.pop("F", 1)
        for n, _ in lib.EnvShadeBounceParams._fields_[3:]:
            setattr(P, n, kw.get(n, f))
        return L.oi_env_shade_bounce(ctypes.byref(P), None)

    cases = [(lambda: resolve(N=0, n_hit=0, n_hit2=0), br, "N=0"),
             (lambda: resolve(N=1 << 31), br, "N=2147483648"),
             (lambda: resolve(n_hit=9), br, "n_hit=9"),
             (lambda: resolve(n_hit=-1), br, "n_hit=-1"),
             (lambda: resolve(S=0), br, "S=0"),
             (lambda: resolve(S=257), br, "S=257"),
             (lambda: resolve(N=(1 << 31) - 1, n_hit=1 << 23, S=256), br, "below 2^31"),
             (lambda: resolve(n_hit2=-1), br, "n_hit2=-1"),
             (lambda: resolve(n_hit2=9), br, "n_hit2=9"),
             (lambda: resolve(hit_slot=None), br, "null pointer"),
             (lambda: resolve(w2b=None), br, "null pointer"),
             (lambda: resolve(bounce=None), br, "null pointer"),
             (lambda: resolve(status=None), br, "null pointer"),
             (lambda: resolve(rays_d=None), br, "null pointer"),
             (lambda: resolve(hit_slot2=None), br, "null pointer"),
             (lambda: resolve(grad2=None), br, "null grad2 / rgb2"),
             (lambda: resolve(rgb2=None), br, "null grad2 / rgb2"),
             (lambda: L.oi_env_shade_bounce(None, None), sh, "null params"),
             (lambda: shade(N=0, n_hit=0), sh, "N=0"),
             (lambda: shade(n_hit=6), sh, "n_hit=6"),
             (lambda: shade(F=0), sh, "F=0"),
             (lambda: shade(F=257), sh, "F=257"),
             (lambda: shade(status=None), sh, "null input"),
             (lambda: shade(hit_slot=None), sh, "null input"),
             (lambda: shade(transfer=None), sh, "null input"),
             (lambda: shade(envs=None), sh, "null input"),
             (lambda: shade(bounce=None), sh, "null bounce"),
             (lambda: shade(shading=None, image=None, indirect=None), sh, "no output"),
             (lambda: shade(rgb=None), sh, "null rgb")]
    for call, entry, text in cases:
        rc = call()
        msg = L.oi_last_error().decode()
        assert rc < 0, (entry, text)
        assert msg.startswith(entry + ":") and text in msg, (entry, text, msg)


def test_host_refusals_need_no_gpu():
    """capture_transfer checks `bounces` before it touches the generator or the device."""
    from oi_amd import inference, ops, trace
    from oi_amd.envlight import EnvLight
    z, b2w = torch.zeros(1, 64), torch.eye(4)
    for bad in (True, False, 2, -1, 1.0, "1", None):
        with pytest.raises(ValueError, match="bounces="):
            trace.capture_transfer(None, z, b2w, bounces=bad)
    with pytest.raises(ValueError, match="transfer_samples=0"):
        trace.capture_transfer(None, z, b2w, transfer_samples=0, bounces=1)
    for kw in (dict(glossy_samples=8), dict(glossy_samples=0, shininess=10.0), dict(shininess=10.0)):
        with pytest.raises(ValueError, match="glossy shade has no bounce input yet"):
            trace.capture_transfer(None, z, b2w, bounces=1, **kw)
    # the bad sample count is still named first, and the keyword passes through the two callers
    with pytest.raises(ValueError, match="transfer_samples="):
        trace.capture_transfer(None, z, b2w, transfer_samples=257, bounces=1)
    with pytest.raises(ValueError, match="bounces="):
        trace.render_surface_env(None, z, b2w, [EnvLight.constant(1)], bounces=2)

    class _Gen:
        class renderer:
            class pack:
                check = staticmethod(lambda: None)
        eval = staticmethod(lambda: None)
    with pytest.raises(ValueError, match="bounces="):
        inference.env_walk(_Gen(), z, b2w, EnvLight.constant(1), n_frames=2, bounces=True)
    # the wrappers check shapes before anything is launched
    zt = torch.zeros
    with pytest.raises(ValueError, match="bounce"):
        ops.env_shade_bounce(zt(4, dtype=torch.uint8), zt(4, dtype=torch.int32), None, 0, zt(9, 4), zt(9, 4), zt(1, 9, 3))
    with pytest.raises(ValueError, match="unknown output"):
        ops.env_shade_bounce(zt(4, dtype=torch.uint8), zt(4, dtype=torch.int32), None, 0, zt(9, 4), zt(3, 9, 4), zt(1, 9, 3),
                             outputs=("specular",))
    # a capture holds its bounce as (1, 3, 9, H, W), or None

    class _S:
        ro = torch.zeros(4, 3)
        N, n_hit, H = 4, 0, 2
    cap = trace.TransferCapture(_S(), torch.zeros(9, 4), {}, 4, bounce=torch.zeros(3, 9, 4))
    assert cap.bounce.shape == (1, 3, 9, 2, 2) and trace.TransferCapture(_S(), torch.zeros(9, 4), {}, 4).bounce is None
