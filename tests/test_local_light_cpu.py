"""CPU-only checks of the local lights (include/oi_local_light.h): the C ABI of the new header, the
invariants of the fp64 restatement (tests/helpers/local_light_ref.py), the directional limit, the rehearsal of the analytic
and golden cases the GPU tests run (tests/test_gpu_local_light.py uses exactly the rehearsed lights), and the host layer's
validation.  No GPU."""
import math

import numpy as np
import pytest

from helpers import cabi
from helpers import local_light_ref as LL
from helpers import occlusion_ref as R
from helpers import trace_ref as T

ENTRIES = ["oi_local_light_begin", "oi_scene_local_light_begin", "oi_scene_shade_local", "oi_surface_shade_local"]


def test_header_declares_four_entries_and_no_struct():
    lib, L = cabi.built_lib()
    names, mirrors = cabi.check_header("oi_local_light.h", lib)
    assert sorted(names) == ENTRIES and mirrors == []
    for n in ENTRIES:
        assert hasattr(L, n)
    assert "struct" not in cabi.read("oi_local_light.h").split("#ifndef OI_LOCAL_LIGHT_H_")[1]
    assert lib.LOCAL_LIGHT_FLOATS == LL.FLOATS == 20 and lib.LOCAL_LIGHT_MIN_DISTANCE == LL.MIN_DISTANCE
    assert "#define OI_LOCAL_LIGHT_FLOATS 20" in cabi.read("oi_local_light.h")
    assert "#define OI_LOCAL_LIGHT_MIN_DISTANCE 1e-3f" in cabi.read("oi_local_light.h")


def _cloud(n=200, seed=3):
    rs = np.random.RandomState(seed)
    nrm = rs.randn(n, 3)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    return nrm * 0.5, nrm, np.arange(n) * 7 + 1


@pytest.mark.parametrize("S", [1, 4, 64])
def test_restatement_invariants(S):
    p, nrm, pix = _cloud()
    q = np.array([0.3, -0.2, 1.1])
    # a point light: the direction is the axis itself and the ray ends at the centre
    a = LL.aimed(p, nrm, pix, q, 0.0, S, R.SEED)
    assert np.array_equal(a["d"], np.broadcast_to(a["axis"], a["d"].shape)) and np.array_equal(a["t_light"], np.broadcast_to(a["dc"], (S, len(p))))
    for radius in (0.05, 0.3):
        a = LL.aimed(p, nrm, pix, q, radius, S, R.SEED)
        assert not a["inside"].any()
        end = p[None] + a["t_light"][..., None] * a["d"]
        assert np.abs(np.linalg.norm(end - q, axis=-1) - radius).max() < 1e-12      # the ray ends ON the sphere
        assert np.abs(np.linalg.norm(a["d"], axis=-1) - 1).max() < 1e-12
        cos_to_axis = (a["d"] * a["axis"][None]).sum(-1)
        assert (cos_to_axis >= a["cos_max"][None] - 1e-12).all()                    # inside the cone the sphere subtends
        assert np.abs(cos_to_axis - a["ca"]).max() < 1e-12
        # the strata are midpoints, so the mean of ca over them is the cone's mean exactly: up to the S roundings of the sum
        assert np.abs(a["ca"].mean(0) - (1 + a["cos_max"]) / 2).max() <= (S + 2) * 2.0 ** -53
    # an origin inside the light
    a = LL.rays(p, nrm, pix, LL.record((0.0, 0.0, 0.0), 0.6), np.eye(4), S, R.SEED)
    assert a["inside"].all() and (a["status"] == LL.MISS).all() and not a["far"].any() and not a["d"].any()


def test_directional_limit_shrinks_as_one_over_distance():
    from oi_amd.relight import Light, LocalLight
    p, n = R.analytic_patch()
    rs = np.random.RandomState(5)
    rgb = rs.rand(len(p), 3)
    eye = np.array([0.4, -0.3, 3.0])
    rd = (p - eye) / np.linalg.norm(p - eye, axis=-1, keepdims=True)
    t = np.linalg.norm(p - eye, axis=-1)
    ro = np.tile(eye, (len(p), 1))
    w2b = np.eye(4)
    light = Light(direction=(0.3, -0.5, 0.8), ambient=(0.2, 0.3, 0.25), diffuse=(0.7, 0.5, 0.6), specular=(0.3, 0.3, 0.2), shininess=6.0)
    ref = T.shade(ro, rd, t, n * 1.5, rgb, w2b, [light.packed()])
    dev = []
    for D in (1e2, 1e3):
        ll = LocalLight.from_light(light, D)
        assert ll.reference_distance == D and abs(np.linalg.norm(ll.position) - D) < 1e-9
        img = LL.shade(ro, p, n * 1.5, rgb, w2b, [ll.packed()])
        dev.append(float(np.abs(img - ref).max()))
        assert dev[-1] <= 3.0 / D * max(light.diffuse + light.specular)            # |p| <= 1: direction and att each within ~1 / D
    print("directional limit: deviation at D = 1e2, 1e3:", dev)
    assert 5.0 < dev[0] / dev[1] < 20.0                                            # ~ 1 / D


def test_analytic_rehearsal_point_light_below_the_occluder():
    """The ray stops at the light: a point light at z = 0.65 stands below the occluder (z in 0.7 .. 0.9), every point of the
    patch faces it and every one is lit; the directional light along +z has an umbra under the occluder."""
    r = LL.analytic_case("below")
    assert r["traced"].all() and r["band"].mean() <= R.EXCLUDED_CAP
    assert r["lit"].all() and (r["vis"] == 1).all()
    assert float((r["o"] + r["far"][..., None] * r["d"])[..., 2].max()) <= 0.65 + 1e-12 < R.C1[2] - R.R1   # every ray ends below the occluder
    o, d, far, traced = R.light_rays(r["points"], r["grad"], r["pix"], np.array(R.ANALYTIC_AXIS), 0.0, 1, R.SEED, bias=LL.ANALYTIC_BIAS)
    hit, _ = LL.sphere_hit(o, d, far, R.C1, R.R1)
    assert traced.all() and hit[0][r["r_xy"] < 0.03].all() and (r["r_xy"] < 0.03).sum() >= 4


def test_analytic_rehearsal_point_light_above_the_occluder():
    """A diverging shadow, wider than the occluder."""
    r = LL.analytic_case("above")
    assert r["traced"].all() and not r["band"].any()
    umbra, lit = r["vis"] == 0, r["vis"] == 1
    print("point light above: umbra", int(umbra.sum()), "r_xy <=", r["r_xy"][umbra].max(), "lit", int(lit.sum()), "r_xy >=", r["r_xy"][lit].min())
    assert int(umbra.sum()) == 148 and int(lit.sum()) == 108
    assert r["r_xy"][umbra].max() <= 0.178 and round(float(r["r_xy"][lit].min()), 3) >= 0.186     # (0.1857: the grid's next ring)
    assert r["r_xy"][umbra].max() > R.R1                                           # wider than the occluder


def test_analytic_rehearsal_sphere_light_penumbra():
    """A light of finite size: an umbra under the occluder, a penumbra over most of the patch.  With this restatement's sampler
    (pix = 3 i + 5, seed 7): 58 points in the umbra (r_xy <= 0.115), 77 % in the penumbra, 0.23 % of the rays in the tangency
    band.  An earlier count with other sample keys had 63 points in the umbra, out to r_xy = 0.121: the grid rings at
    r_xy = 0.115 and 0.121 see a sliver of the light, which 64 samples find at some points and miss at others, depending on
    the keys.  What is asserted holds for any keys: the umbra lies inside 0.121 and holds every grid point within 0.11 of the
    axis (52 of them)."""
    r = LL.analytic_case("sphere")
    umbra, pen = r["vis"] == 0, (r["vis"] > 0) & (r["vis"] < 1)
    print("sphere light: umbra", int(umbra.sum()), "r_xy <=", r["r_xy"][umbra].max(), "penumbra share", pen.mean(), "band share",
          r["band"].mean())
    assert r["traced"].all()
    assert r["r_xy"][umbra].max() <= 0.121 and (r["vis"][r["r_xy"] < 0.11] == 0).all() and int(umbra.sum()) >= 52
    assert pen.mean() >= 0.5 and r["band"].mean() <= R.EXCLUDED_CAP


@pytest.mark.parametrize("seed,pose", R.SOFT_VIEWS)
def test_golden_rehearsal_on_the_oracle(seed, pose):
    """The two golden lights on the oracle's own field: few rays at the step limit, none starting inside the surface, lit rays
    and rays facing away both present.  (The golden objects throw no shadow on themselves from these positions: occlusion
    by an occluder is pinned by the analytic cases.)"""
    out = LL.rehearse_golden(seed, pose)
    print("local light rehearsal", seed, pose, out)
    assert out["n_hit"] > 50
    lights = LL.golden_records(pose)
    w2b = T.view_rays(pose, R.R_SOFT)[4]
    box = [LL.in_frame(lt, w2b)[0] for lt in lights]
    assert np.linalg.norm(box[0]) < 1 and lights[0][3] == 0 and np.linalg.norm(box[1]) > 1 and lights[1][3] > 0
    for i in range(2):
        c = out[f"light{i}"]
        assert c["start_inside"] == 0 and c["inside"] == 0
        assert c["limit"] <= R.REHEARSAL_LIMIT_CAP * max(c["traced"], 1)
        assert c["lit"] > 0 and 0.1 * c["of"] < c["traced"] < c["of"]


def test_host_validation():
    from oi_amd import inference, lib
    from oi_amd.relight import Light, LocalLight, local_lights_given, stack_local_lights
    ok = dict(position=(0.1, 0.2, 0.3), ambient=0.1, diffuse=(0.5, 0.6, 0.7), specular=0.2, shininess=8.0)
    ll = LocalLight(**ok, radius=0.05, reference_distance=2.0, cone_axis=(0, 0, -2.0), cone_inner=0.2, cone_outer=0.5)
    pk = ll.packed()
    assert len(pk) == lib.LOCAL_LIGHT_FLOATS
    assert pk[:4] == [0.1, 0.2, 0.3, 0.05] and pk[4:8] == [0.1, 0.1, 0.1, 2.0] and pk[8:11] == [0.5, 0.6, 0.7]
    assert pk[11] == math.cos(0.5) and pk[12:16] == [0.2, 0.2, 0.2, 8.0] and pk[16:19] == [0.0, 0.0, -2.0] and pk[19] == math.cos(0.2)
    plain = LocalLight(**ok).packed()
    assert plain[11] <= -1 and plain[3] == 0 and plain[7] == 1.0
    assert np.allclose(pk, LL.record(ok["position"], 0.05, (0.1,) * 3, ok["diffuse"], (0.2,) * 3, 8.0, 2.0, (0, 0, -2.0), 0.2, 0.5))
    assert ll.replace(radius=0.0).radius == 0.0 and ll.replace(diffuse=0.3).diffuse == (0.3, 0.3, 0.3)
    assert LocalLight(**ok, cone_axis=(1, 0, 0), cone_inner=1.0, cone_outer=math.pi).packed()[11] > -1     # the widest cone is still one
    bad = [dict(position=(0, float("nan"), 0)), dict(radius=-0.1), dict(radius=float("inf")), dict(reference_distance=0.0),
           dict(reference_distance=-1.0), dict(shininess=float("inf")), dict(diffuse=(0, float("nan"), 0)),
           dict(cone_inner=0.2, cone_outer=0.5), dict(cone_axis=(0, 0, 1)), dict(cone_axis=(0, 0, 1), cone_inner=0.2),
           dict(cone_axis=(0, 0, 0), cone_inner=0.2, cone_outer=0.5), dict(cone_axis=(0, 0, 1), cone_inner=0.5, cone_outer=0.5),
           dict(cone_axis=(0, 0, 1), cone_inner=0.0, cone_outer=0.5), dict(cone_axis=(0, 0, 1), cone_inner=0.5, cone_outer=3.2),
           dict(cone_axis=(0, 0, 1), cone_inner=0.6, cone_outer=0.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            LocalLight(**{**ok, **kw})
    d = Light(direction=(0, 0, 2.0))
    fl = LocalLight.from_light(d, 5.0, centre=(1.0, 0.0, 0.0))
    assert fl.position == (1.0, 0.0, 5.0) and fl.reference_distance == 5.0 and fl.diffuse == d.diffuse and fl.shininess == d.shininess
    assert local_lights_given([ll, fl]) and not local_lights_given([d]) and not local_lights_given(None) and local_lights_given(ll)
    with pytest.raises(ValueError, match="one list"):
        local_lights_given([ll, d])
    with pytest.raises(TypeError):
        stack_local_lights([d], "cpu")
    assert stack_local_lights([ll, fl], "cpu").shape == (2, lib.LOCAL_LIGHT_FLOATS)
    # the orbit: a closed circle of the right radius in the right plane
    pos = inference.light_orbit_positions((0.5, 0.0, -0.5), 2.0, 8, axis=(0, -1, 0), height=0.3)
    assert pos.shape == (8, 3) and pos.dtype == np.float64
    rel = pos - np.array([0.5, 0.0, -0.5])
    assert np.allclose(rel[:, 1], -0.3) and np.allclose(np.hypot(rel[:, 0], rel[:, 2]), 2.0)
    step = np.linalg.norm(np.roll(pos, -1, axis=0) - pos, axis=-1)
    assert np.allclose(step, 2 * 2.0 * math.sin(math.pi / 8))                      # equal chords, the last one back to frame 0
    assert np.allclose(rel.mean(0), [0, -0.3, 0])
    for kw in (dict(radius=0.0), dict(n_frames=0), dict(axis=(0, 0, 0))):
        with pytest.raises(ValueError):
            inference.light_orbit_positions(**{**dict(centre=(0, 0, 0), radius=1.0, n_frames=4), **kw})
